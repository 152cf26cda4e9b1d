"""``decode_batch`` end to end on the 300 leader-padded reads of the signal_map quality batch: against the workflow in
numpy (tests/decode_ref.py), then as the head of the chain raw signal -> ``decode_batch`` -> ``SeedAligner(k=10)`` ->
``align_signal_batch``; and the tables it rejects."""
import numpy as np
import pytest

import decode_ref as D
import signal_map_ref as R

pytestmark = pytest.mark.gpu

# test_chain_from_raw_signal_alone: the shares measured on an MI355X and the floors 0.03 below them
MEASURED_PLACED, MEASURED_ALIGNED = 0.9400, 0.9400
FLOOR_PLACED, FLOOR_ALIGNED = 0.91, 0.91


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def batch():
    """-> (bare ReadBatch of the padded signals, genome, true_starts, lead, places)"""
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import ReadBatch
    model = synthetic.load_model_arrays()
    rb, aligner, true_starts, (raw, sig_off, lead) = R.quality_batch(model)
    bare = ReadBatch.from_signals(raw, sig_off, np.zeros(0, np.int32), np.zeros(rb.n + 1, np.int64))
    return bare, aligner.reference_num, true_starts, lead, R.quality_places(model)


@pytest.fixture(scope='module')
def decoded(batch, km):
    from nadavca_amd import decode_batch
    return decode_batch(batch[0], kmer_model=km)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def test_decode_batch_equals_its_stages_in_numpy(batch, decoded, km, tmp_path):
    bare = batch[0]
    model = (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)
    ref = D.cpu_decode(R.build_host(tmp_path), D.build_host(tmp_path), bare.raw_signal, bare.sig_off, model)
    for name in ('status', 'n_events', 'n_bases', 'seq_off', 'sequence', 'map_base', 'map_sig', 'map_off'):
        got, want = getattr(decoded, name), ref[name]
        assert got.shape == want.shape and np.array_equal(got, want), name
    assert np.array_equal(bits(decoded.score), bits(ref['score']))
    assert decoded.n_decoded == bare.n and decoded.parts == 1
    rb1 = decoded.read_batch(bare)
    assert rb1.raw_signal is bare.raw_signal or np.array_equal(rb1.raw_signal, bare.raw_signal)
    assert np.array_equal(rb1.sig_off, bare.sig_off)
    for name in ('sequence', 'seq_off', 'map_base', 'map_sig', 'map_off'):
        assert np.array_equal(getattr(rb1, name), ref[name]), name
    assert rb1.sequence.dtype == np.int32 and rb1.map_base.dtype == np.int32 and rb1.map_off.dtype == np.int64


def border_share(res, true_starts, lead, places):
    """share of the final event borders of the aligned reads within 2 samples of the true start of their base; a row's
    base is known from its reference position; a row outside the read's true span has no true start and counts as off"""
    g0, length, reverse = places
    hit = total = 0
    for j, read in enumerate(res.live):
        rows = res.alignment_of(j)
        if rows is None:
            continue
        base = g0[read] + length[read] - 1 - rows[:, 0] if reverse[read] else rows[:, 0] - g0[read]
        inside = (base >= 0) & (base < length[read])
        want = np.asarray(true_starts[read])[base[inside]] + lead[read]
        hit += int((np.abs(rows[inside, 1] - want) <= 2).sum())
        total += rows.shape[0]
    return hit / max(total, 1)


def test_chain_from_raw_signal_alone(batch, decoded, km):
    """raw signal -> decode_batch -> SeedAligner(genome, k=10) -> align_signal_batch, bandwidth 40, on the batch's
    3 000-base genome.  Measured on an MI355X: 0.9400 of the 300 reads placed by SeedAligner, all of them on the right
    strand and 0.9574 of them with their pairs inside the true span +- 32 bases; 0.9400 aligned by align_signal_batch;
    0.8511 of the final event borders within 2 samples of the simulator's (0.8898 from the simulator's table).  Every
    placed read must be on the right strand; the placed and the aligned share have floors 0.03 below the measured
    values: 0.91 and 0.91."""
    from nadavca_amd import defaults
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.batchflow import load_config
    from nadavca_amd.seedalign import SeedAligner
    bare, genome, true_starts, lead, places = batch
    g0, length, reverse = places
    rb1 = decoded.read_batch(bare)
    seed = SeedAligner(genome, k=10)
    hits = seed.align(rb1)
    placed = hits.aligned
    G = genome.size
    inside = np.zeros(bare.n, dtype=bool)
    for r in np.nonzero(placed)[0]:
        ref = hits.ref_idx[hits.off[r]:hits.off[r + 1]]
        lo, hi = (G - 1 - ref.max(), G - 1 - ref.min()) if hits.reverse[r] else (ref.min(), ref.max())
        inside[r] = lo >= g0[r] - 32 and hi < g0[r] + length[r] + 32
    right_strand = hits.reverse[placed] == reverse[placed]
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    res = align_signal_batch(None, rb1, config=config, kmer_model=km, aligner=seed)
    aligned = set(res.live[res.status == 0].tolist())
    share = border_share(res, true_starts, lead, places)
    print('placed %.4f of %d reads; of those on the right strand %.4f, on the right strand and inside the true span '
          '+- 32 bases %.4f; aligned %.4f; final borders within 2 samples %.4f (0.8898 from the simulator\'s table)'
          % (placed.mean(), bare.n, right_strand.mean(), (inside[placed] & right_strand).mean(),
             len(aligned) / bare.n, share))
    assert right_strand.all()
    assert placed.mean() >= FLOOR_PLACED
    assert len(aligned) / bare.n >= FLOOR_ALIGNED


def test_undecoded_reads_drop_out_and_an_empty_batch(batch, km):
    from nadavca_amd import decode_batch
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.seedalign import SeedAligner
    bare, genome = batch[0], batch[1]
    raws = [np.full(300, 7, bare.raw_signal.dtype), bare.raw_signal[:bare.sig_off[1]],
            bare.raw_signal[bare.sig_off[1]:bare.sig_off[1] + 40]]
    sub = ReadBatch.from_signals(np.concatenate(raws), R.offsets([x.size for x in raws]), np.zeros(0, np.int32),
                                 np.zeros(4, np.int64))
    dec = decode_batch(sub, kmer_model=km)
    assert dec.status.tolist() == [D.DEC_NO_EVENTS, 0, D.DEC_NO_EVENTS] and dec.n_decoded == 1
    assert dec.n_bases[[0, 2]].tolist() == [0, 0] and np.isnan(dec.score[[0, 2]]).all() and np.isfinite(dec.score[1])
    assert np.diff(dec.seq_off).tolist() == [0, int(dec.n_bases[1]), 0]
    assert np.diff(dec.map_off)[[0, 2]].tolist() == [0, 0]
    res = align_signal_batch(None, dec.read_batch(sub), kmer_model=km, aligner=SeedAligner(genome, k=10))
    assert set(res.live.tolist()) <= {1}
    z = np.zeros(1, dtype=np.int64)
    none = decode_batch(ReadBatch.from_signals(np.zeros(0, np.int16), z, np.zeros(0, np.int32), z), kmer_model=km)
    assert none.n == 0 and none.sequence.size == 0 and none.map_off.tolist() == [0]


def test_tables_decode_batch_rejects(batch):
    from nadavca_amd import decode_batch
    from nadavca_amd.dtw import KmerModel
    bare = batch[0]
    five = KmerModel(3, 1, 5, np.zeros(5 ** 3), np.ones(5 ** 3))
    with pytest.raises(ValueError, match='4-letter'):
        decode_batch(bare, kmer_model=five)
    ten = KmerModel(10, 4, 4, np.zeros(4 ** 10), np.ones(4 ** 10))
    with pytest.raises(ValueError, match=r'k is 2\.\.6'):
        decode_batch(bare, kmer_model=ten)
