"""``signal_map_batch`` end to end: ``align_signal_batch`` with ``SeedAligner`` at bandwidth 40 on the 300-read batch
of the quality tests, once from the simulator's base -> sample table and once from the table ``signal_map_batch``
rebuilds from signal and sequence alone.  The second run is measured against the first, the existing path."""
import copy

import numpy as np
import pytest

import signal_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def batch():
    from nadavca_amd import synthetic
    rb, aligner, true_starts, _ = R.quality_batch(synthetic.load_model_arrays())
    return rb, aligner.reference_num, true_starts


@pytest.fixture(scope='module')
def mapped(batch, km):
    from nadavca_amd import signal_map_batch
    from nadavca_amd.readbatch import ReadBatch
    rb = batch[0]
    bare = ReadBatch.from_signals(rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off)
    return bare, signal_map_batch(bare, kmer_model=km, events=True)


def test_signal_map_batch_equals_its_stages_in_numpy(batch, mapped, km, tmp_path):
    """The public result against the CPU pipeline: integers exactly; the k-mer constants, the moments and the
    transition costs come from torch there and from numpy here, so levels and scores are compared closely."""
    rb, _, true_starts = batch
    _, sm = mapped
    host = R.build_host(tmp_path)
    model = (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)
    ref = R.cpu_signal_map(host, rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off, model)
    assert (sm.status == 0).all() and sm.n_mapped == rb.n
    assert np.array_equal(sm.n_events, ref['n_events']) and np.array_equal(sm.ev_off, ref['ev_off'])
    assert np.array_equal(sm.ev_start, ref['ev_start']) and np.array_equal(sm.ev_len, ref['ev_len'])
    assert np.allclose(sm.ev_level, ref['ev_level'], rtol=1e-12, atol=1e-12)
    assert np.allclose(sm.scale, ref['scale'], rtol=1e-9) and np.allclose(sm.shift, ref['shift'], rtol=1e-9, atol=1e-9)
    agree = np.mean([np.array_equal(sm.map_sig[sm.map_off[r]:sm.map_off[r + 1]],
                                    ref['map_sig'][ref['map_off'][r]:ref['map_off'][r + 1]]) for r in range(rb.n)])
    assert agree >= 0.99          # (a path decided by the last bits of a level may differ)
    n_al = ref['last_event'] - ref['first_event'] + 1
    want = (ref['path_score'] - (ref['first_event'] + ref['n_events'] - 1 - ref['last_event']) * np.log(0.01)) / n_al
    same = (sm.first_event == ref['first_event']) & (sm.last_event == ref['last_event'])
    assert same.mean() >= 0.99 and np.allclose(sm.score[same], want[same], rtol=1e-6)
    res = dict(status=sm.status, map_base=sm.map_base, map_sig=sm.map_sig, map_off=sm.map_off)
    mapped_share, near, far = R.quality(res, rb.seq_off, true_starts)
    assert mapped_share >= 0.98 and near >= 0.98 and far <= 0.002


def border_share(res, true_starts, places):
    """share of the final event borders of the aligned reads within 2 samples of the true start of their base; a row's
    base is known from its reference position, the reads being error-free"""
    g0, length, reverse = places
    hit = total = 0
    for j, read in enumerate(res.live):
        rows = res.alignment_of(j)
        if rows is None:
            continue
        base = g0[read] + length[read] - 1 - rows[:, 0] if reverse[read] else rows[:, 0] - g0[read]
        assert base.min() >= 0 and base.max() < length[read] and (np.diff(base) == 1).all()
        want = np.asarray(true_starts[read])[base]
        hit += int((np.abs(rows[:, 1] - want) <= 2).sum())
        total += rows.shape[0]
    return hit / max(total, 1)


def test_workflow_from_the_rebuilt_table_is_as_good_as_from_the_simulators(batch, mapped, km):
    """Measured: share of borders within 2 samples 0.8898 from the simulator's table, 0.8940 from the rebuilt one;
    0.9633 of the rows both runs cover are identical."""
    from nadavca_amd import defaults, synthetic
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.batchflow import load_config
    from nadavca_amd.seedalign import SeedAligner
    rb, genome, true_starts = batch
    bare, sm = mapped
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    seed = SeedAligner(genome)
    a = align_signal_batch(None, copy.deepcopy(rb), config=config, kmer_model=km, aligner=seed)
    b = align_signal_batch(None, sm.read_batch(bare), config=config, kmer_model=km, aligner=seed)
    live_a, live_b = set(a.live[a.status == 0].tolist()), set(b.live[b.status == 0].tolist())
    assert len(live_a) >= 0.9 * rb.n
    assert live_a <= live_b
    places = R.quality_places(synthetic.load_model_arrays())
    share_a, share_b = border_share(a, true_starts, places), border_share(b, true_starts, places)
    where_b = {int(r): j for j, r in enumerate(b.live)}
    # rows of the reference range both runs cover (a run's range starts at its first and ends at its last anchor, and
    # its first and last events are cut by its own window: those two rows are left out)
    def common(x, y):
        lo, hi = max(x[:, 0].min(), y[:, 0].min()) + 1, min(x[:, 0].max(), y[:, 0].max()) - 1
        return x[(x[:, 0] >= lo) & (x[:, 0] <= hi)], y[(y[:, 0] >= lo) & (y[:, 0] <= hi)]
    pairs = [common(a.alignment_of(j), b.alignment_of(where_b[int(r)])) for j, r in enumerate(a.live)
             if a.status[j] == 0]
    identical = np.mean([np.array_equal(x, y) for x, y in pairs])
    rows_equal = np.mean(np.concatenate([(x == y).all(axis=1) for x, y in pairs]))
    print('borders within 2 samples: %.4f from the simulator\'s table, %.4f from the rebuilt one; reads with identical '
          'rows: %.4f, rows identical: %.4f; aligned %d / %d of %d'
          % (share_a, share_b, identical, rows_equal, len(live_a), len(live_b), rb.n))
    assert share_b >= share_a - 0.01


def test_unmapped_reads_drop_out_downstream(batch, km):
    """A read without events and one whose signal lost 100 bases get no rows, so no anchors: not live."""
    from nadavca_amd import signal_map_batch, synthetic
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.seedalign import SeedAligner
    rb, genome, _ = batch
    cut, cut_seq, _ = R.cut_read(synthetic.load_model_arrays())
    raws = [rb.raw_signal[:rb.sig_off[1]], np.full(300, 7, rb.raw_signal.dtype), cut.astype(rb.raw_signal.dtype)]
    seqs = [rb.sequence[:rb.seq_off[1]], rb.sequence[rb.seq_off[1]:rb.seq_off[2]], cut_seq]
    bare = ReadBatch.from_signals(np.concatenate(raws), R.offsets([x.size for x in raws]), np.concatenate(seqs),
                                  R.offsets([x.size for x in seqs]))
    sm = signal_map_batch(bare, kmer_model=km)
    assert sm.status.tolist() == [0, R.MAP_NO_EVENTS, R.MAP_LOST]
    assert sm.map_off[1] > 0 and sm.map_off[1] == sm.map_off[2] == sm.map_off[3]
    assert np.isnan(sm.score[1]) and sm.first_event[1] == -1
    res = align_signal_batch(None, sm.read_batch(bare), kmer_model=km, aligner=SeedAligner(genome))
    assert res.live.tolist() == [0]


def test_empty_batch(km):
    from nadavca_amd import signal_map_batch
    from nadavca_amd.readbatch import ReadBatch
    z = np.zeros(1, dtype=np.int64)
    sm = signal_map_batch(ReadBatch.from_signals(np.zeros(0, np.int16), z, np.zeros(0, np.int32), z), kmer_model=km)
    assert sm.n == 0 and sm.map_off.tolist() == [0] and sm.map_base.size == 0
