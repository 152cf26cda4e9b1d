"""``signal_locate_batch`` end to end on the 300 leader-padded reads of the signal_map quality batch: against the
workflow in numpy (tests/locate_ref.py), then as the head of the chain raw signal -> ``signal_locate_batch`` ->
``signal_map_batch`` -> ``align_signal_batch`` with the located windows as sequences and the identity as the base
alignment; and on a two-contig ``ReferenceSet``."""
import numpy as np
import pytest

import locate_ref as L
import signal_map_ref as R

pytestmark = pytest.mark.gpu


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
def located(batch, km):
    from nadavca_amd import signal_locate_batch
    return signal_locate_batch(batch[0], batch[1], kmer_model=km, chunks=True)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def test_signal_locate_batch_equals_its_stages_in_numpy(batch, located, km, tmp_path):
    bare, genome = batch[0], batch[1]
    model = (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)
    ref = L.cpu_signal_locate(R.build_host(tmp_path), L.build_host(tmp_path), bare.raw_signal, bare.sig_off, [genome],
                              model)
    ints = ('status', 'contig', 'reverse', 'ref_start', 'ref_end', 'n_events', 'n_chunks', 'n_joined', 'first_event',
            'last_event', 'win_start', 'win_len', 'chunk_off', 'chunk_target', 'chunk_start', 'chunk_end',
            'chunk_first_event', 'chunk_last_event', 'chunk_events', 'chunk_joined')
    for name in ints:
        got, want = getattr(located, name), ref[name]
        assert got.shape == want.shape and np.array_equal(got, want), name
    for name in ('margin', 'score', 'chunk_margin', 'chunk_score'):
        got, want = getattr(located, name), ref[name]
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), name
    assert located.n_located == int((ref['status'] == 0).sum()) >= 0.98 * bare.n


def test_chain_from_raw_signal_alone(batch, located, km):
    """raw signal -> signal_locate_batch -> signal_map_batch -> align_signal_batch(aligner=loc.aligner()), bandwidth
    40.  Measured on an MI355X: 300 of 300 located, mapped and aligned; 0.9867 of the windows' bases mapped, 0.9697 of
    those within 20 samples of the simulator's starts, 0.0273 further off than 40."""
    from nadavca_amd import defaults, signal_map_batch
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.batchflow import load_config
    bare, genome, true_starts, lead, places = batch
    g0, length, reverse = places
    loc = located
    ok = loc.status == 0
    assert (loc.reverse == reverse)[ok].all()
    rb1 = loc.read_batch(bare)
    assert np.array_equal(np.diff(rb1.seq_off), loc.ref_end - loc.ref_start)
    fwd = [genome[s:e] for s, e in zip(loc.ref_start, loc.ref_end)]
    want = [3 - f[::-1] if rv else f for f, rv in zip(fwd, loc.reverse)]
    assert np.array_equal(rb1.sequence, np.concatenate(want))
    sm = signal_map_batch(rb1, kmer_model=km)
    rb2 = sm.read_batch(rb1)
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    res = align_signal_batch(None, rb2, config=config, kmer_model=km, aligner=loc.aligner())
    aligned = set(res.live[res.status == 0].tolist())
    mapped_reads = float((sm.status == 0).mean())
    quality = L.window_quality(dict(map_base=sm.map_base, map_sig=sm.map_sig, map_off=sm.map_off),
                               dict(ref_start=loc.ref_start, ref_end=loc.ref_end, reverse=loc.reverse), places,
                               true_starts, lead)
    # the rows of the aligned reads lie on the located windows
    for j, read in enumerate(res.live):
        rows = res.alignment_of(j)
        if rows is not None:
            assert rows[:, 0].min() >= loc.ref_start[read] and rows[:, 0].max() < loc.ref_end[read]
    print('located %d, mapped %.4f, aligned %.4f of %d reads; bases mapped %.4f, within 20 samples %.4f, beyond 40 %.4f'
          % ((loc.n_located, mapped_reads, len(aligned) / bare.n, bare.n) + quality))
    assert mapped_reads >= 0.97 and len(aligned) >= 0.97 * bare.n
    assert quality[1] >= 0.93 and quality[2] <= 0.05


def test_two_contigs(batch, km):
    """The genome cut into two contigs of 1 700 and 1 300 bases: reads inside one contig are placed there with
    contig-local positions, and no window crosses the join."""
    from nadavca_amd import ReferenceSet, signal_locate_batch
    from nadavca_amd.readbatch import ReadBatch
    bare, genome, _, _, (g0, length, reverse) = batch
    cut = 1700
    refset = ReferenceSet.from_arrays(['a', 'b'], [genome[:cut], genome[cut:]])
    pick = np.concatenate([np.nonzero(g0 + length <= cut - 40)[0][:20], np.nonzero(g0 >= cut + 40)[0][:20],
                           np.nonzero((g0 < cut - 60) & (g0 + length > cut + 60))[0][:4]])
    raws = [bare.raw_signal[bare.sig_off[r]:bare.sig_off[r + 1]] for r in pick]
    sub = ReadBatch.from_signals(np.concatenate(raws), R.offsets([x.size for x in raws]), np.zeros(0, np.int32),
                                 np.zeros(pick.size + 1, np.int64))
    loc = signal_locate_batch(sub, refset, kmer_model=km)
    ok = loc.status == 0
    inside = np.arange(pick.size) < 40
    assert ok[inside].mean() >= 0.95
    want_contig = (g0[pick] >= cut).astype(np.int32)
    first = np.where(want_contig == 1, cut, 0)
    sel = ok & inside
    assert np.array_equal(loc.contig[sel], want_contig[sel]) and np.array_equal(loc.reverse[sel], reverse[pick][sel])
    assert (np.abs(loc.ref_start + first - g0[pick])[sel] <= 32).mean() >= 0.9
    assert (np.abs(loc.ref_end + first - (g0 + length)[pick])[sel] <= 32).mean() >= 0.9
    sizes = np.diff(refset.offsets)
    assert (loc.ref_start[ok] >= 0).all() and (loc.ref_end[ok] <= sizes[loc.contig[ok]]).all()
    ba = loc.aligner().get_base_alignments(loc.read_batch(sub))
    assert np.array_equal(ba.contig, loc.contig) and np.array_equal(np.diff(ba.off), loc.win_len)
    assert loc.aligner().reference_set is refset and loc.aligner().reference_num is refset.codes
    # oriented window start: counted from the contig's end on the reverse strand
    r = int(np.nonzero(ok)[0][0])
    want = sizes[loc.contig[r]] - loc.ref_end[r] if loc.reverse[r] else loc.ref_start[r]
    assert ba.ref_idx[ba.off[r]] == want and ba.read_idx[ba.off[r]] == 0


def test_reads_without_events_and_an_empty_batch(batch, km):
    from nadavca_amd import signal_locate_batch
    from nadavca_amd.readbatch import ReadBatch
    bare, genome = batch[0], batch[1]
    raws = [np.full(300, 7, bare.raw_signal.dtype), bare.raw_signal[:bare.sig_off[1]],
            bare.raw_signal[bare.sig_off[1]:bare.sig_off[1] + 40]]
    sub = ReadBatch.from_signals(np.concatenate(raws), R.offsets([x.size for x in raws]), np.zeros(0, np.int32),
                                 np.zeros(4, np.int64))
    loc = signal_locate_batch(sub, genome, kmer_model=km)
    assert loc.status.tolist() == [L.LOC_NO_EVENTS, 0, L.LOC_NO_EVENTS]
    assert loc.contig.tolist() == [-1, 0, -1] and np.isnan(loc.margin[[0, 2]]).all()
    rb1 = loc.read_batch(sub)
    assert np.diff(rb1.seq_off).tolist() == [0, int(loc.win_len[1]), 0]
    ba = loc.aligner().get_base_alignments(rb1)
    assert np.diff(ba.off).tolist() == [0, int(loc.win_len[1]), 0] and ba.contig is None
    z = np.zeros(1, dtype=np.int64)
    none = signal_locate_batch(ReadBatch.from_signals(np.zeros(0, np.int16), z, np.zeros(0, np.int32), z), genome,
                               kmer_model=km)
    assert none.n == 0 and none.status.size == 0
