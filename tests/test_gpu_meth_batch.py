"""``detect_meth_batch`` (nadavca_amd/detect_meth.py) and its kernels (nadavca_amd/csrc/kernels_meth.hip):

* against the reference's own ``detect_meth`` rows (tests/golden/workflows.npz);
* against ``calculate_meth_scores`` + ``maxs3`` on the host, applied to the rows and the normalised signal of the
  same alignment, over both strands, substitutions, int16 raw data, renorm_rounds 0..3 and patterns that are
  short, long, at the ends of a read, empty or never match;
* against the per-read ``detect_meth`` workflow, CSV to CSV;
* edge cases: reads that do not align, a batch where none does, short reference parts, empty events, and the
  C-ABI's argument checks."""
import csv
import ctypes as C
import io
import types

import numpy as np
import pytest

from est_fixture import EstimatorFixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def km():
    from nadavca_amd.kmer_model import KmerModel
    from nadavca_amd import defaults
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


def _batch_from_specs(specs, genome_num):
    """ReadBatch + batch aligner of simulated read specs (synthetic.make_read_spec), in make_read_batch's layout."""
    from nadavca_amd.readbatch import ReadBatch, BaseAlignmentBatch, SyntheticBatchAligner
    inv = {'A': 0, 'C': 1, 'G': 2, 'T': 3}
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    raws = [np.rint(s['raw_signal']).astype(np.int16) for s in specs]
    seqs = [np.array([inv[b] for b in s['sequence']], dtype=np.int32) for s in specs]
    maps = [sorted(s['sequence_to_signal_mapping'].items()) for s in specs]
    rb = ReadBatch(np.concatenate(raws), off(raws), np.concatenate(seqs), off(seqs),
                   np.array([k for m in maps for k, _ in m], dtype=np.int64),
                   np.array([v for m in maps for _, v in m], dtype=np.int64), off(maps))
    bms = [np.asarray(s['base_mapping'], dtype=np.int64).reshape(-1, 2) for s in specs]
    ba = BaseAlignmentBatch(np.concatenate([b[:, 0] for b in bms]), np.concatenate([b[:, 1] for b in bms]),
                            off(bms), np.array([s['reverse'] for s in specs], dtype=bool))
    return rb, SyntheticBatchAligner(genome_num, ba)


def _csv_rows(text):
    return list(csv.reader(io.StringIO(text)))


def _assert_rows_close(got, exp, rtol, atol):
    assert got[0] == exp[0] and len(got) == len(exp)
    for g, e in zip(got[1:], exp[1:]):
        assert g[:3] == e[:3]                                  # file, position, sequence context
        gs, es = np.array(g[3].split(','), dtype=float), np.array(e[3].split(','), dtype=float)
        assert gs.shape == es.shape == (11,) and np.allclose(gs, es, rtol=rtol, atol=atol), (g, e)
        assert np.isclose(float(g[4]), float(e[4]), rtol=rtol, atol=atol), (g, e)


def test_detect_meth_batch_rows_equal_the_reference(km):
    """The reference's detect_meth rows (oracle/make_golden_workflows.py) from the batch form."""
    from nadavca_amd.detect_meth import detect_meth_batch
    from nadavca_amd.genome import Genome
    from nadavca_amd.readbatch import ReadBatch, BaseAlignmentBatch, SyntheticBatchAligner
    wf = EstimatorFixture('workflows.npz')
    n = int(wf.z['meth_n_reads'])
    rb = ReadBatch.from_reads(wf.reads(normalize=False, subset=range(n)))
    assert rb.raw_signal.dtype == np.int16
    bms = [np.asarray(wf.specs[i]['base_mapping'], dtype=np.int64).reshape(-1, 2) for i in range(n)]
    ba = BaseAlignmentBatch(np.concatenate([b[:, 0] for b in bms]), np.concatenate([b[:, 1] for b in bms]),
                            np.concatenate([[0], np.cumsum([len(b) for b in bms])]),
                            [wf.specs[i]['reverse'] for i in range(n)])
    mb = detect_meth_batch(None, rb, str(wf.z['pattern']), config=dict(wf.config), kmer_model=km,
                           aligner=SyntheticBatchAligner(Genome.to_numerical(wf.genome), ba))
    assert mb.live.tolist() == list(range(n)) and mb.status.tolist() == [0] * n
    buf = io.StringIO(newline='')
    mb.write_csv(buf, names=['read%02d.fast5' % i for i in range(n)])
    exp = _csv_rows(str(wf.z['meth_csv']))
    assert len(exp) > 100
    _assert_rows_close(_csv_rows(buf.getvalue()), exp, 1e-9, 1e-12)


def _host_rows(aligned, sa_host, pattern, km):
    """calculate_meth_scores + maxs3 for every aligned read of an AlignedBatch: (read, position, context,
    scores, aggregate) lists in read order."""
    from nadavca_amd.detect_meth import calculate_meth_scores, maxs3
    out = ([], [], [], [], [])
    for j, i in enumerate(aligned.live.tolist()):
        rows = aligned.alignment_of(j)
        if rows is None:
            continue
        part = np.array(list('ACGT'))[sa_host.reference[sa_host.ref_off[j]:sa_host.ref_off[j + 1]]]
        cut = aligned.normalized_signal(i)[rows[0][1]:rows[-1][2]]
        for pos, context, scores in calculate_meth_scores(cut, rows, types.SimpleNamespace(reference_part=part),
                                                          pattern, km):
            for lst, v in zip(out, (i, pos, context, scores, maxs3(scores))):
                lst.append(v)
    return out


def test_kernel_equals_host_scoring_of_its_own_alignment(km):
    from nadavca_amd import synthetic
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.detect_meth import detect_meth_batch
    model = synthetic.load_model_arrays()
    rb, aligner, _ = synthetic.make_read_batch(300, model, seed=41, genome_length=20000, length=300, spread=60,
                                               substitution_rate=0.03)
    assert rb.raw_signal.dtype == np.int16
    n_rows = {}
    for rounds in (0, 1, 2, 3):
        aligned = align_signal_batch(None, rb, kmer_model=km, renorm_rounds=rounds, aligner=aligner)
        assert aligned.n_aligned > 280
        sa = aligned.approximate.host(('reference', 'ref_off'))
        assert sa.reverse.sum().item() > 100 and (~sa.reverse).sum().item() > 100      # both strands
        j0 = int(np.nonzero(aligned.status == 0)[0][0])
        seq = ''.join(np.array(list('ACGT'))[sa.reference[sa.ref_off[j0]:sa.ref_off[j0 + 1]]])
        R = len(seq)
        patterns = ['CG', 'A', 'GATC', 'CCTGG', seq[40:53],      # a 13-mer, longer than the 11-event window
                    seq[:5], seq[-5:], seq[5:10], seq[R - 6:R - 1],  # at the read's first / last (scorable) positions
                    '', 'CCWGG', 'cg']
        for pattern in patterns:
            mb = detect_meth_batch(None, rb, pattern, kmer_model=km, renorm_rounds=rounds, aligner=aligner)
            assert np.array_equal(mb.live, aligned.live) and np.array_equal(mb.status, aligned.status)
            read, pos, context, scores, aggregate = _host_rows(aligned, sa, pattern, km)
            assert mb.read.tolist() == read, (rounds, pattern)
            assert mb.position.tolist() == pos, (rounds, pattern)
            assert mb.context.tolist() == context, (rounds, pattern)
            if read:
                assert np.allclose(mb.scores, np.array(scores), rtol=1e-12, atol=1e-14), (rounds, pattern)
                assert np.allclose(mb.aggregate, np.array(aggregate), rtol=1e-12, atol=1e-14), (rounds, pattern)
            n_rows[(rounds, pattern)] = len(mb)
        assert n_rows[(rounds, 'CCWGG')] == n_rows[(rounds, 'cg')] == 0
        assert n_rows[(rounds, 'CG')] > 500 and n_rows[(rounds, '')] > 50000
        assert n_rows[(rounds, seq[40:53])] >= 1 and n_rows[(rounds, seq[5:10])] >= 1


def test_write_csv_equals_the_per_read_workflow(km, tmp_path):
    from nadavca_amd import synthetic
    from nadavca_amd.alignment import ApproximateAligner
    from nadavca_amd.detect_meth import detect_meth, detect_meth_batch
    model = synthetic.load_model_arrays()
    genome = np.random.default_rng(31).integers(0, 4, 5000).astype(np.int32)
    specs = [synthetic.make_read_spec(np.random.default_rng([32, i]), genome, model, i, length=260, spread=40,
                                      substitution_rate=0.04) for i in range(40)]
    for s in specs:   # the same int16 samples for both forms
        s['raw_signal'] = np.rint(s['raw_signal']).astype(np.int16)
    per_read = str(tmp_path / 'per_read.csv')
    detect_meth(None, synthetic.reads_from_specs(specs), 'CG', per_read, kmer_model=km,
                aligner=synthetic.make_synthetic_aligner(ApproximateAligner, np.array(list('ACGT'))[genome]))
    rb, aligner = _batch_from_specs(specs, genome)
    batch = str(tmp_path / 'batch.csv')
    detect_meth_batch(None, rb, 'CG', kmer_model=km, aligner=aligner).write_csv(batch)
    exp = _csv_rows(open(per_read, newline='').read())
    assert len(exp) > 100
    _assert_rows_close(_csv_rows(open(batch, newline='').read()), exp, 1e-12, 1e-14)


def test_reads_that_do_not_align_give_no_rows(km):
    from nadavca_amd import synthetic, _lib
    from nadavca_amd.detect_meth import detect_meth_batch
    model = synthetic.load_model_arrays()
    genome = np.random.default_rng(51).integers(0, 4, 4000).astype(np.int32)
    spec = lambda i, **kw: synthetic.make_read_spec(np.random.default_rng([52, i]), genome, model, i, **kw)
    specs = [spec(i, length=200) for i in range(6)]
    specs[1] = dict(specs[1], base_mapping=np.zeros((0, 2), dtype=int))     # no anchors: not live
    specs[2] = spec(2, length=200, dwell=(1, 1))                            # fewer samples than 2 R: no path
    specs[4] = spec(4, length=14, spread=0)                                 # reference part shorter than 11
    rb, aligner = _batch_from_specs(specs, genome)
    mb = detect_meth_batch(None, rb, '', kmer_model=km, aligner=aligner)
    assert mb.live.tolist() == [0, 2, 3, 4, 5]
    assert mb.status[1] == _lib.READ_NO_PATH and mb.status[[0, 2, 4]].tolist() == [0, 0, 0]
    assert set(mb.read.tolist()) == {0, 3, 5}
    assert np.all(np.diff(mb.read) >= 0) and np.all(np.diff(mb.position)[np.diff(mb.read) == 0] > 0)
    # none aligns: an empty MethBatch
    none = [dict(s, base_mapping=np.zeros((0, 2), dtype=int)) for s in specs[:3]]
    rb, aligner = _batch_from_specs(none, genome)
    mb = detect_meth_batch(None, rb, 'CG', kmer_model=km, aligner=aligner)
    assert len(mb) == 0 and mb.live.size == 0 and mb.scores.shape == (0, 11)
    buf = io.StringIO(newline='')
    mb.write_csv(buf)
    assert buf.getvalue().count('\n') == 1


def _restated(seq, means, expected, pattern):
    """detect_meth.py:28-65 on one read with given means (NaN = empty event)."""
    from scipy.special import ndtr
    rows, pos = [], seq.find(pattern)
    while pos != -1:
        lo, hi = pos - 5, pos + 6
        if lo >= 0 and hi <= len(seq) and not np.isnan(means[lo:hi]).any():
            z = np.abs(means[lo:hi] - expected[lo:hi]) / 0.35287208
            s = (-np.log(np.maximum(1e-50, ndtr(-z) * 2.0))).tolist()
            rows.append((pos, s, max(a + b + c for a, b, c in zip(s, s[1:], s[2:]))))
        pos = seq.find(pattern, pos + 1)
    return rows


def test_empty_events_drop_only_the_windows_that_hold_them(km):
    import torch
    from nadavca_amd.device import meth_scores_dev
    from nadavca_amd.detect_meth import pattern_codes
    dev = torch.device('cuda', km.context.device)
    rng = np.random.default_rng(61)
    seqs = [list(rng.choice(list('ACGT'), R)) for R in (80, 60, 50)]
    for p in (6, 14, 20, 30, 45, 60, 70):
        seqs[0][p:p + 2] = ['C', 'G']
    for p in (10, 30):
        seqs[1][p:p + 2] = ['C', 'G']
    seqs = [''.join(s) for s in seqs]
    ref = np.array([{'A': 0, 'C': 1, 'G': 2, 'T': 3}[b] for b in ''.join(seqs)], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    expected = rng.normal(0.0, 1.0, ref.size)
    means = expected + rng.normal(0.0, 0.5, ref.size)
    means[off[0] + 25] = np.nan             # in the windows of p = 20 and 30 only
    means[off[0] + 75] = np.nan             # in the window of p = 70 only
    status = np.array([0, 1, 0], dtype=np.int32)   # read 1 has not aligned: no rows whatever its means
    up = lambda a: torch.from_numpy(a).to(dev)
    occ_off, pos, scores, agg = meth_scores_dev(km.context, up(ref), up(off), up(means), up(expected), up(status),
                                                pattern_codes('CG'))
    occ_off, pos, scores, agg = (t.cpu().numpy() for t in (occ_off, pos, scores, agg))
    want = [_restated(s, means[off[j]:off[j + 1]], expected[off[j]:off[j + 1]], 'CG') if status[j] == 0 else []
            for j, s in enumerate(seqs)]
    kept = {p for p, _, _ in want[0]}
    assert {6, 14, 45, 60} <= kept and not {20, 30, 70} & kept
    assert np.diff(occ_off).tolist() == [len(w) for w in want]
    flat = [r for w in want for r in w]
    assert pos.tolist() == [p for p, _, _ in flat]
    assert np.allclose(scores, np.array([s for _, s, _ in flat]), rtol=1e-12, atol=1e-14)
    assert np.allclose(agg, np.array([a for _, _, a in flat]), rtol=1e-12, atol=1e-14)


def test_c_abi_rejects_bad_arguments(km):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', km.context.device)
    ctx = km.context.handle
    ref = torch.zeros(30, dtype=torch.int32, device=dev)
    means = torch.zeros(30, dtype=torch.float64, device=dev)
    off = torch.tensor([0, 10, 30], dtype=torch.int64, device=dev)
    pat = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    pos = torch.zeros(4, dtype=torch.int64, device=dev)
    sc = torch.zeros(44, dtype=torch.float64, device=dev)
    ag = torch.zeros(4, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def count_rc(ref_=ref, off_=off, means_=means, pat_=pat, m=2, out=count, total=30):
        return lib.nvk_meth_count_dev(ctx, 2, total, p(ref_), p(off_), p(means_), p(None), p(pat_), m, p(out))

    def scores_rc(occ, off_=off, expected=means):
        return lib.nvk_meth_scores_dev(ctx, 2, 30, p(ref), p(off_), p(means), p(expected), p(None), p(pat), 2,
                                       p(occ), p(pos), p(sc), p(ag))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert count_rc() == _lib.NVK_OK
    assert lib.nvk_meth_count_dev(None, 2, 30, p(ref), p(off), p(means), p(None), p(pat), 2, p(count)) \
        == _lib.NVK_ERR_INVALID
    assert invalid(count_rc(ref_=None)) and invalid(count_rc(off_=None)) and invalid(count_rc(means_=None))
    assert invalid(count_rc(pat_=None)) and invalid(count_rc(out=None))
    assert count_rc(pat_=None, m=0) == _lib.NVK_OK
    assert invalid(count_rc(m=-1))
    assert invalid(count_rc(total=29))                                                  # ends elsewhere
    assert invalid(count_rc(off_=torch.tensor([0, 31, 30], dtype=torch.int64, device=dev)))   # decreases
    assert invalid(count_rc(off_=torch.tensor([1, 10, 30], dtype=torch.int64, device=dev)))   # does not start at 0
    occ = torch.tensor([0, 2, 4], dtype=torch.int64, device=dev)
    assert scores_rc(occ) == _lib.NVK_OK
    assert invalid(scores_rc(None)) and invalid(scores_rc(occ, expected=None))
    assert invalid(scores_rc(torch.tensor([0, 3, 2], dtype=torch.int64, device=dev)))
    assert invalid(scores_rc(occ, off_=torch.tensor([0, 10, 29], dtype=torch.int64, device=dev)))
    with pytest.raises(ValueError):
        from nadavca_amd.device import meth_scores_dev
        meth_scores_dev(km.context, ref, torch.tensor([0, 31, 30], dtype=torch.int64, device=dev), means, means,
                        None, [1, 2])
