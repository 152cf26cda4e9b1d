"""The seed aligner's kernel (nadavca_amd/csrc/kernels_seedext.hip, nvk_seed_extend_dev) and ``SeedAligner`` on the GPU:

* per read, score, end cell, pair count and pairs equal the CPU restatement (tests/host_shims/seedext_host.cpp) over
  both strands, error rates 0-10 %, lengths 0-1 500 and 4 500-5 500, random and overhanging reads, bands 1-256 and
  three scoring sets; ``get_base_alignments`` equals the CPU pipeline array for array;
* results do not change when the traceback store runs in chunks;
* the batch workflows give with ``SeedAligner`` what they give with ``SyntheticBatchAligner`` on error-free reads;
* edge cases and the C-ABI's argument checks."""
import ctypes as C
import io

import numpy as np
import pytest

from test_seed_align_cpu import cpu_pipeline, host_extend  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _concat(batches):
    from nadavca_amd.readbatch import ReadBatch
    off = lambda name: np.concatenate([[0]] + [np.diff(getattr(b, name)) for b in batches]).cumsum().astype(np.int64)
    cat = lambda name: np.concatenate([getattr(b, name) for b in batches])
    return ReadBatch(cat('raw_signal'), off('sig_off'), cat('sequence'), off('seq_off'), cat('map_base'),
                     cat('map_sig'), off('map_off'))


@pytest.fixture(scope='module')
def mixed():
    """2 032 reads: 2 000 of 0-1 500 bases at error rates 0-10 % (random and overhanging ones among them) and 32 of
    4 500-5 500 bases, on a 30 000-base reference."""
    from nadavca_amd import synthetic
    genome = np.random.default_rng(21).integers(0, 4, 30000)
    parts = []
    for g, rate in enumerate((0.0, 0.01, 0.03, 0.06, 0.10)):
        rb, _, _ = synthetic.make_error_read_batch(400, genome, seed=100 + g, length=750, spread=750,
                                                   substitution_rate=rate, insertion_rate=rate / 2,
                                                   deletion_rate=rate / 2, random_fraction=0.1,
                                                   overhang_fraction=0.15)
        parts.append(rb)
    rb, _, _ = synthetic.make_error_read_batch(32, genome, seed=7, length=5000, spread=500, substitution_rate=0.04,
                                               insertion_rate=0.02, deletion_rate=0.02, overhang_fraction=0.2)
    parts.append(rb)
    rb = _concat(parts)
    lens = np.diff(rb.seq_off)
    assert rb.n >= 2000 and lens.min() == 0 and lens.max() <= 1500 + 5500 and (lens >= 4500).sum() >= 32
    return genome, rb


CONFIGS = [dict(band=1), dict(band=8), dict(band=64), dict(band=256),
           dict(band=64, match=2, mismatch=4, gap_open=4, gap_extend=2, min_score=40),
           dict(band=16, k=11, match=5, mismatch=3, gap_open=8, gap_extend=1, min_score=20)]


@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: '-'.join('%s%d' % kv for kv in sorted(c.items())))
def test_kernel_equals_restatement(mixed, host_extend, cfg):  # noqa: F811
    import torch
    from nadavca_amd import _lib
    from nadavca_amd.device import seed_extend_dev
    from nadavca_amd.seedalign import SeedAligner
    genome, rb = mixed
    al = SeedAligner(genome, **cfg)
    p = al.params
    strand, diag, _ = (x.cpu().numpy() for x in al.seed(rb))
    # the reads the seeds left alone get a random strand and band, off the matrix included: more bands for the check
    rng = np.random.default_rng(p['band'])
    lens = np.diff(rb.seq_off)
    free = strand < 0
    strand = np.where(free & (rng.random(rb.n) < 0.7), rng.integers(0, 2, rb.n), strand).astype(np.int32)
    diag = np.where(free, rng.integers(-lens - 300, genome.size + 300), diag)
    dev = al.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    score, end, count, pairs = seed_extend_dev(_lib.default_context(), t(rb.sequence), t(rb.seq_off),
                                               t(genome.astype(np.int32)), t(strand), t(diag), p['band'], p['match'],
                                               p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'])
    hit, exp_pairs = host_extend(rb.sequence, rb.seq_off, genome, strand, diag, p['band'], p['match'],
                                 p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'])
    got = np.stack([score.cpu().numpy(), end[:, 0].cpu().numpy(), end[:, 1].cpu().numpy(), count.cpu().numpy()], 1)
    bad = np.nonzero((got != hit).any(1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:5]], hit[bad[:5]])
    pairs = pairs.cpu().numpy()
    for j in range(rb.n):
        assert np.array_equal(pairs[rb.seq_off[j]:rb.seq_off[j] + hit[j, 3]], exp_pairs[j]), j
    assert (hit[:, 3] > 0).sum() > rb.n // 3 and ((strand == 1) & (hit[:, 3] > 0)).any()
    # the public path against the CPU pipeline (seeding on the CPU, the restatement)
    ba = al.get_base_alignments(rb)
    exp = cpu_pipeline(SeedAligner(genome, device='cpu', **cfg), rb, host_extend)
    for g, e in zip((ba.read_idx, ba.ref_idx, ba.off, ba.reverse), exp[:4]):
        assert g.dtype == e.dtype and np.array_equal(g, e)


def test_chunked_store_gives_the_same_results(mixed):
    from nadavca_amd import _lib
    from nadavca_amd.seedalign import SeedAligner
    genome, rb = mixed
    al = SeedAligner(genome, band=64)
    ctx = _lib.default_context()
    ref = al.align(rb)
    ctx.set_workspace_limit(3 << 20)     # ~45 reads of 1 000 bases per chunk; a long read runs on its own
    try:
        got = al.align(rb)
    finally:
        ctx.set_workspace_limit(0)
    for f in ('strand', 'diagonal', 'votes', 'score', 'end', 'off', 'read_idx', 'ref_idx', 'reverse'):
        assert np.array_equal(getattr(got, f), getattr(ref, f)), f


@pytest.fixture(scope='module')
def km():
    from nadavca_amd.kmer_model import KmerModel
    from nadavca_amd import defaults
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def exact_reads():
    from nadavca_amd import synthetic
    rb, syn, genome = synthetic.make_read_batch(64, synthetic.load_model_arrays(), seed=31)
    return rb, syn, genome


def test_error_free_pairs_equal_the_synthetic_aligner(exact_reads):
    from nadavca_amd.seedalign import SeedAligner
    rb, syn, genome = exact_reads
    got, exp = SeedAligner(genome).get_base_alignments(rb), syn.get_base_alignments(rb)
    assert exp.reverse.any() and not exp.reverse.all()
    for f in ('read_idx', 'ref_idx', 'off', 'reverse'):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), f


def test_workflows_equal_the_synthetic_aligner(exact_reads, km):
    import copy
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.detect_meth import detect_meth_batch
    from nadavca_amd.estimate_snps import estimate_snps_batch
    from nadavca_amd.seedalign import SeedAligner
    rb, syn, genome = exact_reads
    seed = SeedAligner(genome)
    a, b = (align_signal_batch(None, copy.deepcopy(rb), kmer_model=km, aligner=x) for x in (seed, syn))
    for f in ('live', 'status', 'alignment', 'ref_off'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert len(a.fits) == len(b.fits) and all(np.array_equal(x, y) for x, y in zip(a.fits, b.fits))
    assert a.n_aligned == rb.n
    # the consensus sums are f64 atomic adds (kernels_consensus.hip), whose order varies from run to run: as in
    # tests/test_gpu_estimator.py the chunks are compared exactly and their posteriors to 1e-12
    for independent in (True, False):
        a, b = (estimate_snps_batch(genome, copy.deepcopy(rb), kmer_model=km, independent=independent, aligner=x)
                for x in (seed, syn))
        assert len(a) == len(b) and len(a) >= 1
        if independent:
            a, b = [a.chunk(j) for j in range(len(a))], [b.chunk(j) for j in range(len(b))]
        for x, y in zip(a, b):
            assert (x.start, x.end) == (y.start, y.end) and np.array_equal(x.coverage, y.coverage)
            assert x.values.shape == y.values.shape and np.max(np.abs(x.values - y.values), initial=0) < 1e-12
    a, b = (detect_meth_batch(None, copy.deepcopy(rb), 'CG', kmer_model=km, aligner=x) for x in (seed, syn))
    assert np.array_equal(a.status, b.status) and np.array_equal(a.live, b.live)
    ta, tb = io.StringIO(newline=''), io.StringIO(newline='')
    a.write_csv(ta)
    b.write_csv(tb)
    assert ta.getvalue() == tb.getvalue() and ta.getvalue().count('\n') > 10


def test_edge_cases():
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.seedalign import SeedAligner
    genome = np.random.default_rng(3).integers(0, 4, 2000)
    z = np.zeros(1, dtype=np.int64)
    empty = ReadBatch(np.zeros(0, np.int16), z, np.zeros(0, np.int32), z, np.zeros(0), np.zeros(0), z)
    hits = SeedAligner(genome).align(empty)
    assert hits.n == 0 and hits.off.tolist() == [0] and hits.read_idx.size == 0
    rb, _, _ = synthetic.make_error_read_batch(6, genome, seed=1, length=0, spread=0)
    hits = SeedAligner(genome).align(rb)
    assert (hits.strand == -1).all() and hits.off[-1] == 0 and not hits.reverse.any()
    rb, _, _ = synthetic.make_error_read_batch(6, genome, seed=1, length=300, spread=0)
    for ref in (genome[:13], genome[:0]):
        hits = SeedAligner(ref).align(rb)
        assert (hits.strand == -1).all() and (hits.score == 0).all() and hits.off[-1] == 0
    assert SeedAligner(genome).align(rb).aligned.all()
    bad = ReadBatch(rb.raw_signal, rb.sig_off, np.where(np.arange(rb.sequence.size) == 5, 4, rb.sequence),
                    rb.seq_off, rb.map_base, rb.map_sig, rb.map_off)
    with pytest.raises(ValueError):
        SeedAligner(genome).align(bad)
    with pytest.raises(ValueError):
        SeedAligner(genome).get_base_alignments(ReadBatch(rb.raw_signal, rb.sig_off, -rb.sequence - 1, rb.seq_off,
                                                          rb.map_base, rb.map_sig, rb.map_off))


def test_c_abi_rejects_bad_arguments():
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    ctx = _lib.default_context()
    dev = torch.device('cuda', ctx.device)
    q = torch.zeros(30, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 10, 30], dtype=torch.int64, device=dev)
    ref = torch.zeros(100, dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    dg = torch.zeros(2, dtype=torch.int32, device=dev)
    hit = torch.zeros(8, dtype=torch.int32, device=dev)
    pairs = torch.zeros(60, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(q_=q, off_=off, ref_=ref, st_=st, dg_=dg, hit_=hit, pairs_=pairs, total=30, w=8, sc=(1, 1, 1, 1, 30),
             c=None):
        return lib.nvk_seed_extend_dev(ctx.handle if c is None else c, 2, total, p(q_), p(off_), p(ref_), 100,
                                       p(st_), p(dg_), w, *sc, p(hit_), p(pairs_))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert call() == _lib.NVK_OK
    assert call(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(q_=None), dict(off_=None), dict(ref_=None), dict(st_=None), dict(dg_=None), dict(hit_=None),
               dict(pairs_=None)):
        assert invalid(call(**kw)), kw
    assert invalid(call(off_=torch.tensor([0, 31, 30], dtype=torch.int64, device=dev)))   # decreases
    assert invalid(call(off_=torch.tensor([1, 10, 30], dtype=torch.int64, device=dev)))   # does not start at 0
    assert invalid(call(total=29))                                                       # does not end at the total
    assert invalid(call(w=0))
    assert call(w=257) == _lib.NVK_ERR_UNSUPPORTED
    for sc in ((0, 1, 1, 1, 30), (1, 17, 1, 1, 30), (1, 1, 0, 1, 30), (1, 1, 1, 17, 30), (1, 1, 1, 1, 0)):
        assert invalid(call(sc=sc)), sc
