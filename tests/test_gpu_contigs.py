"""Multi-contig references on the GPU: the extension kernel with per-read reference bounds
(nvk_seed_extend_bounded_dev) against the CPU restatement on the cut reference, ``SeedAligner`` over a
``refset.ReferenceSet`` against the simulated truth and the CPU pipeline, and the batch workflows over a ReferenceSet
against per-contig runs and against one run over the concatenation as a single sequence."""
import copy
import ctypes as C
import io

import numpy as np
import pytest

from contig_fixture import ContigFixture, NAMES, READS_PER_CONTIG, concat_batches
from test_contigs_cpu import numpy_contig_rule
from test_gpu_seed_align import CONFIGS, mixed  # noqa: F401  (fixture)
from test_seed_align_cpu import host_extend  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


@pytest.fixture(scope='module')
def fx(model):
    return ContigFixture(model)


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


def bounded_on_host(host_extend, rb, genome, strand, diag, lo, hi, p):  # noqa: F811
    """What include/nadavca_hip.h asks of nvk_seed_extend_bounded_dev: per read the restatement of
    nvk_seed_extend_dev on the reference cut to the read's range, with diag - lo; every j moved back by lo."""
    G = genome.size
    hit = np.zeros((rb.n, 4), dtype=np.int32)
    pairs = []
    for j in range(rb.n):
        if strand[j] not in (0, 1):
            hit[j] = (0, -1, -1, 0)
            pairs.append(np.zeros((0, 2), np.int32))
            continue
        cut = genome[G - hi[j]:G - lo[j]] if strand[j] == 1 else genome[lo[j]:hi[j]]
        seq = rb.sequence[rb.seq_off[j]:rb.seq_off[j + 1]]
        h, pr = host_extend(seq, [0, seq.size], cut, [strand[j]], [int(diag[j]) - int(lo[j])], p['band'], p['match'],
                            p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'])
        hit[j] = h[0]
        if h[0, 2] >= 0:
            hit[j, 2] += lo[j]
        pairs.append(pr[0] + np.array([0, lo[j]], dtype=np.int32))
    return hit, pairs


def random_bounds(rng, rb, G, strand, diag):
    """Every read a random strand, a random range [lo, hi) and a diagonal near it: a third of the reads that seeded
    keep their strand and diagonal and get a range that cuts through where they lie; empty ranges, ranges at 0 and at
    G and the full range are among them."""
    n = rb.n
    lens = np.diff(rb.seq_off)
    lo = rng.integers(0, G + 1, n)
    hi = np.minimum(G, lo + rng.integers(0, 3000, n))
    kind = rng.integers(0, 12, n)
    seeded = strand >= 0
    strand = np.where(seeded & (kind < 4), strand, rng.integers(0, 2, n)).astype(np.int32)
    cut = seeded & (kind < 4)            # a boundary inside the read's own span on its diagonal
    edge = np.clip(diag + rng.integers(0, np.maximum(lens, 1)), 0, G)
    lo = np.where(cut & (kind < 2), edge, np.where(cut, np.maximum(0, edge - rng.integers(1, 1500, n)), lo))
    hi = np.where(cut & (kind < 2), np.minimum(G, edge + rng.integers(1, 1500, n)), np.where(cut, edge, hi))
    lo = np.where(kind == 4, 0, lo)                          # ranges at 0
    hi = np.where(kind == 4, rng.integers(0, 2000, n), hi)
    hi = np.where(kind == 5, G, hi)                          # ranges at G
    lo = np.where(kind == 5, G - rng.integers(0, 2000, n), lo)
    hi = np.where(kind == 6, lo, hi)                         # empty ranges
    lo = np.where(kind == 7, 0, lo)                          # the full range
    hi = np.where(kind == 7, G, hi)
    hi = np.maximum(hi, lo)
    near = rng.integers(lo - lens - 40, hi + 40)
    diag = np.where(cut, diag, near)
    skip = rng.random(n) < 0.03
    strand = np.where(skip, -1, strand).astype(np.int32)
    assert (lo >= 0).all() and (hi <= G).all() and (lo <= hi).all()
    assert (lo == hi).any() and (lo == 0).any() and (hi == G).any() and ((lo == 0) & (hi == G)).any()
    return strand, diag.astype(np.int64), lo.astype(np.int32), hi.astype(np.int32)


def run_kernel(al, rb, genome, strand, diag, lo=None, hi=None):
    import torch
    from nadavca_amd import _lib
    from nadavca_amd.device import seed_extend_dev
    p = al.params
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(al.device)
    score, end, count, pairs = seed_extend_dev(_lib.default_context(), t(rb.sequence), t(rb.seq_off),
                                               t(genome.astype(np.int32)), t(strand), t(diag), p['band'], p['match'],
                                               p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'], t(lo),
                                               t(hi))
    got = np.stack([score.cpu().numpy(), end[:, 0].cpu().numpy(), end[:, 1].cpu().numpy(), count.cpu().numpy()], 1)
    return got, pairs.cpu().numpy()


@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: '-'.join('%s%d' % kv for kv in sorted(c.items())))
def test_bounded_kernel_equals_restatement_on_the_cut_reference(mixed, host_extend, cfg):  # noqa: F811
    from nadavca_amd import _lib
    from nadavca_amd.seedalign import SeedAligner
    genome, rb = mixed
    G = genome.size
    al = SeedAligner(genome, **cfg)
    p = al.params
    strand, diag, _ = (x.cpu().numpy() for x in al.seed(rb))
    rng = np.random.default_rng(1000 + p['band'])
    strand, diag, lo, hi = random_bounds(rng, rb, G, strand, diag)
    got, pairs = run_kernel(al, rb, genome, strand, diag, lo, hi)
    hit, exp_pairs = bounded_on_host(host_extend, rb, genome, strand, diag, lo, hi, p)
    bad = np.nonzero((got != hit).any(1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:5]], hit[bad[:5]], lo[bad[:5]], hi[bad[:5]])
    for j in range(rb.n):
        assert np.array_equal(pairs[rb.seq_off[j]:rb.seq_off[j] + hit[j, 3]], exp_pairs[j]), j
    has = hit[:, 3] > 0
    assert has.sum() > rb.n // 8 and ((strand == 1) & has).any() and ((strand == 0) & has).any()
    inside = np.concatenate([pr[:, 1] for pr in exp_pairs if len(pr)])
    owner = np.repeat(np.arange(rb.n), hit[:, 3])
    assert (inside >= lo[owner]).all() and (inside < hi[owner]).all()
    # alignments that stop at a bound: pairs on the range's first and on its last column
    assert (inside == lo[owner]).any() and (inside == hi[owner] - 1).any()
    empty = (lo == hi) & (strand >= 0)
    assert empty.any() and (got[empty] == np.array([0, -1, -1, 0])).all()
    # a chunked traceback store gives the same results
    ctx = _lib.default_context()
    ctx.set_workspace_limit(3 << 20)
    try:
        again, again_pairs = run_kernel(al, rb, genome, strand, diag, lo, hi)
    finally:
        ctx.set_workspace_limit(0)
    assert np.array_equal(again, got)
    for j in range(rb.n):
        s = slice(rb.seq_off[j], rb.seq_off[j] + got[j, 3])
        assert np.array_equal(again_pairs[s], pairs[s]), j
    # with the full range for every read: nvk_seed_extend_dev's outputs
    full, full_pairs = run_kernel(al, rb, genome, strand, diag, np.zeros(rb.n, np.int32), np.full(rb.n, G, np.int32))
    old, old_pairs = run_kernel(al, rb, genome, strand, diag)
    assert np.array_equal(full, old)
    for j in range(rb.n):
        s = slice(rb.seq_off[j], rb.seq_off[j] + old[j, 3])
        assert np.array_equal(full_pairs[s], old_pairs[s]), j


def test_bounded_entry_rejects_bad_bounds():
    import torch
    from nadavca_amd import _lib
    from nadavca_amd.device import seed_extend_dev
    lib = _lib.load()
    ctx = _lib.default_context()
    dev = torch.device('cuda', ctx.device)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    q = torch.zeros(30, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 10, 30], dtype=torch.int64, device=dev)
    ref = torch.zeros(100, dtype=torch.int32, device=dev)
    dg = i32([0, 0])
    hit = torch.zeros(8, dtype=torch.int32, device=dev)
    pairs = torch.zeros(60, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(lo, hi, st=(0, 1)):
        lo, hi = (None if v is None else i32(v) for v in (lo, hi))
        return lib.nvk_seed_extend_bounded_dev(ctx.handle, 2, 30, p(q), p(off), p(ref), 100, p(i32(list(st))), p(dg),
                                               p(lo), p(hi), 8, 1, 1, 1, 1, 30, p(hit), p(pairs))

    assert call([0, 0], [100, 100]) == _lib.NVK_OK
    assert call([5, 100], [5, 100]) == _lib.NVK_OK              # empty ranges, at G too
    assert hit.cpu().reshape(2, 4).tolist() == [[0, -1, -1, 0]] * 2
    for lo, hi in (([-1, 0], [100, 100]), ([0, 0], [100, 101]), ([0, 51], [100, 50]), (None, [100, 100]),
                   ([0, 0], None)):
        assert call(lo, hi) == _lib.NVK_ERR_INVALID and lib.nvk_last_error(), (lo, hi)
    # a skipped read's bounds are not looked at
    assert call([-7, 0], [1000, 100], st=(-1, 0)) == _lib.NVK_OK
    with pytest.raises(ValueError):
        seed_extend_dev(ctx, q, off, ref, i32([0, 1]), dg, 8, 1, 1, 1, 1, 30, i32([0, 60]), i32([100, 50]))
    with pytest.raises(ValueError):
        seed_extend_dev(ctx, q, off, ref, i32([0, 1]), dg, 8, 1, 1, 1, 1, 30, i32([0, 0]), None)


def test_seed_aligner_over_a_reference_set_finds_the_true_pairs(fx):
    from nadavca_amd.seedalign import SeedAligner
    al = SeedAligner(fx.refset)
    assert al.reference_set is fx.refset and np.array_equal(al.reference_num, fx.refset.codes)
    hits = al.align(fx.rb)
    exp = fx.local_alignments()
    assert hits.aligned.all() and hits.contig.dtype == np.int32 and np.array_equal(hits.contig, fx.contig)
    ba = hits.base_alignments()
    for f in ('read_idx', 'ref_idx', 'off', 'reverse', 'contig'):
        assert getattr(ba, f).dtype == getattr(exp, f).dtype and np.array_equal(getattr(ba, f), getattr(exp, f)), f
    assert exp.reverse.sum() == 72
    # the reads of the 400-base contig are paired from its first base to its last
    first, last = ba.ref_idx[ba.off[:-1]], ba.ref_idx[ba.off[1:] - 1]
    assert (first[fx.contig == 2] == 0).all() and (last[fx.contig == 2] == 399).all()


def test_seed_aligner_over_a_reference_set_equals_the_cpu_pipeline(fx, host_extend):  # noqa: F811
    from nadavca_amd import synthetic
    from nadavca_amd.seedalign import SeedAligner
    parts = []
    for c, genome in enumerate(fx.contigs[:3]):
        kw = dict(length=300, spread=40) if genome.size == 400 else {}
        rb, _, _ = synthetic.make_error_read_batch(120, genome, seed=50 + c, substitution_rate=0.03,
                                                   insertion_rate=0.015, deletion_rate=0.015, overhang_fraction=0.15,
                                                   random_fraction=0.05, **kw)
        parts.append(rb)
    rb = concat_batches(parts)
    hits = SeedAligner(fx.refset).align(rb)
    cpu = SeedAligner(fx.refset, device='cpu')
    p = cpu.params
    strand, diag, votes = (x.numpy() for x in cpu.seed(rb))
    rule = numpy_contig_rule(fx.refset, rb.seq_off, strand, diag)
    hit, pairs = bounded_on_host(host_extend, rb, fx.refset.codes, strand, diag, rule[:, 1], rule[:, 2], p)
    aligned = (strand >= 0) & (hit[:, 0] >= p['min_score'])
    flat = np.concatenate(pairs)
    owner = np.repeat(np.arange(rb.n), hit[:, 3])
    exp = dict(strand=strand, diagonal=diag, votes=votes, score=hit[:, 0], end=hit[:, 1:3], aligned=aligned,
               off=np.concatenate([[0], np.cumsum(hit[:, 3])]).astype(np.int64), read_idx=flat[:, 0],
               ref_idx=(flat[:, 1] - rule[owner, 1]).astype(np.int64), reverse=aligned & (strand == 1),
               contig=np.where(aligned, rule[:, 0], -1).astype(np.int32))
    for f, e in exp.items():
        g = getattr(hits, f)
        assert g.dtype == e.dtype and np.array_equal(g, e), f
    truth = np.repeat(np.arange(3), 120)
    assert aligned.sum() > 0.85 * rb.n and (hits.contig[aligned] == truth[aligned]).mean() > 0.98
    lens = fx.refset.offsets[1:] - fx.refset.offsets[:-1]
    assert (hits.ref_idx >= 0).all() and (hits.ref_idx < lens[hits.contig[owner]]).all()


def test_align_signal_batch_over_a_reference_set_equals_the_per_contig_runs(fx, km):
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.seedalign import SeedAligner
    multi = align_signal_batch(None, copy.deepcopy(fx.rb), kmer_model=km, aligner=SeedAligner(fx.refset))
    each = [align_signal_batch(None, copy.deepcopy(rb), kmer_model=km, aligner=SeedAligner(genome))
            for rb, _, genome in fx.parts]
    cat = lambda f: np.concatenate([getattr(e, f) for e in each])
    assert multi.contig_names == NAMES and all(e.contig_names is None and (e.contig == 0).all() for e in each)
    assert np.array_equal(multi.live, np.concatenate([e.live + b for e, b in zip(each, fx.read_base)]))
    assert multi.live.size == fx.rb.n and multi.n_aligned == sum(e.n_aligned for e in each) > 0.9 * fx.rb.n
    assert multi.contig.dtype == np.int32 and np.array_equal(multi.contig, fx.contig[multi.live])
    assert np.array_equal(multi.status, cat('status'))
    assert np.array_equal(np.diff(multi.ref_off), np.concatenate([np.diff(e.ref_off) for e in each]))
    assert np.array_equal(multi.alignment, cat('alignment'))       # contig-local positions, events
    assert len(multi.fits) == len(each[0].fits) > 0
    for r, f in enumerate(multi.fits):
        assert np.array_equal(f, np.concatenate([e.fits[r] for e in each]))
    lens = fx.refset.offsets[1:] - fx.refset.offsets[:-1]
    rows_contig = np.repeat(multi.contig, np.diff(multi.ref_off))
    assert (multi.alignment[:, 0] >= 0).all() and (multi.alignment[:, 0] < lens[rows_contig]).all()


def single_sequence_aligner(fx):
    """The concatenation as ONE sequence, the truth lifted to its coordinates: what a multi-contig run is held to."""
    from nadavca_amd.readbatch import SyntheticBatchAligner
    return SyntheticBatchAligner(fx.refset.codes, fx.global_alignments())


@pytest.mark.parametrize('independent', [False, True])
def test_estimate_snps_batch_over_a_reference_set(fx, km, independent):
    from nadavca_amd.estimate_snps import estimate_snps_batch
    from nadavca_amd.seedalign import SeedAligner
    multi = estimate_snps_batch(fx.refset, copy.deepcopy(fx.rb), kmer_model=km, independent=independent,
                                aligner=SeedAligner(fx.refset))
    single = estimate_snps_batch(fx.refset.codes, copy.deepcopy(fx.rb), kmer_model=km, independent=independent,
                                 aligner=single_sequence_aligner(fx))
    assert len(multi) == len(single) >= 3
    if independent:
        assert np.array_equal(multi.reads, single.reads) and multi.contig_names == NAMES and single.contig is None
        assert np.array_equal(multi.contig, fx.contig[multi.reads])
        multi, single = [multi.chunk(j) for j in range(len(multi))], [single.chunk(j) for j in range(len(single))]
    off = fx.refset.offsets
    seen = set()
    for x, y in zip(multi, single):
        c, start = fx.refset.locate(y.start)
        c_end, end = fx.refset.locate(y.end - 1)
        assert c == c_end                                    # no chunk spans a join
        assert y.contig is None and (x.contig, x.start, x.end) == (NAMES[c], start, end + 1)
        assert 0 <= x.start < x.end <= off[c + 1] - off[c]
        assert np.array_equal(x.coverage, y.coverage)
        assert x.values.shape == y.values.shape and np.max(np.abs(x.values - y.values), initial=0) < 1e-12
        seen.add(x.contig)
    assert seen == set(NAMES[:3])
    # the 400-base contig's reads reach both of its joins: its chunks end within the anchors' trim of them, and the
    # neighbours' chunks were not merged into them
    flush = [x for x in multi if x.contig == NAMES[2]]
    assert min(x.start for x in flush) <= 12 and max(x.end for x in flush) >= 400 - 12


def test_estimate_snps_batch_refuses_another_reference(fx, km):
    from nadavca_amd.estimate_snps import estimate_snps_batch
    from nadavca_amd.refset import ReferenceSet
    from nadavca_amd.seedalign import SeedAligner
    other = ReferenceSet.from_arrays(NAMES[:2], [fx.contigs[1], fx.contigs[0]])
    with pytest.raises(ValueError, match='concatenation'):
        estimate_snps_batch(other, copy.deepcopy(fx.rb), kmer_model=km, aligner=SeedAligner(fx.refset))


def test_detect_meth_batch_and_kmer_training_over_a_reference_set(fx, km):
    from nadavca_amd.detect_meth import detect_meth_batch
    from nadavca_amd.kmer_train import estimate_kmer_model
    from nadavca_amd.seedalign import SeedAligner
    seed, single = SeedAligner(fx.refset), single_sequence_aligner(fx)
    a, b = (detect_meth_batch(None, copy.deepcopy(fx.rb), 'CG', kmer_model=km, aligner=x) for x in (seed, single))
    assert np.array_equal(a.status, b.status) and np.array_equal(a.live, b.live)
    ta, tb = io.StringIO(newline=''), io.StringIO(newline='')
    a.write_csv(ta)
    b.write_csv(tb)
    assert ta.getvalue() == tb.getvalue() and ta.getvalue().count('\n') > 10
    assert a.contig_names == NAMES and b.contig_names is None and (b.contig == 0).all()
    assert a.contig.dtype == np.int32 and np.array_equal(a.contig, fx.contig[a.read])
    assert set(a.contig.tolist()) == {0, 1, 2}
    a, b = (estimate_kmer_model(copy.deepcopy(fx.rb), x, kmer_model=km, rounds=1, min_events=3)
            for x in (seed, single))
    assert a.history == b.history and a.history[0]['kmers_updated'] > 100
    for f in ('mean', 'sigma', 'events', 'samples', 'updated'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
