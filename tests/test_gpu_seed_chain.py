"""The chained mode of the seed aligner on the GPU (nadavca_amd/csrc/kernels_seedchain.hip: nvk_seed_chain_dev, and the
path form of kernels_seedext.hip: nvk_seed_extend_path_dev):

* the chain kernel equals its CPU restatement (tests/host_shims/seedchain_host.cpp) in chain score, anchors and every
  strip centre, on simulated reads of all lengths and on constructed seed lists around the ring's and the load
  blocks' 64;
* the extension along a path equals its restatement in score, end cell, count and pairs over bands 1-256 and two
  scoring sets, on constant, walking, jumping and off-matrix paths, whole-strand and with a range per read; on
  constant paths it also equals nvk_seed_extend_dev itself;
* results do not change when the traceback store runs in chunks;
* ``SeedAligner(chain=1)`` equals the CPU pipeline array for array, over one reference and over a ReferenceSet;
* ``align_signal_batch`` with the chained aligner covers drifting reads that a fixed band of 16 loses;
* the C-ABI's argument checks."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_seed_align import _concat
from test_seed_align_cpu import _batch, host_extend  # noqa: F401  (fixture)
from test_seed_chain_cpu import cpu_chain_pipeline, drifting_reads, host_chain, strips_of  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def _dev(a):
    import torch
    from nadavca_amd import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', _lib.default_context().device))


@pytest.fixture(scope='module')
def mixed():
    """332 reads on a 30 000-base reference that holds two tiled repeats (one unit 30 times over: under the default
    max_occ of 32, so each of its k-mers seeds 30 times; another 40 times over: above it): 300 of 0-1 500 bases at
    error rates 0-10 %, random and overhanging ones among them, 16 of 4 500-5 500 bases with more deletions than
    insertions, 8 of the lengths around the strip's 64, 8 out of the repeats."""
    from nadavca_amd import synthetic
    rng = np.random.default_rng(21)
    unit, unit2 = rng.integers(0, 4, 23), rng.integers(0, 4, 23)
    genome = np.concatenate([rng.integers(0, 4, 12000), np.tile(unit, 20), rng.integers(0, 4, 9000),
                             np.tile(unit, 10), rng.integers(0, 4, 4000), np.tile(unit2, 40),
                             rng.integers(0, 4, 3390)])
    assert genome.size == 30000
    parts = []
    for g, rate in enumerate((0.0, 0.01, 0.03, 0.06, 0.10)):
        rb, _, _ = synthetic.make_error_read_batch(60, genome, seed=100 + g, length=750, spread=750,
                                                   substitution_rate=rate, insertion_rate=rate / 4,
                                                   deletion_rate=rate, random_fraction=0.1, overhang_fraction=0.15)
        parts.append(rb)
    rb, _, _ = synthetic.make_error_read_batch(16, genome, seed=7, length=5000, spread=500, substitution_rate=0.03,
                                               insertion_rate=0.01, deletion_rate=0.05, overhang_fraction=0.2)
    parts.append(rb)
    rc = 3 - genome[::-1]
    parts.append(_batch([(rc if t % 2 else genome)[3000 + 200 * t:3000 + 200 * t + L]
                         for t, L in enumerate((0, 1, 13, 63, 64, 65, 128, 129))]))
    parts.append(_batch([(rc if t % 2 else genome)[x:x + 700] for t, x in
                         enumerate((11700, 11900, 12100, 12300, 21300, 21400, 25400, 26000))]))
    rb = _concat(parts)
    assert rb.n == 332
    return genome, rb


def _chain_both(host_chain, q_off, strand, seed_off, seed_i, seed_p, k, w, max_gap, lookback):  # noqa: F811
    """The kernel and the restatement on the same seeds: -> what differs (a message, or None)"""
    from nadavca_amd import _lib
    from nadavca_amd.device import seed_chain_dev
    strip_off = strips_of(q_off)
    fill = (np.arange(strip_off[-1]) % 1000 - 7000).astype(np.int32)
    centres = _dev(fill.copy())
    score, anchors = seed_chain_dev(_lib.default_context(), _dev(q_off), _dev(strand), _dev(seed_off), _dev(seed_i),
                                    _dev(seed_p), _dev(strip_off), centres, k, w, max_gap, lookback)
    exp, exp_centres = host_chain.chain(q_off, strand, seed_off, seed_i, seed_p, strip_off, fill, k, w, max_gap,
                                        lookback)
    got = np.stack([score.cpu().numpy(), anchors.cpu().numpy()], 1)
    bad = np.nonzero((got != exp).any(1))[0]
    if bad.size:
        return 'reads %s: got %s, expected %s' % (bad[:8], got[bad[:4]], exp[bad[:4]])
    bad = np.nonzero(centres.cpu().numpy() != exp_centres)[0]
    if bad.size:
        return 'strips %s of %d' % (bad[:8], exp_centres.size)
    return None, exp, exp_centres, fill


def test_chain_kernel_equals_restatement(mixed, host_chain):  # noqa: F811
    from nadavca_amd.seedalign import SeedAligner
    genome, rb = mixed
    seen_long = 0
    for cfg, lookback in ((dict(band=16), 64), (dict(band=64, k=11, max_gap=100), 64), (dict(band=4), 7)):
        al = SeedAligner(genome, chain=1, **cfg)
        p = al.params
        strand, _, _, rd, si, sp = al.strand_seeds(rb)
        seed_off, seed_i, seed_p = (x.cpu().numpy() for x in al.sort_seeds(rb.n, rd, si, sp))
        strand = strand.cpu().numpy()
        res = _chain_both(host_chain, rb.seq_off, strand, seed_off, seed_i, seed_p, p['k'], p['band'], p['max_gap'],
                          lookback)
        assert res[0] is None, (cfg, res)
        exp = res[1]
        per = np.diff(seed_off)
        lens = np.diff(rb.seq_off)
        assert ((strand >= 0) & (exp[:, 1] > 10)).sum() > rb.n // 3 and ((strand == 1) & (exp[:, 1] > 10)).any()
        assert per.max() > 4 * lens[per.argmax()]       # the repeat: several seeds per read position
        seen_long += int((exp[lens >= 4000, 1] > 300).sum())
    assert seen_long >= 16


@pytest.mark.parametrize('lookback', [64, 3])
def test_chain_kernel_on_constructed_seed_lists(host_chain, lookback):  # noqa: F811
    """0, 1, 63, 64, 65, 129 and 200 seeds on a drifting diagonal with equal-p and off-chain seeds among them, where
    the 64-lane ring and the 64-seed load blocks wrap; reads without a strand keep their strips."""
    rng = np.random.default_rng(4)
    counts = [0, 1, 63, 64, 65, 129, 200, 64, 128, 2]
    sets, ms = [], []
    for t, n in enumerate(counts):
        m = 64 * int(rng.integers(1, 9)) + int(rng.integers(0, 64)) * (t % 2)
        seeds = set()
        while len(seeds) < n:
            i = int(rng.integers(0, m))
            p = 300 + i + i // 40 + (int(rng.integers(-30, 30)) if rng.random() < 0.2 else 0)
            seeds.add((i, p))
        sets.append(sorted(seeds, key=lambda s: (s[1], s[0])))
        ms.append(m)
    q_off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    seed_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat = [x for s in sets for x in s]
    seed_i = np.array([x[0] for x in flat], dtype=np.int32)
    seed_p = np.array([x[1] for x in flat], dtype=np.int32)
    strand = np.array([0, 1, 0, 1, 0, 1, 0, -1, 2, 0], dtype=np.int32)
    for k, w, max_gap in ((14, 16, 500), (3, 2, 9), (16, 256, 1 << 26)):
        res = _chain_both(host_chain, q_off, strand, seed_off, seed_i, seed_p, k, w, max_gap, lookback)
        assert res[0] is None, (k, res)
        _, exp, centres, fill = res
        assert exp[0].tolist() == [0, 0] and exp[1].tolist() == [k, 1] and exp[7].tolist() == [0, 0]
        strip_off = strips_of(q_off)
        for j in (0, 7, 8):        # no seeds, no strand, a strand that is none: untouched
            assert np.array_equal(centres[strip_off[j]:strip_off[j + 1]], fill[strip_off[j]:strip_off[j + 1]])
        assert exp[6, 1] > 20 or w < 16


@pytest.fixture(scope='module')
def path_reads():
    """123 reads: 120 of 0-1 500 bases at error rates 0-6 % and 3 of 4 500-5 500, on a 30 000-base reference."""
    from nadavca_amd import synthetic
    genome = np.random.default_rng(22).integers(0, 4, 30000)
    parts = []
    for g, rate in enumerate((0.0, 0.03, 0.06)):
        rb, _, _ = synthetic.make_error_read_batch(40, genome, seed=200 + g, length=750, spread=750,
                                                   substitution_rate=rate, insertion_rate=rate / 4,
                                                   deletion_rate=rate, random_fraction=0.1, overhang_fraction=0.15)
        parts.append(rb)
    rb, _, _ = synthetic.make_error_read_batch(3, genome, seed=8, length=5000, spread=500, substitution_rate=0.03,
                                               insertion_rate=0.01, deletion_rate=0.05)
    parts.append(rb)
    return genome, _concat(parts)


SCORING = [dict(), dict(match=2, mismatch=4, gap_open=4, gap_extend=2, min_score=40)]


@pytest.mark.parametrize('scoring', SCORING, ids=['ont2d', 'm2x4o4e2'])
@pytest.mark.parametrize('band', [1, 8, 64, 256])
def test_path_extension_equals_restatement(path_reads, host_chain, band, scoring):  # noqa: F811
    from nadavca_amd import _lib
    from nadavca_amd.device import seed_extend_dev, seed_extend_path_dev
    from nadavca_amd.seedalign import SeedAligner
    genome, rb = path_reads
    G, w = genome.size, band
    al = SeedAligner(genome, band=band, **scoring)
    p = al.params
    sc = (p['band'], p['match'], p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'])
    strand, diag, _ = (x.cpu().numpy() for x in al.seed(rb))
    rng = np.random.default_rng(band)
    lens = np.diff(rb.seq_off)
    free = strand < 0      # the reads the seeds left alone get a random strand and diagonal (some stay skipped)
    strand = np.where(free & (rng.random(rb.n) < 0.7), rng.integers(0, 2, rb.n), strand).astype(np.int32)
    diag = np.where(free, rng.integers(-lens - 300, G + 300), diag).astype(np.int64)
    strip_off = strips_of(rb.seq_off)
    kind = np.arange(rb.n) % 4        # 0: constant, 1: a walk, 2: jumps, 3: off the matrix
    kind[-3:] = (1, 2, 0)             # (the long reads)
    centres = np.zeros(strip_off[-1], dtype=np.int64)
    for j in range(rb.n):
        n = int(strip_off[j + 1] - strip_off[j])
        if kind[j] == 0:
            c = np.full(n, diag[j])
        elif kind[j] == 1:     # steps within +-w, on top of the drift the deletions cause
            c = diag[j] + np.cumsum(rng.integers(-w, w + 1, n))
        elif kind[j] == 2:     # now and then a jump of more than 2w + 1, either way: no cell connects the strips
            jump = rng.choice([-1, 1], n) * rng.integers(2 * w + 2, 2 * w + 40, n)
            c = diag[j] + np.cumsum(np.where(rng.random(n) < 0.4, jump, 0))
        else:
            c = rng.choice([-lens[j] - w - 50, G + w + 50, diag[j], diag[j] + 1, INT_MIN, INT_MAX, INT_MIN + w], n)
        centres[strip_off[j]:strip_off[j + 1]] = np.clip(c, INT_MIN, INT_MAX)
    centres = centres.astype(np.int32)
    # a range per read, in strand coordinates: around where the read lies, some empty, some the whole strand
    lo = np.clip(diag + rng.integers(-100, 200, rb.n), 0, G)
    hi = np.clip(lo + rng.integers(0, 2, rb.n) * rng.integers(0, lens + 300), lo, G)
    whole = rng.random(rb.n) < 0.2
    lo, hi = np.where(whole, 0, lo).astype(np.int32), np.where(whole, G, hi).astype(np.int32)
    ctx = _lib.default_context()
    dev_args = (_dev(rb.sequence), _dev(rb.seq_off), _dev(genome.astype(np.int32)), _dev(strand))
    n_pairs = 0
    for ref_lo, ref_hi in ((None, None), (lo, hi)):
        bounds = () if ref_lo is None else (_dev(ref_lo), _dev(ref_hi))
        score, end, count, pairs = seed_extend_path_dev(ctx, *dev_args, _dev(strip_off), _dev(centres), *sc, *bounds)
        hit, exp_pairs = host_chain.extend(rb.sequence, rb.seq_off, genome, strand, strip_off, centres, *sc,
                                           ref_lo=ref_lo, ref_hi=ref_hi)
        got = np.stack([score.cpu().numpy(), end[:, 0].cpu().numpy(), end[:, 1].cpu().numpy(),
                        count.cpu().numpy()], 1)
        bad = np.nonzero((got != hit).any(1))[0]
        assert bad.size == 0, (ref_lo is None, bad[:10], kind[bad[:10]], got[bad[:5]], hit[bad[:5]])
        pairs = pairs.cpu().numpy()
        for j in range(rb.n):
            assert np.array_equal(pairs[rb.seq_off[j]:rb.seq_off[j] + hit[j, 3]], exp_pairs[j]), (j, kind[j])
        n_pairs += int(hit[:, 3].sum())
        for k in range(3):
            assert (hit[kind == k, 3] > 0).any() or band == 1, k
        # a constant path is the fixed band: what nvk_seed_extend_dev itself returns for these reads
        score, end, count, fixed = seed_extend_dev(ctx, *dev_args, _dev(diag), *sc, *bounds)
        fixed = fixed.cpu().numpy()
        same = np.stack([score.cpu().numpy(), end[:, 0].cpu().numpy(), end[:, 1].cpu().numpy(),
                         count.cpu().numpy()], 1)
        const = np.nonzero(kind == 0)[0]
        assert np.array_equal(same[const], hit[const])
        for j in const:
            assert np.array_equal(fixed[rb.seq_off[j]:rb.seq_off[j] + hit[j, 3]], exp_pairs[j]), j
    assert n_pairs > 1000


def _same_hits(got, ref):
    for f in ('strand', 'diagonal', 'votes', 'score', 'end', 'off', 'read_idx', 'ref_idx', 'reverse', 'contig',
              'chain_score', 'chain_anchors', 'strip_off', 'strip_diagonal'):
        assert np.array_equal(getattr(got, f), getattr(ref, f)), f


def test_chunked_store_gives_the_same_results(mixed):
    from nadavca_amd import _lib
    from nadavca_amd.seedalign import SeedAligner
    genome, rb = mixed
    al = SeedAligner(genome, chain=1, band=64)
    ctx = _lib.default_context()
    ref = al.align(rb)
    assert ref.aligned.sum() > rb.n // 2
    ctx.set_workspace_limit(1 << 20)     # ~15 reads of 1 000 bases per chunk; a long read runs on its own
    try:
        got = al.align(rb)
    finally:
        ctx.set_workspace_limit(0)
    _same_hits(got, ref)


@pytest.mark.parametrize('contigs', [1, 3])
def test_chained_aligner_equals_the_cpu_pipeline(host_chain, contigs):  # noqa: F811
    from nadavca_amd.refset import ReferenceSet
    from nadavca_amd.seedalign import SeedAligner
    genome, rb, truth, _ = drifting_reads()
    ref = genome
    if contigs == 3:
        ref = ReferenceSet.from_arrays(['a', 'b', 'c'], [genome[:7000], genome[7000:12500], genome[12500:]])
    al = SeedAligner(ref, chain=1, band=16)
    hits = al.align(rb)
    exp = cpu_chain_pipeline(SeedAligner(ref, device='cpu', chain=1, band=16), rb, host_chain)
    read_idx, ref_idx, off, reverse, strand, hit, chain, strip_off, centres = exp
    ba = al.get_base_alignments(rb)
    for g, e in zip((ba.read_idx, ba.ref_idx, ba.off, ba.reverse), exp[:4]):
        assert g.dtype == e.dtype and np.array_equal(g, e)
    assert np.array_equal(hits.strand, strand) and np.array_equal(hits.score, hit[:, 0])
    assert np.array_equal(hits.end, hit[:, 1:3])
    assert np.array_equal(hits.chain_score, chain[:, 0]) and np.array_equal(hits.chain_anchors, chain[:, 1])
    assert np.array_equal(hits.strip_off, strip_off) and np.array_equal(hits.strip_diagonal, centres)
    assert hits.aligned.all() and (contigs == 3 or (chain[:, 1] > 300).all())
    if contigs == 3:
        assert len(set(hits.contig.tolist())) >= 2 and np.array_equal(ba.contig, hits.contig)
    else:
        # the reads lie whole inside the reference: nearly all true pairs come back (measured on the CPU: 0.973 ..
        # 0.982 of each read's; tests/test_seed_chain_cpu.py asserts it against the fixed band of 256)
        true = set(zip(np.repeat(np.arange(rb.n), np.diff(truth.off)).tolist(), truth.read_idx.tolist(),
                       truth.ref_idx.tolist()))
        got = zip(np.repeat(np.arange(rb.n), np.diff(off)).tolist(), read_idx.tolist(), ref_idx.tolist())
        assert sum(g in true for g in got) > 0.95 * len(true)
    # with chain=0 the hits carry none of the chain's fields
    plain = SeedAligner(ref, band=16).align(rb)
    assert plain.chain_score is None and plain.chain_anchors is None and plain.strip_off is None
    assert plain.strip_diagonal is None


def test_edge_cases():
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.seedalign import SeedAligner
    genome = np.random.default_rng(3).integers(0, 4, 2000)
    z = np.zeros(1, dtype=np.int64)
    empty = ReadBatch(np.zeros(0, np.int16), z, np.zeros(0, np.int32), z, np.zeros(0), np.zeros(0), z)
    hits = SeedAligner(genome, chain=1).align(empty)
    assert hits.n == 0 and hits.off.tolist() == [0] and hits.read_idx.size == 0
    assert hits.chain_score.size == 0 and hits.strip_off.tolist() == [0] and hits.strip_diagonal.size == 0
    rb, _, _ = synthetic.make_error_read_batch(6, genome, seed=1, length=0, spread=0)
    hits = SeedAligner(genome, chain=1).align(rb)
    assert (hits.strand == -1).all() and hits.off[-1] == 0 and hits.strip_off.tolist() == [0] * 7
    rb, _, _ = synthetic.make_error_read_batch(6, genome, seed=1, length=300, spread=0)
    for ref in (genome[:13], genome[:0]):      # nothing seeds: no strand, no chain, the strips keep d* = 0
        hits = SeedAligner(ref, chain=1).align(rb)
        assert (hits.strand == -1).all() and (hits.score == 0).all() and hits.off[-1] == 0
        assert (hits.chain_score == 0).all() and (hits.chain_anchors == 0).all() and (hits.strip_diagonal == 0).all()
    hits, plain = SeedAligner(genome, chain=1).align(rb), SeedAligner(genome).align(rb)
    assert hits.aligned.all() and (hits.chain_anchors > 50).all()
    for f in ('strand', 'diagonal', 'votes', 'score', 'end', 'off', 'read_idx', 'ref_idx'):   # error-free reads
        assert np.array_equal(getattr(hits, f), getattr(plain, f)), f
    # max_gap 1: only seeds one base apart chain, which error-free reads have all along
    assert (SeedAligner(genome, chain=1, max_gap=1).align(rb).chain_anchors > 50).all()


def test_align_signal_batch_covers_drifting_reads():
    from nadavca_amd import defaults, synthetic
    from nadavca_amd.align_signal import align_signal_batch
    from nadavca_amd.kmer_model import KmerModel
    from nadavca_amd.seedalign import SeedAligner
    km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
    genome, rb, truth, info = drifting_reads(n=8, model=synthetic.load_model_arrays())
    G = genome.size
    cover = {}
    for name, cfg in (('chain', dict(chain=1, band=16)), ('fixed', dict(chain=0, band=16))):
        a = align_signal_batch(None, copy.deepcopy(rb), kmer_model=km, aligner=SeedAligner(genome, **cfg))
        share = np.zeros(rb.n)
        for x, j in enumerate(a.live):
            rows = a.alignment_of(x)
            if rows is None:
                continue
            t = truth.ref_idx[truth.off[j]:truth.off[j + 1]]
            t = G - 1 - t if info['reverse'][j] else t          # forward positions, as the rows'
            b0, b1 = int(t.min()), int(t.max())
            a0, a1 = int(rows[:, 0].min()), int(rows[:, 0].max())
            share[j] = max(0, min(a1, b1) - max(a0, b0) + 1) / (b1 - b0 + 1)
        cover[name] = (a.n_aligned, share)
        print(name, 'aligned', a.n_aligned, 'of', rb.n, 'share of the true span', np.round(share, 3))
    assert cover['chain'][0] == rb.n and (cover['chain'][1] >= 0.9).all(), cover['chain']
    assert not (cover['fixed'][1] >= 0.9).all(), cover['fixed']      # (the test can see the difference)


def test_c_abi_rejects_bad_arguments():
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    ctx = _lib.default_context()
    dev = torch.device('cuda', ctx.device)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    q = torch.zeros(140, dtype=torch.int32, device=dev)
    off = i64([0, 10, 140])
    ref = torch.zeros(300, dtype=torch.int32, device=dev)
    st = i32([0, 0])
    soff, si, sp = i64([0, 1, 3]), i32([2, 5, 70]), i32([40, 30, 95])
    toff, td = i64([0, 1, 4]), i32([0, 0, 0, 0])
    hit = torch.zeros(8, dtype=torch.int32, device=dev)
    pairs = torch.zeros(280, dtype=torch.int32, device=dev)
    out = torch.zeros(4, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def chain(c=None, off_=off, st_=st, soff_=soff, si_=si, sp_=sp, toff_=toff, td_=td, out_=out, total=140,
              n_seeds=3, n_strips=4, k=14, w=16, max_gap=500, lookback=64):
        return lib.nvk_seed_chain_dev(ctx.handle if c is None else c, 2, total, p(off_), p(st_), n_seeds, p(soff_),
                                      p(si_), p(sp_), k, w, max_gap, lookback, n_strips, p(toff_), p(td_), p(out_))

    def extend(c=None, q_=q, off_=off, ref_=ref, st_=st, toff_=toff, td_=td, lo_=None, hi_=None, hit_=hit,
               pairs_=pairs, total=140, n_strips=4, w=8, sc=(1, 1, 1, 1, 30)):
        return lib.nvk_seed_extend_path_dev(ctx.handle if c is None else c, 2, total, p(q_), p(off_), p(ref_), 300,
                                            p(st_), n_strips, p(toff_), p(td_), p(lo_), p(hi_), w, *sc, p(hit_),
                                            p(pairs_))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert chain() == _lib.NVK_OK
    assert out.cpu().tolist() == [14, 1, 28, 2] and td.cpu().tolist() == [38, 25, 25, 25]
    assert extend() == _lib.NVK_OK
    assert extend(lo_=i32([0, 0]), hi_=i32([300, 300])) == _lib.NVK_OK
    for call in (chain, extend):
        assert call(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
        assert invalid(call(off_=None)) and invalid(call(st_=None)) and invalid(call(toff_=None))
        assert invalid(call(td_=None))
        assert invalid(call(off_=i64([0, 141, 140]))) and invalid(call(off_=i64([1, 10, 140])))
        assert invalid(call(total=139))
        assert invalid(call(toff_=i64([1, 2, 4])))            # does not start at 0
        assert invalid(call(toff_=i64([0, 5, 4])))            # decreases
        assert invalid(call(n_strips=5))                      # does not end at the total
        assert invalid(call(toff_=i64([0, 2, 4])))            # not ceil(m / 64) strips per read
        assert invalid(call(w=0))
        assert call(w=257) == _lib.NVK_ERR_UNSUPPORTED
    for kw in (dict(soff_=None), dict(si_=None), dict(sp_=None), dict(out_=None), dict(lookback=0), dict(lookback=65),
               dict(max_gap=0), dict(k=0), dict(k=17), dict(n_seeds=2), dict(soff_=i64([0, 2, 1])),
               dict(soff_=i64([1, 1, 3]))):
        assert invalid(chain(**kw)), kw
    for kw in (dict(q_=None), dict(ref_=None), dict(hit_=None), dict(pairs_=None), dict(lo_=i32([0, 0])),
               dict(hi_=i32([300, 300])), dict(lo_=i32([0, 5]), hi_=i32([300, 4])),
               dict(lo_=i32([0, 0]), hi_=i32([300, 301]))):
        assert invalid(extend(**kw)), kw
    for sc in ((0, 1, 1, 1, 30), (1, 17, 1, 1, 30), (1, 1, 0, 1, 30), (1, 1, 1, 17, 30), (1, 1, 1, 1, 0)):
        assert invalid(extend(sc=sc)), sc
    assert chain() == _lib.NVK_OK and extend() == _lib.NVK_OK
