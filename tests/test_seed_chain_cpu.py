"""The chained mode of the seed aligner (``SeedAligner(chain=1)``) without a GPU:

* the CPU restatement of the chaining stage (tests/host_shims/seedchain_host.cpp: seedchain_host, which the kernel is
  held to in tests/test_gpu_seed_chain.py) against a plain-Python DP over all earlier seeds, and held to a window;
* the restatement of the extension along a path (seedext_path_host) against seedext_host.cpp on constant paths, against
  the brute-force full-matrix alignment where every row's band covers the matrix, and against a plain-Python banded
  alignment with a band per row on walking and jumping paths;
* seeding on the CPU + the two restatements on reads whose diagonal drifts: a band of 16 that follows the chain
  returns what a fixed band of 256 returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_seed_align_cpu import NEG, brute_force, cpu_pipeline, host_extend  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ChainHost:
    """The two restatements of tests/host_shims/seedchain_host.cpp on numpy arrays."""

    def __init__(self, lib):
        self._chain = lib.seedchain_host
        self._chain.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p] * 3
        self._chain.restype = None
        self._ext = lib.seedext_path_host
        self._ext.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 \
            + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
        self._ext.restype = None

    def chain(self, q_off, strand, seed_off, seed_i, seed_p, strip_off, strip_diag, k, w, max_gap, lookback=64):
        """-> (out (n, 2): chain score, anchors; the strip centres: a copy of ``strip_diag`` with the chains' in)"""
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        q_off, seed_off, strip_off = a(q_off, np.int64), a(seed_off, np.int64), a(strip_off, np.int64)
        strand, seed_i, seed_p = a(strand, np.int32), a(seed_i, np.int32), a(seed_p, np.int32)
        centres = np.array(strip_diag, dtype=np.int32)
        n = q_off.size - 1
        out = np.zeros((n, 2), dtype=np.int32)
        p = lambda x: x.ctypes.data
        self._chain(n, p(q_off), p(strand), p(seed_off), p(seed_i), p(seed_p), k, w, max_gap, lookback, p(strip_off),
                    p(centres), p(out))
        return out, centres

    def extend(self, query, q_off, ref, strand, strip_off, strip_diag, w, match=1, mismatch=1, gap_open=1,
               gap_extend=1, min_score=30, ref_lo=None, ref_hi=None):
        """-> (hit (n, 4): score, end i, end j, count; pairs list of (k, 2) arrays)"""
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        query, q_off, ref = a(query, np.int32), a(q_off, np.int64), a(ref, np.int32)
        strand, strip_off, strip_diag = a(strand, np.int32), a(strip_off, np.int64), a(strip_diag, np.int32)
        n = q_off.size - 1
        hit = np.zeros((n, 4), dtype=np.int32)
        pairs = np.zeros((max(int(q_off[-1]), 1), 2), dtype=np.int32)
        p = lambda x: x.ctypes.data
        lo = hi = None
        if ref_lo is not None:
            ref_lo, ref_hi = a(ref_lo, np.int32), a(ref_hi, np.int32)
            lo, hi = p(ref_lo), p(ref_hi)
        self._ext(n, p(query), p(q_off), p(ref), ref.size, p(strand), p(strip_off), p(strip_diag), lo, hi, w, match,
                  mismatch, gap_open, gap_extend, min_score, p(hit), p(pairs))
        return hit, [pairs[q_off[j]:q_off[j] + hit[j, 3]] for j in range(n)]


@pytest.fixture(scope='module')
def host_chain(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('seedchain') / 'seedchain_host.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC',
                    os.path.join(ROOT, 'tests', 'host_shims', 'seedchain_host.cpp'), '-o', so], check=True)
    return ChainHost(C.CDLL(so))


def strips_of(q_off):
    """-> strip_off: the running sum of ceil(m / 64)"""
    return np.concatenate([[0], np.cumsum((np.diff(q_off) + 63) // 64)]).astype(np.int64)


def python_chain(seeds, m, k, w, max_gap, lookback):
    """The rules of nvk_seed_chain_dev (include/nadavca_hip.h) for one read, plain Python, every earlier seed of the
    window tried.  ``seeds``: (i, p) sorted by (p, i).  -> (score, anchors (seed numbers), centres per strip or None)"""
    if not seeds:
        return 0, [], None
    f, pred = [], []
    for t, (it, pt) in enumerate(seeds):
        best, arg = k, -1
        for u in range(max(0, t - lookback), t):
            di, dp = it - seeds[u][0], pt - seeds[u][1]
            if 0 < di <= max_gap and 0 < dp <= max_gap and abs(dp - di) <= w:
                cand = f[u] + min(di, dp, k) - abs(dp - di)
                if cand > k and cand >= best:
                    best, arg = cand, u
        f.append(best)
        pred.append(arg)
    end = f.index(max(f))
    anchors = []
    t = end
    while t >= 0:
        anchors.append(t)
        t = pred[t]
    anchors.reverse()
    centres = []
    for s in range((m + 63) // 64):
        i, t = min((abs(seeds[t][0] - (64 * s + 32)), seeds[t][0], t) for t in anchors)[1:]
        centres.append(seeds[t][1] - i)
    return f[end], anchors, centres


def random_seed_sets(rng, n_sets, max_seeds):
    """Small reads with seed sets full of equal p, equal diagonals and equal scores."""
    sets = []
    for t in range(n_sets):
        m = int(rng.integers(1, 400))
        n = int(rng.integers(0, max_seeds + 1)) if t % 7 else 0
        kind = t % 4
        if kind == 0:      # anywhere: few chain
            i, p = rng.integers(0, m, n), rng.integers(0, 500, n)
        elif kind == 1:    # a few diagonals, many seeds on each: equal diagonals, ties between predecessors
            d = rng.integers(0, 40, 3)
            i = rng.integers(0, m, n)
            p = i + d[rng.integers(0, 3, n)]
        elif kind == 2:    # a drifting diagonal with noise, and repeats: the same i at several p
            i = np.sort(rng.integers(0, m, n))
            p = i + 50 + np.cumsum(rng.integers(0, 2, n)) + rng.integers(-2, 3, n)
            rep = rng.random(n) < 0.3
            p = np.where(rep, p + 7 * rng.integers(1, 4, n), p)
        else:              # a grid: every (i, p) a multiple of 3, ties everywhere
            i, p = 3 * rng.integers(0, m // 3 + 1, n), 3 * rng.integers(0, 60, n)
            i = np.minimum(i, m - 1)
        seeds = sorted(set(zip(np.asarray(i).tolist(), np.asarray(p).tolist())), key=lambda s: (s[1], s[0]))
        sets.append((m, seeds))
    return sets


def run_chain_sets(host_chain, sets, k, w, max_gap, lookback, strand=None):
    q_off = np.concatenate([[0], np.cumsum([m for m, _ in sets])]).astype(np.int64)
    seed_off = np.concatenate([[0], np.cumsum([len(s) for _, s in sets])]).astype(np.int64)
    flat = [x for _, s in sets for x in s]
    seed_i = np.array([x[0] for x in flat], dtype=np.int32)
    seed_p = np.array([x[1] for x in flat], dtype=np.int32)
    strip_off = strips_of(q_off)
    fill = np.arange(strip_off[-1], dtype=np.int32) - 12345     # what a read without a chain keeps
    strand = np.zeros(len(sets), np.int32) if strand is None else strand
    out, centres = host_chain.chain(q_off, strand, seed_off, seed_i, seed_p, strip_off, fill, k, w, max_gap, lookback)
    return out, centres, strip_off, fill


@pytest.mark.parametrize('lookback', [64, 5, 1])
def test_chain_restatement_equals_plain_python(host_chain, lookback):
    rng = np.random.default_rng(17)
    sets = random_seed_sets(rng, 160, 60 if lookback == 64 else 40)
    assert max(len(s) for _, s in sets) <= 64    # lookback 64: every earlier seed is inside the window
    strand = np.where(np.arange(len(sets)) % 11 == 10, -1, np.arange(len(sets)) % 2).astype(np.int32)
    chained = windowed = 0
    for k, w, max_gap in ((5, 4, 50), (14, 16, 500), (3, 1, 7)):
        out, centres, strip_off, fill = run_chain_sets(host_chain, sets, k, w, max_gap, lookback, strand)
        for j, (m, seeds) in enumerate(sets):
            score, anchors, exp = python_chain(seeds if strand[j] >= 0 else [], m, k, w, max_gap, lookback)
            assert (out[j, 0], out[j, 1]) == (score, len(anchors)), (k, j)
            got = centres[strip_off[j]:strip_off[j + 1]]
            assert np.array_equal(got, exp if exp is not None else fill[strip_off[j]:strip_off[j + 1]]), (k, j)
            chained += len(anchors) > 3
            if lookback < 64 and seeds and strand[j] >= 0:
                windowed += python_chain(seeds, m, k, w, max_gap, 64)[0] != score
    assert chained > 50
    assert lookback == 64 or windowed > 10     # (the window does cost some chains their best predecessor)


def banded(q, r, centres, w, match, mismatch, gap_open, gap_extend):
    """The rules of nvk_seed_extend_path_dev, plain Python over dicts of cells: row i's band is centred on
    centres[i // 64].  -> (score, end (i, j), pairs)"""
    m, G = len(q), len(r)
    O, X = gap_open + gap_extend, gap_extend
    cell = lambda i, j: 0 <= i < m and 0 <= j < G and abs(j - i - centres[i // 64]) <= w
    H, E, F, src, ee, fe = {}, {}, {}, {}, {}, {}
    best = (-1, -1, -1)
    for i in range(m):
        d = centres[i // 64]
        for j in range(max(0, i + d - w), min(G - 1, i + d + w) + 1):
            dg = (H[i - 1, j - 1] if cell(i - 1, j - 1) else 0) + (match if q[i] == r[j] else -mismatch)
            e = f = NEG
            ee[i, j] = fe[i, j] = False
            if cell(i, j - 1):
                e = max(H[i, j - 1] - O, E[i, j - 1] - X)
                ee[i, j] = E[i, j - 1] - X > H[i, j - 1] - O
            if cell(i - 1, j):
                f = max(H[i - 1, j] - O, F[i - 1, j] - X)
                fe[i, j] = F[i - 1, j] - X > H[i - 1, j] - O
            E[i, j], F[i, j] = e, f
            b = max(dg, e, f)
            H[i, j] = max(b, 0)
            src[i, j] = 0 if b <= 0 else 1 if dg == b else 2 if e == b else 3
            if H[i, j] > best[0]:
                best = (H[i, j], i, j)
    score, i, j = best
    if score < 0:
        return 0, (-1, -1), []
    pairs, state = [], 'H'
    while cell(i, j):
        if state == 'H':
            s = src[i, j]
            if s == 0:
                break
            if s == 1:
                if q[i] == r[j]:
                    pairs.append((i, j))
                if i == 0 or j == 0:
                    break
                i, j = i - 1, j - 1
            else:
                state = 'E' if s == 2 else 'F'
        elif state == 'E':
            ext = ee[i, j]
            j -= 1
            state = 'E' if ext else 'H'
        else:
            ext = fe[i, j]
            i -= 1
            state = 'F' if ext else 'H'
    return score, (best[1], best[2]), pairs[::-1]


def test_constant_path_equals_the_fixed_band_restatement(host_extend, host_chain):  # noqa: F811
    """The random cases of test_seed_align_cpu.test_restatement_equals_brute_force (the same generator and seed), and
    longer reads of several strips."""
    rng = np.random.default_rng(5)
    for trial in range(460):
        G = int(rng.integers(1, 28))
        m = int(rng.integers(1, 24))
        if trial >= 400:
            G, m = int(rng.integers(100, 400)), int(rng.integers(65, 300))
        ref = rng.integers(0, 4, G)
        st = int(rng.integers(0, 2))
        r = 3 - ref[::-1] if st else ref
        if trial % 3 == 0:
            x = int(rng.integers(0, G))
            q = np.array(list(r[x:x + m]) or [0])
            q = np.array([b if rng.random() > 0.2 else int(rng.integers(0, 4)) for b in q])
            q = np.delete(q, rng.integers(0, q.size, int(rng.integers(0, 3)))) if q.size > 3 else q
            m = q.size
        else:
            q = rng.integers(0, 4, m)
        sc = [(1, 1, 1, 1), (2, 3, 2, 1), (1, 2, 3, 1), (3, 1, 1, 2)][trial % 4]
        if trial % 2 == 0:
            w = int(rng.integers(1, 40))
            d = int(rng.integers(G - 1 - w, w - (m - 1) + 1)) if G - 1 - w <= w - (m - 1) else None
            if d is None:
                w, d = m + G, 0
        else:
            w = int(rng.integers(1, 4))
            d = int(rng.integers(-m, G))
        hit, pairs = host_extend(q, [0, m], ref, [st], [d], w, *sc, min_score=1)
        n_strips = (m + 63) // 64
        got, got_pairs = host_chain.extend(q, [0, m], ref, [st], [0, n_strips], [d] * n_strips, w, *sc, min_score=1)
        assert np.array_equal(got, hit), (trial, got, hit)
        assert np.array_equal(got_pairs[0], pairs[0]), trial
        # and with the read's range given as the whole strand
        got, got_pairs = host_chain.extend(q, [0, m], ref, [st], [0, n_strips], [d] * n_strips, w, *sc, min_score=1,
                                           ref_lo=[0], ref_hi=[G])
        assert np.array_equal(got, hit) and np.array_equal(got_pairs[0], pairs[0]), trial


def test_a_band_over_the_whole_matrix_equals_brute_force_on_any_path(host_chain):
    rng = np.random.default_rng(6)
    for trial in range(60):
        G, m = int(rng.integers(1, 120)), int(rng.integers(1, 200))
        ref = rng.integers(0, 4, G)
        st = int(rng.integers(0, 2))
        r = 3 - ref[::-1] if st else ref
        if trial % 2:
            x = int(rng.integers(0, G))
            q = np.array([b if rng.random() > 0.15 else int(rng.integers(0, 4)) for b in np.resize(r[x:], m)])
        else:
            q = rng.integers(0, 4, m)
        sc = [(1, 1, 1, 1), (2, 3, 2, 1), (1, 2, 3, 1), (3, 1, 1, 2)][trial % 4]
        exp = brute_force(list(q), list(r), *sc)
        n_strips = (m + 63) // 64
        w = m + G + 30
        centres = rng.integers(-30, 31, n_strips)      # every row's band still holds -(m-1) .. G-1
        hit, pairs = host_chain.extend(q, [0, m], ref, [st], [0, n_strips], centres, w, *sc, min_score=1)
        assert (hit[0, 0], (hit[0, 1], hit[0, 2])) == (exp[0], exp[1]), (trial, hit, exp)
        if exp[0] >= 1:
            assert [tuple(p) for p in pairs[0]] == exp[2], trial


def test_path_restatement_equals_plain_python_on_walks_and_jumps(host_chain):
    rng = np.random.default_rng(7)
    cut = 0
    for trial in range(80):
        G, m = int(rng.integers(150, 400)), int(rng.integers(65, 330))
        ref = rng.integers(0, 4, G)
        st = int(rng.integers(0, 2))
        r = 3 - ref[::-1] if st else ref
        x = int(rng.integers(0, G // 3))
        q = np.array([b if rng.random() > 0.1 else int(rng.integers(0, 4)) for b in np.resize(r[x:], m + 20)])
        q = np.delete(q, rng.integers(0, q.size, 20))     # deletions: the true diagonal drifts
        m = q.size
        n_strips = (m + 63) // 64
        w = int(rng.integers(1, 7))
        kind = trial % 4
        if kind == 0:      # a walk: steps within +-w
            centres = x + np.cumsum(rng.integers(-w, w + 1, n_strips))
        elif kind == 1:    # a walk after the drift: about 4 per strip
            centres = x + 4 * np.arange(n_strips) + rng.integers(-1, 2, n_strips)
        elif kind == 2:    # jumps of more than 2w + 1: no cell connects the strips
            centres = x + np.cumsum(rng.choice([-1, 1], n_strips) * rng.integers(2 * w + 2, 40, n_strips))
        else:              # partly or wholly off the matrix
            centres = rng.choice([-m - 50, G + 50, x, x + 3, -(1 << 31), (1 << 31) - 1], n_strips)
        sc = [(1, 1, 1, 1), (2, 3, 2, 1), (1, 2, 3, 1), (3, 1, 1, 2)][trial % 4]
        exp = banded(list(q), list(r), [int(c) for c in centres], w, *sc)
        hit, pairs = host_chain.extend(q, [0, m], ref, [st], [0, n_strips], centres, w, *sc, min_score=1)
        assert (hit[0, 0], (hit[0, 1], hit[0, 2])) == (exp[0], exp[1]), (trial, hit, exp)
        assert [tuple(p) for p in pairs[0]] == (exp[2] if exp[0] >= 1 else []), trial
        cut += kind == 2 and exp[0] < brute_force(list(q), list(r), *sc)[0]
    assert cut > 5


def cpu_chain_pipeline(aligner, rb, host_chain):
    """``SeedAligner.align`` with chain=1 on the CPU: seeding, the strand's seeds and their sort by the aligner's torch
    code, the chain and the extension along it by the two restatements.  -> (read_idx, ref_idx, off, reverse, strand,
    hit, chain (n, 2), strip_off, centres), ``ref_idx`` contig-local for an aligner over a ReferenceSet."""
    import torch
    p = aligner.params
    strand, diag, _, seed_read, seed_i, seed_p = aligner.strand_seeds(rb)
    seed_off, seed_i, seed_p = (x.numpy() for x in aligner.sort_seeds(rb.n, seed_read, seed_i, seed_p))
    ref_lo = ref_hi = None
    if aligner.reference_set is not None:
        _, ref_lo, ref_hi = (x.numpy() for x in aligner.contig_of(rb, strand, diag))
    strand, diag = strand.numpy(), diag.numpy()
    strip_off = strips_of(rb.seq_off)
    fill = np.repeat(diag.astype(np.int32), np.diff(strip_off))
    chain, centres = host_chain.chain(rb.seq_off, strand, seed_off, seed_i, seed_p, strip_off, fill, p['k'], p['band'],
                                      p['max_gap'])
    hit, pairs = host_chain.extend(rb.sequence, rb.seq_off, aligner.reference_num, strand, strip_off, centres,
                                   p['band'], p['match'], p['mismatch'], p['gap_open'], p['gap_extend'],
                                   p['min_score'], ref_lo, ref_hi)
    off = np.concatenate([[0], np.cumsum(hit[:, 3])]).astype(np.int64)
    flat = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int32)
    ref_idx = flat[:, 1].astype(np.int64)
    if ref_lo is not None:
        ref_idx -= np.repeat(ref_lo.astype(np.int64), hit[:, 3])
    reverse = (strand == 1) & (hit[:, 0] >= p['min_score'])
    return flat[:, 0].astype(np.int32), ref_idx, off, reverse, strand, hit, chain, strip_off, centres


def drifting_reads(n=16, seed=9, model=None):
    """Reads that lose more bases than they gain: 3 000 +- 300 bases of a 20 000-base genome, substitutions 0.03,
    deletions 0.06, no insertions: the true diagonal drifts by about 180."""
    from nadavca_amd import synthetic
    genome = np.random.default_rng(8).integers(0, 4, 20000)
    rb, truth, info = synthetic.make_error_read_batch(n, genome, seed=seed, length=3000, spread=300,
                                                      substitution_rate=0.03, insertion_rate=0.0, deletion_rate=0.06,
                                                      model=model)
    return genome, rb, truth, info


def true_pairs(truth, read_idx, ref_idx, off):
    """-> per read (true pairs among those returned, true pairs there are)"""
    got, has = [], []
    for j in range(truth.off.size - 1):
        t = set(zip(truth.read_idx[truth.off[j]:truth.off[j + 1]].tolist(),
                    truth.ref_idx[truth.off[j]:truth.off[j + 1]].tolist()))
        g = zip(read_idx[off[j]:off[j + 1]].tolist(), ref_idx[off[j]:off[j + 1]].tolist())
        got.append(sum(x in t for x in g))
        has.append(len(t))
    return np.array(got), np.array(has)


def test_a_narrow_band_along_the_chain_recovers_drifting_reads(host_extend, host_chain):  # noqa: F811
    from nadavca_amd.seedalign import SeedAligner
    genome, rb, truth, _ = drifting_reads()
    share = {}
    for name, cfg in (('yardstick', dict(band=256)), ('fixed16', dict(band=16)), ('fixed64', dict(band=64))):
        out = cpu_pipeline(SeedAligner(genome, device='cpu', **cfg), rb, host_extend)
        share[name] = true_pairs(truth, *out[:3])
    out = cpu_chain_pipeline(SeedAligner(genome, device='cpu', chain=1, band=16), rb, host_chain)
    share['chain16'] = true_pairs(truth, *out[:3])
    has = share['yardstick'][1]
    rel = {k: v[0] / has for k, v in share.items()}
    for k, v in rel.items():
        print('%-10s share of true pairs: min %.4f median %.4f max %.4f, total %d of %d' % (
            k, v.min(), np.median(v), v.max(), share[k][0].sum(), has.sum()))
    chain, centres, strip_off = out[6], out[8], out[7]
    steps = max(int(np.abs(np.diff(centres[strip_off[j]:strip_off[j + 1]])).max()) for j in range(rb.n))
    print('chains of %d .. %d seeds; largest move of the centre between two strips: %d' % (
        chain[:, 1].min(), chain[:, 1].max(), steps))
    # the condition: read for read at least 0.9 of what the band that holds the whole drift returns
    assert (rel['chain16'] >= 0.9 * rel['yardstick']).all(), (rel['chain16'], rel['yardstick'])
    # neither fixed band comes near (which is what this test can see): measured medians 0.2313 and 0.6804
    assert (rel['fixed16'] < 0.5 * rel['yardstick']).all() and np.median(rel['fixed64']) < 0.9
    # the batch total.  Measured (seed 9): the yardstick returns 42 779 of the 43 777 true pairs and so does the chain
    # at band 16, read for read (shares 0.9730 .. 0.9821 both; fixed band 16: 9 831 pairs, fixed band 64: 29 179): a gap
    # of 0.  The margin is that gap plus one read's worth of pairs, 43 777 / 16 = 2 736
    gap = int(share['yardstick'][0].sum()) - int(share['chain16'][0].sum())
    assert gap <= 0 + int(has.sum()) // rb.n, gap
    # measured: chains of 681 .. 1 041 seeds, and the centre moves by at most 14 diagonals from one strip to the next,
    # inside the band's half-width
    assert steps <= 16


def test_chain_parameters_are_checked():
    from nadavca_amd.seedalign import PARAMS, SeedAligner
    ref = np.random.default_rng(0).integers(0, 4, 100)
    assert PARAMS['chain'] == 0 and PARAMS['max_gap'] == 500
    for bad in (dict(chain=2), dict(chain=-1), dict(chain=True), dict(chain=1.0), dict(max_gap=0),
                dict(max_gap=(1 << 26) + 1), dict(max_gap=2.5)):
        with pytest.raises(ValueError):
            SeedAligner(ref, device='cpu', **bad)
    al = SeedAligner(ref, device='cpu', chain=1, max_gap=1)
    assert al.params['chain'] == 1 and al.params['max_gap'] == 1


def test_strand_seeds_are_the_voted_strands_seeds():
    """``strand_seeds`` against the plain-Python seeding of test_seed_align_cpu, and ``seed`` unchanged beside it."""
    from nadavca_amd.seedalign import SeedAligner
    from test_seed_align_cpu import _batch
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 4, 600)
    rc = 3 - ref[::-1]
    reads = [ref[50:150], rc[200:320], rng.integers(0, 4, 80), ref[:5], np.concatenate([ref[300:340], ref[100:140]])]
    rb = _batch(reads)
    k = 9
    al = SeedAligner(ref, device='cpu', k=k, band=8)
    strand, diag, votes, rd, si, sp = al.strand_seeds(rb)
    s2, d2, v2 = al.seed(rb)
    assert np.array_equal(strand.numpy(), s2.numpy()) and np.array_equal(diag.numpy(), d2.numpy())
    assert np.array_equal(votes.numpy(), v2.numpy())
    seed_off, seed_i, seed_p = (x.numpy() for x in al.sort_seeds(rb.n, rd, si, sp))
    for j, read in enumerate(reads):
        exp = []
        if strand[j] >= 0:
            seq = rc if strand[j] == 1 else ref
            exp = sorted(((p, i) for i in range(len(read) - k + 1) for p in range(seq.size - k + 1)
                          if np.array_equal(read[i:i + k], seq[p:p + k])))
        got = list(zip(seed_p[seed_off[j]:seed_off[j + 1]].tolist(), seed_i[seed_off[j]:seed_off[j + 1]].tolist()))
        assert got == exp, j
    assert strand.tolist() == [0, 1, -1, -1, 0] and seed_off[-1] > 200


def test_both_entries_declared_bound_and_exported():
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail('the library is not built: %s' % _lib.LIB_PATH)
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in (('nvk_seed_chain_dev', 17), ('nvk_seed_extend_path_dev', 21)):
        m = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert m, '%s is not declared' % name
        params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == n_args
        for p, a in zip(params, args):
            want = C.c_void_p if '*' in p else C.c_int64 if p.startswith('int64_t') else C.c_int
            assert a is want, (name, p)
        assert hasattr(lib, name)
    # the two earlier entries keep their arguments
    assert len(_lib.SIGNATURES['nvk_seed_extend_dev'][1]) == 17
    assert len(_lib.SIGNATURES['nvk_seed_extend_bounded_dev'][1]) == 19
    assert callable(device.seed_chain_dev) and callable(device.seed_extend_path_dev)
    assert 'kernels_seedchain.hip' in open(os.path.join(ROOT, 'nadavca_amd', 'csrc', 'Makefile')).read()
