"""GPU tests of the rank-test kernel (csrc/kernels_siteranks.hip) through the C-ABI on constructed pile-ups: the six
integer outputs equal to the numpy restatement (tests/site_ranks_ref.py), the exact p-value equal bit for bit and NaN in
the same places, the same bits on a second call, the device layer around the kernel, and the invalid-argument
returns."""
import ctypes as C

import numpy as np
import pytest

import site_ranks_ref

pytestmark = pytest.mark.gpu

# (n_a, n_b): 64 and 65 are the lanes' edges of the element loop, 255 / 256 those of the recurrence's smaller sample
SHAPES = [(1, 1), (1, 64), (5, 5), (63, 65), (64, 64), (65, 130), (255, 64), (64, 255), (256, 3), (256, 256), (300, 40),
          (1000, 1500)]
KINDS = ['continuous', 'integers', 'equal', 'disjoint', 'inf']
NEVER = 1 << 40                                   # an exact_cells above every n m here


def values(kind, rng, n, m, t):
    if kind == 'continuous':
        return rng.normal(0.0, 1.0, n), rng.normal(0.4 * (t % 3), 1.0 + 0.5 * (t % 2), m)
    if kind == 'integers':
        return rng.integers(0, 6, n).astype(float), rng.integers(0, 6, m).astype(float)
    if kind == 'equal':
        return np.full(n, 1.25), np.full(m, 1.25)
    if kind == 'disjoint':
        lo, hi = rng.random(n), 2.0 + rng.random(m)
        return (lo, hi) if t % 2 == 0 else (lo + 5.0, hi)
    a, b = rng.normal(0.0, 1.0, n), rng.normal(0.0, 1.0, m)          # 'inf': +-inf and both zeros among them
    for x in (a, b):
        x[rng.random(x.size) < 0.15] = np.inf
        x[rng.random(x.size) < 0.15] = -np.inf
        x[rng.random(x.size) < 0.1] = 0.0
        x[rng.random(x.size) < 0.1] = -0.0
    return a, b


def build_case(kind, seed):
    """One input with every shape of SHAPES as a listed key 10 t + 3, unlisted keys 10 t + 5 between them (in A, in B
    or in both), and three more listed keys: 10 t + 7 with rows only in A (t = 0), only in B (t = 1), in neither
    (t = 2).  -> rows sorted by (key, value) per sample, the listed keys, and per listed key its (A, B)."""
    rng = np.random.default_rng(seed)
    rows = {'a': ([], []), 'b': ([], [])}
    listed, runs = [], {}

    def add(which, key, v):
        rows[which][0].append(np.full(v.size, key, dtype=np.int64))
        rows[which][1].append(np.asarray(v, dtype=np.float64))

    for t, (n, m) in enumerate(SHAPES):
        A, B = values(kind, rng, n, m, t)
        add('a', 10 * t + 3, A)
        add('b', 10 * t + 3, B)
        listed.append(10 * t + 3)
        runs[10 * t + 3] = (A, B)
        if t % 3 != 0:
            add('a', 10 * t + 5, rng.normal(0.0, 1.0, 1 + t))
        if t % 3 != 1:
            add('b', 10 * t + 5, rng.normal(0.0, 1.0, 2 + t))
    empty = np.zeros(0)
    extra = [rng.normal(0.0, 1.0, 6), rng.normal(0.0, 1.0, 9)]
    add('a', 7, extra[0])
    add('b', 17, extra[1])
    runs[7], runs[17], runs[27] = (extra[0], empty), (empty, extra[1]), (empty, empty)
    listed = sorted(listed + [7, 17, 27])
    out = {}
    for which, (k, v) in rows.items():
        k, v = np.concatenate(k), np.concatenate(v)
        order = np.lexsort((v, k))
        out[which] = (k[order], v[order])
    return out['a'], out['b'], np.array(listed, dtype=np.int64), runs


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def run_kernel(ctx, a, b, site_key, exact_cells):
    """nvk_site_rank_tests_dev on host arrays already sorted by (key, value): -> the seven outputs as numpy arrays."""
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    ka, va, kb, vb = up(a[0], np.int64), up(a[1], np.float64), up(b[0], np.int64), up(b[1], np.float64)
    sk = up(site_key, np.int64)
    n = int(sk.numel())
    ints = [torch.full((n,), -99, dtype=torch.int64, device=dev) for _ in range(6)]
    ks_p = torch.full((n,), -99.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.nvk_site_rank_tests_dev(ctx.handle, int(ka.numel()), p(ka), p(va), int(kb.numel()), p(kb), p(vb), n, p(sk),
                                     int(exact_cells), *[p(t) for t in ints], p(ks_p))
    assert rc == _lib.NVK_OK, lib.nvk_last_error()
    return [t.cpu().numpy() for t in ints] + [ks_p.cpu().numpy()]


def served(n, m, exact_cells):
    """The contract's rule for the exact p-value."""
    return n > 0 and m > 0 and min(n, m) <= 255 and n * m <= exact_cells


@pytest.mark.parametrize('kind', KINDS)
def test_every_shape_against_the_restatement(ctx, kind):
    a, b, site_key, runs = build_case(kind, 100 + KINDS.index(kind))
    # the restatement once per site, the exact p-value wherever the recurrence serves the shape at all
    want = [site_ranks_ref.one_site(*runs[int(q)], NEVER) for q in site_key]
    w_int = [np.array([w[i] for w in want], dtype=np.int64) for i in range(6)]
    w_p = np.array([w[6] for w in want])
    sizes = [(runs[int(q)][0].size, runs[int(q)][1].size) for q in site_key]
    assert sorted(s for s in sizes if s[0] and s[1]) == sorted(SHAPES)
    assert np.isnan(w_p[[sizes.index((256, 256)), sizes.index((1000, 1500))]]).all()
    assert not np.isnan(w_p[sizes.index((256, 3))]) and not np.isnan(w_p[sizes.index((64, 255))])
    if kind == 'equal':
        assert all(w[2] == 0 and w[3] == 0 and w[5] == (w[0] + w[1]) ** 3 - (w[0] + w[1]) for w in want if w[0] and w[1])
        assert set(w_p[~np.isnan(w_p)]) == {1.0}
    if kind == 'disjoint':
        assert all(max(w[2], w[3]) == w[0] * w[1] and w[4] in (0, 2 * w[0] * w[1]) for w in want if w[0] and w[1])
        assert w_p[sizes.index((5, 5))] == 2.0 / 252.0
    if kind in ('integers', 'inf'):
        assert all(w[5] > 0 for w, s in zip(want, sizes) if min(s) >= 40)
    # exact_cells on both sides of every shape's n m, and on both ends
    limits = sorted({n * m - d for n, m in SHAPES for d in (0, 1)} | {0, NEVER})
    first = None
    for exact_cells in limits:
        got = run_kernel(ctx, a, b, site_key, exact_cells)
        for i, name in enumerate(('n_a', 'n_b', 'ks_plus', 'ks_minus', 'u2', 'tie')):
            assert np.array_equal(got[i], w_int[i]), (name, exact_cells)
        mask = np.array([served(n, m, exact_cells) for n, m in sizes])
        assert site_ranks_ref.same_bits(got[6], np.where(mask, w_p, np.nan)), exact_cells
        if exact_cells == NEVER:
            first = got
    # a second run gives the same bits
    again = run_kernel(ctx, a, b, site_key, NEVER)
    assert all(np.array_equal(x, y) for x, y in zip(first[:6], again[:6]))
    assert site_ranks_ref.same_bits(first[6], again[6])
    # the listed keys that a sample does not hold
    for q, counts in ((7, (6, 0)), (17, (0, 9)), (27, (0, 0))):
        i = int(np.nonzero(site_key == q)[0][0])
        assert (first[0][i], first[1][i]) == counts and all(first[j][i] == 0 for j in range(2, 6))
        assert np.isnan(first[6][i])


def test_one_site_spanning_the_input_and_many_sites(ctx):
    rng = np.random.default_rng(9)
    A, B = np.sort(rng.normal(0.0, 1.0, 300)), np.sort(rng.normal(0.3, 1.0, 40))
    a, b = (np.full(300, 5, np.int64), A), (np.full(40, 5, np.int64), B)
    got = run_kernel(ctx, a, b, [5], 16384)
    want = site_ranks_ref.one_site(A, B, 16384)
    assert [int(g[0]) for g in got[:6]] == list(want[:6]) and got[6][0] == want[6] and want[6] < 1.0
    # a sample without rows
    none = (np.zeros(0, np.int64), np.zeros(0))
    got = run_kernel(ctx, a, none, [5], 16384)
    assert [int(g[0]) for g in got[:6]] == [300, 0, 0, 0, 0, 0] and np.isnan(got[6][0])
    got = run_kernel(ctx, none, none, [5, 6], 16384)
    assert all((g == 0).all() for g in got[:6]) and np.isnan(got[6]).all()
    # 300 sites of coverage 8 .. 24, levels rounded to two places so that some tie
    keys = np.sort(rng.choice(5000, 300, replace=False))
    rows = []
    for _ in range(2):
        cov = rng.integers(8, 25, 300)
        k = np.repeat(keys, cov)
        v = np.round(rng.normal(0.0, 0.3, k.size) + 0.01 * (k % 7), 2)
        order = np.lexsort((v, k))
        rows.append((k[order], v[order]))
    got = run_kernel(ctx, rows[0], rows[1], keys, 16384)
    want = site_ranks_ref.rank_tests(*rows[0], *rows[1], keys, 16384)
    for g, w in zip(got[:6], want[:6]):
        assert np.array_equal(g, w)
    assert site_ranks_ref.same_bits(got[6], want[6]) and not np.isnan(want[6]).any() and (want[5] > 0).any()
    assert 0.0 < want[6].min() < 0.05 and want[6].max() <= 1.0


def test_device_layer_drops_sorts_and_lists(ctx):
    """``device.site_rank_tests_dev`` on unsorted rows with keys of -1 and NaN values among them."""
    import torch
    from nadavca_amd import device
    rng = np.random.default_rng(21)
    dev = torch.device('cuda', ctx.device)
    rows = []
    for s in range(2):
        k = rng.integers(-1, 40, 700).astype(np.int64)
        v = np.round(rng.normal(0.0, 1.0, 700), 1)
        v[rng.random(700) < 0.05] = np.nan
        rows.append((k, v))
    for min_coverage, exact_cells in ((1, 16384), (12, 16384), (15, 250)):
        want = site_ranks_ref.device_layer(*rows[0], *rows[1], min_coverage, exact_cells)
        got = device.site_rank_tests_dev(ctx, *[torch.from_numpy(x).to(dev) for r in rows for x in r], min_coverage,
                                         exact_cells)
        got = [t.cpu().numpy() for t in got]
        assert len(got) == 8 and all(np.array_equal(g, w) for g, w in zip(got[:7], want[:7]))
        assert site_ranks_ref.same_bits(got[7], want[7])
        assert got[0].dtype == np.int64 and got[7].dtype == np.float64
    assert 0 < want[0].size < 40 and np.isnan(want[7]).any() and not np.isnan(want[7]).all()
    for bad in (dict(min_coverage=0), dict(exact_cells=-1)):
        with pytest.raises(ValueError):
            device.site_rank_tests_dev(ctx, *[torch.from_numpy(x).to(dev) for r in rows for x in r],
                                       **dict(dict(min_coverage=5, exact_cells=100), **bad))


def test_c_abi_rejects_bad_arguments(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    key = torch.tensor([2, 2, 2, 4, 4], dtype=torch.int64, device=dev)
    val = torch.tensor([0.1, 0.2, 0.3, 0.0, 1.0], dtype=torch.float64, device=dev)
    site = torch.tensor([2, 4], dtype=torch.int64, device=dev)
    outs = [torch.full((2,), -99, dtype=torch.int64, device=dev) for _ in range(6)]
    ks_p = torch.full((2,), -99.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(c=None, na=5, ka=key, va=val, nb=5, kb=key, vb=val, ns=2, sk=site, cells=100, o=None, pp=ks_p):
        o = outs if o is None else o
        return lib.nvk_site_rank_tests_dev(ctx.handle if c is None else c, na, p(ka), p(va), nb, p(kb), p(vb), ns,
                                           p(sk), cells, *[p(t) for t in o], p(pp))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert call() == _lib.NVK_OK
    assert outs[0].tolist() == [3, 2] and outs[1].tolist() == [3, 2] and outs[2].tolist() == [0, 0]
    assert outs[4].tolist() == [9, 4] and outs[5].tolist() == [3 * 6, 2 * 6] and ks_p.tolist() == [1.0, 1.0]
    # n_sites == 0: OK and nothing is written, whatever the other pointers are
    marks = [torch.full((2,), -99, dtype=torch.int64, device=dev) for _ in range(6)]
    assert call(ns=0, o=marks) == _lib.NVK_OK and all(t.tolist() == [-99, -99] for t in marks)
    assert call(ns=0, sk=None, o=[None] * 6, pp=None, ka=None, va=None, kb=None, vb=None) == _lib.NVK_OK
    # an empty sample may be NULL
    assert call(na=0, ka=None, va=None) == _lib.NVK_OK and outs[0].tolist() == [0, 0] and outs[1].tolist() == [3, 2]
    assert np.isnan(ks_p.cpu().numpy()).all()
    assert call(cells=0) == _lib.NVK_OK and np.isnan(ks_p.cpu().numpy()).all() and outs[4].tolist() == [9, 4]
    assert call(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(na=-1), dict(nb=-1), dict(ns=-1), dict(cells=-1), dict(ka=None), dict(va=None), dict(kb=None),
               dict(vb=None), dict(sk=None), dict(pp=None)):
        assert invalid(call(**kw)), kw
    for i in range(6):
        assert invalid(call(o=[None if j == i else t for j, t in enumerate(outs)])), i
