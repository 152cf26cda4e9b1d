"""GPU tests of the mixture kernel (csrc/kernels_sitemix.hip) through the C-ABI on constructed pile-ups: the integer
table equal to the numpy restatement (tests/site_mixtures_ref.py), the floats within 1e-9 relative + 1e-9 absolute of it
(device exp and log against numpy's: the tolerance of ``allele_ref.check_against``) with NaN and infinities in the same
places, the same bits on a second call, the device layer around the kernel, and the invalid-argument returns."""
import ctypes as C

import numpy as np
import pytest

import site_mixtures_ref as ref
from site_ranks_ref import same_bits

pytestmark = pytest.mark.gpu

# (n_a, n_b): N = 128 is the last site whose rows stay in registers (CACHE = 2), 129 the first that re-reads them
SHAPES = [(2, 2), (5, 5), (1, 64), (63, 65), (64, 64), (64, 65), (300, 40), (1000, 1500)]
KINDS = ['null', 'bimodal', 'rounded', 'equal', 'disjoint', 'offset']


def values(kind, rng, n, m, t):
    if kind == 'null':
        return rng.normal(0.0, 0.35, n), rng.normal(0.0, 0.35, m)
    if kind == 'bimodal':
        b = rng.normal(0.0, 0.35, m)
        b[rng.random(m) < 0.5] += 1.5
        return rng.normal(0.0, 0.35, n), b
    if kind == 'rounded':                                 # many ties
        return np.round(rng.normal(0.0, 0.35, n), 1), np.round(rng.normal(0.3, 0.35, m), 1)
    if kind == 'equal':
        return np.full(n, 1.25), np.full(m, 1.25)
    if kind == 'disjoint':
        lo, hi = rng.random(n), 100.0 + rng.random(m)
        return (lo, hi) if t % 2 == 0 else (lo + 5.0, hi)
    return 1e6 + rng.normal(0.0, 1.0, n), 1e6 + rng.normal(0.5, 1.0, m)       # 'offset': the centred arithmetic


def build_case(kind, seed):
    """One input with every shape of SHAPES as a listed key 10 t + 3, unlisted keys 10 t + 5 between them (in A, in B
    or in both), and three more listed keys: 7 with rows only in A, 17 only in B, 27 in neither.  -> rows sorted by
    (key, value) per sample, the listed keys, and per listed key its (A, B) sorted."""
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
        runs[10 * t + 3] = (np.sort(A), np.sort(B))
        if t % 3 != 0:
            add('a', 10 * t + 5, rng.normal(0.0, 1.0, 1 + t))
        if t % 3 != 1:
            add('b', 10 * t + 5, rng.normal(0.0, 1.0, 2 + t))
    empty = np.zeros(0)
    extra = [np.sort(rng.normal(0.0, 1.0, 6)), np.sort(rng.normal(0.0, 1.0, 9))]
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


def run_kernel(ctx, a, b, site_key, iterations=32, min_sd_ratio=0.1):
    """nvk_site_mixture_tests_dev on host arrays already sorted by (key, value): -> (counts, fit) numpy arrays."""
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    ka, va, kb, vb = up(a[0], np.int64), up(a[1], np.float64), up(b[0], np.int64), up(b[1], np.float64)
    sk = up(site_key, np.int64)
    n = int(sk.numel())
    counts = torch.full((n, 5), -99, dtype=torch.int64, device=dev)
    fit = torch.full((n, 17), -99.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.nvk_site_mixture_tests_dev(ctx.handle, int(ka.numel()), p(ka), p(va), int(kb.numel()), p(kb), p(vb), n,
                                        p(sk), int(iterations), float(min_sd_ratio), p(counts), p(fit))
    assert rc == _lib.NVK_OK, lib.nvk_last_error()
    return counts.cpu().numpy(), fit.cpu().numpy()


@pytest.mark.parametrize('kind', KINDS)
def test_every_shape_against_the_restatement(ctx, kind):
    a, b, site_key, runs = build_case(kind, 300 + KINDS.index(kind))
    want = ref.fit_runs([runs[int(q)] for q in site_key], 32, 0.1)
    sizes = [(runs[int(q)][0].size, runs[int(q)][1].size) for q in site_key]
    assert sorted(s for s in sizes if s[0] and s[1]) == sorted(SHAPES)
    both = np.array([bool(s[0] and s[1]) for s in sizes])
    F = {name: i for i, name in enumerate(ref.FIT_NAMES)}
    if kind == 'equal':
        assert (want[0][:, 2:] == 0).all() and (want[1][both][:, [0, 6, 16]] == np.inf).all()
    else:
        assert (want[0][both, 2] == 1).all() and (want[0][both, 3] == 32).all() and np.isfinite(want[1][both]).all()
    if kind == 'disjoint':
        big = both & (np.array([s[0] + s[1] for s in sizes]) >= 10)
        wa, wb = want[1][big, F['wa']], want[1][big, F['wb']]
        assert (np.minimum(wa, 1.0 - wa) < 1e-12).all() and (np.abs(wa + wb - 1.0) < 1e-12).all()
    if kind == 'offset':
        assert (np.abs(want[1][both, F['mean0']] - 1e6) < 10).all() and (want[1][both, F['sd0']] < 5).all()
    got = run_kernel(ctx, a, b, site_key)
    worst = ref.check_against(*got, *want)
    print('%s: largest |difference| / (1 + |value|) %.3g' % (kind, worst))
    # a second run gives the same bits
    again = run_kernel(ctx, a, b, site_key)
    assert np.array_equal(got[0], again[0]) and same_bits(got[1], again[1])
    # the listed keys that a sample does not hold
    for q, n_m in ((7, [6, 0]), (17, [0, 9]), (27, [0, 0])):
        i = int(np.nonzero(site_key == q)[0][0])
        assert got[0][i].tolist() == n_m + [0, 0, 0] and np.isnan(got[1][i]).all()
    # other settings of the two parameters: one step and no room below the site's spread; many steps
    for iterations, ratio in ((1, 1.0), (5, 0.5), (100, 0.01)):
        want = ref.fit_runs([runs[int(q)] for q in site_key], iterations, ratio)
        ref.check_against(*run_kernel(ctx, a, b, site_key, iterations, ratio), *want)
        if kind != 'equal':
            assert (want[0][both, 3] == iterations).all()


def test_one_site_spanning_the_input_and_many_sites(ctx):
    rng = np.random.default_rng(9)
    A, B = np.sort(rng.normal(0.0, 1.0, 300)), np.sort(rng.normal(0.3, 1.0, 40))
    a, b = (np.full(300, 5, np.int64), A), (np.full(40, 5, np.int64), B)
    got = run_kernel(ctx, a, b, [5])
    want = ref.one_site(A, B)
    ref.check_against(got[0], got[1], want[0][None], want[1][None])
    # a sample without rows
    none = (np.zeros(0, np.int64), np.zeros(0))
    got = run_kernel(ctx, a, none, [5])
    assert got[0].tolist() == [[300, 0, 0, 0, 0]] and np.isnan(got[1]).all()
    got = run_kernel(ctx, none, none, [5, 6])
    assert (got[0] == 0).all() and np.isnan(got[1]).all()
    # 600 sites of coverage 8 .. 24, levels rounded to two places so that some tie, every third bimodal in B
    keys = np.sort(rng.choice(5000, 600, replace=False))
    rows = []
    for s in range(2):
        cov = rng.integers(8, 25, 600)
        k = np.repeat(keys, cov)
        v = rng.normal(0.0, 0.3, k.size) + 0.01 * (k % 7)
        v[(k % 3 == 0) & (rng.random(k.size) < 0.5 * s)] += 1.2
        v = np.round(v, 2)
        order = np.lexsort((v, k))
        rows.append((k[order], v[order]))
    got = run_kernel(ctx, rows[0], rows[1], keys)
    want = ref.mixture_tests(*rows[0], *rows[1], keys, 32, 0.1)
    worst = ref.check_against(*got, *want)
    print('600 sites: largest |difference| / (1 + |value|) %.3g' % worst)
    assert (want[0][:, 2] == 1).all()
    again = run_kernel(ctx, rows[0], rows[1], keys)
    assert np.array_equal(got[0], again[0]) and same_bits(got[1], again[1])
    # the order of a sum depends on the site's rows only, never on the launch: the same sites alone
    alone = run_kernel(ctx, rows[0], rows[1], keys[100:103])
    assert same_bits(alone[1], got[1][100:103])


def test_device_layer_drops_sorts_and_lists(ctx):
    """``device.site_mixture_tests_dev`` on unsorted rows with keys of -1 and NaN and infinite values among them."""
    import torch
    from nadavca_amd import device
    rng = np.random.default_rng(21)
    dev = torch.device('cuda', ctx.device)
    rows = []
    for s in range(2):
        k = rng.integers(-1, 40, 900).astype(np.int64)
        v = np.round(rng.normal(0.0, 1.0, 900), 1)
        v[rng.random(900) < 0.05] = np.nan
        v[rng.random(900) < 0.03] = np.inf
        v[rng.random(900) < 0.03] = -np.inf
        rows.append((k, v))
    tensors = lambda: [torch.from_numpy(x).to(dev) for r in rows for x in r]
    for min_coverage, iterations, ratio in ((1, 32, 0.1), (18, 32, 0.1), (22, 3, 0.3)):
        want = ref.device_layer(*rows[0], *rows[1], min_coverage, iterations, ratio)
        got = [t.cpu().numpy() for t in device.site_mixture_tests_dev(ctx, *tensors(), min_coverage, iterations, ratio)]
        assert len(got) == 3 and np.array_equal(got[0], want[0]) and got[1].shape == (want[0].size, 5)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.float64
        ref.check_against(got[1], got[2], want[1], want[2])
    assert 0 < want[0].size < 40
    for bad in (dict(min_coverage=0), dict(iterations=0), dict(iterations=1025), dict(min_sd_ratio=0.0),
                dict(min_sd_ratio=1.01)):
        with pytest.raises(ValueError):
            device.site_mixture_tests_dev(ctx, *tensors(), **dict(dict(min_coverage=5, iterations=32,
                                                                       min_sd_ratio=0.1), **bad))


def test_c_abi_rejects_bad_arguments(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    key = torch.tensor([2, 2, 2, 4, 4], dtype=torch.int64, device=dev)
    val = torch.tensor([0.1, 0.2, 0.9, 0.0, 1.0], dtype=torch.float64, device=dev)
    site = torch.tensor([2, 4], dtype=torch.int64, device=dev)
    counts = torch.full((2, 5), -99, dtype=torch.int64, device=dev)
    fit = torch.full((2, 17), -99.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(c=None, na=5, ka=key, va=val, nb=5, kb=key, vb=val, ns=2, sk=site, it=32, ratio=0.1, oc=counts, of=fit):
        return lib.nvk_site_mixture_tests_dev(ctx.handle if c is None else c, na, p(ka), p(va), nb, p(kb), p(vb), ns,
                                              p(sk), it, ratio, p(oc), p(of))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert call() == _lib.NVK_OK
    assert counts.tolist() == [[3, 3, 1, 32, 32], [2, 2, 1, 32, 32]] and torch.isfinite(fit).all()
    # n_sites == 0: OK and nothing is written, whatever the other pointers are
    marks = torch.full((2, 5), -99, dtype=torch.int64, device=dev)
    assert call(ns=0, oc=marks) == _lib.NVK_OK and (marks == -99).all()
    assert call(ns=0, sk=None, oc=None, of=None, ka=None, va=None, kb=None, vb=None) == _lib.NVK_OK
    # an empty sample may be NULL
    assert call(na=0, ka=None, va=None) == _lib.NVK_OK
    assert counts.tolist() == [[0, 3, 0, 0, 0], [0, 2, 0, 0, 0]] and torch.isnan(fit).all()
    assert call(it=1, ratio=1.0) == _lib.NVK_OK and call(it=1024) == _lib.NVK_OK
    assert counts.tolist() == [[3, 3, 1, 1024, 1024], [2, 2, 1, 1024, 1024]]
    assert call(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(na=-1), dict(nb=-1), dict(ns=-1), dict(it=0), dict(it=1025), dict(it=-3), dict(ratio=0.0),
               dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float('nan')), dict(ka=None), dict(va=None),
               dict(kb=None), dict(vb=None), dict(sk=None), dict(oc=None), dict(of=None)):
        assert invalid(call(**kw)), kw
