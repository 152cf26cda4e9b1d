"""CPU check behind nadavca_amd/csrc/path_step.h, the path comparison of the forward sweep (csrc/kernels_align3.hip):
the host build of the header (tests/host_shims/path_step_host.cpp, a ctypes library) over seeded and adversarial pairs.

The sweep takes `upd = tdiff > 0` wherever no lane's pair is inside the tie margin and forms gt_tol's margin only in
the block it enters when one is (path_cmp_fast + the cold-block rule); path_cmp_full forms the margin every time, as the
sweep did before.  The header's lemma says the two give the same update bit and the same tie class for |G| < 2^27; here
that is counted over more than 10^6 pairs, the full form is compared with a numpy restatement of xmath.h's gt_tol /
near_tol / within_ulps, and one case pins the bound: far enough above it the forms do differ, so a guard that checks
nothing would be noticed.  The same cases go once more through a stand-alone program built with the address and
undefined-behaviour sanitizers.  What the kernel does with it is tests/test_gpu_path_margin.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, 'tests', 'host_shims')
GBIG = 1 << 24                       # path_step.h: scale of an empty maximum
TIE_EXACT, TIE_NEAR, TIE_ULP = 1, 2, 4
G_MAX = (1 << 27) - 1                # the lemma's bound


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp('path_step')), 'path_step_host.so')
    subprocess.run(['g++', '-O2', '-shared', '-fPIC', os.path.join(SHIMS, 'path_step_host.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.path_step_host_run.argtypes = [C.c_longlong] + [C.c_void_p] * 5
    lib.path_step_host_run.restype = C.c_longlong
    lib.path_step_host_take.argtypes = [C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.path_step_host_margin.argtypes = [C.c_double, C.c_int]
    lib.path_step_host_margin.restype = C.c_double
    lib.path_step_host_top_margin.argtypes = [C.c_double, C.c_int]
    lib.path_step_host_top_margin.restype = C.c_double
    return lib


def run(lib, cases):
    dv, Gin, bestn, G = cases
    out = np.empty(len(dv), dtype=np.int32)
    differ = lib.path_step_host_run(len(dv), dv.ctypes.data, Gin.ctypes.data, bestn.ctypes.data, G.ctypes.data,
                                    out.ctypes.data)
    return differ, out


def make_cases(seed, n, g_abs_max, g_fixed=None):
    """n pairs around maxima bestn in [0.5, 1) on scales |G| <= g_abs_max (or all |G| = g_fixed), plus the empty maximum.
    The candidate is built ON the maximum's scale (dva) and then moved to a scale of its own by a power of two, which is
    exact: dv = dva * 2^-sh, Gin = G - sh."""
    rng = np.random.default_rng(seed)
    bestn = rng.uniform(0.5, 1.0, n)
    edge = rng.integers(0, 16, n)
    bestn[edge == 0] = 0.5
    bestn[edge == 1] = np.nextafter(1.0, 0.0)
    if g_fixed is None:
        # magnitudes spread over the binades up to the bound, the bound itself and 0 among them
        mag = np.minimum(np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(0, 28, n)).astype(np.int64), g_abs_max)
        pick = rng.integers(0, 8, n)
        mag[pick == 0] = g_abs_max
        mag[pick == 1] = g_abs_max - rng.integers(0, 1000, n)[pick == 1]
        mag[(pick == 2) & (edge > 12)] = 0
    else:
        mag = np.full(n, g_fixed, dtype=np.int64)
    G = (mag * rng.choice([-1, 1], n)).astype(np.int64)
    # the candidate: relative distances 2^-60 .. 4 on both sides, the ulp neighbours, equality, 0, +inf
    kind = rng.integers(0, 12, n)
    k = rng.integers(-2, 61, n)
    side = rng.choice([-1.0, 1.0], n)
    rel = np.ldexp(rng.uniform(1.0, 2.0, n), -k.astype(np.int32)) * side
    rel[kind == 0] = np.ldexp(side[kind == 0], -k[kind == 0].astype(np.int32))        # exact powers of two
    # the tie margin's own edge, 2^-24, and the margin of gt_tol, |G| 2^-52, with a little on either side
    at24 = kind == 1
    rel[at24] = side[at24] * np.ldexp(1.0 + rng.integers(-64, 65, at24.sum()) * 2.0 ** -30, -24)
    atm = kind == 2
    rel[atm] = side[atm] * np.abs(G[atm]) * 2.0 ** -52 * rng.choice([0.5, 1.0, 1.0 + 2.0 ** -20, 2.0, 63.0, 64.0, 65.0], atm.sum())
    dva = bestn * (1.0 + rel)
    dva = np.maximum(dva, 0.0)
    up = kind == 3
    dva[up] = np.nextafter(bestn[up], 2.0)
    dn = kind == 4
    dva[dn] = np.nextafter(bestn[dn], 0.0)
    few = kind == 5                                             # a few ulps off
    dva[few] = bestn[few] + rng.integers(-40, 41, few.sum()) * 2.0 ** -53
    dva[kind == 6] = bestn[kind == 6]
    rare = rng.integers(0, 64, n)
    dva[rare == 0] = 0.0
    dva[rare == 1] = np.inf
    sh = rng.integers(-500, 501, n)
    sh[rare == 2] = 0
    dv = np.ldexp(dva, (-sh).astype(np.int32))
    Gin = G - sh
    # a candidate so small that dva * 2^-24 flushes to zero (the engine flushes FP64 denormals)
    dv[rare == 2] = np.ldexp(rng.uniform(1.0, 2.0, (rare == 2).sum()), rng.integers(-1022, -1000, (rare == 2).sum()).astype(np.int32))
    # the empty maximum: bestn = 0 on the scale GBIG, against candidates of every kind on scales of their own
    empty = rng.integers(0, 10, n) == 0
    bestn[empty] = 0.0
    G[empty] = GBIG
    Gin[empty] = rng.integers(-100000, 100001, empty.sum())
    dv[empty] = np.where(rng.integers(0, 4, empty.sum()) == 0, 0.0, np.ldexp(rng.uniform(0.5, 1.0, empty.sum()),
                                                                          rng.integers(-1000, 1000, empty.sum()).astype(np.int32)))
    flush = empty & (rare == 2)                                 # ... and one that stays finite and tiny on that scale
    Gin[flush] = GBIG
    dv[flush] = 2.0 ** -1010
    return (np.ascontiguousarray(dv, dtype=np.float64), np.ascontiguousarray(Gin, dtype=np.int32),
            np.ascontiguousarray(bestn, dtype=np.float64), np.ascontiguousarray(G, dtype=np.int32))


def ftz(x):
    return np.where(np.abs(x) < 2.0 ** -1022, 0.0, x)


def restated_full(cases):
    """upd and class as xmath.h has them (gt_tol, near_tol, eq, within_ulps), denormals flushed."""
    dv, Gin, bestn, G = cases
    with np.errstate(over='ignore', invalid='ignore'):
        dva = ftz(np.ldexp(dv, np.clip(G.astype(np.int64) - Gin, -5000, 5000).astype(np.int32)))
        tdiff = ftz(dva - bestn)
        margin = ftz(bestn * (np.abs(G.astype(np.int64)).astype(np.float64) * 2.0 ** -52))
        upd = tdiff > margin
        near = np.abs(tdiff) < ftz(dva * 2.0 ** -24)
        cls = np.where(tdiff == 0.0, TIE_EXACT, np.where(np.abs(tdiff) <= ftz(margin * 64.0), TIE_ULP, TIE_NEAR))
    return upd, near, np.where(near, cls, 0)


N_CASES = 1 << 21


@pytest.fixture(scope='module')
def cases():
    return make_cases(2027, N_CASES, G_MAX)


def test_fast_form_equals_full_form_below_the_bound(lib, cases):
    differ, out = run(lib, cases)
    assert len(out) >= 10 ** 6
    full, fast = out & 15, (out >> 4) & 15
    assert differ == 0 and np.array_equal(full, fast)
    near, upd0 = (out >> 8) & 1, (out >> 9) & 1
    # the lemma itself: outside the tie margin tdiff > 0 already is the full form's bit
    assert np.array_equal(upd0[near == 0], (full & 1)[near == 0])
    # ... and inside it the margin is needed: the table holds pairs where tdiff > 0 alone would be wrong
    assert ((near == 1) & (upd0 != (full & 1))).sum() > 1000
    # enough of everything
    cls = full >> 1
    dv, Gin, bestn, G = cases
    for c in (TIE_EXACT, TIE_ULP, TIE_NEAR):
        assert (cls == c).sum() > 10000, c
    assert ((near == 0) & (full & 1 == 1)).sum() > 100000 and ((near == 0) & (full & 1 == 0)).sum() > 100000
    assert (np.abs(G.astype(np.int64)) == G_MAX).sum() > 100000 and (G == 0).sum() > 100
    assert (bestn == 0.0).sum() > 100000 and (bestn == 0.5).sum() > 10000 and np.isinf(dv).sum() > 1000
    assert ((bestn == 0.0) & (dv == 2.0 ** -1010)).sum() > 100 and ((dv > 0) & (dv < 2.0 ** -999)).sum() > 1000


def test_full_form_is_gt_tol(lib, cases):
    _, out = run(lib, cases)
    upd, near, cls = restated_full(cases)
    assert np.array_equal(out & 1, upd.astype(np.int32))
    assert np.array_equal((out >> 8) & 1, near.astype(np.int32))
    assert np.array_equal((out >> 1) & 7, cls.astype(np.int32))


def test_the_bound_is_real(lib):
    """Far enough above the bound the two forms differ: a pair outside the 2^-24 tie margin and inside gt_tol's margin
    |G| 2^-52.  (That takes |G| 2^-52 > 2^-24 / (1 - 2^-24): at |G| = 2^28 exactly the margin is bestn 2^-24, still
    below dva 2^-24, and the forms agree — counted here as well; from 2^29 on they differ on every seed.)"""
    differ28, _ = run(lib, make_cases(2028, 1 << 18, None, g_fixed=1 << 28))
    differ29, out = run(lib, make_cases(2028, 1 << 18, None, g_fixed=1 << 29))
    print('forms differ on %d pairs at |G| = 2^28, on %d at 2^29' % (differ28, differ29))
    assert differ29 > 100
    bad = ((out & 15) != ((out >> 4) & 15))
    assert np.all(((out >> 8) & 1)[bad] == 0)          # every one of them outside the tie margin: no cold block there
    differ, _ = run(lib, make_cases(2028, 1 << 18, G_MAX))
    assert differ == 0                                   # (the same seed below the bound)


def test_take_and_margins(lib):
    bestn, G = C.c_double(), C.c_int32()
    for dv, Gin in ((0.75, 7), (3.0, -5), (2.0 ** -900, 123456), (1.0, GBIG), (np.nextafter(0.5, 0.0), 0)):
        lib.path_step_host_take(dv, Gin, C.byref(bestn), C.byref(G))
        m, e = np.frexp(dv)
        assert (bestn.value, G.value) == (m, Gin - e) and 0.5 <= bestn.value < 1.0
        # the margin where it is needed is the one an update used to store
        assert lib.path_step_host_margin(bestn.value, G.value) == m * (abs(Gin - e) * 2.0 ** -52)
        # the last row's arg-max keeps its maximum unnormalised
        assert lib.path_step_host_top_margin(dv, Gin) == dv * (abs(int(e) - Gin) * 2.0 ** -52)
    assert lib.path_step_host_margin(0.0, GBIG) == 0.0 and lib.path_step_host_top_margin(0.0, 0) == 0.0


def test_the_cases_under_the_sanitizers(lib, cases, tmp_path):
    """tests/host_shims/path_step_main.cpp: a plain program with its own main, address + undefined-behaviour sanitizers
    linked in; every case goes through the header in it and comes out as the ctypes library has it."""
    flags = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run(['g++'] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('the toolchain has no sanitizer runtimes')   # (an empty program: nothing of the code under test)
    exe = str(tmp_path / 'path_step_main')
    build = subprocess.run(['g++'] + flags + [os.path.join(SHIMS, 'path_step_main.cpp'), '-o', exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    dv, Gin, bestn, G = cases
    path = tmp_path / 'cases.bin'
    with open(path, 'wb') as f:
        f.write(np.int64(len(dv)).tobytes())
        for a in (dv, bestn, Gin, G):
            f.write(a.tobytes())
    got = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    differ, out = run(lib, cases)
    x = np.bitwise_xor.reduce(np.arange(1, len(out) + 1, dtype=np.uint64) * out.astype(np.uint32).astype(np.uint64))
    assert got.stdout.split() == [str(len(out)), str(differ), str(int(x))]
