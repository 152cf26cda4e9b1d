"""wave_max_i (csrc/wave.h), the wave's maximum in a scalar register, feeds the sweeps' rescale decision.  A rescale by
any common power of two is exact, so a wrong maximum changes no event and no parity test can see it: the library's
self-test entry nvk_selftest_wave_max (include/nadavca_hip.h) runs the very function on rows of 64 values, one wave per
row, and this test compares it with numpy's maximum of each row.  Equality is exact.

The rows: the maximum at each of the 64 lanes in turn, every other lane the sentinel the sweeps give a lane without a
value (-0x40000000, which must come through unchanged when every lane holds it); the maximum on either side of the
lane boundaries 15/16, 31/32 and 47/48 — the ones the DPP row broadcasts cross — with the second-largest value right
across; equal maxima in several lanes; values at the ends of the int32 range; 256 seeded random rows."""
import numpy as np
import pytest

SENTINEL = -0x40000000
INT_MIN, INT_MAX = -0x80000000, 0x7fffffff


def rows_of_cases():
    """-> (names, int32 [n, 64])"""
    names, rows = [], []

    def add(name, row):
        names.append(name)
        rows.append(np.asarray(row, dtype=np.int64))

    for lane in range(64):                      # the maximum at each lane, everything else the sentinel
        r = np.full(64, SENTINEL)
        r[lane] = 250 - 3 * lane                # (exponent-sized values, a different one per row)
        add('max_at_lane_%d' % lane, r)
        r = np.full(64, SENTINEL)
        r[lane] = -1074 - lane                  # a negative maximum above the sentinel
        add('negative_max_at_lane_%d' % lane, r)
    add('all_sentinel', np.full(64, SENTINEL))
    for lo in (15, 31, 47):                     # across the boundaries of the 16-lane rows and of the halves
        for a, b in ((lo, lo + 1), (lo + 1, lo)):
            r = np.full(64, SENTINEL)
            r[a], r[b] = 1000, 999
            add('max_at_%d_second_at_%d' % (a, b), r)
            r = np.arange(64) - 500             # the rest ascending, below both
            r[a], r[b] = 1000, 999
            add('max_at_%d_second_at_%d_ramp' % (a, b), r)
    for lanes in ((0, 63), (15, 16), (31, 32), (47, 48), (0, 16, 32, 48), (15, 31, 47, 63), tuple(range(64))):
        r = np.full(64, SENTINEL)
        r[list(lanes)] = 77
        add('equal_maxima_%s' % '_'.join(map(str, lanes[:4])), r)
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):   # the ends of the int32 range
        r = np.full(64, INT_MIN + 1)
        add('all_int_min_plus_1_l%d' % lane, r)
        r = np.full(64, INT_MIN + 1)
        r[lane] = INT_MIN + 2
        add('int_min_plus_2_at_%d' % lane, r)
        r = np.full(64, INT_MAX - 1)
        r[lane] = INT_MAX
        add('int_max_at_%d' % lane, r)
        r = np.full(64, INT_MIN + 1)
        r[lane] = INT_MAX
        add('int_max_over_int_min_at_%d' % lane, r)
    rng = np.random.default_rng(20261021)
    for i in range(256):
        if i < 128:                             # the whole range
            r = rng.integers(INT_MIN + 1, INT_MAX, 64, endpoint=True)
        else:                                   # exponent-sized values with sentinel lanes among them, as the sweeps hold
            r = rng.integers(-1100, 1025, 64)
            r[rng.random(64) < rng.uniform(0.0, 0.95)] = SENTINEL
        add('random_%d' % i, r)
    rows = np.stack(rows)
    assert rows.min() >= INT_MIN + 1 and rows.max() <= INT_MAX
    return names, rows.astype(np.int32)


def test_the_rows_hold_what_the_docstring_says():
    names, rows = rows_of_cases()
    assert len(set(names)) == len(names) and rows.shape == (len(names), 64) and rows.dtype == np.int32
    arg = {n: int(np.argmax(r)) for n, r in zip(names, rows)}
    assert [arg['max_at_lane_%d' % l] for l in range(64)] == list(range(64))
    assert rows[names.index('all_sentinel')].tolist() == [SENTINEL] * 64
    assert sum(n.startswith('random_') for n in names) == 256


@pytest.mark.gpu
def test_wave_max_equals_numpy_max():
    from nadavca_amd import _lib
    names, rows = rows_of_cases()
    want = rows.max(axis=1)
    got = _lib.default_context().selftest_wave_max(rows)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(names[i], int(got[i]), int(want[i])) for i in bad[:8]]
    assert got[names.index('all_sentinel')] == SENTINEL


@pytest.mark.gpu
def test_wave_max_no_rows_and_bad_shape():
    from nadavca_amd import _lib
    ctx = _lib.default_context()
    assert ctx.selftest_wave_max(np.zeros((0, 64), dtype=np.int32)).shape == (0,)
    with pytest.raises(ValueError):
        ctx.selftest_wave_max(np.zeros((3, 32), dtype=np.int32))
