"""The order in which the sweeps leave their rows (csrc/kernels_align3.hip serves a row switch as a scalar event of the
oldest open row; the derivation stands next to the gap bound in csrc/kernels_plan.hip), checked on the host.

There is no read-back of a plan's offsets, so the planner's geometry is restated from the bands
(tests/switch_order_cases.py, plan_geometry): bands as the reference forms them — prefix maximum of the starts, suffix
minimum of the ends, so both are non-decreasing in the row —, the spans LO / HI, the skew, the gap bound

    g[r] = max(1 - mel(r-1), LO(r-1) - LO(r), HI(r-1) - HI(r))      (transition rows, min event length <= 2)
    g[r] = max(mel - 1, 1)                                           (everything else)

and the least offsets above it (uniform offsets c r where the planner keeps those).  Checked, on the reads of
tests/test_gpu_row_switch.py and on a seeded few hundred make_dp_case reads across bandwidths and min event lengths:

* the bound itself: g[r] >= BE(r-1) - BE(r) and g[r] >= BS(r-1) - BS(r), the two inequalities of the derivation;
* the offsets: off[r] - off[r-1] >= g[r], and off + BE (forward) and off + BS (reverse) non-decreasing in r.

On the device the sweeps hold the same order to account themselves: a lane found past its row's end at a rescale step
hands the read to the exact kernel, and tests/test_gpu_row_switch.py asserts that none is."""
import numpy as np
import pytest

import switch_order_cases as soc


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


def check_plan(p, what):
    T = p['T']
    assert (np.diff(p['BS']) >= 0).all() and (np.diff(p['BE']) >= 0).all(), what   # the bands move one way
    g, off = p['g'], p['off']
    if T > 1:
        assert (g[1:] >= p['BE'][:-1] - p['BE'][1:]).all(), what
        assert (g[1:] >= p['BS'][:-1] - p['BS'][1:]).all(), what
        d = np.diff(off)
        assert (d >= g[1:]).all() and (d <= max(p['c'], p['cw'])).all(), what
        if T > 64 and p['fixp']:   # (the lane is free, and idle, before its next row starts)
            idle_from = p['HI'][:-64] - p['LO'][64:] + 1
            assert (off[64:] - off[:-64] > idle_from).all(), what
    assert soc.leaving_order_holds(p), what


def test_the_switch_cases_leave_their_rows_in_order(model):
    batches = soc.build_cases(model)
    n = 0
    for b in batches:
        for c, rows in zip(b['cases'], b['rows']):
            p = soc.plan_geometry(c, b['bw'], b['mel'], b['tr'])
            assert p['T'] == rows, (b['name'], p['T'])
            check_plan(p, b['name'])
            n += 1
    assert n >= 36


def test_the_clipped_cases_have_flat_band_ends(model):
    """Several rows leave on the same step: band ends equal to N on the last rows, band starts 0 on the first."""
    seen = 0
    for b in soc.build_cases(model):
        if 'clipped_ends' not in b['name']:
            continue
        p = soc.plan_geometry(b['cases'][0], b['bw'], b['mel'], b['tr'])
        last, first = p['BE'][-3:], p['BS'][:3]
        assert (last == p['N']).all() and (first == 0).all(), (b['name'], last, first)
        # ... and with equal band ends the rows' leaving steps differ by their offsets alone
        assert np.unique(p['BE'][-6:]).size == 1 and np.unique(p['BS'][:6]).size == 1, b['name']
        seen += 1
    assert seen == 4


def test_seeded_reads_leave_their_rows_in_order(model):
    rng = np.random.default_rng(soc.SEED)
    n = n_fixp = n_neg = n_team = 0
    for tr in (False, True):
        for mel in (0, 1, 2, 3, 4):
            for bw in (4, 12, 40, 150):
                for it in range(8):
                    R = int(rng.integers(2, 260))
                    lo = int(rng.integers(max(mel, 1), max(mel, 1) + 4))
                    c = soc.make_read(model, tr, mel, R, bw, lo, lo + int(rng.integers(1, 9)), it,
                                      anchor_density=float(rng.choice([0.1, 0.6, 1.0])), jitter=int(rng.integers(0, 12)))
                    p = soc.plan_geometry(c, bw, mel, tr)
                    check_plan(p, (tr, mel, bw, R, it))
                    n += 1
                    n_fixp += int(p['fixp'])
                    n_neg += int((p['g'][1:] < 1).any())
                    n_team += int(p['cw'] != 0)
    print('reads %d, with per-row offsets %d, with a gap below 1 %d, swept by teams %d' % (n, n_fixp, n_neg, n_team))
    assert n == 320 and n_fixp > 40 and n_neg > 20 and n_team > 5


def test_a_band_that_moved_backwards_would_break_the_order():
    """What the derivation rests on: with band ends that fall from one row to the next the bound of the plain modes
    does not hold the order, so the check above is not one that passes whatever it is given."""
    T = 6
    BE = np.array([10, 10, 10, 7, 7, 7])
    p = dict(off=np.arange(T), BE=BE, BS=np.zeros(T, dtype=np.int64))
    assert not soc.leaving_order_holds(p)
