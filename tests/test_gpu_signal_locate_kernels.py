"""nvk_signal_locate_dev against its CPU restatement (tests/host_shims/locate_host.cpp, the full matrix without tiles),
bit for bit in every f64 and i32, for both instantiations of the kernel: tiles of 1024 columns with 768 valid ones
(max_events up to 128) and with 512 (up to 256).  The cases are tests/locate_ref.py's: target lengths around the block and tile widths,
Q = 0, 1, 2 and max_events, targets that meet inside a tile and on a tile's edge, the cone's extreme, noise events at
both ends, grid-valued ties, 40 random queries against 2 x 3000 columns."""
import numpy as np
import pytest

import locate_ref as L

pytestmark = pytest.mark.gpu

WIDTHS = (128, 256)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return L.build_host(tmp_path_factory.mktemp('locate_host'))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def run_dev(ctx, case, max_events, **over):
    import torch
    from nadavca_amd.device import signal_locate_dev
    dev = torch.device('cuda', ctx.device)
    c = dict(case, **over)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    score, hit = signal_locate_dev(ctx, t(c['level']), t(c['q_off']), t(c['mu']), t(c['ac']), t(c['mc']),
                                   t(c['col_off']), max_events, *c['costs'])
    return score.cpu().numpy(), hit.cpu().numpy()


def run_host(host, case):
    return host.locate(case['level'], case['q_off'], case['mu'], case['ac'], case['mc'], case['col_off'],
                       *case['costs'])


def assert_same(got, want, name):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, name
    bad = np.argwhere(bits(got[0]) != bits(want[0]))
    assert bad.size == 0, (name, 'score', bad[:5].tolist())
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (name, 'hit', bad[:5].tolist())


@pytest.mark.parametrize('max_events', WIDTHS)
def test_constructed_cases(ctx, host, max_events):
    for name, case in L.kernel_cases(max_events):
        assert int(np.diff(case['q_off']).max()) <= max_events
        assert_same(run_dev(ctx, case, max_events), run_host(host, case), name)


@pytest.mark.parametrize('max_events', WIDTHS)
def test_queries_of_zero_one_two_and_max_events(ctx, host, max_events):
    name, case = L.kernel_cases(max_events)[0]
    assert sorted(set(np.diff(case['q_off']).tolist()))[:3] == [0, 1, 2] and np.diff(case['q_off']).max() == max_events
    V = L.valid_width(max_events)
    assert np.diff(case['col_off']).tolist() == [1, 2, 3, 255, 256, 257, V - 1, V, V + 1, 2 * V + 3]
    score, hit = run_dev(ctx, case, max_events)
    empty = np.diff(case['q_off']) == 0
    assert np.isneginf(score[empty]).all() and (hit[empty] == -1).all()
    assert np.isfinite(score[~empty]).all() and (hit[~empty] >= 0).all()


@pytest.mark.parametrize('max_events', WIDTHS)
def test_cone_extreme(ctx, host, max_events):
    """All skips over 2 Q - 1 columns, ending on the first and on the last valid column of a tile: the path's first
    column is the first one of the tile's halo that a valid column depends on."""
    case, want = L.cone_case(max_events)
    got = run_dev(ctx, case, max_events)
    assert_same(got, run_host(host, case), 'cone')
    for blk, end, start in want:
        assert got[1][0, blk].tolist() == [end, max_events - 1, start, 0]
        assert end - start == 2 * (max_events - 1)
    assert sorted(np.argsort(got[0][0])[-2:].tolist()) == sorted(w[0] for w in want)


@pytest.mark.parametrize('max_events', WIDTHS)
def test_noise_events_at_both_ends_are_trimmed(ctx, max_events):
    name, case = [c for c in L.kernel_cases(max_events) if c[0] == 'noise at both ends'][0]
    score, hit = run_dev(ctx, case, max_events)
    end, last, start, first = hit[0, int(np.argmax(score[0]))].tolist()
    Q = int(case['q_off'][1])
    assert first == 7 and last == Q - 1 - 9
    V = L.valid_width(max_events)
    assert abs(start - (V - 30)) <= 2 and abs(end - (V + 9)) <= 2


def test_results_do_not_depend_on_the_instantiation(ctx):
    """The same queries (Q <= 128) through both tile shapes: the cut does not show."""
    name, case = L.kernel_cases(128)[-1]
    assert_same(run_dev(ctx, case, 128), run_dev(ctx, case, 256), name)


def test_bad_arguments(ctx):
    from nadavca_amd._lib import NadavcaHipError
    name, case = L.small_cases()[0]
    run_dev(ctx, case, 128)
    for k in range(4):
        for bad in (0.5, float('nan'), float('-inf')):
            costs = list(case['costs'])
            costs[k] = bad
            with pytest.raises(ValueError):
                run_dev(ctx, case, 128, costs=tuple(costs))
    with pytest.raises(NadavcaHipError):
        run_dev(ctx, case, 257)
    with pytest.raises(ValueError):
        run_dev(ctx, case, 0)
    with pytest.raises(ValueError):     # a query above max_events
        run_dev(ctx, case, int(np.diff(case['q_off']).max()) - 1)
    q_off = case['q_off'].copy()
    q_off[0] = 1
    with pytest.raises(ValueError):
        run_dev(ctx, case, 128, q_off=q_off)
    col_off = case['col_off'].copy()
    col_off[-1] += 1                    # the targets end beyond the column tables
    with pytest.raises(ValueError):
        run_dev(ctx, case, 128, col_off=col_off)


def test_no_queries_and_no_targets(ctx):
    name, case = L.small_cases()[0]
    nb = L.n_blocks_of(case['col_off'])
    score, hit = run_dev(ctx, case, 128, level=np.zeros(0), q_off=np.zeros(1, np.int64))
    assert score.shape == (0, nb) and hit.shape == (0, nb, 4)
    z = np.zeros(0)
    score, hit = run_dev(ctx, case, 128, mu=z, ac=z, mc=z, col_off=np.zeros(1, np.int64))
    assert score.shape == (case['q_off'].size - 1, 0)


def test_small_workspace_cap_changes_nothing(ctx, host):
    """The queries in parts under a cap of three queries' block table, and under the context's workspace limit,
    against one part."""
    import torch
    from nadavca_amd import locate
    name, case = L.kernel_cases(128)[-1]
    dev = torch.device('cuda', ctx.device)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    args = [t(case[k]) for k in ('level', 'q_off', 'mu', 'ac', 'mc', 'col_off')] + [128] + list(case['costs'])
    nq, nb = case['q_off'].size - 1, L.n_blocks_of(case['col_off'])
    whole, parts = locate.locate_queries_dev(ctx, *args, cap=1 << 30)
    assert parts == 1
    capped, parts = locate.locate_queries_dev(ctx, *args, cap=3 * nb * locate.TABLE_BYTES)
    assert parts == -(-nq // 3)
    ctx.set_workspace_limit(nb * locate.TABLE_BYTES - 1)     # below one query's table: a query per part
    try:
        limited, n_limited = locate.locate_queries_dev(ctx, *args)
    finally:
        ctx.set_workspace_limit(0)
    assert n_limited == nq
    score, hit = run_host(host, case)
    want = L.reduce_blocks(score, hit, np.diff(case['q_off']), *L.block_tables(case['col_off']))
    for got in (whole, capped, limited):
        for a, b in zip(got, want):
            a = a.cpu().numpy()
            assert np.array_equal(bits(a), bits(b)) if b.dtype == np.float64 else np.array_equal(a, b)
