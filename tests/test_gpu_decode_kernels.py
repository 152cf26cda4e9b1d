"""nvk_viterbi_decode_dev against its CPU restatement (tests/host_shims/decode_host.cpp: the full matrix, a flat
traceback, the path read forwards), bit for bit in every f64 and i32, for k = 2..6 and so for every workgroup size of
the sweep (1, 4, 16, 64 and 256 threads).  The cases are tests/decode_ref.py's: E = 0, 1, 2, 3, 64, 65 and 300, central
0 and k - 1, a ``status_in`` entry, grid-valued ties, for every k; at k = 6 also the packaged table and 64 simulated
reads, whole and cut into parts by the workspace limit."""
import numpy as np
import pytest

import decode_ref as D
import signal_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return D.build_host(tmp_path_factory.mktemp('decode_host'))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope='module')
def simulated(host, tmp_path_factory):
    """-> (the k = 6 case, the shim's results for it)"""
    case, _ = D.simulated_case(R.build_host(tmp_path_factory.mktemp('map_host')))
    return case, run_host(host, case, threads=8)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def run_dev(ctx, case, **over):
    """-> (hit, score, seq, base_event, parts) as numpy arrays"""
    import torch
    from nadavca_amd.device import viterbi_decode_dev
    dev = torch.device('cuda', ctx.device)
    c = dict(case, **over)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cap_off = c.get('cap_off')
    cap_off = D.capacities(c['ev_off'], c['k']) if cap_off is None else cap_off
    st = None if c['status_in'] is None else t(c['status_in'])
    out = viterbi_decode_dev(ctx, t(c['level']), t(c['ev_off']), c['k'], c['central'], t(c['mean']), t(c['ac']),
                             t(c['mc']), *c['costs'], st, t(cap_off))
    return tuple(x.cpu().numpy() for x in out[:4]) + (out[4],)


def run_host(host, case, **kw):
    return host.decode(case['level'], case['ev_off'], case['k'], case['central'], case['mean'], case['ac'], case['mc'],
                       *case['costs'], status_in=case['status_in'], **kw)


def assert_same(got, want, case, name):
    """hit and score whole; seq and base_event over every read's n_bases entries (the rest of a capacity is scratch)"""
    assert np.array_equal(got[0], want[0]), (name, 'hit', np.argwhere(got[0] != want[0])[:5].tolist())
    bad = np.argwhere(bits(got[1]) != bits(want[1]))
    assert bad.size == 0, (name, 'score', bad[:5].tolist())
    cap_off = D.capacities(case['ev_off'], case['k'])
    for r in range(case['ev_off'].size - 1):
        sl = slice(int(cap_off[r]), int(cap_off[r]) + int(want[0][r, 2]))
        assert np.array_equal(got[2][sl], want[2][sl]), (name, 'seq', r)
        assert np.array_equal(got[3][sl], want[3][sl]), (name, 'base_event', r)


@pytest.mark.parametrize('k', [2, 3, 4, 5, 6])
def test_constructed_cases(ctx, host, k):
    for name, case in D.kernel_cases(k):
        got = run_dev(ctx, case)
        assert_same(got, run_host(host, case), case, name)
        assert got[4] == 1
    name, case = D.kernel_cases(k)[0]
    assert np.diff(case['ev_off']).tolist() == D.KERNEL_LENGTHS + [33]
    hit, score = run_dev(ctx, case)[:2]
    assert hit[0].tolist() == [D.DEC_NO_EVENTS, 0, 0, -1] and hit[-1].tolist() == [7, 33, 0, -1]
    assert np.isneginf(score[[0, -1]]).all() and np.isfinite(score[1:-1]).all()
    assert hit[1, 2] == k and (hit[1:-1, 0] == 0).all()


@pytest.mark.parametrize('central', [0, 1, 2])
def test_hand_made_path(ctx, central):
    case = D.hand_case(central)
    hit, score, seq, be, _ = run_dev(ctx, case)
    assert hit[0, :3].tolist() == [0, 12, 10]
    assert seq[:10].tolist() == D.HAND_BASES and be[:10].tolist() == D.HAND_BASE_EVENT[central]


def test_packaged_table_and_simulated_reads(ctx, simulated):
    case, want = simulated
    assert case['k'] == 6 and case['ev_off'].size - 1 == 64 and (want[0][:, 0] == 0).all()
    got = run_dev(ctx, case)
    assert_same(got, want, case, 'k 6')
    assert got[4] == 1


def test_small_workspace_limits_change_nothing(ctx, simulated):
    """The k = 6 batch under limits that cut it into at least three parts, and under one smaller than its largest read's
    store (every read a part of its own): the same bits as in one piece."""
    case, want = simulated
    E = np.diff(case['ev_off'])
    per_read = (E - 1) * (4 ** 6 // 2)
    try:
        for limit, least in ((int(per_read.sum()) // 3, 3), (int(per_read.sum()) // 7, 7), (int(per_read.max()) - 8, 64)):
            ctx.set_workspace_limit(limit)
            got = run_dev(ctx, case)
            assert got[4] >= least and (least < 64 or got[4] == 64), (limit, got[4])
            assert_same(got, want, case, 'limit %d' % limit)
    finally:
        ctx.set_workspace_limit(0)


def test_bad_arguments(ctx):
    from nadavca_amd._lib import NadavcaHipError
    name, case = D.kernel_cases(3)[0]
    run_dev(ctx, case)
    big = dict(case, k=7, mean=np.zeros(4 ** 7), ac=np.zeros(4 ** 7), mc=np.ones(4 ** 7))
    with pytest.raises(NadavcaHipError, match='outside 2..6'):
        run_dev(ctx, big)
    with pytest.raises(NadavcaHipError):
        run_dev(ctx, dict(big, k=1))
    for central in (-1, 3):
        with pytest.raises(ValueError):
            run_dev(ctx, case, central=central)
    cap_off = D.capacities(case['ev_off'], 3)
    short = cap_off.copy()
    short[-2:] -= 1                     # the read of 300 events: a capacity one short
    with pytest.raises(ValueError, match='room for'):
        run_dev(ctx, case, cap_off=short)
    down = cap_off.copy()
    down[3] = down[2] - 1               # descending offsets
    with pytest.raises(ValueError):
        run_dev(ctx, case, cap_off=down)
    ev_off = case['ev_off'].copy()
    ev_off[2] = ev_off[3] + 1
    with pytest.raises(ValueError):
        run_dev(ctx, case, ev_off=ev_off)
    for at in range(3):
        for bad in (0.5, float('nan'), float('-inf')):
            costs = list(case['costs'])
            costs[at] = bad
            with pytest.raises(ValueError):
                run_dev(ctx, case, costs=tuple(costs))


def test_no_reads(ctx):
    name, case = D.kernel_cases(3)[0]
    hit, score, seq, be, parts = run_dev(ctx, case, level=np.zeros(0), ev_off=np.zeros(1, np.int64), status_in=None)
    assert hit.shape == (0, 4) and score.size == 0 and seq.size == 0 and be.size == 0 and parts == 0
