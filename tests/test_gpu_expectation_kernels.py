"""nvk_kmer_expectations_dev against its CPU restatement (tests/host_shims/kmer_fb_host.cpp: the full matrices, the sums
over all states on arrays, the events descending), bit for bit in the ten stats, z and status, for k = 2..6 and so for
every workgroup size of the counts sweep (1, 4, 16, 64 and 256 threads).  The cases are tests/decode_ref.py's (E = 0, 1,
2, 3, 64, 65 and 300, a ``status_in`` entry), the three extreme cases of tests/posterior_ref.py, and at k = 6 the
packaged table and 64 simulated reads, whole and cut into parts by the workspace limit; z also against
nvk_kmer_posterior_dev's."""
import math

import numpy as np
import pytest

import decode_ref as D
import expect_ref as X
import posterior_ref as P
import signal_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return X.build_host(tmp_path_factory.mktemp('expect_host'))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope='module')
def simulated(host, tmp_path_factory):
    """-> (the k = 6 case, the shim's results for it)"""
    case, _ = D.simulated_case(R.build_host(tmp_path_factory.mktemp('map_host')))
    return case, X.run_host(host, case, threads=8)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def tensors(ctx, case, over):
    import torch
    dev = torch.device('cuda', ctx.device)
    c = dict(case, **over)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    w = c['w'] if 'w' in c else tuple(math.exp(x) for x in c['costs'])
    st = None if c['status_in'] is None else t(c['status_in'])
    return c, (t(c['level']), t(c['ev_off'])), (t(c['mean']), t(c['ac']), t(c['mc'])) + tuple(w) + (st,)


def run_dev(ctx, case, **over):
    """-> (stats, z, status, parts) as numpy arrays"""
    from nadavca_amd.device import kmer_expectations_dev
    c, events, rest = tensors(ctx, case, over)
    out = kmer_expectations_dev(ctx, *events, c['k'], *rest)
    return tuple(x.cpu().numpy() for x in out[:3]) + (out[3],)


def posterior_z(ctx, case):
    from nadavca_amd.device import kmer_posterior_dev
    c, events, rest = tensors(ctx, case, {})
    return kmer_posterior_dev(ctx, *events, c['k'], 0, *rest)[1].cpu().numpy()


def assert_same(got, want, name):
    for what, a, b in zip(('stats', 'z'), got[:2], want[:2]):
        assert a.shape == b.shape, (name, what, a.shape, b.shape)
        bad = np.argwhere(bits(a) != bits(b))
        assert bad.size == 0, (name, what, bad.shape[0], bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
    assert np.array_equal(got[2], want[2]), (name, 'status')


@pytest.mark.parametrize('k', [2, 3, 4, 5, 6])
def test_constructed_cases(ctx, host, k):
    for name, case in D.kernel_cases(k):
        got = run_dev(ctx, case)
        assert_same(got, X.run_host(host, case), name)
        assert got[3] == 1
        assert np.array_equal(bits(got[1]), bits(posterior_z(ctx, case))), name
    name, case = D.kernel_cases(k)[0]
    assert np.diff(case['ev_off']).tolist() == D.KERNEL_LENGTHS + [33]
    stats, z, status, _ = run_dev(ctx, case)
    assert status.tolist() == [D.DEC_NO_EVENTS] + [0] * len(D.KERNEL_LENGTHS[1:]) + [7]
    assert (z[[0, -1]] == 0.0).all() and (z[1:-1, 0] > 0.0).all() and (stats[[0, -1]] == 0.0).all()
    E = np.array(D.KERNEL_LENGTHS[1:], dtype=np.float64)
    total = (stats[1:-1, 6] + stats[1:-1, 7]) + stats[1:-1, 8]
    # (the bound of tests/test_expectation_cpu.py)
    assert (np.abs(total - (E - 1.0)) <= np.finfo(np.float64).eps * (2 * E + 1.5 * E * E)).all()
    assert (stats[1:-1, 0] > 0.0).all() and (stats[1, 6:9] == 0.0).all()


def test_extreme_cases(ctx, host):
    for name, case in P.extreme_cases():
        got = run_dev(ctx, case)
        assert_same(got, X.run_host(host, case), name)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert np.array_equal(bits(got[1]), bits(posterior_z(ctx, case))), name
    cases = dict(P.extreme_cases())
    assert run_dev(ctx, cases['far event'])[0][0, 9] == 1.0
    assert run_dev(ctx, cases['large ac'])[0][0, 9] == 0.0


def test_packaged_table_and_simulated_reads(ctx, simulated):
    case, want = simulated
    assert case['k'] == 6 and case['ev_off'].size - 1 == 64 and (want[2] == 0).all()
    got = run_dev(ctx, case)
    assert_same(got, want, 'k 6')
    assert got[3] == 1
    assert np.array_equal(bits(got[1]), bits(posterior_z(ctx, case)))


def test_small_workspace_limits_change_nothing(ctx, simulated):
    """The k = 6 batch under limits that cut it into at least three and at least seven parts, and under one smaller
    than its largest read's rows (every read a part of its own): the same bits as in one piece."""
    case, want = simulated
    per_read = np.diff(case['ev_off']) * (8 * 4 ** 6)
    try:
        for limit, least in ((int(per_read.sum()) // 3, 3), (int(per_read.sum()) // 7, 7), (int(per_read.max()) - 8, 64)):
            ctx.set_workspace_limit(limit)
            got = run_dev(ctx, case)
            assert got[3] >= least and (least < 64 or got[3] == 64), (limit, got[3])
            assert_same(got, want, 'limit %d' % limit)
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
    good = tuple(math.exp(x) for x in case['costs'])
    for at in range(3):
        for bad in (0.0, 1.5, float('nan'), -0.25, float('inf')):
            w = list(good)
            w[at] = bad
            with pytest.raises(ValueError):
                run_dev(ctx, case, w=tuple(w))
    with pytest.raises(ValueError, match='2\\^-10'):
        run_dev(ctx, case, w=(2.0 ** -11, 2.0 ** -11, 0.5))
    run_dev(ctx, case, w=(2.0 ** -10, 2.0 ** -11, 0.5))
    ev_off = case['ev_off'].copy()
    ev_off[2] = ev_off[3] + 1               # descending offsets
    with pytest.raises(ValueError):
        run_dev(ctx, case, ev_off=ev_off)


def test_no_reads(ctx):
    name, case = D.kernel_cases(3)[0]
    stats, z, status, parts = run_dev(ctx, case, level=np.zeros(0), ev_off=np.zeros(1, np.int64), status_in=None)
    assert stats.shape == (0, 10) and z.shape == (0, 2) and status.size == 0 and parts == 0
