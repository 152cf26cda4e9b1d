"""nvk_repeat_count_dev against its CPU restatement (tests/host_shims/repeats_host.cpp: the full matrix, every cell
carrying what the kernel's cells carry), bit for bit in every f64 and equal in every i32.  The cases are
tests/repeats_ref.py's: chains of 3, 5, 63, 64, 65, 128, 129, 255 and 256 states in one call (so the three
instantiations and both sides of their limits), E = 0, 1, too few for a path, 64, 65 and 300, a ``status_in`` entry,
windows of one read's events, grid-valued ties, the hand-made path; then the items of the simulated batch, twice with
the same bits; the argument checks."""
import numpy as np
import pytest

import repeats_ref as P
import signal_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return P.build_host(tmp_path_factory.mktemp('repeats_host'))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def run_dev(ctx, case, timing=False, **over):
    """-> (hit, score) as numpy arrays"""
    import torch
    from nadavca_amd.device import repeat_count_dev
    dev = torch.device('cuda', ctx.device)
    c = dict(case, **over)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    st = None if c['status_in'] is None else t(c['status_in'])
    out = repeat_count_dev(ctx, t(c['level']), t(c['items']), t(c['mu']), t(c['ac']), t(c['mc']), t(c['st_off']),
                           t(c['chain_par']), *c['costs'], c['trim'], st, timing=timing)
    return tuple(x.cpu().numpy() for x in out[:2]) + tuple(out[2:])


def assert_same(got, want, name):
    bad = np.nonzero((got[0] != want[0]).any(1) | (bits(got[1]) != bits(want[1])).any(1))[0]
    assert bad.size == 0, (name, bad[:5].tolist(), got[0][bad[:2]].tolist(), want[0][bad[:2]].tolist())


def test_constructed_cases(ctx, host):
    for name, case in P.kernel_cases():
        assert_same(run_dev(ctx, case), P.run_host(host, case), name)


def test_hand_made_path(ctx):
    case, (first, last, loops, i1, i2) = P.hand_case()
    hit, score, ms = run_dev(ctx, case, timing=True)
    assert hit[0].tolist() == [P.REP_OK, case['level'].size, first, last, 4, i1, i2, 0]
    assert score[0, 0] == score[0, 1] + float(P.HAND_TAIL) * case['trim'] and ms > 0.0


def test_simulated_items_twice(ctx, host, tmp_path):
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    rb, loci, truth, _, _ = P.simulated_batch(model)
    case = P.cpu_count_repeats(R.build_host(tmp_path), host, rb, loci, model)['case']
    assert case['items'].shape[0] == 2 * rb.n
    want = P.run_host(host, case)
    first, second = run_dev(ctx, case), run_dev(ctx, case)
    assert_same(first, want, 'simulated')
    assert_same(second, first, 'simulated, again')
    assert (want[0][:, 0] == P.REP_OK).all()


def test_bad_arguments(ctx):
    from nadavca_amd._lib import NadavcaHipError
    name, case = P.kernel_cases()[1]
    run_dev(ctx, case)
    n_chains, N0 = case['chain_par'].shape[0], int(case['st_off'][1])
    assert N0 == 3
    for bad in ((1, 1, 1, 2), (1, 0, 0, 2), (1, 0, 2, 1), (1, 0, 1, 3), (2, 0, 1, 2), (1, -1, 1, 2), (0, 1, 1, 2)):
        par = case['chain_par'].copy()
        par[0] = bad
        with pytest.raises(ValueError, match='chain 0'):
            run_dev(ctx, case, chain_par=par)
    for bad in ((n_chains, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 3, 2), (0, 0, case['level'].size + 1)):
        items = case['items'].copy()
        items[1] = bad
        with pytest.raises(ValueError, match='item 1'):
            run_dev(ctx, case, items=items)
    st_off = case['st_off'].copy()
    st_off[1] = st_off[2] + 1
    with pytest.raises(ValueError):
        run_dev(ctx, case, st_off=st_off)
    for at in range(4):
        for bad in (0.5, float('nan'), float('-inf')):
            costs = list(case['costs']) + [case['trim']]
            costs[at] = bad
            with pytest.raises(ValueError):
                run_dev(ctx, case, costs=tuple(costs[:3]), trim=costs[3])
    # a chain of 2 states is invalid, one of 257 unsupported
    two = P.pack([(np.zeros(2), np.zeros(2), np.ones(2), (1, 0, 1, 1))], [(0, 0, 4)], np.zeros(4), P.GRID_COSTS,
                 P.GRID_TRIM)
    with pytest.raises(ValueError, match='chain 0'):
        run_dev(ctx, two)
    big = P.pack([(np.zeros(257), np.zeros(257), np.ones(257), (5, 3, 3, 9))], [(0, 0, 4)], np.zeros(4), P.GRID_COSTS,
                 P.GRID_TRIM)
    with pytest.raises(NadavcaHipError, match='above 256'):
        run_dev(ctx, big)


def test_no_items(ctx):
    name, case = P.kernel_cases()[1]
    hit, score = run_dev(ctx, case, items=np.zeros((0, 3), np.int64), status_in=None)
    assert hit.shape == (0, 8) and score.shape == (0, 4)
