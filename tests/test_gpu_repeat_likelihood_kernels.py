"""nvk_repeat_likelihoods_dev against its CPU restatement (tests/host_shims/repeatlik_host.cpp: the full (E, L, N)
trellis), bit for bit in out_z and out_x and equal in status, every item of tests/repeatlik_ref.py's case in one call
per window: chains of 3, 5, 63, 64, 65, 128, 129, 255 and 256 states (the three instantiations and both sides of their
limits); windows of 1, 2, LB - 1, LB, LB + 1, 2 LB + 1 and 128 layers for both LB (one wave, the hand-over between
waves, the largest workgroup); loops over 2, 3 and 6 states, their ends in one lane, in two and in two slots of a
lane; E = 0, 1, 2, too few for a path, 64, 65 and 300; more trips than the window holds; events on the floor; 300
events of narrow Gaussians; a ``status_in`` entry; items that share events.  Then the chosen items of the simulated
batch, twice with the same bits, and the argument checks."""
import numpy as np
import pytest

import repeatlik_ref as K
import repeats_ref as P
import signal_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return K.build_host(tmp_path_factory.mktemp('repeatlik_host'))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def run_dev(ctx, case, layers, timing=False, **over):
    """-> (z, x, status) as numpy arrays"""
    import torch
    from nadavca_amd.device import repeat_likelihoods_dev
    dev = torch.device('cuda', ctx.device)
    c = dict(case, **over)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    st = None if c['status_in'] is None else t(c['status_in'])
    out = repeat_likelihoods_dev(ctx, t(c['level']), t(c['items']), t(c['mu']), t(c['ac']), t(c['mc']), t(c['st_off']),
                                 t(c['chain_par']), *c['weights'], layers, st, timing=timing)
    return tuple(v.cpu().numpy() for v in out[:3]) + tuple(out[3:])


def assert_same(got, want, name):
    bad = np.nonzero((bits(got[0]) != bits(want[0])).any(1) | (bits(got[1]) != bits(want[1])) | (got[2] != want[2]))[0]
    assert bad.size == 0, (name, bad[:5].tolist(), got[2][bad[:3]].tolist(), want[2][bad[:3]].tolist(),
                           got[1][bad[:3]].tolist(), want[1][bad[:3]].tolist())


@pytest.fixture(scope='module')
def case():
    return K.kernel_case()


@pytest.mark.parametrize('layers', K.KERNEL_LAYERS)
def test_kernel_equals_restatement(ctx, host, case, layers):
    got, want = run_dev(ctx, case, layers), K.run_host(host, case, layers)
    assert_same(got, want, layers)
    status = want[2]
    E = case['items'][:, 2] - case['items'][:, 1]
    assert (status[E == 0] == K.REP_NO_EVENTS).all() and status[5] == 7 and (status == K.REP_NO_PATH).any()
    ok = status == K.REP_OK
    assert ok.sum() > 40 and (want[0][ok] > 0.0).any(1).all() and (want[0][~ok] == 0.0).all()
    assert want[1][case['sharp']] < -1000.0


def test_hand_made_chain(ctx, host):
    case = K.hand_case()
    z, x, status, ms = run_dev(ctx, case, K.HAND_LAYERS, timing=True)
    assert_same((z, x, status), K.run_host(host, case, K.HAND_LAYERS), 'hand')
    ll = K.loglik(z, x)[0]
    post = np.exp(ll - ll.max())
    assert post[P.HAND_LOOPS] / post.sum() > 0.99 and ms > 0.0


def test_simulated_items_twice(ctx, host, tmp_path):
    """The items ``count_repeats_batch(layers=48)`` runs on the simulated batch: equal to the shim, and the same bits
    from a second call"""
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    rb, loci, truth, _, _ = P.simulated_batch(model)
    res = P.cpu_count_repeats(R.build_host(tmp_path), P.build_host(tmp_path), rb, loci, model)
    case = dict(res['case'])
    case['weights'] = K.weights_of(case)
    case['items'], case['status_in'] = case['items'][2 * np.arange(rb.n) + res['strand']], res['status'].astype(np.int32)
    want = K.run_host(host, case, K.SIM_LAYERS)
    first, second = run_dev(ctx, case, K.SIM_LAYERS), run_dev(ctx, case, K.SIM_LAYERS)
    assert_same(first, want, 'simulated')
    assert_same(second, first, 'simulated, again')
    assert (want[2] == K.REP_OK).all()


def test_bad_arguments(ctx, case):
    from nadavca_amd._lib import NadavcaHipError
    small = K.small_cases()
    run_dev(ctx, small, 4)
    with pytest.raises(ValueError, match='layers'):
        run_dev(ctx, small, 0)
    with pytest.raises(NadavcaHipError, match='above 128'):
        run_dev(ctx, small, K.MAX_LAYERS + 1)
    for at in range(4):
        for bad in (0.0, 1.5, float('nan'), -0.1, float('inf')):
            w = list(small['weights'])
            w[at] = bad
            with pytest.raises(ValueError, match=r'\(0, 1\]'):
                run_dev(ctx, small, 4, weights=tuple(w))
    with pytest.raises(ValueError, match='2\\^-10'):
        run_dev(ctx, small, 4, weights=(2.0 ** -11, 2.0 ** -11, 0.5, 0.01))
    run_dev(ctx, small, 4, weights=(2.0 ** -11, 2.0 ** -10, 0.5, 0.01))
    n_chains = small['chain_par'].shape[0]
    N0 = int(small['st_off'][1])
    for bad in ((1, 1, 1, 2), (1, 0, 0, 2), (1, 0, 2, 1), (1, 0, 1, N0), (N0 - 1, 0, 1, N0 - 1), (1, -1, 1, 2), (0, 1, 1, 2)):
        par = small['chain_par'].copy()
        par[0] = bad
        with pytest.raises(ValueError, match='chain 0'):
            run_dev(ctx, small, 4, chain_par=par)
    for bad in ((n_chains, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 3, 2), (0, 0, small['level'].size + 1)):
        items = small['items'].copy()
        items[1] = bad
        with pytest.raises(ValueError, match='item 1'):
            run_dev(ctx, small, 4, items=items)
    st_off = small['st_off'].copy()
    st_off[1] = st_off[2] + 1
    with pytest.raises(ValueError):
        run_dev(ctx, small, 4, st_off=st_off)
    two = K.with_weights(P.pack([(np.zeros(2), np.zeros(2), np.ones(2), (1, 0, 1, 1))], [(0, 0, 4)], np.zeros(4),
                                P.LOG_COSTS, P.LOG_TRIM))
    with pytest.raises(ValueError, match='chain 0'):
        run_dev(ctx, two, 4)
    big = K.with_weights(P.pack([(np.zeros(257), np.zeros(257), np.ones(257), (5, 3, 3, 9))], [(0, 0, 4)], np.zeros(4),
                                P.LOG_COSTS, P.LOG_TRIM))
    with pytest.raises(NadavcaHipError, match='above 256'):
        run_dev(ctx, big, 4)


def test_no_items(ctx):
    small = K.small_cases()
    z, x, status = run_dev(ctx, small, 7, items=np.zeros((0, 3), np.int64), status_in=None)
    assert z.shape == (0, 7) and x.shape == (0,) and status.shape == (0,)
