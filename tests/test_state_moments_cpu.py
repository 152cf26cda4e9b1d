"""The rules of ``estimate_decode_model`` without a GPU: the C++ restatement of nvk_kmer_state_moments_dev against a
log-domain forward-backward in plain numpy, the identities that tie its per-state moments to the events and to the
per-read moments of nvk_kmer_expectations_dev, the M-step of nadavca_amd/decode_train.py against its own expected
log-likelihood and against a restatement with per-state loops, and the re-estimation as a whole on reads drawn from the
HMM itself, seen through a table whose means are displaced."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import decode_ref as D
import expect_ref as X
import moments_ref as M
import posterior_ref as P

# The shim against the log-domain restatement, every moment as |difference| / max(1, |value|): the project's standing
# bound for such pairs.  Measured on the cases of the first test: 1.41e-13 at the most (k = 4, central 3; the far-event
# case 1.34e-13, every other case within 8.6e-14), log Z within 5.2e-15 (the narrow-sigma case).
TOL = 1e-9
EPS = float(np.finfo(np.float64).eps)
ROUNDS = 5


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return M.build_host(tmp_path_factory.mktemp('moments_host'))


@pytest.fixture(scope='module')
def exp_host(tmp_path_factory):
    return X.build_host(tmp_path_factory.mktemp('expect_host'))


@pytest.fixture(scope='module')
def hmm():
    return X.hmm_case()


def train_args(hmm, rounds, start_mean, **over):
    """The arguments of ``train_rounds`` / ``train_loop`` after the steps, for the HMM case from ``start_mean``"""
    n = hmm['ev_off'].size - 1
    kw = dict(fit=1, fit_params=('scale',), update=('mean',), min_weight=8.0, min_sigma=0.05, sigma_scale=1.0,
              p_stay=0.7, p_skip=0.01, scale=None, shift=None)
    kw.update(over)
    return (np.diff(hmm['ev_off']), np.ones(n, bool), start_mean, np.asarray(hmm['model'][4]), rounds, kw['fit'],
            kw['fit_params'], kw['update'], kw['min_weight'], kw['min_sigma'], kw['sigma_scale'], kw['p_stay'],
            kw['p_skip'], kw['scale'], kw['shift'])


@pytest.fixture(scope='module')
def shim_steps(host, exp_host, hmm):
    return M.shim_steps(exp_host, host, hmm['level'], hmm['ev_off'], hmm['model'][0], threads=8)


@pytest.fixture(scope='module')
def shim_train(shim_steps, hmm):
    """ROUNDS rounds on the shims from the displaced table -> the dict of ``train_rounds``"""
    return M.train_rounds(*shim_steps, *train_args(hmm, ROUNDS, M.displaced_means(hmm)))


def all_cases():
    return [c for k in (2, 3, 4) for c in D.kernel_cases(k)] + P.extreme_cases()


@pytest.mark.parametrize('name,case', all_cases(), ids=[c[0] + ' (%d)' % i for i, c in enumerate(all_cases())])
def test_shim_equals_the_log_domain_forward_backward(host, name, case):
    """k = 2..4 on the kernels' cases (E = 0, 1, 2, 3, 64, 65 and 300, a ``status_in`` entry) and the three extreme
    cases: every read's 3 S moments, the batch's totals and log Z within 1e-9 of max(1, |value|)."""
    w = tuple(math.exp(c) for c in case['costs'])
    total, z, status, per_read = M.run_host(host, case)
    off = case['ev_off']
    worst, want_total = [0.0, 0.0], np.zeros_like(total)
    for r in range(off.size - 1):
        if status[r] != 0:
            assert (per_read[r] == 0.0).all() and (z[r] == 0.0).all()
            continue
        want, want_z = M.python_moments(case['level'][off[r]:off[r + 1]], case['k'], case['mean'], case['ac'],
                                        case['mc'], *w)
        want_total += want
        worst[0] = max(worst[0], float((np.abs(per_read[r] - want) / np.maximum(1.0, np.abs(want))).max()))
        worst[1] = max(worst[1], abs(float(P.log_z(z[r])[0]) - want_z) / max(1.0, abs(want_z)))
    worst[0] = max(worst[0], float((np.abs(total - want_total) / np.maximum(1.0, np.abs(want_total))).max()))
    print('%s: largest difference of a moment %.3g, of log Z %.3g' % (name, worst[0], worst[1]))
    assert worst[0] <= TOL and worst[1] <= TOL, worst


def test_z_and_status_are_the_posterior_shims(host, tmp_path):
    post = P.build_host(tmp_path)
    for name, case in P.small_cases() + P.extreme_cases() + D.kernel_cases(3)[:1]:
        _, z, status, _ = M.run_host(host, case)
        _, want_z, want_status = P.run_host(post, case, 0)
        assert np.array_equal(z.view(np.int64), want_z.view(np.int64)) and np.array_equal(status, want_status), name


def test_the_weights_sum_to_the_events_and_the_first_moments_to_the_levels(host):
    """Per read SUM_s G0 = E and SUM_s G1 = SUM x_i to rounding.  One event's 4^k shares g sum to 1 within 32 eps (D is
    a sum of positive terms through at most 16 + 8 + 2 additions, 1 / D and every product round once more); every
    accumulator rounds E times on partial sums below E, over the states together below eps E^2; ``np.sum`` over the S
    states adds below eps S E.  So |SUM G0 - E| <= eps E (32 + E + S), and for G1 the same times the largest |x| (with
    one more rounding per term, 33, and ``np.sum`` of the levels themselves, E more): eps E max|x| (33 + 2 E + S)."""
    for name, case in [c for k in (2, 3, 4) for c in D.kernel_cases(k)[:2]] + P.extreme_cases():
        _, _, status, per_read = M.run_host(host, case)
        off, S = case['ev_off'], 4 ** case['k']
        for r in np.nonzero(status == 0)[0]:
            x = case['level'][off[r]:off[r + 1]]
            E, top = float(x.size), max(1.0, float(np.abs(x).max()))
            gap0 = abs(float(np.sum(per_read[r, 0])) - E)
            gap1 = abs(float(np.sum(per_read[r, 1])) - float(np.sum(x)))
            assert gap0 <= EPS * E * (32 + E + S), (name, r, gap0)
            assert gap1 <= EPS * E * top * (33 + 2 * E + S), (name, r, gap1)
            assert (per_read[r, 0] >= 0.0).all() and (per_read[r, 2] >= 0.0).all()


def test_moments_agree_with_the_expectations_shim(host, exp_host):
    """SUM_s mc[s] G0[s], SUM_s mc[s] mean[s] G0[s] and SUM_s mc[s] G1[s] of a read are the M0, Mm and Mx of
    nvk_kmer_expectations_dev (the same posteriors, summed over the states first there and over the events first
    here): within 1e-9 relative."""
    worst = 0.0
    for name, case in D.kernel_cases(3)[:2] + D.kernel_cases(4)[:1] + P.extreme_cases():
        _, _, status, per_read = M.run_host(host, case)
        stats, _, want_status = X.run_host(exp_host, case)
        assert np.array_equal(status, want_status)
        mc, mean = case['mc'], case['mean']
        for r in np.nonzero(status == 0)[0]:
            got = (np.sum(mc * per_read[r, 0]), np.sum(mc * mean * per_read[r, 0]), np.sum(mc * per_read[r, 1]))
            for g, want in zip(got, (stats[r, 0], stats[r, 3], stats[r, 1])):
                worst = max(worst, abs(float(g) - float(want)) / abs(float(want)))
                assert abs(float(g) - float(want)) <= TOL * abs(float(want)), (name, r, float(g), float(want))
    print('largest relative difference to M0, Mm, Mx: %.3g' % worst)


def expected_loglik(G, mean, sigma, c):
    """Per state the expected log-likelihood the M-step raises, up to a constant: -G0 log(c sigma) -
    (G2 - 2 mean G1 + mean^2 G0) / (2 (c sigma)^2)"""
    sd = c * sigma
    return -G[0] * np.log(sd) - (G[2] - 2.0 * mean * G[1] + mean * mean * G[0]) / (2.0 * sd * sd)


def test_m_step_maximises_its_expected_loglik_and_equals_the_loops(shim_steps, hmm):
    """With both groups updated every state's (mean, sigma) is the maximum of its own expected log-likelihood: a move
    of the mean by +- 1e-3 or of sigma by a factor 1 +- 1e-3 lowers it (a state whose sigma sits on ``min_sigma`` is
    asserted for the mean only).  The vectorised M-step and the one with per-state loops agree bit for bit, for every
    choice of ``update``; a state under ``min_weight`` keeps its bits."""
    from nadavca_amd import decode_train
    n = hmm['ev_off'].size - 1
    mean0, sigma0 = M.displaced_means(hmm), np.asarray(hmm['model'][4], dtype=np.float64)
    G, _ = shim_steps[1](mean0, sigma0, np.ones(n), np.zeros(n), 1.1, 0.7, 0.01)
    c = 1.1
    for update in (('mean',), ('sd',), ('mean', 'sd')):
        for min_weight in (8.0, float(np.median(G[0]))):
            got = decode_train.m_step(G, mean0, sigma0, c, update, min_weight, 0.05)
            want = M.m_step(G, mean0, sigma0, c, update, min_weight, 0.05)
            for a, b in zip(got, want):
                assert np.array_equal(np.asarray(a).view(np.int64) if a.dtype != bool else a,
                                      np.asarray(b).view(np.int64) if b.dtype != bool else b), (update, min_weight)
            keep = ~got[2]
            assert np.array_equal(got[2], G[0] >= min_weight)
            assert np.array_equal(got[0][keep].view(np.int64), mean0[keep].view(np.int64))
            assert np.array_equal(got[1][keep].view(np.int64), sigma0[keep].view(np.int64))
    assert 0 < (G[0] >= float(np.median(G[0]))).sum() < G.shape[1]
    mean, sigma, updated = decode_train.m_step(G, mean0, sigma0, c, ('mean', 'sd'), 8.0, 0.05)
    assert updated.all()
    best = expected_loglik(G, mean, sigma, c)
    free = sigma > 0.05
    assert free.any()
    for d in (-1e-3, 1e-3):
        assert (expected_loglik(G, mean + d, sigma, c) < best).all(), d
        assert (expected_loglik(G, mean, sigma * (1.0 + d), c)[free] < best[free]).all(), d
    assert (expected_loglik(G, mean0, sigma0, c) <= best).all()


def test_objective_does_not_fall_over_five_rounds(shim_train):
    """30 reads of 200 events drawn from the k = 3 HMM, the table's means displaced by N(0, (0.15 spread)^2): the
    objective of every round is at least the one before, less 1e-9 of its size (the slack of
    tests/test_expectation_cpu.py).  Measured: -7871.20, -7780.54, -7734.27, -7706.59, -7688.06, -7681.18."""
    obj = shim_train['objective']
    print('objective per round:', ' '.join('%.4f' % v for v in obj))
    assert obj.size == ROUNDS + 1 and np.isfinite(obj).all()
    assert (np.diff(obj) >= -1e-9 * np.abs(obj[:-1])).all(), np.diff(obj).tolist()


def test_every_round_brings_the_means_closer_to_the_truth(shim_steps, shim_train, hmm):
    """The same run: the RMS error of the means against the table the reads were drawn from, raw and after the best
    affine map, is after every round below the start's and below the previous round's.  Measured: raw 0.1544 (start),
    0.1430, 0.1375, 0.1341, 0.1317, 0.1301; after the affine map 0.1489, 0.1381, 0.1323, 0.1286, 0.1259, 0.1241."""
    true, start = np.asarray(hmm['model'][3]), M.displaced_means(hmm)
    errors = [M.mean_errors(true, start)]
    for rounds in range(1, ROUNDS + 1):
        # (rounds = r is the first r rounds of the longer run: the chain identity, asserted below)
        out = shim_train if rounds == ROUNDS else M.train_rounds(*shim_steps, *train_args(hmm, rounds, start))
        errors.append(M.mean_errors(true, out['mean']))
    print('RMS error of the means, raw:    ' + ' '.join('%.4f' % e[0] for e in errors))
    print('RMS error after the affine map: ' + ' '.join('%.4f' % e[1] for e in errors))
    for which in range(2):
        values = [e[which] for e in errors]
        assert all(v < values[0] for v in values[1:]), (which, values)
        assert all(b < a for a, b in zip(values[:-1], values[1:])), (which, values)
    assert all(h['kmers_updated'] == 64 for h in shim_train['history'])
    assert shim_train['updated'].all() and abs(shim_train['weight'].sum() - 6000.0) < 1e-6


def test_a_state_under_min_weight_keeps_its_bits(shim_steps, shim_train, hmm):
    start = M.displaced_means(hmm)
    cut = float(np.median(shim_train['weight']))
    out = M.train_rounds(*shim_steps, *train_args(hmm, 2, start, min_weight=cut))
    kept = ~out['updated']
    assert 0 < kept.sum() < 64 and out['history'][-1]['kmers_updated'] == int(out['updated'].sum())
    assert np.array_equal(out['weight'] >= cut, out['updated'])
    # (a state may be updated in the first round and not in the second: compare with the table after the first)
    first = M.train_rounds(*shim_steps, *train_args(hmm, 1, start, min_weight=cut))
    assert np.array_equal(out['mean'][kept].view(np.int64), first['mean'][kept].view(np.int64))
    never = kept & ~first['updated']
    assert never.any() and np.array_equal(out['mean'][never].view(np.int64), start[never].view(np.int64))
    assert np.array_equal(out['sigma'].view(np.int64), np.asarray(hmm['model'][4]).view(np.int64))


def test_the_loop_equals_the_restatement_and_the_chain_identity(host, exp_host):
    """``decode_train.train_loop`` and ``moments_ref.train_rounds`` on the same steps (the shims, 6 reads drawn from the
    HMM, three rounds, means and sigmas updated): every field bit for bit, the objective within 4 ulp (its terms pass
    through numpy's log there and Python's here).  And ``rounds=3`` equals three chained calls of one round, each from
    the table, scale and shift the one before left, bit for bit; a chained call's first objective is the longer run's
    of the same round (its second is taken before the next round's fit, so only the last call's is the longer run's)."""
    from nadavca_amd import decode_train
    case = X.hmm_case(n=6)
    steps = M.shim_steps(exp_host, host, case['level'], case['ev_off'], 3)
    loop_steps = M.as_loop_steps(*steps)
    over = dict(update=('mean', 'sd'), min_weight=4.0)
    start = M.displaced_means(case)
    want = M.train_rounds(*steps, *train_args(case, 3, start, **over))
    mean, sigma, weight, updated, fit, objective, history = decode_train.train_loop(
        *loop_steps, *train_args(case, 3, start, **over))
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    for name, got in (('mean', mean), ('sigma', sigma), ('weight', weight)):
        assert np.array_equal(bits(got), bits(want[name])), name
    assert np.array_equal(updated, want['updated'])
    assert np.array_equal(bits(fit.scale), bits(want['fit']['scale']))
    assert np.array_equal(bits(fit.shift), bits(want['fit']['shift']))
    assert (np.abs(objective - want['objective']) <= 4 * np.spacing(np.abs(want['objective']))).all()
    assert [h['kmers_updated'] for h in history] == [h['kmers_updated'] for h in want['history']]
    assert [h['rms_mean_change'] for h in history] == [h['rms_mean_change'] for h in want['history']]
    assert all(h['parts'] == 1 for h in history) and not np.array_equal(bits(sigma), bits(case['model'][4]))
    # the chain
    m, s, sc, sh = start, np.asarray(case['model'][4]), None, None
    for r in range(3):
        args = list(train_args(case, 1, m, scale=sc, shift=sh, **over))
        args[3] = s
        m, s, w, u, f, obj, _ = decode_train.train_loop(*loop_steps, *args)
        sc, sh = f.scale, f.shift
        assert bits(obj)[0] == bits(objective)[r], r
    assert bits(obj)[1] == bits(objective)[3]
    for got, full in ((m, mean), (s, sigma), (w, weight), (sc, fit.scale), (sh, fit.shift)):
        assert np.array_equal(bits(got), bits(full))
    assert np.array_equal(u, updated)
    # fit = 0: the per-read values stay, and the estimate still carries a DecodeFit
    out = decode_train.train_loop(*loop_steps, *train_args(case, 1, start, fit=0, fit_params=()))
    assert (out[4].scale == 1.0).all() and (out[4].shift == 0.0).all() and out[4].rounds == 0 and out[5].size == 2


def test_bad_arguments():
    from nadavca_amd import decode_train
    good = dict(rounds=1, fit=1, fit_params=('scale',), update=('mean',), min_weight=8.0, min_sigma=0.05, min_events=32)
    assert decode_train.check_args(**good) == (1, 1, ('scale',), ('mean',))
    assert decode_train.check_args(**dict(good, update='sd', fit=0, fit_params=()))[1:] == (0, (), ('sd',))
    for bad in (dict(rounds=0), dict(rounds=1.5), dict(update=()), dict(update=('mean', 'var')), dict(min_weight=0.0),
                dict(min_sigma=float('nan')), dict(min_events=0), dict(fit=-1), dict(fit_params=('table',))):
        with pytest.raises(ValueError):
            decode_train.check_args(**dict(good, **bad))


def test_entry_declared_bound_and_exported():
    import nadavca_amd
    from nadavca_amd import _lib, decode_train, device
    header = open(os.path.join(M.ROOT, 'include', 'nadavca_hip.h')).read()
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail('the library is not built: %s' % _lib.LIB_PATH)
    lib = C.CDLL(_lib.LIB_PATH)
    name = 'nvk_kmer_state_moments_dev'
    m = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert m, '%s is not declared' % name
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(params) == len(args) == 18
    for p, a in zip(params, args):
        want = C.POINTER(C.c_int64) if p.startswith('int64_t *out_parts') else \
            C.POINTER(C.c_double) if p.startswith('double *out_ms') else C.c_void_p if '*' in p else \
            C.c_int64 if p.startswith('int64_t') else C.c_double if p.startswith('double') else C.c_int
        assert a is want, (name, p)
    assert hasattr(lib, name)
    # the arguments are nvk_kmer_expectations_dev's, name for name but the output
    other = re.search(r'int nvk_kmer_expectations_dev\(([^;]*)\);', header).group(1).replace('\n', ' ')
    assert [p.strip() for p in other.split(',')] == [p.replace('out_moments', 'out_stats') for p in params]
    assert callable(device.kmer_state_moments_dev)
    assert nadavca_amd.estimate_decode_model is decode_train.estimate_decode_model
    assert nadavca_amd.DecodeModelEstimate is decode_train.DecodeModelEstimate
    assert 'estimate_decode_model' in nadavca_amd.__all__ and 'DecodeModelEstimate' in nadavca_amd.__all__
