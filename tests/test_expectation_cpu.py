"""The rules of ``decode_batch(fit=n)`` without a GPU: the C++ restatement of nvk_kmer_expectations_dev against a
log-domain Baum-Welch E-step in plain numpy, the identities that tie its counts and moments to derivatives of log Z,
the M-step of nadavca_amd/decode_fit.py against its own expected log-likelihood and against a restatement with per-read
loops, and the fit as a whole on reads drawn from the HMM itself."""
import math

import numpy as np
import pytest

import decode_ref as D
import expect_ref as X
import posterior_ref as P

# The shim against the log-domain restatement, every stat as |difference| / max(1, |value|).  Measured on the cases of
# the first test: 8.6e-15 at the most (N_skip at k = 3; the moments within 5.7e-15), log Z within 7.2e-15 (7.11e-15); the
# allowance is 10 times the measured figure.
TOL_STATS = 8.6e-14
TOL_LOGZ = 7.2e-14
EPS = float(np.finfo(np.float64).eps)
H = 1e-5


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return X.build_host(tmp_path_factory.mktemp('expect_host'))


@pytest.fixture(scope='module')
def hmm():
    return X.hmm_case()


@pytest.fixture(scope='module')
def shim_fit(host, hmm):
    """8 rounds on the shim from the median / MAD start -> the fit dict"""
    n = hmm['ev_off'].size - 1
    return X.fit_rounds(X.shim_e_step(host, hmm['level'], hmm['ev_off'], hmm['model'], threads=8),
                        np.diff(hmm['ev_off']), np.ones(n, bool), 8, ('scale', 'sigma', 'moves'), 1.0, 0.7, 0.01)


def reads_of(case):
    off = case['ev_off']
    return [case['level'][off[r]:off[r + 1]] for r in range(off.size - 1)]


@pytest.mark.parametrize('name,case', P.small_cases(), ids=[c[0] for c in P.small_cases()])
def test_shim_equals_the_log_domain_baum_welch(host, name, case):
    """k = 2 and 3, reads of 1, 2, 3 and 65 events: the ten stats and log Z.  Measured: the stats within 8.6e-15 of
    max(1, |value|) (k = 2: 1.4e-15), log Z within 7.2e-15; allowed: 10 times that (TOL_STATS 8.6e-14, TOL_LOGZ
    7.2e-14)."""
    w = tuple(math.exp(c) for c in case['costs'])
    stats, z, status = X.run_host(host, case)
    assert (status == 0).all()
    worst = [0.0, 0.0]
    for r, level in enumerate(reads_of(case)):
        want, want_z = X.python_expectations(level, case['k'], case['mean'], case['ac'], case['mc'], *w)
        worst[0] = max(worst[0], float((np.abs(stats[r] - want) / np.maximum(1.0, np.abs(want))).max()))
        worst[1] = max(worst[1], abs(float(P.log_z(z[r])[0]) - want_z))
    print('%s: largest difference of a stat %.3g, of log Z %.3g' % (name, worst[0], worst[1]))
    assert worst[0] <= TOL_STATS and worst[1] <= TOL_LOGZ, worst


def test_z_and_status_are_the_posterior_shims(host, tmp_path):
    post = P.build_host(tmp_path)
    for name, case in P.small_cases() + P.extreme_cases() + D.kernel_cases(3)[:1]:
        stats, z, status = X.run_host(host, case)
        _, want_z, want_status = P.run_host(post, case, 0)
        assert np.array_equal(z.view(np.int64), want_z.view(np.int64)) and np.array_equal(status, want_status), name
        assert (stats[status != 0] == 0.0).all(), name


def test_the_moves_sum_to_the_events_less_one(host):
    """The three shares of a move sum to 1 within 2 eps (two additions of values below 1, three divisions), and each of
    the three accumulators rounds E - 1 times on partial sums below E: |N_stay + N_step + N_skip - (E - 1)| <= 2 eps E +
    1.5 eps E^2 (3e-11 at E = 300; measured: 4.0e-13 at the most, on the 300 events of the narrow-sigma case)."""
    for name, case in P.small_cases() + P.extreme_cases() + D.kernel_cases(4)[:1]:
        stats, _, status = X.run_host(host, case)
        E = np.diff(case['ev_off']).astype(np.float64)
        done = status == 0
        total = (stats[:, 6] + stats[:, 7]) + stats[:, 8]
        gap = np.abs(total[done] - (E[done] - 1.0))
        print('%s: N sums off by %.3g at the most' % (name, gap.max()))
        assert (gap <= 2 * EPS * E[done] + 1.5 * EPS * E[done] * E[done]).all(), name
        assert (stats[done, 6:9] >= 0.0).all() and (stats[done, 0] > 0.0).all(), name


def test_counts_and_moments_are_derivatives_of_log_z(host):
    """On the 65-event read at k = 3, where no event sits on the floor (asserted): d log Z / d log w_kind = N_kind, and
    d log Z / d beta at the levels x + beta equals -2 (Mx - Mm), both by central differences at h = 1e-5.  Allowed:
    h^2 E for the truncation (h^2 / 6 times a third derivative, which for a sum over E events is below 6 E times the
    largest per-event factor: 1 for the counts, (2 mc |x - mean|)^3 <= 8 mc_max^3 d_max^3 with d_max the widest
    level-to-mean distance for beta) plus 2 eps |log Z| / h for the rounding of the two values of log Z."""
    name, case = P.small_cases()[1]
    off = case['ev_off']
    one = D.pack([case['level'][off[3]:off[4]]], case['k'], 0, (case['mean'], case['ac'], case['mc']), case['costs'])
    E = 65
    assert one['level'].size == E
    w = [math.exp(c) for c in one['costs']]
    stats, z, _ = X.run_host(host, one, tuple(w))
    assert stats[0, 9] == 0.0
    lz = lambda **kw: float(P.log_z(X.run_host(host, dict(one, **kw.pop('case', {})), **kw)[1])[0])
    round_off = 2 * EPS * abs(float(P.log_z(z)[0])) / H
    for kind in range(3):
        up, down = list(w), list(w)
        up[kind], down[kind] = w[kind] * math.exp(H), w[kind] * math.exp(-H)
        slope = (lz(w=tuple(up)) - lz(w=tuple(down))) / (2 * H)
        print('d log Z / d log w[%d] = %.9f, N = %.9f' % (kind, slope, stats[0, 6 + kind]))
        assert abs(slope - stats[0, 6 + kind]) <= H * H * E + round_off
    slope = (lz(case=dict(level=one['level'] + H), w=tuple(w)) - lz(case=dict(level=one['level'] - H), w=tuple(w))) \
        / (2 * H)
    want = -2.0 * (stats[0, 1] - stats[0, 3])
    factor = (2.0 * one['mc'].max() * np.abs(one['level'][:, None] - one['mean'][None, :]).max()) ** 3
    print('d log Z / d beta = %.9f, -2 (Mx - Mm) = %.9f' % (slope, want))
    assert abs(slope - want) <= H * H * E * max(1.0, factor) + round_off


def expected_loglik(stats, n_events, a, b, rho, q):
    """The expected log-likelihood the M-step raises, up to a constant, as a function of the per-read increments, the
    factor on sigma and the shares: SUM E log a - E log rho - (the weighted residual at (a, b)) / rho^2, and
    SUM N_kind log q_kind"""
    M0, Mx, Mxx, Mm, Mxm, Mmm = (stats[:, j] for j in range(6))
    E = n_events.astype(np.float64)
    resid = a * a * Mxx + 2 * a * b * Mx + b * b * M0 - 2 * a * Mxm - 2 * b * Mm + Mmm
    return float(np.sum(E * np.log(a) - E * math.log(rho) - resid / (rho * rho))
                 + np.sum(stats[:, 6:9].sum(axis=0) * np.log(q)))


def test_m_step_maximises_its_expected_loglik_and_equals_the_loops(host, hmm):
    """The M-step is three conditional maximisations: (a, b) of every read at rho = 1, rho at the new (a, b), and q.
    At each of them every coordinate perturbation (a factor 1 +- 1e-3, for b a step of +- 1e-3, for q a move of 1e-3 of
    the smallest share between two kinds) lowers the expected
    log-likelihood.  The vectorised M-step and the one with per-read loops agree bit for bit."""
    from nadavca_amd import decode_fit
    n = hmm['ev_off'].size - 1
    n_events, ok = np.diff(hmm['ev_off']), np.ones(n, bool)
    stats, _ = X.shim_e_step(host, hmm['level'], hmm['ev_off'], hmm['model'], threads=8)(np.ones(n), np.zeros(n), 1.0,
                                                                                         0.7, 0.01)
    params = ('scale', 'sigma', 'moves')
    a, b, rho, q, used = decode_fit.m_step(stats, n_events, ok, params)
    for got, want in zip((a, b, np.float64(rho), q, used), X.m_step(stats, n_events, ok, params)):
        assert np.array_equal(np.asarray(got), np.asarray(want))
    assert used.all() and (q > decode_fit.Q_FLOOR).all() and abs(q.sum() - 1.0) < 4 * EPS
    best = expected_loglik(stats, n_events, a, b, 1.0, q)
    d = 1e-3
    for r in range(n):
        for f in (1 - d, 1 + d):
            moved = a.copy()
            moved[r] *= f
            assert expected_loglik(stats, n_events, moved, b, 1.0, q) < best, ('a', r, f)
            moved = b.copy()
            moved[r] += d if f > 1 else -d
            assert expected_loglik(stats, n_events, a, moved, 1.0, q) < best, ('b', r, f)
    best = expected_loglik(stats, n_events, a, b, rho, q)
    for f in (1 - d, 1 + d):
        assert expected_loglik(stats, n_events, a, b, rho * f, q) < best, ('rho', f)
    for i in range(3):
        for j in range(3):
            if i != j:
                moved = q.copy()
                moved[i], moved[j] = moved[i] - d * q.min(), moved[j] + d * q.min()
                assert expected_loglik(stats, n_events, a, b, rho, moved) < best, ('q', i, j)
    # a group that is not fitted stays: no scale, no sigma, no moves
    a1, b1, rho1, q1, _ = decode_fit.m_step(stats, n_events, ok, ('sigma',))
    assert (a1 == 1.0).all() and (b1 == 0.0).all() and q1 is None and rho1 != 1.0
    a2, b2, rho2, q2, _ = decode_fit.m_step(stats, n_events, ok, ('scale',))
    assert np.array_equal(a2, a) and np.array_equal(b2, b) and rho2 == 1.0 and q2 is None
    # a read with a zero M0, a read that is not eligible: both keep their values and stay out of the pooled sums
    broken = stats.copy()
    broken[0, :6] = 0.0
    a3, b3, rho3, q3, used3 = decode_fit.m_step(broken, n_events, np.arange(n) != 1, params)
    assert used3.tolist() == [False, False] + [True] * (n - 2) and a3[0] == a3[1] == 1.0 and b3[0] == b3[1] == 0.0
    for got, want in zip((a3, b3, np.float64(rho3), q3, used3), X.m_step(broken, n_events, np.arange(n) != 1, params)):
        assert np.array_equal(np.asarray(got), np.asarray(want))


def test_objective_does_not_fall_over_eight_rounds(shim_fit):
    """30 reads of 200 events drawn from the k = 3 HMM with q = (0.5, 0.45, 0.05): the objective of every round is at
    least the one before, less 1e-9 of its size.  Measured: it rises from -7875.52 to -7551.57, by 157.1 in the first
    round and 4.7 in the last."""
    obj = shim_fit['objective']
    print('objective per round:', ' '.join('%.4f' % v for v in obj))
    assert obj.size == 9 and np.isfinite(obj).all()
    assert (np.diff(obj) >= -1e-9 * np.abs(obj[:-1])).all(), np.diff(obj).tolist()


def test_fit_recovers_scale_and_shift_of_reads_drawn_from_the_hmm(host, hmm, shim_fit):
    """The same case: the RMS error of the total per-read scale (relative) and shift against the truth after 8 rounds
    is at most what the log-domain numpy EM reaches from the same start, plus 10 %, and strictly below the start's.
    Measured: scale 0.1174 (median / MAD start) -> 0.0409 (shim) and 0.0409 (numpy EM); shift 0.1580 -> 0.1071 and
    0.1071; the pooled sigma factor returns to 1.006 and q to (0.497, 0.436, 0.067)."""
    n = hmm['ev_off'].size - 1
    ref = X.fit_rounds(X.numpy_e_step(hmm['level'], hmm['ev_off'], hmm['model']), np.diff(hmm['ev_off']),
                       np.ones(n, bool), 8, ('scale', 'sigma', 'moves'), 1.0, 0.7, 0.01)
    start = X.rms_errors(hmm, np.ones(n), np.zeros(n))
    got = X.rms_errors(hmm, shim_fit['scale'], shim_fit['shift'])
    want = X.rms_errors(hmm, ref['scale'], ref['shift'])
    print('RMS error of scale: start %.4f, shim %.4f, numpy EM %.4f; of shift: %.4f, %.4f, %.4f; sigma factor %.4f; q %s'
          % (start[0], got[0], want[0], start[1], got[1], want[1], shim_fit['sigma_scale'], shim_fit['q'].round(4)))
    for which in range(2):
        assert got[which] <= 1.1 * want[which] and got[which] < start[which], (which, start, got, want)
    assert (shim_fit['floored'] == 0).all()
    assert np.abs(shim_fit['counts'].sum(axis=1) - 199.0).max() < 1e-9


def test_the_loop_equals_the_restatement(host):
    """``decode_fit.fit_loop`` and ``expect_ref.fit_rounds`` on the same E-step (the shim, 6 reads drawn from the HMM, two
    rounds): every field bit for bit, the objective within 4 ulp (its terms pass through numpy's log there and Python's
    here, as on the device)."""
    from nadavca_amd import decode_fit
    case = X.hmm_case(n=6)
    n_events, ok = np.diff(case['ev_off']), np.ones(6, bool)
    e_step = X.shim_e_step(host, case['level'], case['ev_off'], case['model'])
    args = (n_events, ok, 2, ('scale', 'sigma', 'moves'), 1.0, 0.7, 0.01)
    want = X.fit_rounds(e_step, *args)
    got = decode_fit.fit_loop(lambda *values: e_step(*values) + (1,), *args)
    for name in ('scale', 'shift', 'q', 'counts', 'floored'):
        assert np.array_equal(getattr(got, name), want[name]), name
    assert (got.sigma_scale, got.p_stay, got.p_skip) == (want['sigma_scale'], want['p_stay'], want['p_skip'])
    assert got.rounds == 2 and got.parts == 1
    assert (np.abs(got.objective - want['objective']) <= 4 * np.spacing(np.abs(want['objective']))).all()
    # where the reads start: one round, then one more from its values, is two rounds
    one = decode_fit.fit_loop(lambda *values: e_step(*values) + (1,), n_events, ok, 1, *args[3:])
    then = decode_fit.fit_loop(lambda *values: e_step(*values) + (1,), n_events, ok, 1, args[3], one.sigma_scale,
                               one.p_stay, one.p_skip, one.scale, one.shift)
    assert np.array_equal(then.scale, got.scale) and np.array_equal(then.shift, got.shift)
    assert np.array_equal(then.objective, got.objective[1:]) and then.sigma_scale == got.sigma_scale
