"""The CPU side of the ``decode_batch(fit=n)`` tests: the restatement of tests/host_shims/kmer_fb_host.cpp on numpy
arrays, the rules of nvk_kmer_expectations_dev once more as a log-domain Baum-Welch E-step in plain numpy
(``logaddexp``, no scaling, every move summed at the state it enters; small k), the M-step of
nadavca_amd/decode_fit.py with per-read Python loops, the workflow on ``decode_ref.cpu_decode`` (``cpu_fit``), and the
case drawn from the HMM itself that the CPU tests share."""
import contextlib
import math
import os

import numpy as np

import decode_ref as D
import posterior_ref as P
import signal_map_ref as R

ROOT = R.ROOT
LN2 = math.log(2.0)
Q_FLOOR = 2.0 ** -9
STAT_NAMES = ('M0', 'Mx', 'Mxx', 'Mm', 'Mxm', 'Mmm', 'N_stay', 'N_step', 'N_skip', 'floored')


class ExpectHost:
    def __init__(self, lib):
        self._f = P.sweep_entry(lib, 'kmer_expectations_host')

    def expectations(self, level, ev_off, k, mean, ac, mc, w_stay, w_step, w_skip, status_in=None, threads=1):
        """-> (stats f64 (n, 10), z f64 (n, 2), status i32 (n,)); a read that is not processed has zeros.  ``threads``:
        the reads are independent; more than one spreads them over that many calls at once."""
        n = np.size(ev_off) - 1
        stats = np.zeros((max(n, 1), 10), dtype=np.float64)
        z, status = P.spread_reads(self._f, level, ev_off, k, None, (mean, ac, mc), (w_stay, w_step, w_skip), status_in,
                                   stats, threads)
        return stats[:n], z, status


def build_host(directory):
    return ExpectHost(P.build_shim(directory))


def run_host(host, case, w=None, **kw):
    return P.run_case(host.expectations, case, w, **kw)


def python_expectations(level, k, mean, ac, mc, w_stay, w_step, w_skip):
    """The rules of nvk_kmer_expectations_dev for ONE read with events in the log domain, without scaling: the
    posteriors gamma(i, s) from alpha + beta, and every move's posterior summed at the state it ENTERS (alpha of the
    predecessor, the move's weight, the emission and beta of the entered state) where the kernel sums at the state it
    leaves -> (stats (10,), log Z)"""
    level = np.asarray(level, dtype=np.float64)
    E = level.size
    mean, mc = (np.asarray(x, dtype=np.float64) for x in (mean, mc))
    em, lb, la, lbeta, pred, lw = P.log_alpha_beta(level, k, mean, ac, mc, w_stay, w_step, w_skip)
    g = la + lbeta
    gamma = np.exp(g - np.logaddexp.reduce(g, axis=1)[:, None])
    g0, g1, g2 = (gamma * mc).sum(axis=1), (gamma * mc * mean).sum(axis=1), (gamma * mc * mean * mean).sum(axis=1)
    stats = np.zeros(10)
    stats[:6] = [g0.sum(), (g0 * level).sum(), (g0 * level * level).sum(), g1.sum(), (g1 * level).sum(), g2.sum()]
    if E > 1:
        # (E - 1, 21, S): the move into s at event i + 1 from its predecessor of that row at event i
        xi = la[:-1][:, pred] + lw[None, :, :] + (lb[1:] + lbeta[1:])[:, None, :]
        kind = np.stack([np.logaddexp.reduce(xi[:, rows].reshape(E - 1, -1), axis=1)
                         for rows in (slice(4, 5), slice(0, 4), slice(5, 21))], axis=1)
        stats[6:9] = np.exp(kind - np.logaddexp.reduce(kind, axis=1)[:, None]).sum(axis=0)
    stats[9] = float((em.max(axis=1) <= P.EM_FLOOR).sum())
    return stats, float(np.logaddexp.reduce(la[E - 1]))


# ---- the M-step and the loop, with per-read loops --------------------------------------------------------------------
def m_step(stats, n_events, eligible, params):
    """``decode_fit.m_step`` read by read in Python floats; the pooled sums by ``np.sum`` over the same arrays
    -> (a, b, rho, q or None, used)"""
    n = len(n_events)
    a, b, R, used = np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for r in range(n):
        M0, Mx, Mxx, Mm, Mxm, Mmm = (float(v) for v in stats[r][:6])
        E = float(n_events[r])
        try:
            Vxx = Mxx - Mx * Mx / M0
            Vxm = Mxm - Mx * Mm / M0
            Vmm = Mmm - Mm * Mm / M0
            if 'scale' in params:
                ar = (Vxm + math.sqrt(Vxm * Vxm + 2.0 * E * Vxx)) / (2.0 * Vxx)
                br = (Mm - ar * Mx) / M0
                Rr = ar * ar * Vxx - 2.0 * ar * Vxm + Vmm
            else:
                ar, br, Rr = 1.0, 0.0, Mxx - 2.0 * Mxm + Mmm
        except (ZeroDivisionError, ValueError, OverflowError):
            continue
        good = bool(eligible[r]) and M0 > 0.0 and Vxx > 0.0 and all(math.isfinite(v) for v in (ar, br, Rr)) \
            and all(math.isfinite(float(v)) for v in stats[r][6:9])
        if good:
            a[r], b[r], R[r], used[r] = ar, br, Rr, True
    E = np.asarray(n_events).astype(np.float64)
    rho, q = 1.0, None
    if 'sigma' in params and used.any():
        ratio = 2.0 * np.sum(R[used]) / np.sum(E[used])
        if np.isfinite(ratio) and ratio > 0.0:
            rho = float(np.sqrt(ratio))
    if 'moves' in params and used.any():
        N = np.array([np.sum(np.asarray(stats)[used, 6 + j]) for j in range(3)])
        total = np.sum(N)
        if np.isfinite(total) and total > 0.0:
            q = np.maximum(N / total, Q_FLOOR)
            q = q / np.sum(q)
    return a, b, rho, q, used


def moves_of(q):
    w = np.array([q[0], q[1] / 4.0, q[2] / 16.0])
    total = np.sum(w)
    return float(w[0] / total), float(w[2] / total)


def objective(z, n_events, scale, eligible, p_stay, p_skip):
    """SUM over the eligible reads of log Z - (E - 1) log(w_stay + 4 w_step + 16 w_skip) + E log(scale)"""
    w_stay, w_step, w_skip = P.weights(p_stay, p_skip)
    norm = math.log(w_stay + 4.0 * w_step + 16.0 * w_skip)
    terms = [(math.log(z[r][0]) + z[r][1] * LN2) - (float(n_events[r]) - 1.0) * norm
             + float(n_events[r]) * math.log(scale[r]) for r in range(len(n_events)) if eligible[r]]
    return float(np.sum(np.array(terms)))


def fit_rounds(e_step, n_events, eligible, rounds, params, sigma_scale, p_stay, p_skip, scale=None, shift=None):
    """The loop of ``decode_fit.fit_loop``; ``e_step(scale, shift, sigma_scale, p_stay, p_skip)`` -> (stats, z)
    -> dict of the DecodeFit's fields"""
    n = len(n_events)
    scale = np.ones(n) if scale is None else np.array(scale, dtype=np.float64)
    shift = np.zeros(n) if shift is None else np.array(shift, dtype=np.float64)
    values = []
    for r in range(rounds + 1):
        stats, z = e_step(scale, shift, sigma_scale, p_stay, p_skip)
        values.append(objective(z, n_events, scale, eligible, p_stay, p_skip))
        if r == rounds:
            break
        a, b, rho, q, _ = m_step(stats, n_events, eligible, params)
        scale, shift = a * scale, a * shift + b
        sigma_scale = sigma_scale * rho
        if q is not None:
            p_stay, p_skip = moves_of(q)
    w = P.weights(p_stay, p_skip)
    q = np.array([w[0], 4.0 * w[1], 16.0 * w[2]])
    return dict(scale=scale, shift=shift, sigma_scale=sigma_scale, p_stay=p_stay, p_skip=p_skip, q=q / np.sum(q),
                objective=np.array(values), counts=np.array(stats)[:, 6:9].copy(),
                floored=np.array(stats)[:, 9].astype(np.int64))


def shim_e_step(host, level, ev_off, model, status_in=None, threads=1):
    """-> the ``e_step`` of ``fit_rounds`` on the shim, for stage-2 levels ``level``"""
    k = model[0]
    owner = np.repeat(np.arange(ev_off.size - 1), np.diff(ev_off))

    def e_step(scale, shift, sigma_scale, p_stay, p_skip):
        mean, ac, mc = D.state_tables(model, sigma_scale)
        stats, z, _ = host.expectations(level * scale[owner] + shift[owner], ev_off, k, mean, ac, mc,
                                        *P.weights(p_stay, p_skip), status_in=status_in, threads=threads)
        return stats, z
    return e_step


def numpy_e_step(level, ev_off, model):
    """... and on ``python_expectations``, read by read"""
    k = model[0]

    def e_step(scale, shift, sigma_scale, p_stay, p_skip):
        mean, ac, mc = D.state_tables(model, sigma_scale)
        out = [python_expectations(level[ev_off[r]:ev_off[r + 1]] * scale[r] + shift[r], k, mean, ac, mc,
                                   *P.weights(p_stay, p_skip)) for r in range(ev_off.size - 1)]
        return np.array([o[0] for o in out]), np.array([[math.exp(o[1] - LN2 * math.floor(o[1] / LN2)),
                                                         math.floor(o[1] / LN2)] for o in out])
    return e_step


@contextlib.contextmanager
def _events_replaced(events):
    """``decode_ref.cpu_decode`` with its stages 1 and 2 answered by ``events``: the way to run its stages 3 and 4 on
    levels that another stage has moved"""
    kept = D.cpu_events
    D.cpu_events = lambda *args, **kw: events
    try:
        yield
    finally:
        D.cpu_events = kept


def cpu_fit(map_host, dec_host, exp_host, raw, sig_off, model, rounds, params=('scale', 'sigma', 'moves'), p_stay=0.7,
            p_skip=0.01, sigma_scale=1.0, threads=None, post_host=None, start=None):
    """``decode_batch(fit=rounds)`` on the CPU: stages 1 and 2 of ``decode_ref``, the rounds on the shim, then
    ``decode_ref.cpu_decode`` (and, with ``post_host``, ``posterior_ref.cpu_qualities``) on the fitted levels, sigma and
    weights.  ``start``: a fit dict whose scale and shift the reads start from
    -> (the fit as a dict, cpu_decode's dict, cpu_qualities' dict or None)"""
    threads = min(16, os.cpu_count() or 1) if threads is None else threads
    scaled, ev_off, ev_start, status_in = D.cpu_events(map_host, raw, sig_off, model)
    n_events, eligible = np.diff(ev_off), status_in == 0
    fit = fit_rounds(shim_e_step(exp_host, scaled, ev_off, model, status_in, threads), n_events, eligible, rounds,
                     params, sigma_scale, p_stay, p_skip, None if start is None else start['scale'],
                     None if start is None else start['shift'])
    owner = np.repeat(np.arange(ev_off.size - 1), n_events)
    fitted = scaled * fit['scale'][owner] + fit['shift'][owner]
    kw = dict(p_stay=fit['p_stay'], p_skip=fit['p_skip'])
    with _events_replaced((fitted, ev_off, ev_start, status_in)):
        res = D.cpu_decode(map_host, dec_host, raw, sig_off, model, sigma_scale=fit['sigma_scale'], threads=threads,
                           **kw)
    # (cpu_qualities takes the table from ``res``, which cpu_decode formed at the fitted sigma)
    qual = None if post_host is None else P.cpu_qualities(post_host, res, model, threads=threads, **kw)
    return fit, res, qual


# ---- the case drawn from the HMM itself ------------------------------------------------------------------------------
HMM_Q = (0.5, 0.45, 0.05)


def hmm_case(n=30, n_events=200, k=3, seed=5):
    """``n`` reads of ``n_events`` events drawn from the k-mer HMM of a random table with the move shares HMM_Q, each
    seen through its own scale and shift: the truth is x = alpha_true y + beta_true.  Stage 2's median / MAD rescale of
    y is the start.  -> dict: model, level (the stage-2 levels), ev_off, start_scale / start_shift (stage 2's, on y),
    true_scale / true_shift (on y)"""
    from nadavca_amd import synthetic
    rng = np.random.default_rng(seed)
    model = synthetic.synth_model_arrays(seed=40 + k, k=k, central=0)
    mean, sd = np.asarray(model[3]), np.asarray(model[4])
    S = 4 ** k
    med_l, mad_l = R.median_mad(mean)
    levels, start_scale, start_shift, true_scale, true_shift = [], [], [], [], []
    for _ in range(n):
        s, x = int(rng.integers(0, S)), []
        for i in range(n_events):
            if i:
                move = rng.choice(3, p=HMM_Q)
                for _ in range(move):
                    s = (s * 4 + int(rng.integers(0, 4))) % S
            x.append(rng.normal(mean[s], sd[s]))
        alpha, beta = float(rng.uniform(0.8, 1.25)), float(rng.normal(0.0, 0.3))
        y = (np.array(x) - beta) / alpha
        med_e, mad_e = R.median_mad(y)
        levels.append((y - med_e) * (mad_l / mad_e) + med_l)
        start_scale.append(mad_l / mad_e)
        start_shift.append(med_l - med_e * (mad_l / mad_e))
        true_scale.append(alpha)
        true_shift.append(beta)
    arr = lambda v: np.array(v, dtype=np.float64)
    return dict(model=model, level=np.concatenate(levels), ev_off=R.offsets([n_events] * n),
                start_scale=arr(start_scale), start_shift=arr(start_shift), true_scale=arr(true_scale),
                true_shift=arr(true_shift))


def rms_errors(case, scale, shift):
    """The total scale and shift on y (stage 2's composed with the fit's) against the truth -> (RMS of
    total_scale / true_scale - 1, RMS of total_shift - true_shift)"""
    total_scale = scale * case['start_scale']
    total_shift = scale * case['start_shift'] + shift
    rel = total_scale / case['true_scale'] - 1.0
    return float(np.sqrt(np.mean(rel * rel))), float(np.sqrt(np.mean((total_shift - case['true_shift']) ** 2)))
