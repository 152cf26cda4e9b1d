"""The CPU side of the ``estimate_decode_model`` tests: the restatement of tests/host_shims/kmer_fb_host.cpp on numpy
arrays, the rules of nvk_kmer_state_moments_dev once more as a log-domain forward-backward in plain numpy
(``logaddexp``, no scaling; small k), the M-step and the loop of nadavca_amd/decode_train.py with per-state Python
loops, the workflow on ``decode_ref.cpu_events`` (``cpu_train``), and the displaced table of the HMM case that the
tests share."""
import ctypes as C
import math
import os

import numpy as np

import decode_ref as D
import expect_ref as X
import posterior_ref as P
import signal_map_ref as R

ROOT = R.ROOT


class MomentsHost:
    def __init__(self, lib):
        self._f = P.sweep_entry(lib, 'kmer_state_moments_host')
        self._total = lib.state_moments_total_host
        self._total.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 3
        self._total.restype = None

    def moments(self, level, ev_off, k, mean, ac, mc, w_stay, w_step, w_skip, status_in=None, threads=1):
        """-> (moments f64 (3, S): the batch's totals; z f64 (n, 2); status i32 (n,); per_read f64 (n, 3, S): every
        read's own G, zeros for a read that is not processed).  ``threads``: the reads are independent up to the
        totals; more than one spreads them over that many calls at once."""
        n, S = np.size(ev_off) - 1, 4 ** k
        per_read = np.zeros((max(n, 1), 3, S), dtype=np.float64)
        z, status = P.spread_reads(self._f, level, ev_off, k, None, (mean, ac, mc), (w_stay, w_step, w_skip), status_in,
                                   per_read, threads)
        total = np.zeros((3, S), dtype=np.float64)
        self._total(n, 3 * S, per_read.ctypes.data, np.ascontiguousarray(status).ctypes.data, total.ctypes.data)
        return total, z, status, per_read[:n]


def build_host(directory):
    return MomentsHost(P.build_shim(directory))


def run_host(host, case, w=None, **kw):
    return P.run_case(host.moments, case, w, **kw)


def python_moments(level, k, mean, ac, mc, w_stay, w_step, w_skip):
    """The rules of nvk_kmer_state_moments_dev for ONE read with events in the log domain, without scaling: the
    posteriors gamma(i, s) from alpha + beta, and their sums over the events -> (G (3, S), log Z)"""
    level = np.asarray(level, dtype=np.float64)
    _, _, la, lbeta, _, _ = P.log_alpha_beta(level, k, mean, ac, mc, w_stay, w_step, w_skip)
    g = la + lbeta
    gamma = np.exp(g - np.logaddexp.reduce(g, axis=1)[:, None])
    G = np.stack([gamma.sum(axis=0), (gamma * level[:, None]).sum(axis=0),
                  (gamma * level[:, None] * level[:, None]).sum(axis=0)])
    return G, float(np.logaddexp.reduce(la[-1]))


# ---- the M-step and the loop, with per-state loops -------------------------------------------------------------------
def m_step(moments, mean, sigma, c, update, min_weight, min_sigma):
    """``decode_train.m_step`` state by state in Python floats -> (mean, sigma, updated)"""
    S = len(mean)
    new_mean, new_sigma = np.array(mean, dtype=np.float64), np.array(sigma, dtype=np.float64)
    updated = np.zeros(S, dtype=bool)
    for s in range(S):
        G0, G1, G2 = (float(moments[m][s]) for m in range(3))
        if not G0 >= min_weight:
            continue
        m = G1 / G0
        var = G2 / G0 - m * m
        sd = max(math.sqrt(max(var, 0.0)) / c, min_sigma)
        if not (math.isfinite(m) and math.isfinite(sd)):
            continue
        updated[s] = True
        if 'mean' in update:
            new_mean[s] = m
        if 'sd' in update:
            new_sigma[s] = sd
    return new_mean, new_sigma, updated


def train_rounds(fit_e_step, moments_step, n_events, eligible, mean, sigma, rounds, fit, fit_params, update,
                 min_weight, min_sigma, sigma_scale, p_stay, p_skip, scale=None, shift=None):
    """The loop of ``decode_train.train_loop`` on ``expect_ref.fit_rounds``; ``fit_e_step(mean, sigma)`` -> the
    ``e_step`` of ``fit_rounds`` ((stats, z)), ``moments_step(...)`` -> (moments, z) -> dict of the estimate's fields"""
    n = len(n_events)
    mean, sigma = np.array(mean, dtype=np.float64), np.array(sigma, dtype=np.float64)
    scale = np.ones(n) if scale is None else np.array(scale, dtype=np.float64)
    shift = np.zeros(n) if shift is None else np.array(shift, dtype=np.float64)
    values, history, last = [], [], None
    weight, updated = np.zeros(mean.size), np.zeros(mean.size, dtype=bool)
    for _ in range(rounds):
        if fit > 0:
            last = X.fit_rounds(fit_e_step(mean, sigma), n_events, eligible, fit, fit_params, sigma_scale, p_stay, p_skip,
                                scale, shift)
            scale, shift = last['scale'], last['shift']
            sigma_scale, p_stay, p_skip = last['sigma_scale'], last['p_stay'], last['p_skip']
        moments, z = moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip)
        values.append(X.objective(z, n_events, scale, eligible, p_stay, p_skip))
        new_mean, new_sigma, updated = m_step(moments, mean, sigma, sigma_scale, update, min_weight, min_sigma)
        moved = [float(new_mean[s] - mean[s]) ** 2 for s in range(mean.size) if updated[s]]
        history.append(dict(kmers_updated=len(moved),
                            rms_mean_change=float(np.sqrt(np.mean(np.array(moved)))) if moved else 0.0))
        weight = np.array(moments[0], dtype=np.float64)
        mean, sigma = new_mean, new_sigma
    _, z = moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip)
    values.append(X.objective(z, n_events, scale, eligible, p_stay, p_skip))
    if last is None:
        last = X.fit_rounds(fit_e_step(mean, sigma), n_events, eligible, 0, fit_params, sigma_scale, p_stay, p_skip,
                            scale, shift)
    return dict(mean=mean, sigma=sigma, weight=weight, updated=updated, fit=last, objective=np.array(values),
                history=history)


def tables_of(k, mean, sigma):
    """A table as the model tuple ``decode_ref.state_tables`` reads (k, central, alphabet, mean, sigma)"""
    return (k, 0, 4, mean, sigma)


def shim_steps(exp_host, mom_host, level, ev_off, k, status_in=None, threads=1):
    """-> (fit_e_step, moments_step) of ``train_rounds`` on the two shims, for stage-2 levels ``level``"""
    owner = np.repeat(np.arange(ev_off.size - 1), np.diff(ev_off))

    def fit_e_step(mean, sigma):
        return X.shim_e_step(exp_host, level, ev_off, tables_of(k, mean, sigma), status_in, threads)

    def moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip):
        m, ac, mc = D.state_tables(tables_of(k, mean, sigma), sigma_scale)
        total, z, _, _ = mom_host.moments(level * scale[owner] + shift[owner], ev_off, k, m, ac, mc,
                                          *P.weights(p_stay, p_skip), status_in=status_in, threads=threads)
        return total, z
    return fit_e_step, moments_step


def numpy_steps(level, ev_off, k):
    """... and on ``expect_ref.python_expectations`` and ``python_moments``, read by read, the totals by ``np.sum``"""
    n = ev_off.size - 1

    def fit_e_step(mean, sigma):
        return X.numpy_e_step(level, ev_off, tables_of(k, mean, sigma))

    def moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip):
        m, ac, mc = D.state_tables(tables_of(k, mean, sigma), sigma_scale)
        out = [python_moments(level[ev_off[r]:ev_off[r + 1]] * scale[r] + shift[r], k, m, ac, mc,
                              *P.weights(p_stay, p_skip)) for r in range(n)]
        z = np.array([[math.exp(o[1] - X.LN2 * math.floor(o[1] / X.LN2)), math.floor(o[1] / X.LN2)] for o in out])
        return np.sum(np.array([o[0] for o in out]), axis=0), z
    return fit_e_step, moments_step


def as_loop_steps(fit_e_step, moments_step, parts=1):
    """The steps of ``train_rounds`` as ``decode_train.train_loop`` takes them: every E-step also says its parts"""
    return (lambda mean, sigma: (lambda *values: fit_e_step(mean, sigma)(*values) + (parts,)),
            lambda *values: moments_step(*values) + (parts,))


def cpu_train(map_host, exp_host, mom_host, raw, sig_off, model, rounds, fit=1, fit_params=('scale',),
              update=('mean',), min_weight=8.0, min_sigma=0.05, p_stay=0.7, p_skip=0.01, sigma_scale=1.0, threads=None,
              start=None, anchor=None):
    """``estimate_decode_model`` on the CPU: stages 1 and 2 of ``decode_ref`` against the start table (or ``anchor``,
    the means an earlier call rescaled onto), then the rounds on the shims -> (the dict of ``train_rounds``, the
    stage-2 results (scaled, ev_off, ev_start, status_in))"""
    threads = min(16, os.cpu_count() or 1) if threads is None else threads
    k = model[0]
    target = model if anchor is None else tables_of(k, anchor, model[4])
    events = D.cpu_events(map_host, raw, sig_off, target)
    scaled, ev_off, _, status_in = events
    steps = shim_steps(exp_host, mom_host, scaled, ev_off, k, status_in, threads)
    out = train_rounds(*steps, np.diff(ev_off), status_in == 0, model[3], model[4], rounds, fit, fit_params, update,
                       min_weight, min_sigma, sigma_scale, p_stay, p_skip, None if start is None else start['scale'],
                       None if start is None else start['shift'])
    return out, events


# ---- the displaced table of the HMM case ----------------------------------------------------------------------------
DISPLACE = 0.15   # the standard deviation of the displacement, in units of the spread (standard deviation) of the means


def displaced_means(case, seed=7):
    """The true means of an ``expect_ref.hmm_case`` moved by N(0, (DISPLACE * spread)^2) -> the start table's means"""
    true = np.asarray(case['model'][3], dtype=np.float64)
    rng = np.random.default_rng(seed)
    return true + rng.normal(0.0, DISPLACE * float(np.std(true)), true.size)


def mean_errors(true, mean):
    """-> (the RMS of mean - true; the same after the best affine map a * mean + b onto ``true``, by least squares)"""
    true, mean = np.asarray(true, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    raw = float(np.sqrt(np.mean((mean - true) ** 2)))
    a, b = np.polyfit(mean, true, 1)
    return raw, float(np.sqrt(np.mean((a * mean + b - true) ** 2)))
