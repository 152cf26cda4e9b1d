"""The CPU side of the posterior tests: the restatement of tests/host_shims/kmer_fb_host.cpp on numpy arrays (the shim,
the spreading of reads over threads and the log-domain alpha and beta serve expect_ref and moments_ref too), the rules
of nvk_kmer_posterior_dev once more as a log-domain forward-backward in plain numpy (``logaddexp``, no scaling; small
k), what ``decode_batch(qualities=True)`` does with the operator's outputs in numpy with per-read loops
(``cpu_qualities``), the measures of the quality claim, and the constructed cases the test files share."""
import ctypes as C
import math
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import decode_ref as D
import signal_map_ref as R

ROOT = R.ROOT
LN2 = math.log(2.0)
EM_FLOOR = -300.0
# quality[b] = the number of these that base_post[b] reaches: 1 - 10^(-j / 10), j = 1..60
THRESHOLDS = 1.0 - np.power(10.0, -np.arange(1, 61, dtype=np.float64) / 10.0)
PHRED_BINS = [(0, 1), (1, 2), (2, 3), (3, 5), (5, 10), (10, 20), (20, 61)]   # [lo, hi) on the integer quality

_p = lambda x: x.ctypes.data
_a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)


def weights(p_stay, p_skip):
    """-> (w_stay, w_step, w_skip): the numbers whose logs ``decode_ref.transition_costs`` takes"""
    return p_stay, 1.0 - p_stay - p_skip, p_skip


def build_shim(directory):
    """tests/host_shims/kmer_fb_host.cpp, compiled once per directory -> the CDLL"""
    so = os.path.join(str(directory), 'kmer_fb_host.so')
    if not os.path.exists(so):
        subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
                        os.path.join(ROOT, 'tests', 'host_shims', 'kmer_fb_host.cpp'), '-o', so], check=True)
    return C.CDLL(so)


def sweep_entry(lib, name, pos=False):
    """An entry of the shim that takes the sweeps' arguments (``pos``: after k, as the posterior entry does)"""
    f = getattr(lib, name)
    f.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_int] * pos + [C.c_void_p] * 3 \
        + [C.c_double] * 3 + [C.c_void_p] * 4
    f.restype = None
    return f


def spread_reads(f, level, ev_off, k, pos, tables, w, status_in, out, threads):
    """An entry of ``sweep_entry`` on a batch.  ``out``: the entry's own output, zeroed; indexed by read unless it is
    per event (the posterior's marginals, ``pos`` not None).  ``threads``: the reads are independent; more than one
    spreads them over that many calls at once -> (z f64 (n, 2), status i32 (n,))"""
    level, mean, ac, mc = (_a(x, np.float64) for x in (level,) + tuple(tables))
    ev_off = _a(ev_off, np.int64)
    n = ev_off.size - 1
    z, status = np.zeros((max(n, 1), 2), dtype=np.float64), np.zeros(max(n, 1), dtype=np.int32)
    st = None if status_in is None else _a(status_in, np.int32)

    def run(lo, hi):
        # (the offsets stay the batch's: the call starts at read lo of every per-read array)
        f(hi - lo, _p(level), _p(ev_off[lo:]), k, *(() if pos is None else (pos,)), _p(mean), _p(ac), _p(mc), *w,
          None if st is None else _p(st[lo:]), _p(out if pos is not None else out[lo:]), _p(z[lo:]), _p(status[lo:]))

    if threads <= 1 or n < 2:
        run(0, n)
    else:
        cuts = [n * t // (4 * threads) for t in range(4 * threads + 1)]
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(lambda c: run(*c), [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]))
    return z[:n], status[:n]


class PosteriorHost:
    def __init__(self, lib):
        self._f = sweep_entry(lib, 'kmer_posterior_host', pos=True)

    def posterior(self, level, ev_off, k, pos, mean, ac, mc, w_stay, w_step, w_skip, status_in=None, threads=1):
        """-> (marg f64 (events, 4), z f64 (n, 2), status i32 (n,)).  ``threads``: the reads are independent; more than
        one spreads them over that many calls at once."""
        events = np.size(level)
        marg = np.zeros((max(events, 1), 4), dtype=np.float64)
        z, status = spread_reads(self._f, level, ev_off, k, pos, (mean, ac, mc), (w_stay, w_step, w_skip), status_in,
                                 marg, threads)
        return marg[:events], z, status


def build_host(directory):
    return PosteriorHost(build_shim(directory))


def run_case(method, case, w=None, pos=None, **kw):
    """A shim's method on a case of ``decode_ref.pack``; the weights default to exp of the case's costs"""
    w = tuple(math.exp(c) for c in case['costs']) if w is None else w
    return method(case['level'], case['ev_off'], case['k'], *(() if pos is None else (pos,)), case['mean'], case['ac'],
                  case['mc'], *w, status_in=case['status_in'], **kw)


def run_host(host, case, pos, w=None, **kw):
    return run_case(host.posterior, case, w, pos, **kw)


def log_z(z):
    """log Z of the reads from the operator's (sum, exponent) pairs"""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide='ignore'):
        return np.log(z[:, 0]) + z[:, 1] * LN2


def log_alpha_beta(level, k, mean, ac, mc, w_stay, w_step, w_skip):
    """The forward-backward of the three operators for ONE read with events in the log domain, without scaling: every
    predecessor and successor of every state looked up flat and joined by logaddexp -> (em (E, S) before the floor, lb
    after it, log alpha, log beta, pred (21, S): per move the state it comes from, lw (21, 1): the moves' log
    weights)"""
    level = np.asarray(level, dtype=np.float64)
    E, S = level.size, 4 ** k
    mean, ac, mc = (np.asarray(x, dtype=np.float64) for x in (mean, ac, mc))
    s = np.arange(S)
    pred = np.stack([a * 4 ** (k - 1) + s // 4 for a in range(4)] + [s] + [c * 4 ** (k - 2) + s // 16 for c in range(16)])
    lw = np.log(np.array([w_step] * 4 + [w_stay] + [w_skip] * 16))[:, None]
    em = ac[None, :] - ((level[:, None] - mean[None, :]) * (level[:, None] - mean[None, :])) * mc[None, :]
    lb = np.maximum(em, EM_FLOOR)
    la = np.zeros((E, S))
    la[0] = lb[0]
    for i in range(1, E):
        la[i] = np.logaddexp.reduce(la[i - 1][pred] + lw, axis=0) + lb[i]
    lbeta = np.zeros((E, S))
    for i in range(E - 2, -1, -1):
        # beta(i, p) = sum over the moves (p -> s) of w * b(i+1, s) * beta(i+1, s): scatter the terms onto p
        term = lw + (lb[i + 1] + lbeta[i + 1])[None, :]
        acc = np.full(S, -np.inf)
        for row_pred, row_term in zip(pred, term):
            np.logaddexp.at(acc, row_pred, row_term)
        lbeta[i] = acc
    return em, lb, la, lbeta, pred, lw


def python_posterior(level, k, pos, mean, ac, mc, w_stay, w_step, w_skip):
    """The rules of nvk_kmer_posterior_dev for ONE read with events: the letter marginals from alpha + beta of
    ``log_alpha_beta`` -> (marg (E, 4), log Z)"""
    _, _, la, lbeta, _, _ = log_alpha_beta(level, k, mean, ac, mc, w_stay, w_step, w_skip)
    letter = (np.arange(4 ** k) >> (2 * (k - 1 - pos))) & 3
    g = la + lbeta
    cls = np.stack([np.logaddexp.reduce(g[:, letter == x], axis=1) for x in range(4)], axis=1)
    return np.exp(cls - np.logaddexp.reduce(cls, axis=1)[:, None]), float(np.logaddexp.reduce(la[-1]))


# ---- the workflow on the operator's outputs ------------------------------------------------------------------------
def qualities_of(post):
    """-> uint8: the number of THRESHOLDS each posterior reaches"""
    return np.searchsorted(THRESHOLDS, post, side='right').astype(np.uint8)


def read_base_post(marg, n_events, sequence, base_event):
    """One read: ``marg`` (E, 4), its decoded ``sequence`` and per base the first event of its state (-1: none) ->
    base_post.  A base with an event takes the largest marginal of its own letter over its dwell (its first event up to
    the next such base's first event; to E for the last); a base a skip passes the smaller of its two neighbours'
    values; the bases before the first and after the last base with an event the nearest such base's value."""
    sequence, base_event = np.asarray(sequence), np.asarray(base_event)
    post = np.full(sequence.size, np.nan)
    own = np.nonzero(base_event >= 0)[0]
    ends = np.append(base_event[own[1:]], n_events)
    for b, lo, hi in zip(own, base_event[own], ends):
        post[b] = marg[lo:hi, sequence[b]].max()
    for b in range(sequence.size):
        if base_event[b] >= 0:
            continue
        before, after = own[own < b], own[own > b]
        if before.size and after.size:
            post[b] = min(post[before[-1]], post[after[0]])
        else:
            post[b] = post[before[-1]] if before.size else post[after[0]]
    return post


def cpu_qualities(post_host, res, model, p_stay=0.7, p_skip=0.01, threads=None):
    """``res``: what ``decode_ref.cpu_decode`` returned (same ``p_stay`` / ``p_skip``) -> dict of ``base_post``,
    ``quality`` (flat, aligned with res['sequence']), ``loglik`` per read, and the operator's ``marg`` and ``z``"""
    k, central = model[0], model[1]
    threads = min(16, os.cpu_count() or 1) if threads is None else threads
    marg, z, status = post_host.posterior(res['scaled'], res['ev_off'], k, central, res['mean'], res['ac'], res['mc'],
                                          *weights(p_stay, p_skip), status_in=res['status_in'], threads=threads)
    assert np.array_equal(status, res['status'])
    n = res['ev_off'].size - 1
    posts = []
    for r in range(n):
        if status[r] != 0:
            continue
        e0, e1 = int(res['ev_off'][r]), int(res['ev_off'][r + 1])
        seq = res['sequence'][res['seq_off'][r]:res['seq_off'][r + 1]]
        rows = slice(int(res['map_off'][r]), int(res['map_off'][r + 1]))
        be = np.full(seq.size, -1, dtype=np.int64)
        # (the tables hold the first sample of a base's first event, and the events' first samples ascend in a read)
        be[res['map_base'][rows]] = np.searchsorted(res['ev_start'][e0:e1], res['map_sig'][rows])
        posts.append(read_base_post(marg[e0:e1], e1 - e0, seq, be))
    base_post = np.concatenate(posts) if posts else np.zeros(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        loglik = np.where(status == 0, log_z(z) / res['n_events'].astype(np.float64), np.nan)
    return dict(base_post=base_post, quality=qualities_of(base_post), loglik=loglik, marg=marg, z=z)


# ---- the quality claim ---------------------------------------------------------------------------------------------
def base_verdicts(truth, decoded):
    """``truth`` aligned to its best substring of ``decoded`` by edit distance (``decode_ref.identity``'s recurrence,
    kept as a matrix; the end column is the first minimum; the traceback prefers the diagonal, then a decoded-only
    base) -> int8 per decoded base: 1 right (on a diagonal with the same letter), 0 wrong (on a diagonal with another
    letter, or decoded-only), -1 outside the substring"""
    truth, decoded = np.asarray(truth), np.asarray(decoded)
    n, m = truth.size, decoded.size
    M = np.zeros((n + 1, m + 1), dtype=np.int64)
    ramp = np.arange(m + 1, dtype=np.int64)
    for i, t in enumerate(truth, start=1):
        cur = np.empty(m + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(M[i - 1, :-1] + (decoded != t), M[i - 1, 1:] + 1)
        M[i] = np.minimum.accumulate(cur - ramp) + ramp
    verdict = np.full(m, -1, dtype=np.int8)
    i, j = n, int(np.argmin(M[n]))
    while i > 0:
        if j > 0 and M[i, j] == M[i - 1, j - 1] + (decoded[j - 1] != truth[i - 1]):
            verdict[j - 1] = decoded[j - 1] == truth[i - 1]
            i, j = i - 1, j - 1
        elif j > 0 and M[i, j] == M[i, j - 1] + 1:
            verdict[j - 1] = 0
            j -= 1
        else:
            i -= 1
    return verdict


def auc(score, right):
    """The chance that a right base has the larger score than a wrong one, ties counting half"""
    score, right = np.asarray(score, dtype=np.float64), np.asarray(right, dtype=bool)
    wrong = np.sort(score[~right])
    below = np.searchsorted(wrong, score[right], side='left')
    upto = np.searchsorted(wrong, score[right], side='right')
    return float((below + 0.5 * (upto - below)).sum()) / (right.sum() * wrong.size)


def quality_claim(truths, sequence, seq_off, base_post, quality):
    """-> (table: per Phred bin (lo, hi, bases, error rate); AUC of base_post against correctness; the error rates below
    and at or above the median posterior; the number of bases counted), over the decoded bases inside the true
    sequences' substrings"""
    verdicts = np.concatenate([base_verdicts(t, sequence[seq_off[r]:seq_off[r + 1]]) for r, t in enumerate(truths)])
    inside = verdicts >= 0
    right, post, q = verdicts[inside] == 1, base_post[inside], quality[inside].astype(np.int64)
    table = []
    for lo, hi in PHRED_BINS:
        sel = (q >= lo) & (q < hi)
        table.append((lo, hi, int(sel.sum()), float((~right[sel]).mean()) if sel.any() else float('nan')))
    median = np.median(post)
    return table, auc(post, right), float((~right[post < median]).mean()), float((~right[post >= median]).mean()), \
        int(inside.sum())


def assert_quality_claim(claim):
    """The three assertions of the quality tests; prints the table first"""
    table, area, err_low, err_high, counted = claim
    print('%d decoded bases inside the true sequences' % counted)
    for lo, hi, bases, err in table:
        print('Phred [%2d, %2d%s  %6d bases  error rate %.3f' % (lo, min(hi, 60), ']' if hi > 60 else ')', bases, err))
    print('AUC %.4f; error rate below the median posterior %.4f, at or above it %.4f' % (area, err_low, err_high))
    rates = [row[3] for row in table]
    assert all(row[2] > 0 for row in table), table
    assert all(a > b for a, b in zip(rates[:-1], rates[1:])), rates
    assert area >= 0.69, area
    assert err_high <= 0.5 * err_low, (err_low, err_high)


# ---- constructed cases ---------------------------------------------------------------------------------------------
def small_cases():
    """Cases for the log-domain restatement: k = 2 and 3, reads of 1, 2, 3 and 65 events, random tables"""
    from nadavca_amd import synthetic
    rng = np.random.default_rng(91)
    cases = []
    for k in (2, 3):
        model = synthetic.synth_model_arrays(seed=20 + k, k=k, central=0)
        levels = [D.emit(rng, model, E) for E in (1, 2, 3, 65)]
        cases.append(('k %d' % k, D.pack(levels, k, 0, D.state_tables(model), D.LOG_COSTS)))
    return cases


def narrow_case():
    """k = 2, 300 events, sigma 0.02 around 16 levels 0.25 apart, noise 0.1: most events lie several sigma from every
    level, so log Z is far below the -745 at which an unscaled double recurrence reaches zero"""
    rng = np.random.default_rng(92)
    mean = np.arange(16) * 0.25 - 2.0
    sd = np.full(16, 0.02)
    model = (2, 0, 4, mean, sd)
    level = D.emit(rng, model, 300, noise=0.1)
    return D.pack([level], 2, 0, (mean, -np.log(sd * math.sqrt(2 * math.pi)), 1.0 / (2 * sd * sd)), D.LOG_COSTS)


def large_ac_case():
    """k = 2, 300 events on the levels themselves with ac = 3.5: every event multiplies the likelihood by about e^3.5, so
    log Z is above the +709.78 at which an unscaled double recurrence overflows"""
    rng = np.random.default_rng(93)
    mean = rng.permutation(16) * 0.25 - 2.0
    model = (2, 0, 4, mean, np.full(16, 0.05))
    level = D.emit(rng, model, 300, noise=0.0)
    return D.pack([level], 2, 0, (mean, np.full(16, 3.5), np.full(16, 200.0)), D.LOG_COSTS)


def far_event_case(k=2):
    """40 events of a random table, event 20 moved 50 sigma above the largest mean: em is below the floor for every
    state there"""
    from nadavca_amd import synthetic
    rng = np.random.default_rng(94)
    model = synthetic.synth_model_arrays(seed=30 + k, k=k, central=0)
    level = D.emit(rng, model, 40)
    level[20] = float(np.max(model[3]) + 50.0 * np.max(model[4]))
    return D.pack([level], k, 0, D.state_tables(model), D.LOG_COSTS)


def extreme_cases():
    return [('narrow sigma', narrow_case()), ('large ac', large_ac_case()), ('far event', far_event_case())]
