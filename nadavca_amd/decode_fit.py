"""``decode_batch(fit=n)``: a Baum-Welch fit of the parameters ``decode_batch`` otherwise guesses, before it decodes.

The model is read-side: a read's stage-2 level x (after the median / MAD rescale) is taken as alpha x + beta ~
N(mean_s, (c sigma_s)^2) in state s, with alpha and beta per read, and c and the three move weights pooled over the
batch.  So the Viterbi and the posterior operators run on the result unchanged: on the levels (x * alpha) + beta, the
table's constants at sigma * c, and the fitted weights.

A round is one E-step on the device (``nvk_kmer_expectations_dev``: per read the posterior-weighted moments of its
levels against the states' means and the expected number of each move, ten doubles) and one M-step here, on the host in
numpy f64 from the n x 10 stats: one small copy per round.  Pooled sums use ``np.sum`` and per-read work is
elementwise, so a restatement with per-read loops agrees bit for bit (tests/expect_ref.py).

THE M-STEP.  With M0 .. Mmm the moments of the CURRENT levels and E the read's events:

    Vxx = Mxx - Mx Mx / M0,  Vxm = Mxm - Mx Mm / M0,  Vmm = Mmm - Mm Mm / M0
    a = (Vxm + sqrt(Vxm^2 + 2 E Vxx)) / (2 Vxx)      the root of 2 Vxx a^2 - 2 Vxm a - E = 0: the E log a of the
                                                     Jacobian is what keeps the scale from shrinking (plain least
                                                     squares would pull every level onto one mean)
    b = (Mm - a Mx) / M0
    R = a^2 Vxx - 2 a Vxm + Vmm                      the read's weighted residual at (a, b)
    c <- c sqrt(2 SUM R / SUM E)
    q_kind = SUM N_kind / SUM N                      under w_stay + 4 w_step + 16 w_skip = 1

These are conditional maximisations of the expected log-likelihood, one after the other (a and b at the current c, then
c at the new a and b; the weights are separate), so every round raises the objective without being a joint optimum of
a and c.  The increments compose into cumulative values, alpha <- a alpha and beta <- a beta + b, which are always
applied to the stage-2 levels as (level * alpha) + beta, two rounded operations.  A read with M0 <= 0, Vxx <= 0 or a
result that is not finite keeps its values and stays out of the round's pooled sums; a read that stage 2 did not accept
takes no part at all.

THE WEIGHTS.  The operators take per-edge weights; q is their normalised reading (a state has 1 stay, 4 step and 16
skip edges).  Each q is held at Q_FLOOR = 2^-9 or above and the three renormalised, which keeps every weight inside
(0, 1) and max(w_stay, w_step) above the operators' 2^-10; then they go back to ``decode_batch``'s convention, w / SUM w
with w = (q_stay, q_step / 4, q_skip / 16), as p_stay and p_skip.

THE OBJECTIVE of a round is SUM over the reads of log Z - (E - 1) log(w_stay + 4 w_step + 16 w_skip) + E log alpha:
the log-likelihood of the stage-2 levels under one normalisation of the weights (without the middle term a change of
convention would show up as a fall).

Limits: c and the weights are pooled, not per read; there is no drift term (alpha and beta are constant over a read);
the table itself is not re-estimated (``estimate_decode_model`` does that from raw signal, ``estimate_kmer_model`` from
aligned reads).
"""
import math

import numpy as np

from .rawsignal import transition_weights

FIT_PARAMS = ('scale', 'sigma', 'moves')
Q_FLOOR = 2.0 ** -9
LN2 = math.log(2.0)


class DecodeFit:
    """What ``decode_batch(fit=n)`` fitted (``DecodeBatch.fit``), numpy arrays and floats.  Per read: ``scale`` and
    ``shift`` (the cumulative alpha and beta on the stage-2 levels; 1 and 0 for a read that took no part).  Pooled:
    ``sigma_scale`` (the ``sigma_scale`` argument times the fitted c), ``p_stay`` and ``p_skip`` -- the three are usable
    as the arguments of a later call -- and ``q`` (the shares of stay, step and skip among the moves).  ``objective``:
    f64 (n + 1,), before every round and after the last; ``counts``: f64 (reads, 3), the expected stay, step and skip
    moves per read under the fitted values; ``floored``: int64 per read, its events whose every emission sat on the
    floor under them (their moments are the floor's, not the model's); ``parts``: the parts the E-step ran in."""

    def __init__(self, scale, shift, sigma_scale, p_stay, p_skip, q, objective, counts, floored, parts, params):
        self.scale, self.shift = scale, shift
        self.sigma_scale, self.p_stay, self.p_skip, self.q = sigma_scale, p_stay, p_skip, q
        self.objective, self.counts, self.floored, self.parts = objective, counts, floored, parts
        self.params = params
        self.rounds = int(objective.size) - 1


def check_params(fit, fit_params):
    """-> (rounds, the groups to fit as a tuple in FIT_PARAMS' order)"""
    if int(fit) != fit or int(fit) < 0:
        raise ValueError('decode_batch: fit is a number of rounds, 0 or more')
    params = (fit_params,) if isinstance(fit_params, str) else tuple(fit_params)
    unknown = [p for p in params if p not in FIT_PARAMS]
    if unknown or (int(fit) > 0 and not params):
        raise ValueError('decode_batch: fit_params holds %s; it is a non-empty choice of %s'
                         % (unknown or 'nothing', ', '.join(FIT_PARAMS)))
    return int(fit), tuple(p for p in FIT_PARAMS if p in params)


def m_step(stats, n_events, eligible, params):
    """One M-step (module docstring).  ``stats``: f64 (n, 10) of the E-step; ``n_events``: per read; ``eligible``: bool
    per read, those the E-step processed; ``params``: the groups to fit.
    -> (a, b per read: the increments, 1 and 0 where nothing changes; rho: the factor on c; q: the three shares or
    None when the moves are not fitted or no move was counted; used: bool per read, those in the pooled sums)"""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 10)
    M0, Mx, Mxx, Mm, Mxm, Mmm = (stats[:, j] for j in range(6))
    E = np.asarray(n_events).astype(np.float64)
    n = stats.shape[0]
    with np.errstate(all='ignore'):
        Vxx = Mxx - Mx * Mx / M0
        Vxm = Mxm - Mx * Mm / M0
        Vmm = Mmm - Mm * Mm / M0
        if 'scale' in params:
            a = (Vxm + np.sqrt(Vxm * Vxm + 2.0 * E * Vxx)) / (2.0 * Vxx)
            b = (Mm - a * Mx) / M0
            R = a * a * Vxx - 2.0 * a * Vxm + Vmm
        else:
            a, b = np.ones(n), np.zeros(n)
            R = Mxx - 2.0 * Mxm + Mmm
        used = np.asarray(eligible, dtype=bool) & (M0 > 0.0) & (Vxx > 0.0) & np.isfinite(a) & np.isfinite(b) \
            & np.isfinite(R) & np.isfinite(stats[:, 6:9]).all(axis=1)
    a, b = np.where(used, a, 1.0), np.where(used, b, 0.0)
    rho = 1.0
    if 'sigma' in params and used.any():
        ratio = 2.0 * np.sum(R[used]) / np.sum(E[used])
        if np.isfinite(ratio) and ratio > 0.0:
            rho = float(np.sqrt(ratio))
    q = None
    if 'moves' in params and used.any():
        N = np.array([np.sum(stats[used, 6 + j]) for j in range(3)])
        total = np.sum(N)
        if np.isfinite(total) and total > 0.0:
            q = np.maximum(N / total, Q_FLOOR)
            q = q / np.sum(q)
    return a, b, rho, q, used


def moves_of(q):
    """The shares q as ``decode_batch``'s p_stay and p_skip: w = (q_stay, q_step / 4, q_skip / 16) over their sum"""
    w = np.array([q[0], q[1] / 4.0, q[2] / 16.0])
    total = np.sum(w)
    return float(w[0] / total), float(w[2] / total)


def shares_of(p_stay, p_skip):
    """... and back: the shares of stay, step and skip among the moves under p_stay and p_skip"""
    w_stay, w_step, w_skip = transition_weights(p_stay, p_skip)
    q = np.array([w_stay, 4.0 * w_step, 16.0 * w_skip])
    return q / np.sum(q)


def objective(z, n_events, scale, eligible, p_stay, p_skip):
    """The objective of the module docstring from the E-step's ``z`` (n, 2) at the values it ran with"""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    E = np.asarray(n_events).astype(np.float64)
    w_stay, w_step, w_skip = transition_weights(p_stay, p_skip)
    norm = math.log(w_stay + 4.0 * w_step + 16.0 * w_skip)
    sel = np.asarray(eligible, dtype=bool)
    term = (np.log(z[sel, 0]) + z[sel, 1] * LN2) - (E[sel] - 1.0) * norm + E[sel] * np.log(scale[sel])
    return float(np.sum(term))


def fit_loop(e_step, n_events, eligible, rounds, params, sigma_scale, p_stay, p_skip, scale=None, shift=None):
    """The rounds, on whatever runs the E-step.  ``e_step(scale, shift, sigma_scale, p_stay, p_skip)`` -> (stats (n, 10),
    z (n, 2), parts) as numpy arrays, on the levels (level * scale) + shift.  ``scale`` / ``shift``: where the reads
    start (default 1 and 0).  After the last round the E-step runs once more, for the last objective and the counts
    under the fitted values.  -> DecodeFit"""
    n = int(np.asarray(n_events).size)
    eligible = np.asarray(eligible, dtype=bool)
    scale = np.ones(n) if scale is None else np.array(scale, dtype=np.float64)
    shift = np.zeros(n) if shift is None else np.array(shift, dtype=np.float64)
    sigma_scale, p_stay, p_skip = float(sigma_scale), float(p_stay), float(p_skip)
    values, parts = [], 0
    for r in range(rounds + 1):
        stats, z, parts = e_step(scale, shift, sigma_scale, p_stay, p_skip)
        values.append(objective(z, n_events, scale, eligible, p_stay, p_skip))
        if r == rounds:
            break
        a, b, rho, q, _ = m_step(stats, n_events, eligible, params)
        scale, shift = a * scale, a * shift + b
        sigma_scale = sigma_scale * rho
        if q is not None:
            p_stay, p_skip = moves_of(q)
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 10)
    return DecodeFit(scale, shift, sigma_scale, p_stay, p_skip, shares_of(p_stay, p_skip), np.array(values),
                     stats[:, 6:9].copy(), stats[:, 9].astype(np.int64), parts, params)


def device_e_step(context, scaled, owner, ev_off, status_in, k, tables, timer=None, names=('forward', 'counts')):
    """The ``e_step`` of ``fit_loop`` on the device, for stage-2 levels ``scaled`` and their reads ``owner``.
    ``tables(sigma_scale)`` -> (mean, ac, mc) on the device; ``timer(name, ms)``: called with the two launches'
    milliseconds of every call, under ``names``."""
    from .device import kmer_expectations_dev

    def e_step(scale, shift, c, ps, pk):
        level = fitted_levels_dev(scaled, owner, scale, shift)
        out = kmer_expectations_dev(context, level, ev_off, k, *tables(c), *transition_weights(ps, pk), status_in,
                                    timing=timer is not None)
        if timer is not None:
            for name, ms in zip(names, out[4]):
                timer(name, ms)
        return out[0].cpu().numpy(), out[1].cpu().numpy(), out[3]
    return e_step


def fit_on_device(st, kmer_model, rounds, params, sigma_scale, p_stay, p_skip, start=None, timer=None):
    """The fit of a ``DecodeStages`` after its stage 2 (``st.scaled``, ``st.ev_off``, ``st.status_in``) -> DecodeFit.
    ``start``: a DecodeFit whose per-read ``scale`` and ``shift`` the reads start from; ``timer(name, ms)``: called
    with the forward and counts launches' milliseconds of every E-step (bench tool)."""
    from .batchflow import seg_index
    from .decode import state_tables_dev
    dev = st.ev_off.device
    owner, _ = seg_index(st.ev_off, int(st.scaled.numel()))
    n_events = (st.ev_off[1:] - st.ev_off[:-1]).cpu().numpy()
    eligible = st.ok.cpu().numpy()
    e_step = device_e_step(kmer_model.context, st.scaled, owner, st.ev_off, st.status_in, kmer_model.get_k(),
                           lambda c: state_tables_dev(kmer_model, c, dev), timer)
    return fit_loop(e_step, n_events, eligible, rounds, params, sigma_scale, p_stay, p_skip,
                    None if start is None else start.scale, None if start is None else start.shift)


def fitted_levels_dev(scaled, owner, scale, shift):
    """(level * scale) + shift on the device, two rounded operations; ``scale`` / ``shift``: numpy, per read"""
    import torch
    if scaled.numel() == 0:
        return scaled
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(scaled.device)
    return scaled * to(scale)[owner] + to(shift)[owner]
