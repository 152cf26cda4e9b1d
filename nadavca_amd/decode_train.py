"""``estimate_decode_model``: re-estimate the k-mer table's levels from raw signal alone, by Baum-Welch over the 4^k
states of ``decode_batch``.

``decode_batch(fit=n)`` fits what lies around the table (per read a scale and shift, pooled a factor on sigma and the
move weights) and takes the table as given; ``estimate_kmer_model`` re-estimates the table, but from reads aligned to a
reference with hard event borders.  This module does the part of Baum-Welch that adapts the model itself, with neither
a reference nor an aligner: per state the posterior weight of the batch's events and the moments of their levels under
it (``nvk_kmer_state_moments_dev``, contract in include/nadavca_hip.h), and from them the state's new mean and sigma.

STAGES.  Stages 1 and 2 of ``decode_batch`` run once, against the START table: normalisation, events, and the median /
MAD rescale onto the table's means.  The stage-2 levels then stay fixed; the per-read scale and shift absorb whatever
the table's change moves.

A ROUND is
  * ``fit`` rounds of ``decode_fit.fit_loop`` on the current table, from the current per-read scale and shift
    (``fit=0``: none);
  * one call of the operator at the fitted values: G0[s] = SUM g, G1[s] = SUM g x, G2[s] = SUM g x^2 over every event
    of every processed read, g the posterior of state s at the event and x the fitted level;
  * the M-step here, in numpy f64.  A state with G0 >= ``min_weight`` takes mean = G1 / G0 ('mean' in ``update``) and,
    with 'sd' in ``update``, var = G2 / G0 - mean * mean around that G1 / G0 and
    sigma = max(sqrt(max(var, 0)) / c, min_sigma), c the current factor on sigma (the operators run at sigma * c, so
    the table's own sigma is the fitted one divided by c).  Every other state keeps its bits.
Both steps raise the likelihood of the stage-2 levels, so the objective of ``decode_fit`` (``DecodeModelEstimate
.objective``: taken at every round's operator call, and once more after the last M-step) does not fall.

``train_loop`` is written on whatever runs the two E-steps, as ``decode_fit.fit_loop`` is, so the CPU restatement of
the tests (tests/moments_ref.py) and the device share it.

Limits.  Per-state transitions are not estimated: the three move weights stay pooled.  4-letter tables with k in 2..6
only, and there is no command-line sub-command.  There is no gauge fixing: a common stretch of the table and of the
per-read scales is not pinned (``decode_batch(fit=n)`` refits the scale anyway).  An event whose every emission sits on
the -300 floor is counted like any other (``DecodeFit.floored`` says how many there are).  ``min_weight`` and the other
defaults are uncalibrated.
"""
import numpy as np

from . import decode_fit, defaults
from .rawsignal import transition_weights

UPDATE = ('mean', 'sd')


class DecodeModelEstimate:
    """What ``estimate_decode_model`` returns.  ``model``: the final KmerModel; numpy arrays of its table (``mean``,
    ``sigma``) and of the last round (``weight``: its G0 per state; ``updated``: the states it replaced); ``fit``: the
    last ``DecodeFit`` (per-read scale and shift on the stage-2 levels, and ``anchor``, the means those levels were
    rescaled onto), usable as ``start=`` of a later call on the same batch or as ``fit_start=`` of ``decode_batch``;
    ``objective``: f64 (rounds + 1,), at every round's operator call and after the last M-step; ``history``: per round
    a dict of ``kmers_updated``, ``rms_mean_change`` (over the updated states) and ``parts`` (of the operator's call)."""

    def __init__(self, model, k, central, alphabet, mean, sigma, weight, updated, fit, objective, history):
        self.model, self.k, self.central, self.alphabet = model, k, central, alphabet
        self.mean, self.sigma, self.weight, self.updated = mean, sigma, weight, updated
        self.fit, self.objective, self.history = fit, objective, history

    def save(self, path):
        """The table as ``.npz`` in the packaged layout (save_kmer_model_npz)."""
        from .kmer_train import save_kmer_model_npz
        save_kmer_model_npz(path, self.k, self.central, self.alphabet, self.mean, self.sigma)


def check_update(update):
    """-> the groups to update as a tuple in UPDATE's order"""
    groups = (update,) if isinstance(update, str) else tuple(update)
    unknown = [g for g in groups if g not in UPDATE]
    if unknown or not groups:
        raise ValueError('estimate_decode_model: update holds %s; it is a non-empty choice of %s'
                         % (unknown or 'nothing', ', '.join(UPDATE)))
    return tuple(g for g in UPDATE if g in groups)


def m_step(moments, mean, sigma, c, update, min_weight, min_sigma):
    """One M-step (module docstring).  ``moments``: f64 (3, S) of the operator; ``mean`` / ``sigma``: the current
    table; ``c``: the current factor on sigma.  -> (mean, sigma, updated: bool per state); a state that is not updated
    keeps its bits"""
    G0, G1, G2 = np.asarray(moments, dtype=np.float64).reshape(3, -1)
    mean, sigma = np.asarray(mean, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    updated = G0 >= float(min_weight)
    with np.errstate(all='ignore'):
        m = G1 / G0
        var = G2 / G0 - m * m
        sd = np.maximum(np.sqrt(np.maximum(var, 0.0)) / float(c), float(min_sigma))
    updated = updated & np.isfinite(m) & np.isfinite(sd)
    new_mean = np.where(updated, m, mean) if 'mean' in update else mean.copy()
    new_sigma = np.where(updated, sd, sigma) if 'sd' in update else sigma.copy()
    return new_mean, new_sigma, updated


def train_loop(fit_e_step, moments_step, n_events, eligible, mean, sigma, rounds, fit, fit_params, update, min_weight,
               min_sigma, sigma_scale, p_stay, p_skip, scale=None, shift=None):
    """The rounds, on whatever runs the E-steps.  ``fit_e_step(mean, sigma)`` -> the ``e_step`` of
    ``decode_fit.fit_loop`` on that table; ``moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip)`` ->
    (moments (3, S), z (n, 2), parts) as numpy arrays, on the levels (level * scale) + shift.  ``scale`` / ``shift``:
    where the reads start (default 1 and 0).  After the last round the operator runs once more, for the last objective,
    and with ``fit`` = 0 so does the E-step of ``fit_loop``, for the ``DecodeFit``.
    -> (mean, sigma, weight, updated, DecodeFit, objective (rounds + 1,), history)"""
    n = int(np.asarray(n_events).size)
    eligible = np.asarray(eligible, dtype=bool)
    mean, sigma = np.array(mean, dtype=np.float64), np.array(sigma, dtype=np.float64)
    scale = np.ones(n) if scale is None else np.array(scale, dtype=np.float64)
    shift = np.zeros(n) if shift is None else np.array(shift, dtype=np.float64)
    sigma_scale, p_stay, p_skip = float(sigma_scale), float(p_stay), float(p_skip)
    values, history, last = [], [], None
    weight, updated = np.zeros(mean.size), np.zeros(mean.size, dtype=bool)
    for _ in range(rounds):
        if fit > 0:
            last = decode_fit.fit_loop(fit_e_step(mean, sigma), n_events, eligible, fit, fit_params, sigma_scale, p_stay,
                                       p_skip, scale, shift)
            scale, shift = last.scale, last.shift
            sigma_scale, p_stay, p_skip = last.sigma_scale, last.p_stay, last.p_skip
        moments, z, parts = moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip)
        values.append(decode_fit.objective(z, n_events, scale, eligible, p_stay, p_skip))
        new_mean, new_sigma, updated = m_step(moments, mean, sigma, sigma_scale, update, min_weight, min_sigma)
        change = float(np.sqrt(np.mean((new_mean[updated] - mean[updated]) ** 2))) if updated.any() else 0.0
        history.append(dict(kmers_updated=int(updated.sum()), rms_mean_change=change, parts=int(parts)))
        weight = np.array(np.asarray(moments, dtype=np.float64).reshape(3, -1)[0])
        mean, sigma = new_mean, new_sigma
    _, z, _ = moments_step(mean, sigma, scale, shift, sigma_scale, p_stay, p_skip)
    values.append(decode_fit.objective(z, n_events, scale, eligible, p_stay, p_skip))
    if last is None:
        last = decode_fit.fit_loop(fit_e_step(mean, sigma), n_events, eligible, 0, fit_params, sigma_scale, p_stay,
                                   p_skip, scale, shift)
    return mean, sigma, weight, updated, last, np.array(values), history


def device_steps(context, scaled, ev_off, status_in, k, timer=None):
    """The two E-steps of ``train_loop`` on the device, for stage-2 levels ``scaled`` (device tensors) -> (fit_e_step,
    moments_step).  ``timer(name, ms)``: called with the launches' milliseconds of every call (bench tool)."""
    from .batchflow import seg_index
    from .decode import tables_dev
    from .device import kmer_state_moments_dev
    dev = ev_off.device
    owner, _ = seg_index(ev_off, int(scaled.numel()))

    def fit_e_step(mean, sigma):
        return decode_fit.device_e_step(context, scaled, owner, ev_off, status_in, k,
                                        lambda c: tables_dev(mean, sigma, c, dev), timer, ('fit forward', 'fit counts'))

    def moments_step(mean, sigma, scale, shift, c, ps, pk):
        level = decode_fit.fitted_levels_dev(scaled, owner, scale, shift)
        out = kmer_state_moments_dev(context, level, ev_off, k, *tables_dev(mean, sigma, c, dev),
                                     *transition_weights(ps, pk), status_in, timing=timer is not None)
        if timer is not None:
            for name, ms in zip(('forward', 'moments', 'reduce'), out[4]):
                timer(name, ms)
        return out[0].cpu().numpy(), out[1].cpu().numpy(), out[3]

    return fit_e_step, moments_step


def train_stages(read_batch, context, anchor, min_events, window, threshold, var_floor):
    """Stages 1 and 2 of ``decode_batch`` on the device, the rescale onto the median and MAD of ``anchor`` (numpy: a
    table's means) -> (scaled levels, ev_off, status_in, ok)"""
    import torch
    from .decode import DEC_NO_EVENTS, DEC_OK
    from .rawsignal import rescale_by_moments_dev, signal_events_dev
    device = torch.device('cuda', context.device)
    ev = signal_events_dev(read_batch, context, window, threshold, var_floor, lambda name: None)
    target = torch.from_numpy(np.ascontiguousarray(anchor, dtype=np.float64)).to(device)
    pool_off = torch.tensor([0, int(target.numel())], dtype=torch.int64, device=device)
    scaled, _, _, ok = rescale_by_moments_dev(context, ev.ev_level, ev.ev_off, target, pool_off, min_events=min_events)
    return scaled, ev.ev_off, torch.where(ok, DEC_OK, DEC_NO_EVENTS).to(torch.int32), ok


def check_args(rounds, fit, fit_params, update, min_weight, min_sigma, min_events):
    """-> (rounds, fit rounds, the fit's groups, the update's groups)"""
    if isinstance(rounds, bool) or int(rounds) != rounds or rounds < 1:
        raise ValueError('estimate_decode_model: rounds must be an integer >= 1, not %r' % (rounds,))
    if int(min_events) < 1:
        raise ValueError('estimate_decode_model: min_events is at least 1')
    for name, v in (('min_weight', min_weight), ('min_sigma', min_sigma)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError('estimate_decode_model: %s must be a finite number > 0, not %r' % (name, v))
    fit, groups = decode_fit.check_params(fit, fit_params)
    return int(rounds), fit, groups, check_update(update)


def estimate_decode_model(read_batch, kmer_model=defaults.KMER_MODEL_FILE, rounds=3, fit=1, fit_params=('scale',),
                          update=('mean',), min_weight=8.0, min_sigma=0.05, p_stay=0.7, p_skip=0.01, sigma_scale=1.0,
                          min_events=32, window=2, threshold=5.0, var_floor=0.02, start=None, context=None):
    """Re-estimate ``kmer_model`` (a KmerModel or a path; 4 letters, k in 2..6) from the raw signal of ``read_batch``
    alone (module docstring); any sequence or table the batch carries is ignored.  ``rounds`` (>= 1): operator calls
    and M-steps; ``fit`` / ``fit_params``: the rounds of ``decode_batch``'s fit before each of them and what it fits;
    ``update``: a choice of 'mean' and 'sd'; ``min_weight``: the posterior weight (in events) a state needs to be
    replaced; ``min_sigma``: the floor of a re-estimated sigma; ``p_stay``, ``p_skip``, ``sigma_scale``, ``min_events``,
    ``window``, ``threshold``, ``var_floor``: ``decode_batch``'s.  ``start``: the ``fit`` of an earlier call on the
    same batch: the reads start from its per-read scale and shift, on stage-2 levels rescaled onto its ``anchor`` (its
    pooled values are passed as ``sigma_scale``, ``p_stay`` and ``p_skip``), so that ``rounds=n`` equals n chained
    calls of one round bit for bit.  The defaults are uncalibrated.  -> DecodeModelEstimate."""
    from .decode import check_table
    from .kmer_model import KmerModel
    from .rawsignal import resolve_kmer_model, transition_costs
    kmer_model = resolve_kmer_model(kmer_model, context)
    check_table(kmer_model)
    rounds, fit, groups, update = check_args(rounds, fit, fit_params, update, min_weight, min_sigma, min_events)
    transition_costs(p_stay, p_skip, 'estimate_decode_model')
    rb, context = read_batch, kmer_model.context
    if start is not None and start.scale.shape != (rb.n,):
        raise ValueError('estimate_decode_model: start holds %d reads, the batch %d' % (start.scale.size, rb.n))
    k, central = kmer_model.get_k(), kmer_model.get_central_position()
    mean = np.array(kmer_model.mean, dtype=np.float64)
    sigma = np.array(kmer_model.sigma, dtype=np.float64)
    anchor = np.array(getattr(start, 'anchor', mean), dtype=np.float64)
    scaled, ev_off, status_in, ok = train_stages(rb, context, anchor, min_events, window, threshold, var_floor)
    n_events = (ev_off[1:] - ev_off[:-1]).cpu().numpy()
    fit_e_step, moments_step = device_steps(context, scaled, ev_off, status_in, k)
    mean, sigma, weight, updated, last, objective, history = train_loop(
        fit_e_step, moments_step, n_events, ok.cpu().numpy(), mean, sigma, rounds, fit, groups, update, min_weight,
        min_sigma, sigma_scale, p_stay, p_skip, None if start is None else start.scale,
        None if start is None else start.shift)
    last.anchor = anchor
    model = KmerModel(k, central, 4, mean, sigma, context=context)
    return DecodeModelEstimate(model, k, central, 4, mean, sigma, weight, updated, last, objective, history)
