"""What the raw-signal workflows (``signal_map_batch``, ``signal_locate_batch``, ``decode_batch``) share: the k-mer
model argument, the Gaussian constants and transition costs their operators take, the first three device stages
(upload, per-read median / MAD normalisation, event detection), the rescale by moments, the base -> sample rows."""
import math

import numpy as np

from .batchflow import load_kmer_model, seg_index


def resolve_kmer_model(kmer_model, context=None):
    """``kmer_model``: a KmerModel, or a path, which is loaded on ``context`` (default: the process-wide one)"""
    if isinstance(kmer_model, (str, bytes)) or hasattr(kmer_model, '__fspath__'):
        from .kmer_model import load_kmer_model as load_on
        return load_on(kmer_model, context=context) if context is not None else load_kmer_model(kmer_model)
    return kmer_model


def offsets_of(counts):
    """The exclusive prefix sum of ``counts`` (an integer tensor of size n) -> int64 tensor of size n + 1"""
    import torch
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=counts.device), torch.cumsum(counts, 0)])


def gaussian_constants(sigma, sigma_scale):
    """-> (ac, mc) numpy f64 of the Gaussians with sigma * ``sigma_scale``: log density = ac - (x - mean)^2 * mc"""
    sd = np.asarray(sigma, dtype=np.float64) * float(sigma_scale)
    return -np.log(sd * math.sqrt(2.0 * math.pi)), 1.0 / (2.0 * sd * sd)


def transition_weights(p_stay, p_skip):
    """-> (w_stay, w_step, w_skip): the very numbers whose logs ``transition_costs`` takes"""
    return p_stay, 1.0 - p_stay - p_skip, p_skip


def transition_costs(p_stay, p_skip, who):
    """-> (l_stay, l_step, l_skip): the logs of p_stay, 1 - p_stay - p_skip and p_skip; ``who``: the caller's name"""
    if not (0.0 < p_stay < 1.0 and 0.0 < p_skip < 1.0 and p_stay + p_skip < 1.0):
        raise ValueError('%s: p_stay, p_skip and 1 - p_stay - p_skip must lie inside (0, 1)' % who)
    w_stay, w_step, w_skip = transition_weights(p_stay, p_skip)
    return math.log(w_stay), math.log(w_step), math.log(w_skip)


class SignalEvents:
    """What ``signal_events_dev`` makes, device tensors: ``norm`` (normalised samples) / ``sig_off``, ``flags`` (1 where
    an event starts), ``ev_pos`` (those samples), ``ev_off``, per event ``ev_start`` (in the read), ``ev_len``, level"""
    __slots__ = ('norm', 'sig_off', 'flags', 'ev_pos', 'ev_off', 'ev_start', 'ev_len', 'ev_level')


def detect_events_dev(context, norm, sig_off, window, threshold, var_floor):
    """Event detection on normalised signals -> (flags, ev_pos, ev_off, ev_start, ev_len, ev_level), device tensors."""
    import torch
    from .device import event_flags_dev, event_levels_dev
    flags = event_flags_dev(context, norm, sig_off, window, threshold, var_floor)
    ev_pos = torch.nonzero(flags).reshape(-1)
    ev_off = offsets_of(flags)[sig_off].contiguous()
    start, length, level = event_levels_dev(context, norm, sig_off, ev_pos)
    return flags, ev_pos, ev_off, start, length, level


def signal_events_dev(read_batch, context, window, threshold, var_floor, tick, into=None):
    """The raw signals of ``read_batch`` uploaded, normalised per read in place (``nvk_normalize_groups_dev``) and cut
    into events -> ``into`` (default: a new SignalEvents) with those fields set.  ``tick(name)`` is called after each
    stage: 'upload' (which so also counts what the caller uploaded before), 'normalise', 'events'."""
    import torch
    from .device import normalize_groups_dev
    device = torch.device('cuda', context.device)
    rb, ev = read_batch, SignalEvents() if into is None else into
    raw = torch.from_numpy(rb.raw_signal).to(device)
    if raw.dtype != torch.float64:
        raw = raw.to(torch.float64)
    ev.sig_off = torch.from_numpy(rb.sig_off).to(device)
    tick('upload')
    ev.norm = normalize_groups_dev(context, raw, ev.sig_off, out=raw)[0] if rb.n and raw.numel() else raw
    tick('normalise')
    ev.flags, ev.ev_pos, ev.ev_off, ev.ev_start, ev.ev_len, ev.ev_level = detect_events_dev(
        context, ev.norm, ev.sig_off, window, threshold, var_floor)
    tick('events')
    return ev


def rescale_by_moments_dev(context, level, ev_off, target, target_off, ok_extra=None, min_events=1):
    """Per read the events' levels mapped so that their median and MAD are those of a target's levels, both from
    ``nvk_normalize_groups_dev``'s exact selections: (level - med_e) * (mad_l / mad_e) + med_l.  ``target`` /
    ``target_off``: one group of levels per read (the reads' own expected levels), or a single group that serves every
    read (``[0, target.numel()]``).  A read takes part if it has at least ``min_events`` events, a MAD above 0 and a
    target that is not empty (and ``ok_extra``, bool per read, where given); one that does not keeps its levels, with
    scale 1 and shift 0.  -> (scaled levels, shift, scale, ok bool per read): scaled = scale * level + shift."""
    import torch
    from .device import _one, normalize_groups_dev
    n = int(ev_off.numel()) - 1
    _, cs_e = normalize_groups_dev(context, _one(level), ev_off)
    _, cs_l = normalize_groups_dev(context, _one(target), target_off)
    n_target = target_off[1:] - target_off[:-1]
    if int(target_off.numel()) - 1 != n:        # the single group, for every read
        cs_l, n_target = cs_l.expand(n, 2), n_target.expand(n)
    ok = (ev_off[1:] - ev_off[:-1] >= int(min_events)) & (n_target > 0) & (cs_e[:, 1] > 0)
    if ok_extra is not None:
        ok = ok & ok_extra
    scale = torch.where(ok, cs_l[:, 1] / torch.where(ok, cs_e[:, 1], torch.ones_like(cs_e[:, 1])),
                        torch.ones(n, dtype=torch.float64, device=ev_off.device))
    med_e = torch.where(ok, cs_e[:, 0], torch.zeros_like(scale))
    med_l = torch.where(ok, cs_l[:, 0], torch.zeros_like(scale))
    owner, _ = seg_index(ev_off, int(level.numel()))
    scaled = (level - med_e[owner]) * scale[owner] + med_l[owner]
    return scaled, med_l - med_e * scale, scale, ok


def map_rows_dev(owner, inner, base_event, ev_start, ev_off, n):
    """The base -> sample rows of ``ReadBatch``'s layout, one per base with an event, from per base its read
    (``owner``), its index in the read (``inner``), its first event in the read (``base_event``, -1: none) -> (map_base,
    map_sig: that event's first sample, map_off int64 (n + 1), keep: bool per base, k_owner: the rows' reads)."""
    import torch
    keep = base_event >= 0
    k_owner = owner[keep]
    map_sig = ev_start[ev_off[:-1][k_owner] + base_event[keep].to(torch.int64)]
    return (inner[keep].to(torch.int32), map_sig, offsets_of(torch.bincount(k_owner, minlength=n)), keep, k_owner)
