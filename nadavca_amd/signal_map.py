"""``signal_map_batch``: the base -> sample tables of a ``ReadBatch`` from raw signal and basecalled sequence alone.

Every batch workflow starts from the basecaller's base -> sample table (``ReadBatch.map_base`` / ``map_sig``, the
reference's ``Read.sequence_to_signal_mapping`` from a fast5's ``Events`` or ``Move`` data): it is what
``readbatch.signal_alignments`` turns into anchors.  Raw signal with a FASTQ, or a BAM written without moves, has no
such table.  This module rebuilds it the way nanopolish / f5c ``eventalign`` and tombo ``resquiggle`` do, on the device:

1. per-read median / MAD normalisation (``nvk_normalize_groups_dev``);
2. event detection: a two-window t-like statistic per sample, borders at its local maxima above a threshold
   (``nvk_event_flags_dev``), then the mean level of every event (``nvk_event_levels_dev``);
3. a rescale by moments: the events' median and MAD are mapped onto those of the read's own expected k-mer levels;
4. an adaptive-banded alignment of the events to those levels, one wave per read (``nvk_event_align_dev``), with free
   ends, so that leaders, adapters and tails stay unaligned.

The rules of 2 and 4 are the contract of include/nadavca_hip.h.  Integer plumbing between the kernels is torch.
With ``SeedAligner`` for the approximate alignment every workflow then runs from signal + sequence + reference:

    rb = ReadBatch.from_signals(raw, sig_off, sequence, seq_off)
    rb = signal_map_batch(rb).read_batch(rb)
    align_signal_batch(None, rb, aligner=SeedAligner(reference_codes))
"""
import math

from . import _lib, defaults
from .batchflow import seg_index
from .rawsignal import (SignalEvents, gaussian_constants, map_rows_dev, rescale_by_moments_dev, resolve_kmer_model,
                        signal_events_dev)
from .readbatch import ReadBatch

MAP_OK, MAP_NO_EVENTS, MAP_LOST = _lib.MAP_OK, _lib.MAP_NO_EVENTS, _lib.MAP_LOST


class SignalMapBatch:
    """What ``signal_map_batch`` returns, numpy arrays.  Per read: ``status`` (0 mapped, MAP_NO_EVENTS: no event, no
    base, or events that all have one level; MAP_LOST: the band lost the path), ``n_events``, ``score`` (mean
    log-likelihood per aligned event, NaN unless mapped), ``shift`` / ``scale`` (aligned level = scale * event level +
    shift), ``first_event`` / ``last_event`` aligned (-1 unless mapped).  Flat: ``map_base`` / ``map_sig`` / ``map_off``
    in the layout of ``ReadBatch`` — one row per base that got at least one event, bases ascending, ``map_sig`` the
    first sample of the base's first event; a read that is not mapped has no rows.  With ``events=True``: ``ev_off``
    (int64, n + 1) and per event ``ev_start`` (first sample, inside the read), ``ev_len``, ``ev_level`` (normalised,
    before the rescale); otherwise None."""

    def __init__(self, status, n_events, score, shift, scale, first_event, last_event, map_base, map_sig, map_off,
                 ev_off=None, ev_start=None, ev_len=None, ev_level=None):
        self.status, self.n_events, self.score, self.shift, self.scale = status, n_events, score, shift, scale
        self.first_event, self.last_event = first_event, last_event
        self.map_base, self.map_sig, self.map_off = map_base, map_sig, map_off
        self.ev_off, self.ev_start, self.ev_len, self.ev_level = ev_off, ev_start, ev_len, ev_level
        self.n = int(status.size)
        self.n_mapped = int((status == MAP_OK).sum())

    def read_batch(self, rb):
        """A new ``ReadBatch`` with ``rb``'s signals and sequences and these tables; it goes into every batch workflow
        as one that came with a basecaller's table does."""
        if rb.n != self.n:
            raise ValueError('SignalMapBatch.read_batch: the batch holds %d reads, the map %d' % (rb.n, self.n))
        return ReadBatch(rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off, self.map_base, self.map_sig, self.map_off)


def base_tables_dev(kmer_model, sequence, seq_off, sigma_scale):
    """Per base of the reads (int32 codes / int64 offsets, device tensors): the level of its k-mer and the constants
    of its Gaussian with sigma * ``sigma_scale`` -> (mu, ac, mc) f64.  The k-mer is that of csrc/kmer.h without
    contexts (base 0 outside the read); a code outside the alphabet is read as 0.  The walk over the k-mers is the
    expected-signal kernel's: it runs three times, over the table of means and over the two tables of constants."""
    import torch
    from .dtw import KmerModel
    from .device import _dp
    lib = _lib.load()
    dev = sequence.device
    n, total = int(seq_off.numel()) - 1, int(sequence.numel())
    alphabet = kmer_model.get_alphabet_size()
    codes = torch.where((sequence < 0) | (sequence >= alphabet), torch.zeros_like(sequence), sequence).contiguous()
    tables = (None,) + gaussian_constants(kmer_model.sigma, sigma_scale)
    none = torch.zeros(1, dtype=torch.int32, device=dev)
    none_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    out = []
    for table in tables:
        model = kmer_model if table is None else KmerModel(
            kmer_model.get_k(), kmer_model.get_central_position(), alphabet, table, kmer_model.sigma,
            context=kmer_model.context)
        v = torch.zeros(max(total, 1), dtype=torch.float64, device=dev)
        if total:
            _lib.check(lib.nvk_expected_signal_batch_dev(model.handle, n, total, _dp(codes), _dp(seq_off), _dp(none),
                                                         _dp(none_off), _dp(none), _dp(none_off), _dp(v)),
                       'nvk_expected_signal_batch_dev')
        out.append(v[:total])
        if table is not None:
            model.close()
    return out


def dwell_costs(n_events, n_bases):
    """-> (l_stay, l_step) f64 per read from its event and base counts (tensors):
    p_stay = max(1 - 1 / max(E / K, 1.0001), 0.05), l_stay = log p_stay, l_step = log max(1 - p_stay - 1e-10, 1e-3)."""
    import torch
    E, K = n_events.to(torch.float64), torch.clamp(n_bases.to(torch.float64), min=1.0)
    p_stay = torch.clamp(1.0 - 1.0 / torch.clamp(E / K, min=1.0001), min=0.05)
    return torch.log(p_stay), torch.log(torch.clamp(1.0 - p_stay - 1e-10, min=1e-3))


class SignalMapStages(SignalEvents):
    """The device tensors between the stages of one ``signal_map_batch`` call (``signal_map_stages``)."""
    __slots__ = ('seq_off', 'mu', 'ac', 'mc', 'status_in', 'shift', 'scale', 'scaled', 'l_stay', 'l_step', 'hit',
                 'path_score', 'base_event')


def signal_map_stages(read_batch, kmer_model, window, threshold, var_floor, band, sigma_scale, trim_cost, skip_cost,
                      timer=None):
    """The four stages on the device -> SignalMapStages.  ``timer(name)``: called after each stage (bench tool)."""
    import torch
    from .device import event_align_dev
    context = kmer_model.context
    device = torch.device('cuda', context.device)
    rb, st = read_batch, SignalMapStages()
    tick = timer if timer is not None else (lambda name: None)
    st.seq_off = torch.from_numpy(rb.seq_off).to(device)
    sequence = torch.from_numpy(rb.sequence).to(device)
    signal_events_dev(rb, context, window, threshold, var_floor, tick, into=st)
    st.mu, st.ac, st.mc = base_tables_dev(kmer_model, sequence, st.seq_off, sigma_scale)
    # (a read with no event, no base or a zero MAD of its events is not aligned)
    st.scaled, st.shift, st.scale, ok = rescale_by_moments_dev(context, st.ev_level, st.ev_off, st.mu, st.seq_off)
    st.status_in = torch.where(ok, 0, MAP_NO_EVENTS).to(torch.int32)
    st.l_stay, st.l_step = dwell_costs(st.ev_off[1:] - st.ev_off[:-1], st.seq_off[1:] - st.seq_off[:-1])
    tick('rescale')
    st.hit, st.path_score, st.base_event = event_align_dev(
        context, st.scaled, st.ev_off, st.mu, st.ac, st.mc, st.seq_off, st.l_stay, st.l_step, st.status_in, band,
        trim_cost, skip_cost)
    tick('align')
    return st


def signal_map_batch(read_batch, kmer_model=defaults.KMER_MODEL_FILE, window=2, threshold=5.0, var_floor=0.02,
                     band=128, sigma_scale=0.5, trim_cost=math.log(0.01), skip_cost=math.log(1e-10), context=None,
                     events=False):
    """The base -> sample table of every read of ``read_batch`` from its raw signal and its sequence (module
    docstring); any table the batch carries is ignored.  ``kmer_model``: a KmerModel or a path; ``context``: the
    context a model loaded from a path is made on (default: the process-wide one).  ``window`` (1..8), ``threshold``,
    ``var_floor``: the event detector's; ``band``: 64 or 128 cells per anti-diagonal; ``sigma_scale``: the model's
    sigma is multiplied by it (an event's level is a mean over several samples: it scatters less than a sample);
    ``trim_cost`` / ``skip_cost``: log cost of an event left outside the alignment at either end, and of a base
    without an event.  The detector and cost defaults are uncalibrated: they are the values at which the simulated
    reads of the test suite (dwell 3-17 samples, noise 0.35, the packaged 6-mer table) map best, not values fitted
    to real data.  -> SignalMapBatch.  A read that is not mapped gets no rows: downstream it has no anchors and is
    not live, like a read the aligner did not place."""
    import torch
    kmer_model = resolve_kmer_model(kmer_model, context)
    if band not in (64, 128):
        raise ValueError('signal_map_batch: band is 64 or 128')
    rb = read_batch
    st = signal_map_stages(rb, kmer_model, window, threshold, var_floor, band, sigma_scale, trim_cost, skip_cost)
    status = st.hit[:, 0]
    first, last = st.hit[:, 2].to(torch.int64), st.hit[:, 3].to(torch.int64)
    n_ev = st.hit[:, 1].to(torch.int64)
    ok = status == MAP_OK
    # out_score holds the trims of both ends; the score is the mean over the events in between
    trimmed = (first + (n_ev - 1 - last)).to(torch.float64) * float(trim_cost)
    score = torch.where(ok, (st.path_score - trimmed) / torch.clamp(last - first + 1, min=1).to(torch.float64),
                        torch.full_like(st.path_score, float('nan')))
    total_bases = int(rb.seq_off[-1])
    owner, inner = seg_index(st.seq_off, total_bases)
    map_base, map_sig, map_off, _, _ = map_rows_dev(owner, inner, st.base_event, st.ev_start, st.ev_off, rb.n)
    host = lambda t: t.cpu().numpy()
    ev = (host(st.ev_off), host(st.ev_start), host(st.ev_len), host(st.ev_level)) if events else (None,) * 4
    return SignalMapBatch(host(status), host(st.hit[:, 1]), host(score), host(st.shift), host(st.scale),
                          host(st.hit[:, 2]), host(st.hit[:, 3]), host(map_base), host(map_sig), host(map_off), *ev)
