"""``decode_batch``: a base sequence and its base -> sample table for every read of a ``ReadBatch``, from raw signal alone.

``signal_locate_batch`` places raw signal on a reference by a dense DP against every column: it serves references of
some 10^5 bases.  This module takes the other classic route, the k-mer HMM decode of the event-based basecallers
(Nanocall's class): Viterbi over the 4^k k-mer states of the table and the read's events.  The decoded sequence is
rough (about three bases in four), but it is a sequence: ``SeedAligner`` is indexed and places it on a genome of any
size, and the Viterbi path is at the same time the base -> sample table (the "move table") that every batch workflow
starts from.  On the device:

1. per-read median / MAD normalisation (``nvk_normalize_groups_dev``) and event detection, both ``signal_map_batch``'s;
2. a rescale by moments: the events' per-read median and MAD are mapped onto those of the table's 4^k means
   (``rawsignal.rescale_by_moments_dev``, one group for every read).  A read with fewer than ``min_events`` events or a
   zero MAD is ``DEC_NO_EVENTS``;
3. the operator (``nvk_viterbi_decode_dev``, contract in include/nadavca_hip.h): per read the best path's score, the
   sequence it spells and per base the first event of the state that owns it;
4. a compaction of the operator's outputs, which it lays out by capacity, in torch;
5. with ``qualities=True`` the forward-backward operator (``nvk_kmer_posterior_dev``): per event the posterior of each
   letter at the state's ``central`` position, summed over ALL paths, and log Z per read.  A base takes the largest
   posterior of its own letter over its dwell (``base_post``), and ``quality`` is its Phred value cut to 0..60, counted
   on a fixed table of thresholds.  The scale is ordered, not calibrated: the transition weights are guesses, and on the
   simulated reads it is over-confident above Q20.

With ``fit=n`` n rounds of a Baum-Welch fit run between stages 2 and 3 (nadavca_amd/decode_fit.py: the E-step is
``nvk_kmer_expectations_dev``, the M-step numpy on the host): per read a scale and shift on the stage-2 levels, pooled
over the batch a factor on the table's sigma and the move weights.  Stages 3 to 5 then run on the fitted levels, table
constants and weights, unchanged.

So one operator stands where ``signal_locate_batch`` and ``signal_map_batch`` do on that route:

    rb0 = ReadBatch.from_signals(raw, sig_off, np.zeros(0, np.int32), np.zeros(n + 1, np.int64))
    dec = decode_batch(rb0)
    rb1 = dec.read_batch(rb0)                      # decoded sequences + base -> sample tables
    align_signal_batch(None, rb1, aligner=SeedAligner(reference, k=10))

Limits: a homopolymer beyond k bases is not resolved (a step from a state to itself is a stay); leader and tail signal
are not trimmed, they decode as bases that a local aligner leaves unaligned; 4-letter tables with k in 2..6 only, no
RNA.
"""
import math

import numpy as np

from . import _lib, decode_fit, defaults
from .batchflow import seg_index
from .rawsignal import (SignalEvents, gaussian_constants, map_rows_dev, offsets_of, rescale_by_moments_dev,
                        resolve_kmer_model, signal_events_dev, transition_costs, transition_weights)
from .readbatch import ReadBatch

DEC_OK, DEC_NO_EVENTS = _lib.DEC_OK, _lib.DEC_NO_EVENTS
K_MIN, K_MAX = 2, 6


class DecodeBatch:
    """What ``decode_batch`` returns, numpy arrays.  Per read: ``status`` (DEC_OK; DEC_NO_EVENTS: fewer than
    ``min_events`` events or events that all have one level), ``n_events``, ``n_bases`` (0 unless decoded), ``score``
    (the best path's log-likelihood per event, NaN unless decoded), ``seq_off`` (int64, n + 1).  Flat: ``sequence``
    (int32 base codes, read j at [seq_off[j], seq_off[j+1])) and ``map_base`` / ``map_sig`` / ``map_off`` in the layout
    of ``ReadBatch`` — one row per base with an event, bases ascending, ``map_sig`` the first sample of that event; the
    first ``central`` and the last k - 1 - ``central`` bases of a read and a base a skip passes have none.
    With ``qualities=True`` (else None): ``loglik`` per read (log Z per event, NaN unless decoded; ``score - loglik`` is
    the log posterior of the whole Viterbi path per event) and, flat and aligned with ``sequence``, ``base_post`` (f64:
    the largest posterior of the base's letter over its dwell; a base a skip passes takes the smaller of its two
    neighbours' values, the bases before the first and after the last base with an event the nearest one's) and
    ``quality`` (uint8, 0..60: the number of thresholds 1 - 10^(-j/10), j = 1..60, that ``base_post`` reaches).
    With ``fit=n`` or ``fit_start`` (else None): ``fit``, the ``decode_fit.DecodeFit`` the other results were computed
    with."""

    def __init__(self, status, n_events, n_bases, score, seq_off, sequence, map_base, map_sig, map_off, parts=0,
                 loglik=None, base_post=None, quality=None, post_parts=0, fit=None):
        self.status, self.n_events, self.n_bases, self.score = status, n_events, n_bases, score
        self.seq_off, self.sequence = seq_off, sequence
        self.map_base, self.map_sig, self.map_off = map_base, map_sig, map_off
        self.parts = parts   # parts the operator cut the batch into under the workspace cap
        self.loglik, self.base_post, self.quality = loglik, base_post, quality
        self.post_parts = post_parts   # ... and the forward-backward operator its own
        self.fit = fit
        self.n = int(status.size)
        self.n_decoded = int((status == DEC_OK).sum())

    def write_fastq(self, path, names=None):
        """The decoded reads as FASTQ: letters ``ACGT``, quality character ``chr(33 + quality)``; a read that did not
        decode is left out.  ``names``: one per read of the batch (default ``read_<index>``).  -> reads written"""
        if self.quality is None:
            raise ValueError('DecodeBatch.write_fastq: no qualities; call decode_batch(..., qualities=True)')
        if names is not None and len(names) != self.n:
            raise ValueError('DecodeBatch.write_fastq: %d names for %d reads' % (len(names), self.n))
        letters = np.frombuffer(b'ACGT', dtype=np.uint8)[self.sequence].tobytes().decode('ascii')
        marks = (self.quality + np.uint8(33)).tobytes().decode('ascii')
        decoded = np.nonzero(self.status == DEC_OK)[0]
        with open(path, 'w') as out:
            for r in decoded:
                lo, hi = int(self.seq_off[r]), int(self.seq_off[r + 1])
                out.write('@%s\n%s\n+\n%s\n' % (names[r] if names is not None else 'read_%d' % r, letters[lo:hi],
                                                marks[lo:hi]))
        return int(decoded.size)

    def read_batch(self, rb):
        """A new ``ReadBatch`` with ``rb``'s signals, the decoded sequences and these tables.  A read that is not
        decoded gets an empty sequence and no rows: downstream it drops out like a read the aligner did not place."""
        if rb.n != self.n:
            raise ValueError('DecodeBatch.read_batch: the batch holds %d reads, the decode %d' % (rb.n, self.n))
        return ReadBatch(rb.raw_signal, rb.sig_off, self.sequence, self.seq_off, self.map_base, self.map_sig,
                         self.map_off)


# quality[b] = the number of these that base_post[b] reaches.  Computed once, here, in numpy f64: the device only
# compares against them, so a host restatement with the same table agrees in every integer
PHRED_THRESHOLDS = 1.0 - np.power(10.0, -np.arange(1, 61, dtype=np.float64) / 10.0)


def check_table(kmer_model):
    """The operator's limits on the table, as a ValueError that names them"""
    alphabet, k = kmer_model.get_alphabet_size(), kmer_model.get_k()
    if alphabet != 4:
        raise ValueError('decode_batch: the table has %d letters; only 4-letter tables are decoded' % alphabet)
    if not K_MIN <= k <= K_MAX:
        raise ValueError('decode_batch: the table has k = %d; k is %d..%d' % (k, K_MIN, K_MAX))


def tables_dev(mean, sigma, sigma_scale, device):
    """-> (mean, ac, mc) f64 on ``device``: the levels and the constants of their Gaussians with
    sigma * ``sigma_scale``, formed as ``signal_map.base_tables_dev`` forms them"""
    import torch
    tables = (np.asarray(mean, dtype=np.float64),) + gaussian_constants(sigma, sigma_scale)
    return [torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in tables]


def state_tables_dev(kmer_model, sigma_scale, device):
    """``tables_dev`` of the model's 4^k states"""
    return tables_dev(kmer_model.mean, kmer_model.sigma, sigma_scale, device)


def capacity_offsets(ev_off, k):
    """Where the operator writes each read's bases: k + 2 (E - 1) entries for a read with events -> int64 (n + 1)"""
    import torch
    n_ev = ev_off[1:] - ev_off[:-1]
    cap = torch.where(n_ev >= 1, k + 2 * (n_ev - 1), torch.zeros_like(n_ev))
    return offsets_of(cap)


def traceback_bytes(n_events, k):
    """Bytes of the operator's traceback store for reads of ``n_events`` events (numpy): 4^k / 2 per event but the
    first"""
    return int(np.maximum(np.asarray(n_events, dtype=np.int64) - 1, 0).sum()) * (4 ** k // 2)


def row_store_bytes(n_events, k):
    """Bytes of the forward-backward operator's row store for reads of ``n_events`` events (numpy): 8 * 4^k per event"""
    return int(np.asarray(n_events, dtype=np.int64).sum()) * 8 * 4 ** k


def base_qualities_dev(marg, z, ok, n_ev, ev_off, map_off, owner, keep, sequence, event):
    """The forward-backward operator's outputs as per-read and per-base values, in torch on the device -> (loglik per
    read, base_post and quality per base).  ``owner`` / ``keep`` / ``event``: per base its read, whether it has an event,
    and that event; ``map_off``: the reads' offsets into the bases with an event (the rows)."""
    import torch
    dev = marg.device
    loglik = torch.where(ok, (torch.log(z[:, 0]) + z[:, 1] * math.log(2.0)) / torch.clamp(n_ev, min=1).to(torch.float64),
                         torch.full_like(z[:, 0], float('nan')))
    n_rows = int(map_off[-1])
    if n_rows == 0:
        return loglik, torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev)
    # per event of a decoded read the row whose dwell it lies in: the rows' first events ascend, and a read's first
    # event is a row's
    first = torch.zeros(int(ev_off[-1]), dtype=torch.int64, device=dev)
    first[ev_off[:-1][owner[keep]] + event[keep]] = 1
    used = ok[seg_index(ev_off)[0]]
    row_of = (torch.cumsum(first, 0) - 1)[used]
    value = marg[used].gather(1, sequence[keep][row_of].to(torch.int64)[:, None])[:, 0]
    rows = torch.zeros(n_rows, dtype=torch.float64, device=dev).scatter_reduce(0, row_of, value, 'amax',
                                                                              include_self=False)
    # a base without an event: the rows before and after it in its own read
    before = torch.cumsum(keep.to(torch.int64), 0) - 1
    after = before + 1
    has_before, has_after = before >= map_off[:-1][owner], after < map_off[1:][owner]
    v_before, v_after = rows[torch.clamp(before, min=0)], rows[torch.clamp(after, max=n_rows - 1)]
    base_post = torch.where(keep | ~has_after, v_before,
                            torch.where(has_before, torch.minimum(v_before, v_after), v_after))
    thresholds = torch.from_numpy(PHRED_THRESHOLDS).to(dev)
    return loglik, base_post, torch.searchsorted(thresholds, base_post, right=True).to(torch.uint8)


class DecodeStages(SignalEvents):
    """The device tensors between the stages of one ``decode_batch`` call (``decode_stages``)."""
    __slots__ = ('mean', 'ac', 'mc', 'scaled', 'ok', 'status_in', 'cap_off', 'costs', 'weights', 'hit', 'path_score',
                 'seq', 'base_event', 'parts', 'fit')


def decode_stages(read_batch, kmer_model, p_stay, p_skip, sigma_scale, min_events, window, threshold, var_floor,
                  timer=None, fit=None):
    """Stages 1 to 3 on the device -> DecodeStages.  ``timer(name)``: called after each stage (bench tool).  ``fit``:
    None, or (rounds, groups, start) of ``decode_fit``: the fit runs after stage 2, and ``scaled``, the table
    constants, ``costs`` and ``weights`` are then the fitted ones."""
    import torch
    from .device import viterbi_decode_dev
    context = kmer_model.context
    device = torch.device('cuda', context.device)
    rb, st = read_batch, DecodeStages()
    tick = timer if timer is not None else (lambda name: None)
    st.costs = transition_costs(p_stay, p_skip, 'decode_batch')
    st.weights, st.fit = transition_weights(p_stay, p_skip), None
    st.mean, st.ac, st.mc = state_tables_dev(kmer_model, sigma_scale, device)
    signal_events_dev(rb, context, window, threshold, var_floor, tick, into=st)
    pool_off = torch.tensor([0, int(st.mean.numel())], dtype=torch.int64, device=device)
    st.scaled, _, _, st.ok = rescale_by_moments_dev(context, st.ev_level, st.ev_off, st.mean, pool_off,
                                                    min_events=min_events)
    st.status_in = torch.where(st.ok, DEC_OK, DEC_NO_EVENTS).to(torch.int32)
    st.cap_off = capacity_offsets(st.ev_off, kmer_model.get_k())
    tick('rescale')
    if fit is not None:
        rounds, groups, start = fit
        if start is not None and start.scale.shape != (rb.n,):
            raise ValueError('decode_batch: fit_start holds %d reads, the batch %d' % (start.scale.size, rb.n))
        st.fit = decode_fit.fit_on_device(st, kmer_model, rounds, groups, sigma_scale, p_stay, p_skip, start)
        st.costs = transition_costs(st.fit.p_stay, st.fit.p_skip, 'decode_batch')
        st.weights = transition_weights(st.fit.p_stay, st.fit.p_skip)
        st.mean, st.ac, st.mc = state_tables_dev(kmer_model, st.fit.sigma_scale, device)
        st.scaled = decode_fit.fitted_levels_dev(st.scaled, seg_index(st.ev_off, int(st.scaled.numel()))[0],
                                                 st.fit.scale, st.fit.shift)
        tick('fit')
    st.hit, st.path_score, st.seq, st.base_event, st.parts = viterbi_decode_dev(
        context, st.scaled, st.ev_off, kmer_model.get_k(), kmer_model.get_central_position(), st.mean, st.ac, st.mc,
        *st.costs, st.status_in, st.cap_off)
    tick('decode')
    return st


def decode_batch(read_batch, kmer_model=defaults.KMER_MODEL_FILE, p_stay=0.7, p_skip=0.01, sigma_scale=1.0,
                 min_events=32, window=2, threshold=5.0, var_floor=0.02, context=None, qualities=False, fit=0,
                 fit_params=decode_fit.FIT_PARAMS, fit_start=None):
    """A base sequence and its base -> sample table for every read of ``read_batch`` from its raw signal alone (module
    docstring); any sequence or table the batch carries is ignored.  ``kmer_model``: a KmerModel or a path (4 letters,
    k in 2..6, else ValueError); ``context``: the context a model loaded from a path is made on (default: the
    process-wide one).  ``p_stay`` / ``p_skip``: the chances that an event stays in its k-mer or passes one;
    ``sigma_scale``: the model's sigma is multiplied by it; ``min_events`` (>= 1): a read with fewer is not decoded;
    ``window``, ``threshold``, ``var_floor``: the event detector's.  The defaults are uncalibrated: they are the values
    at which the simulated reads of the test suite (dwell 3-17 samples, noise 0.35, the packaged 6-mer table) decode
    best (the batch of the quality test is the tuning set), not values fitted to real data.  ``qualities``: also run
    the forward-backward operator and fill ``loglik``, ``base_post`` and ``quality`` (stage 5 of the module docstring);
    the other results do not change.  ``fit``: rounds of the Baum-Welch fit (module docstring; 0: none, and nothing
    changes); ``fit_params``: what it fits, a choice of 'scale' (per read, scale and shift), 'sigma' (pooled, the factor
    on sigma) and 'moves' (pooled, ``p_stay`` / ``p_skip``), the rest staying at the arguments; ``fit_start``: the
    ``DecodeBatch.fit`` of an earlier call on the same batch, whose per-read scale and shift the reads start from (its
    pooled values are passed as ``sigma_scale``, ``p_stay`` and ``p_skip``; with ``fit=0`` they are only applied).
    -> DecodeBatch."""
    import torch
    kmer_model = resolve_kmer_model(kmer_model, context)
    check_table(kmer_model)
    if int(min_events) < 1:
        raise ValueError('decode_batch: min_events is at least 1')
    rounds, groups = decode_fit.check_params(fit, fit_params)
    rb = read_batch
    st = decode_stages(rb, kmer_model, p_stay, p_skip, sigma_scale, min_events, window, threshold, var_floor,
                       fit=(rounds, groups, fit_start) if rounds > 0 or fit_start is not None else None)
    dev = st.ev_off.device
    status, n_ev, n_bases = st.hit[:, 0], st.hit[:, 1].to(torch.int64), st.hit[:, 2].to(torch.int64)
    ok = status == DEC_OK
    score = torch.where(ok, st.path_score / torch.clamp(n_ev, min=1).to(torch.float64),
                        torch.full_like(st.path_score, float('nan')))
    # the compaction: read r's n_bases entries lie at cap_off[r]
    seq_off = offsets_of(n_bases)
    owner, inner = seg_index(seq_off)
    at = st.cap_off[:-1][owner] + inner
    sequence, event = st.seq[at], st.base_event[at].to(torch.int64)
    map_base, map_sig, map_off, keep, _ = map_rows_dev(owner, inner, event, st.ev_start, st.ev_off, rb.n)
    host = lambda t: t.cpu().numpy()
    extra = {}
    if qualities:
        from .device import kmer_posterior_dev
        marg, z, _, post_parts = kmer_posterior_dev(
            kmer_model.context, st.scaled, st.ev_off, kmer_model.get_k(), kmer_model.get_central_position(), st.mean,
            st.ac, st.mc, *st.weights, st.status_in)
        loglik, base_post, quality = base_qualities_dev(marg, z, ok, n_ev, st.ev_off, map_off, owner, keep, sequence,
                                                        event)
        extra = dict(loglik=host(loglik), base_post=host(base_post), quality=host(quality), post_parts=post_parts)
    return DecodeBatch(host(status), host(st.hit[:, 1]), host(st.hit[:, 2]), host(score), host(seq_off),
                       host(sequence), host(map_base), host(map_sig), host(map_off), st.parts, fit=st.fit,
                       **extra)
