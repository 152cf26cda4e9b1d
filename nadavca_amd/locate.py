"""``signal_locate_batch``: where every read of a ``ReadBatch`` lies on a small reference, from its raw signal alone.

``SeedAligner`` seeds from a basecalled sequence and ``signal_map_batch`` aligns the events to it.  This module needs
neither: the k-mer table turns the reference into expected levels, the event detector turns the signal into levels,
and a subsequence DTW between the two finds the read, as UNCALLED, sigmap, RawHash, DTWax and SquiggleFilter do for
viral and mitochondrial genomes, plasmids and amplicon panels.  The cost is a dense DP of every read against every
column of both strands: it serves references of up to some 10^5 bases, there is no index.  On the device:

1. per-read median / MAD normalisation (``nvk_normalize_groups_dev``) and 2. event detection, both
   ``signal_map_batch``'s own;
3. the column tables of the targets — per contig its forward strand, then its reverse complement — by
   ``signal_map.base_tables_dev``;
4. a rescale by moments (``rawsignal.rescale_by_moments_dev``): the events' per-read median and MAD are mapped onto
   those of ALL columns pooled (there is no sequence to take them from).  A read with fewer than ``min_events`` events
   or a zero MAD is ``LOC_NO_EVENTS``;
5. chunks: a read of E events is cut into nc = ceil(E / max_events) chunks at (E * c) // nc, each one query;
6. the operator (``nvk_signal_locate_dev``, contract in include/nadavca_hip.h): per (query, block of 256 columns) the
   best path's end value, end, start and trimmed events.  The queries run in parts whose block table fits a cap;
7. a reduction per chunk: best = the largest block best (the smallest block among equal ones); second = the largest
   block best among the blocks of other targets and those of the same target that do not intersect
   [end - 2 Q, end + 2 Q]; margin = (best - second) / Q, nats per event, +inf without another block;
8. the chain, per read: the anchor is the chunk of largest margin (the first among equal ones); below ``min_margin``
   the read is ``LOC_AMBIGUOUS``.  Walking outwards from the anchor in both directions a chunk joins when it is on the
   anchor's target, its margin is >= ``min_margin`` and, against the last joined chunk, -16 <= gap <= between + 16:
   ``gap`` the columns between the two paths, ``between`` the events between them (those of unjoined chunks in between
   and the trimmed ones at the two facing ends).  The window runs from the smallest start column to the largest end
   column + 1 of the joined chunks.

With it every batch workflow runs from raw signal and a FASTA alone:

    rb0 = ReadBatch.from_signals(raw, sig_off, np.zeros(0, np.int32), np.zeros(n + 1, np.int64))
    loc = signal_locate_batch(rb0, reference)
    rb1 = loc.read_batch(rb0)
    rb2 = signal_map_batch(rb1).read_batch(rb1)
    align_signal_batch(None, rb2, aligner=loc.aligner())
"""
import math

import numpy as np

from . import _lib, defaults
from .batchflow import seg_index
from .rawsignal import (SignalEvents, offsets_of, rescale_by_moments_dev, resolve_kmer_model, signal_events_dev,
                        transition_costs)
from .readbatch import BaseAlignmentBatch, ReadBatch
from .refset import ReferenceSet

LOC_OK, LOC_NO_EVENTS, LOC_AMBIGUOUS = _lib.LOC_OK, _lib.LOC_NO_EVENTS, _lib.LOC_AMBIGUOUS
BLOCK = _lib.LOC_BLOCK
GAP_SLACK = 16                 # columns two joined paths may overlap by, or lie apart beyond the events between them
DEFAULT_TABLE_CAP = 256 << 20  # bytes of block table per part while the context has no workspace limit
TABLE_BYTES = 24               # per (query, block): an f64 and four i32


class LocatedAligner:
    """The identity alignment of a located batch (``LocateBatch.aligner``): it drops in where ``SeedAligner`` does.
    ``reference_num``: the reference as base codes (the concatenation of a ``ReferenceSet``, which ``reference_set``
    then is, else None)."""

    def __init__(self, loc):
        self._loc = loc
        self.reference_set = loc.reference_set
        self.reference_num = loc.reference_num

    def get_base_alignments(self, read_batch):
        """-> BaseAlignmentBatch: read base b of a located read on oriented window start + b; no pairs otherwise."""
        loc = self._loc
        if read_batch.n != loc.n:
            raise ValueError('LocatedAligner: the batch holds %d reads, the location %d' % (read_batch.n, loc.n))
        off = np.zeros(loc.n + 1, dtype=np.int64)
        np.cumsum(loc.win_len, out=off[1:])
        owner = np.repeat(np.arange(loc.n), loc.win_len)
        inner = np.arange(int(off[-1]), dtype=np.int64) - off[:-1][owner]
        return BaseAlignmentBatch(inner, loc.win_start[owner] + inner, off, loc.reverse,
                                  contig=None if loc.reference_set is None else loc.contig)


class LocateBatch:
    """What ``signal_locate_batch`` returns, numpy arrays.  Per read: ``status`` (LOC_OK; LOC_NO_EVENTS: fewer than
    ``min_events`` events or events that all have one level; LOC_AMBIGUOUS: no chunk stands out by ``min_margin``),
    ``contig`` (int32, -1 unless located), ``reverse`` (bool), ``ref_start`` / ``ref_end`` (int64: the window on the
    forward strand, inside the contig; -1 unless located), ``margin`` (the anchor chunk's, nats per event) and
    ``score`` (the anchor chunk's best end value per event), both NaN for LOC_NO_EVENTS, ``n_events``, ``n_chunks``,
    ``n_joined``, ``first_event`` / ``last_event`` (the first and last event on the joined chunks' paths, counted in
    the read; -1 unless located), ``win_start`` / ``win_len`` (the window in the oriented coordinates of its target,
    ``BaseAlignmentBatch``'s: counted from the contig's end on the reverse strand).
    With ``chunks=True``: ``chunk_off`` (int64, n + 1) and per chunk ``chunk_target`` (2 * contig + strand),
    ``chunk_start`` / ``chunk_end`` (first and last column of its best path), ``chunk_first_event`` /
    ``chunk_last_event`` (in the read), ``chunk_events``, ``chunk_score``, ``chunk_margin``, ``chunk_joined``;
    otherwise None."""

    CHUNK_FIELDS = ('chunk_off', 'chunk_target', 'chunk_start', 'chunk_end', 'chunk_first_event', 'chunk_last_event',
                    'chunk_events', 'chunk_score', 'chunk_margin', 'chunk_joined')

    def __init__(self, reference, fields, chunk_fields=None):
        self.reference_set = reference if isinstance(reference, ReferenceSet) else None
        self.reference_num = reference.codes if self.reference_set is not None else reference
        for k, v in fields.items():
            setattr(self, k, v)
        for k in LocateBatch.CHUNK_FIELDS:
            setattr(self, k, None if chunk_fields is None else chunk_fields[k])
        self.n = int(self.status.size)
        self.n_located = int((self.status == LOC_OK).sum())

    def read_batch(self, rb):
        """A new ``ReadBatch`` with ``rb``'s signals and, as each read's sequence, the reference window it was located
        on, in the read's orientation; the base -> sample tables are empty (``signal_map_batch`` fills them).  A read
        that is not located gets an empty sequence."""
        if rb.n != self.n:
            raise ValueError('LocateBatch.read_batch: the batch holds %d reads, the location %d' % (rb.n, self.n))
        _, codes, col_off, _ = target_tables(self.reference_set if self.reference_set is not None
                                             else self.reference_num)
        seq_off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.win_len, out=seq_off[1:])
        owner = np.repeat(np.arange(self.n), self.win_len)
        inner = np.arange(int(seq_off[-1]), dtype=np.int64) - seq_off[:-1][owner]
        target = 2 * self.contig.astype(np.int64) + self.reverse
        sequence = codes[col_off[target[owner]] + self.win_start[owner] + inner]
        return ReadBatch.from_signals(rb.raw_signal, rb.sig_off, sequence, seq_off)

    def aligner(self):
        return LocatedAligner(self)


def target_tables(reference):
    """``reference``: base codes or a ``ReferenceSet`` -> (the set or None, codes int32, col_off int64, contig lengths):
    the targets laid end to end, per contig its forward strand, then its reverse complement."""
    if isinstance(reference, ReferenceSet):
        refset, contigs = reference, [reference.contig_codes(c) for c in range(reference.n_contigs)]
    else:
        refset, contigs = None, [np.ascontiguousarray(reference, dtype=np.int32).reshape(-1)]
    parts, lengths = [], []
    for c in contigs:
        parts += [c.astype(np.int32), (3 - c[::-1]).astype(np.int32)]
        lengths += [c.size, c.size]
    codes = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    col_off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=col_off[1:])
    return refset, codes, col_off, np.array([c.size for c in contigs], dtype=np.int64)


def block_tables(col_off):
    """The blocks of the operator's output over targets at ``col_off`` (int64 tensor) -> (target, first column, end
    column) per block, int64 tensors."""
    import torch
    lens = col_off[1:] - col_off[:-1]
    blk_off = offsets_of((lens + (BLOCK - 1)) // BLOCK)
    target, inner = seg_index(blk_off)
    lo = inner * BLOCK
    return target, lo, torch.minimum(lo + BLOCK, lens[target])


def cut_chunks(n_ev, ok, max_events):
    """Stage 5 on tensors: per read its event count and whether it takes part -> (chunk_off per read, and per chunk its
    read, its first event inside the read and its event count)."""
    import torch
    E = torch.where(ok, n_ev, torch.zeros_like(n_ev))
    nc = (E + (max_events - 1)) // max_events
    chunk_off = offsets_of(nc)
    read, c = seg_index(chunk_off)
    first = (E[read] * c) // nc[read]
    return chunk_off, read, first, (E[read] * (c + 1)) // nc[read] - first


def reduce_blocks(score, hit, n_events, blk_target, blk_lo, blk_hi):
    """Stage 7 for a part of the queries: ``score`` (q, blocks) / ``hit`` (q, blocks, 4) of the operator, ``n_events``
    per query, the block tables -> (best block, best score, second score, margin, the best block's hit (q, 4))."""
    import torch
    nq, nb = score.shape
    idx = torch.arange(nb, dtype=torch.int64, device=score.device)
    best = score.amax(dim=1)
    blk = torch.where(score == best[:, None], idx[None, :], nb).amin(dim=1).clamp(max=nb - 1)
    top = hit[torch.arange(nq, device=score.device), blk].to(torch.int64)
    end, reach = top[:, 0], 2 * n_events
    near = (blk_target[None, :] == blk_target[blk][:, None]) & (blk_lo[None, :] <= (end + reach)[:, None]) \
        & (blk_hi[None, :] - 1 >= (end - reach)[:, None])
    second = torch.where(near, float('-inf'), score).amax(dim=1)
    margin = torch.nan_to_num((best - second) / n_events.to(torch.float64), nan=float('-inf'), posinf=float('inf'),
                              neginf=float('-inf'))
    return blk, best, second, margin, top


def table_cap(context):
    """Bytes of block table a part may take: ``nvk_ctx_set_workspace_limit``'s value, or the default."""
    limit = int(getattr(context, 'workspace_limit', 0) or 0)
    return limit if limit > 0 else DEFAULT_TABLE_CAP


def locate_queries_dev(context, level, q_off, mu, ac, mc, col_off, max_events, l_stay, l_step, l_skip, trim_cost,
                       cap=None):
    """Stages 6 and 7: the operator over the queries in parts whose block table fits ``cap`` bytes (default:
    ``table_cap``; a single query's table larger than the cap runs on its own), each part reduced before the next
    runs -> (best block, best, second, margin, hit (q, 4)) per query and the number of parts."""
    import torch
    from .device import signal_locate_dev
    dev = q_off.device
    nq = int(q_off.numel()) - 1
    blk_target, blk_lo, blk_hi = block_tables(col_off)
    nb = int(blk_target.numel())
    cap = table_cap(context) if cap is None else int(cap)
    per = max(1, cap // max(nb * TABLE_BYTES, 1))
    out, parts = [], 0
    q_host = q_off.cpu()
    for q0 in range(0, nq if nb else 0, per):
        q1 = min(nq, q0 + per)
        lo, hi = int(q_host[q0]), int(q_host[q1])
        score, hit = signal_locate_dev(context, level[lo:hi], (q_off[q0:q1 + 1] - lo).contiguous(), mu, ac, mc, col_off,
                                       max_events, l_stay, l_step, l_skip, trim_cost)
        n_events = q_off[q0 + 1:q1 + 1] - q_off[q0:q1]
        out.append(reduce_blocks(score, hit, n_events, blk_target, blk_lo, blk_hi))
        parts += 1
    if not out or nb == 0:
        z = lambda dt: torch.zeros(nq if nb == 0 else 0, dtype=dt, device=dev)
        ninf = torch.full((nq if nb == 0 else 0,), float('-inf'), dtype=torch.float64, device=dev)
        return (z(torch.int64), ninf, ninf.clone(), ninf.clone(),
                torch.full((nq if nb == 0 else 0, 4), -1, dtype=torch.int64, device=dev)), parts
    return tuple(torch.cat([o[k] for o in out]) for k in range(5)), parts


def chain_chunks(chunk_off, target, start, end, first_event, last_event, margin, min_margin):
    """Stage 8 on per-chunk rows (tensors, any device; ``first_event`` / ``last_event`` counted in the read) ->
    (status per read: LOC_OK or LOC_AMBIGUOUS, LOC_NO_EVENTS for a read without chunks; anchor: the anchor's flat chunk
    index, -1 without chunks; joined bool per chunk).  Integer arithmetic but for the comparisons of the margins."""
    import torch
    dev = chunk_off.device
    n, total = int(chunk_off.numel()) - 1, int(target.numel())
    nc = chunk_off[1:] - chunk_off[:-1]
    status = torch.where(nc > 0, LOC_AMBIGUOUS, LOC_NO_EVENTS).to(torch.int32)
    anchor = torch.full((n,), -1, dtype=torch.int64, device=dev)
    joined = torch.zeros(total, dtype=torch.bool, device=dev)
    if total == 0:
        return status, anchor, joined
    read, inner = seg_index(chunk_off, total)
    top = torch.full((n,), float('-inf'), dtype=torch.float64, device=dev).scatter_reduce(
        0, read, margin, 'amax', include_self=True)
    first = torch.full((n,), total, dtype=torch.int64, device=dev).scatter_reduce(
        0, read, torch.where(margin == top[read], inner, total), 'amin', include_self=True)
    has = nc > 0
    a_in = torch.where(has, first, 0)                      # the anchor inside its read
    a_flat = torch.where(has, chunk_off[:-1] + a_in, 0)
    anchor = torch.where(has, a_flat, -1)
    located = has & (margin[a_flat] >= min_margin)
    status = torch.where(located, LOC_OK, status.to(torch.int64)).to(torch.int32)
    joined[a_flat[located]] = True
    base = chunk_off[:-1]
    for direction in (1, -1):
        last = a_in.clone()
        for d in range(1, int(nc.max())):
            c = a_in + direction * d
            live = located & (c >= 0) & (c < nc)
            at, prev = base + torch.where(live, c, a_in), base + last
            at, prev = torch.where(has, at, 0), torch.where(has, prev, 0)
            if direction > 0:
                gap = start[at] - end[prev] - 1
                between = first_event[at] - last_event[prev] - 1
            else:
                gap = start[prev] - end[at] - 1
                between = first_event[prev] - last_event[at] - 1
            join = live & (target[at] == target[a_flat]) & (margin[at] >= min_margin) & (gap >= -GAP_SLACK) \
                & (gap <= between + GAP_SLACK)
            joined[at[join]] = True
            last = torch.where(join, c, last)
    return status, anchor, joined


class LocateStages(SignalEvents):
    """The device tensors between the stages of one ``signal_locate_batch`` call (``signal_locate_stages``)."""
    __slots__ = ('mu', 'ac', 'mc', 'col_off', 'scaled', 'ok', 'chunk_off', 'chunk_read', 'chunk_first', 'chunk_events',
                 'q_off', 'q_level', 'blk', 'best', 'second', 'margin', 'hit', 'parts', 'n_blocks', 'costs')


def signal_locate_stages(read_batch, targets, kmer_model, max_events, min_events, p_stay, p_skip, sigma_scale,
                         trim_cost, window, threshold, var_floor, timer=None):
    """Stages 1 to 7 on the device -> LocateStages.  ``targets``: what ``target_tables`` returned; ``timer(name)``:
    called after each stage (bench tool)."""
    import torch
    from .signal_map import base_tables_dev
    context = kmer_model.context
    device = torch.device('cuda', context.device)
    rb, st = read_batch, LocateStages()
    tick = timer if timer is not None else (lambda name: None)
    _, codes, col_off, _ = targets
    st.col_off = torch.from_numpy(col_off).to(device)
    sequence = torch.from_numpy(codes).to(device)
    signal_events_dev(rb, context, window, threshold, var_floor, tick, into=st)
    st.mu, st.ac, st.mc = base_tables_dev(kmer_model, sequence, st.col_off, sigma_scale)
    tick('tables')
    pool_off = torch.tensor([0, int(st.mu.numel())], dtype=torch.int64, device=device)
    st.scaled, _, _, st.ok = rescale_by_moments_dev(context, st.ev_level, st.ev_off, st.mu, pool_off,
                                                    min_events=min_events)
    st.chunk_off, st.chunk_read, st.chunk_first, st.chunk_events = cut_chunks(st.ev_off[1:] - st.ev_off[:-1], st.ok,
                                                                               max_events)
    # the queries' levels end to end: the events of the reads that take part
    owner, _ = seg_index(st.ev_off, int(st.ev_level.numel()))
    st.q_level = st.scaled[st.ok[owner]].contiguous()
    st.q_off = offsets_of(st.chunk_events)
    tick('rescale')
    st.costs = transition_costs(p_stay, p_skip, 'signal_locate_batch')
    (st.blk, st.best, st.second, st.margin, st.hit), st.parts = locate_queries_dev(
        context, st.q_level, st.q_off, st.mu, st.ac, st.mc, st.col_off, max_events, *st.costs, trim_cost)
    st.n_blocks = int(block_tables(st.col_off)[0].numel())
    tick('locate')
    return st


def signal_locate_batch(read_batch, reference, kmer_model=defaults.KMER_MODEL_FILE, max_events=128, min_events=32,
                        min_margin=0.2, p_stay=0.5, p_skip=0.02, sigma_scale=0.5, trim_cost=math.log(0.01), window=2,
                        threshold=5.0, var_floor=0.02, context=None, chunks=False):
    """Where every read of ``read_batch`` lies on ``reference`` (base codes 0..3 or a ``ReferenceSet``), from its raw
    signal alone (module docstring); any sequence or table the batch carries is ignored.  ``kmer_model``: a KmerModel
    or a path; ``context``: the context a model loaded from a path is made on (default: the process-wide one).
    ``max_events`` (1..256): events per chunk; ``min_events`` (>= 1): a read with fewer is not tried; ``min_margin``:
    nats per event by which a chunk's best place must beat its second; ``p_stay`` / ``p_skip``: the chances that an
    event stays on its column or jumps one; ``sigma_scale`` and ``trim_cost`` as in ``signal_map_batch``; ``window``,
    ``threshold``, ``var_floor``: the event detector's.  The defaults are uncalibrated: they are the values a numpy
    prototype used on the simulated reads of the test suite (dwell 3-17 samples, noise 0.35, the packaged 6-mer table,
    a 3 000-base genome), not values fitted to real data.  -> LocateBatch."""
    import torch
    kmer_model = resolve_kmer_model(kmer_model, context)
    if not 1 <= int(max_events) <= _lib.LOC_MAX_EVENTS:
        raise ValueError('signal_locate_batch: max_events is 1..%d' % _lib.LOC_MAX_EVENTS)
    if int(min_events) < 1:
        raise ValueError('signal_locate_batch: min_events is at least 1')
    rb, max_events = read_batch, int(max_events)
    targets = target_tables(reference)
    refset, _, _, contig_len = targets
    st = signal_locate_stages(rb, targets, kmer_model, max_events, min_events, p_stay, p_skip, sigma_scale, trim_cost,
                              window, threshold, var_floor)
    dev = st.ev_off.device
    n = rb.n
    blk_target = block_tables(st.col_off)[0]
    q_target = blk_target[st.blk] if blk_target.numel() else torch.zeros_like(st.blk)
    end, last, start, first = st.hit[:, 0], st.hit[:, 1], st.hit[:, 2], st.hit[:, 3]
    first_g, last_g = st.chunk_first + first, st.chunk_first + last
    status, anchor, joined = chain_chunks(st.chunk_off, q_target, start, end, first_g, last_g, st.margin,
                                          float(min_margin))
    ok = status == LOC_OK
    read = st.chunk_read[joined]
    big = torch.iinfo(torch.int64).max
    seg_min = lambda v: torch.full((n,), big, dtype=torch.int64, device=dev).scatter_reduce(0, read, v[joined], 'amin')
    seg_max = lambda v: torch.full((n,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, read, v[joined], 'amax')
    minus = torch.full((n,), -1, dtype=torch.int64, device=dev)
    win_start = torch.where(ok, seg_min(start), 0)
    win_len = torch.where(ok, seg_max(end) + 1 - win_start, 0)
    at = torch.clamp(anchor, min=0)
    has = anchor >= 0
    empty = st.margin.numel() == 0
    pick = lambda v, fill: torch.full((n,), fill, dtype=v.dtype, device=dev) if empty else torch.where(
        has, v[at], torch.full((n,), fill, dtype=v.dtype, device=dev))
    target = pick(q_target, 0)
    contig = torch.where(ok, target // 2, minus)
    reverse = ok & (target % 2 == 1)
    length = torch.from_numpy(contig_len).to(dev)[torch.clamp(contig, min=0)] if contig_len.size else minus
    ref_start = torch.where(ok, torch.where(reverse, length - win_start - win_len, win_start), minus)
    ref_end = torch.where(ok, ref_start + win_len, minus)
    nan = float('nan')
    host = lambda t: t.cpu().numpy()
    fields = dict(
        status=host(status), contig=host(contig.to(torch.int32)), reverse=host(reverse), ref_start=host(ref_start),
        ref_end=host(ref_end), margin=host(pick(st.margin, nan)),
        score=host(pick(st.best / st.chunk_events.to(torch.float64), nan)),
        n_events=host((st.ev_off[1:] - st.ev_off[:-1]).to(torch.int32)),
        n_chunks=host((st.chunk_off[1:] - st.chunk_off[:-1]).to(torch.int32)),
        n_joined=host(torch.bincount(read, minlength=n).to(torch.int32)),
        first_event=host(torch.where(ok, seg_min(first_g), minus).to(torch.int32)),
        last_event=host(torch.where(ok, seg_max(last_g), minus).to(torch.int32)),
        win_start=host(win_start), win_len=host(win_len))
    chunk_fields = None
    if chunks:
        chunk_fields = dict(chunk_off=host(st.chunk_off), chunk_target=host(q_target.to(torch.int32)),
                            chunk_start=host(start), chunk_end=host(end), chunk_first_event=host(first_g),
                            chunk_last_event=host(last_g), chunk_events=host(st.chunk_events.to(torch.int32)),
                            chunk_score=host(st.best), chunk_margin=host(st.margin), chunk_joined=host(joined))
    return LocateBatch(refset if refset is not None else np.ascontiguousarray(reference, dtype=np.int32).reshape(-1),
                       fields, chunk_fields)
