"""ProbabilityEstimator / Chunk (mirrors /root/reference/nadavca/estimator.py:7-236).

Same public methods and results as the reference; the difference is the execution plan: the
reference loops over reads and calls the DP once per read, here every stage is one batched GPU
launch over all reads —
    refine_alignment (tweak pre-pass)  -> expected levels -> [host: spline tweak, scipy]
    -> estimate_log_likelihoods -> normalise / strand-flip / per-position sum (consensus kernel)
    -> windowed posterior kernel.
Nothing numerical runs on the CPU except the spline FIT of ``Read.tweak_signal_normalization``
(FITPACK ``splrep``, a host step of the reference adjacent to the path, the same scipy call); its
evaluation over the signals is a kernel that restates FITPACK's ``splev`` bit for bit.  From the
log-likelihoods on, the buffers stay on the device, and the steps after them (``consensus_chunks``,
``independent_chunks``) are the ones ``estimate_snps_batch`` runs.
"""
import numpy

from . import dtw
from .alphabet import alphabet
from .batchflow import check_status
from .device import DeviceBatch, estimate_log_likelihoods_dev, consensus_accumulate_dev, posterior_segments_dev
from .genome import Genome


class Chunk:
    def __init__(self, start, end, values, coverage=None, contig=None):
        self.start = start
        self.end = end
        self.values = values
        self.coverage = coverage
        self.contig = contig   # the contig's name where the reference was a refset.ReferenceSet (start / end local)
        if coverage is None:
            self.coverage = numpy.ones(end - start, dtype=int)

    def __lt__(self, other):
        if self.start == other.start:
            return self.end < other.end
        return self.start < other.start

    @staticmethod
    def print_head(file):
        file.write('index\tbase\tcoverage\t{}\n'.format('\t'.join(alphabet)))

    def print(self, file, reference):
        for i in range(self.start, self.end):
            values_string = '\t'.join(map('{:18.16f}'.format, self.values[i - self.start]))
            file.write('{}\t{}\t{}\t{}\n'.format(i, reference[i], self.coverage[i - self.start],
                                                 values_string))


class _Prepared:
    """Per-read inputs of the DP, sliced exactly as estimator.py:59-74 / 158-170 do."""
    __slots__ = ('read', 'apx', 'reference_part', 'signal_range', 'context_before', 'context_after')


class ProbabilityEstimator:
    def __init__(self, kmer_model, aligner, config):
        self.kmer_model = kmer_model
        self.aligner = aligner
        self.bandwidth = config['bandwidth']
        self.snp_prior = config['snp_prior_probability']
        self.min_event_length = config['min_event_length']
        self.model_wobbling = config['model_wobbling']
        self.model_transitions = config['model_transitions']
        self.normalization_event_length = config['normalization_event_length']
        self.tweak_signal_normalization = config['tweak_signal_normalization']

    # ---- slicing (host) ------------------------------------------------------------------------
    def _get_read_context(self, read, read_sequence_range):
        start, end = read_sequence_range
        k = self.kmer_model.get_k()
        central = self.kmer_model.get_central_position()
        # a negative slice start wraps, as in the reference (estimator.py:53)
        before = Genome.to_numerical(read.sequence[start - central: start])
        after = Genome.to_numerical(read.sequence[end: end + k - central - 1])
        return before, after

    def _prepare(self, read, reference=None):
        apx = self.aligner.get_signal_alignment(read, self.bandwidth)
        if apx is None:
            return None
        p = _Prepared()
        p.read, p.apx = read, apx
        if reference is None:
            part = apx.reference_part
        else:  # estimator.py:64-68 re-slices the caller's reference
            s, e = apx.reference_range
            part = reference[s:e]
            if apx.reverse_complement:
                part = Genome.reverse_complement(part)
        p.reference_part = Genome.to_numerical(part)
        p.signal_range = apx.signal_range
        p.context_before, p.context_after = self._get_read_context(read, apx.read_sequence_range)
        return p

    @staticmethod
    def _dp_tuple(p, signal):
        s, e = p.signal_range
        return (signal[s:e], p.reference_part, p.context_before, p.context_after, p.apx.alignment)

    # ---- alignment -------------------------------------------------------------------------------
    def get_refined_alignments(self, reads):
        """Batched ``get_refined_alignment``: list of (approximate_alignment, (R,3) int array) or
        None per read (estimator.py:158-196)."""
        prepared = [self._prepare(r) for r in reads]
        live = [p for p in prepared if p is not None]
        events = dtw.refine_alignment_batch(
            [self._dp_tuple(p, p.read.normalized_signal) for p in live], self.bandwidth,
            self.min_event_length, self.kmer_model, self.model_transitions) if live else []
        it = iter(events)
        evs = [None if p is None else next(it) for p in prepared]
        # None where the read was not aligned or the band holds no valid path
        return [None if ev is None or len(ev) == 0 else (p.apx, self._alignment_rows(p, ev))
                for p, ev in zip(prepared, evs)]

    def get_refined_alignment(self, read):
        return self.get_refined_alignments([read])[0]

    def _alignment_rows(self, p, ev):
        s0 = p.signal_range[0]
        start_ref, end_ref = p.apx.reference_range
        res = numpy.zeros((len(ev), 3), dtype=int)
        pos = numpy.arange(len(ev))
        res[:, 0] = (end_ref - pos - 1) if p.apx.reverse_complement else (start_ref + pos)
        res[:, 1] = ev[:, 0] + s0
        res[:, 2] = ev[:, 1] + s0
        return res

    def _device(self):
        import torch
        return torch.device('cuda', self.kmer_model.context.device)

    def refine_and_renormalize(self, reads, renorm_rounds):
        """``align_signal``'s per-read loop (align_signal.py:55-80) for all reads at once and without
        leaving the device between rounds: align, then alternately re-fit the normalisation linearly
        against the model's expected levels (even rounds) and align again (odd rounds) —
        ``device.refine_renorm_loop_dev``.  Every read's ``normalized_signal`` ends up rescaled as in
        the reference.  -> list of (approximate_alignment, (R,3) int array) or None per read."""
        from .device import refine_renorm_loop_dev
        prepared = [self._prepare(r) for r in reads]
        live = [p for p in prepared if p is not None]
        if not live:
            return [None] * len(prepared)
        batch = dtw.FlatBatch([self._dp_tuple(p, p.read.normalized_signal) for p in live])
        dbatch = DeviceBatch(batch, self._device())
        events, status, fits = refine_renorm_loop_dev(dbatch, self.bandwidth, self.min_event_length,
                                                      self.kmer_model, self.model_transitions, renorm_rounds)
        events, status = events.cpu().numpy(), status.cpu().numpy()
        fits = [f.cpu().numpy() for f in fits]
        # (a too-wide band is a ValueError here, not the NadavcaHipError of the dtw operators: kept as it was)
        check_status('refine_alignment', status, too_wide='invalid')
        out, j = [], 0
        for p in prepared:
            if p is None:
                out.append(None)
                continue
            if status[j] != 0:
                out.append(None)
            else:
                # the same two linear maps for the samples outside the aligned slice (the reference
                # rescales the whole read, align_signal.py:73)
                for f in fits:
                    p.read.normalized_signal = (p.read.normalized_signal - f[j, 1]) / f[j, 0]
                out.append((p.apx, self._alignment_rows(p, events[batch.ref_off[j]:batch.ref_off[j + 1]])))
            j += 1
        return out

    # ---- SNP scoring -----------------------------------------------------------------------------
    def _log_likelihood_batch(self, reference, reads):
        """Stages shared by both modes: -> (live prepared reads, DeviceBatch, ll (sum R, 4), status), the last
        three on the device.  A refused read raises (batchflow.check_status), as the per-read operators do."""
        prepared = [self._prepare(r, reference) for r in reads]
        live = [p for p in prepared if p is not None]
        if not live:
            return [], None, None, None
        if self.tweak_signal_normalization:
            pre = dtw.refine_alignment_batch(
                [self._dp_tuple(p, p.read.normalized_signal) for p in live], self.bandwidth,
                self.min_event_length, self.kmer_model, False)
            expected = self.kmer_model.get_expected_signal_batch(
                [(p.reference_part, p.context_before, p.context_after) for p in live])
            fitted, splines = [], []
            for p, ev, exp in zip(live, pre, expected):
                if len(ev) == 0:
                    # the reference would index an empty array here and fail; keep the untweaked signal
                    p.read.tweaked_normalized_signal = p.read.normalized_signal
                    continue
                # the fit on the host (FITPACK splrep, the reference's call), the evaluation over the
                # whole signal for all reads in one kernel
                splines.append(p.read.fit_signal_tweak(numpy.asarray(ev) + p.signal_range[0], exp))
                fitted.append(p.read)
            from .read import Read
            Read.apply_signal_tweaks_device(fitted, splines, context=self.kmer_model.context)
            signals = [p.read.tweaked_normalized_signal for p in live]
        else:
            signals = [p.read.normalized_signal for p in live]
        dbatch = DeviceBatch(dtw.FlatBatch([self._dp_tuple(p, s) for p, s in zip(live, signals)]), self._device())
        ll, status = estimate_log_likelihoods_dev(dbatch, self.bandwidth, self.min_event_length, self.kmer_model,
                                                  self.model_wobbling)
        check_status('estimate_log_likelihoods', status)
        return live, dbatch, ll, status

    @staticmethod
    def group_ranges(ranges):
        """Merge sorted (start, end) chunk intervals into groups while next.start < current_end;
        touching chunks do not merge (estimator.py:205-220)."""
        ranges = sorted(ranges)
        groups, cur_s, cur_e = [], None, None
        for idx, (s, e) in enumerate(ranges):
            if cur_s is None:
                cur_s, cur_e = s, e
            cur_e = max(cur_e, e)
            if idx + 1 >= len(ranges) or ranges[idx + 1][0] >= cur_e:
                groups.append((cur_s, cur_e))
                cur_s = cur_e = None
        return groups

    def local_consensus(self, reference, reads):
        """This process's share of the consensus: per-position sums of the normalised,
        strand-corrected log-likelihoods of ``reads`` over the whole reference, the coverage, and
        the chunk intervals (estimator.py:199-231).  -> (acc (L,4) f64, cov (L,) i64 device tensors, ranges)."""
        import torch
        acc = torch.zeros((len(reference), self.kmer_model.alphabet_size), dtype=torch.float64, device=self._device())
        cov = torch.zeros(len(reference), dtype=torch.int64, device=self._device())
        live, dbatch, ll, status = self._log_likelihood_batch(reference, reads)
        if not live:
            return acc, cov, []
        start = _upload([p.apx.reference_range[0] for p in live], numpy.int64, dbatch.device)
        reverse = _upload([p.apx.reverse_complement for p in live], numpy.int32, dbatch.device)
        consensus_accumulate_dev(self.kmer_model.context, dbatch, ll, start, reverse, status,
                                 self.normalization_event_length, len(reference), acc, cov)
        ok = (status == dtw.READ_OK).cpu().numpy()
        return acc, cov, [tuple(int(v) for v in p.apx.reference_range) for p, o in zip(live, ok) if o]

    def estimate_probabilities(self, reference, reads):
        """Consensus over all reads (estimator.py:199-236) -> list of Chunk(start, end, posterior,
        coverage), one per group of overlapping reads."""
        acc, cov, ranges = self.local_consensus(reference, reads)
        return consensus_chunks(self.kmer_model, self.snp_prior, reference, acc, cov, ranges)

    def estimate_probabilities_independent(self, reference, reads):
        """``[estimate_probabilities(reference, [read])[0] for read in reads]`` in batched form
        (estimate_snps.py:63-68); None for a read that yields no chunk."""
        live, dbatch, ll, status = self._log_likelihood_batch(reference, reads)
        if not live:
            return [None] * len(reads)
        # the reference's base codes over every read's chunk, laid out as ll
        codes = _upload(numpy.concatenate([_codes(reference, *p.apx.reference_range) for p in live]), numpy.int32,
                        dbatch.device)
        reverse = _upload([p.apx.reverse_complement for p in live], numpy.int32, dbatch.device)
        ok, values, row_off = independent_posteriors(self.kmer_model, self.snp_prior, self.normalization_event_length,
                                                     dbatch, ll, status, reverse, codes)
        kept = [p for p, o in zip(live, ok) if o]
        result = {id(p.read): Chunk(*p.apx.reference_range, values[a:b]) for p, a, b in zip(kept, row_off, row_off[1:])}
        return [result.get(id(r)) for r in reads]


# ---- the steps after the log-likelihoods, shared by ProbabilityEstimator and estimate_snps_batch ---------------
def _upload(values, dtype, device):
    import torch
    return torch.from_numpy(numpy.ascontiguousarray(values, dtype=dtype)).to(device)


def _codes(reference, s, e):
    """Base codes (i32) of ``reference[s:e]``; bases are converted only here (KeyError on anything but ACGT)."""
    part = reference[s:e]
    if numpy.asarray(part).dtype.kind in 'iu':
        return numpy.asarray(part, dtype=numpy.int32)
    return Genome.to_numerical(part).astype(numpy.int32)


def group_sums(acc, ranges):
    """Group the chunk intervals (estimator.py:205-220), each group's sums end to end: -> (groups, seg_off, ll_cat)."""
    groups = ProbabilityEstimator.group_ranges(ranges)
    seg_off = numpy.cumsum([0] + [e - s for s, e in groups], dtype=numpy.int64)
    pos = numpy.concatenate([numpy.arange(s, e) for s, e in groups] + [numpy.zeros(0, numpy.int64)])
    return groups, seg_off, acc[_upload(pos, numpy.int64, acc.device)]


def consensus_chunks(kmer_model, snp_prior, reference, acc, cov, ranges, distributed=False, group=None, dst=0):
    """Per-position sums (``acc``, ``cov``: device tensors) and the chunk intervals of the reads in them -> grouped
    posteriors (estimator.py:205-236), a Chunk list.  Distributed: the sums of all ranks meet in ONE reduce of the
    packed device buffer, the intervals in a small all-gather; the posterior runs on ``dst`` (None elsewhere)."""
    if distributed:
        from . import distributed as D
        ranges = D.gather_ranges(ranges, device=acc.device, group=group)
        total = D.reduce_consensus_tensors(acc, cov, dst=dst, group=group)
        if total is None:
            return None
        acc, cov = total
    groups, seg_off, ll_cat = group_sums(acc, ranges)
    if not groups:
        return []
    codes = numpy.concatenate([_codes(reference, s, e) for s, e in groups])
    post = posterior_segments_dev(kmer_model.context, ll_cat, _upload(codes, numpy.int32, acc.device),
                                  _upload(seg_off, numpy.int64, acc.device), kmer_model.get_k(), snp_prior)
    post, cov = post.cpu().numpy(), cov.cpu().numpy()
    return [Chunk(s, e, post[seg_off[g]:seg_off[g + 1]], cov[s:e].copy()) for g, (s, e) in enumerate(groups)]


def independent_posteriors(kmer_model, snp_prior, normalization_event_length, dbatch, ll, status, reverse,
                           ref_codes):
    """Every read of ``dbatch`` its own segment (estimate_snps.py:63-68): its normalised, strand-corrected rows of
    ``ll`` and their posterior.  ``ref_codes``: the reference's base codes over the reads' chunks, laid out as
    ``ll``.  -> (ok: status 0 per read, posterior rows of the ok reads end to end, their row offsets)."""
    context = kmer_model.context
    acc, _ = consensus_accumulate_dev(context, dbatch, ll, dbatch.ref_off[:-1].contiguous(), reverse, status,
                                      normalization_event_length, dbatch.total_ref)
    post = posterior_segments_dev(context, acc, ref_codes, dbatch.ref_off, kmer_model.get_k(), snp_prior)
    ok = (status == dtw.READ_OK).cpu().numpy()
    lens = numpy.diff(dbatch.ref_off.cpu().numpy())
    rows = numpy.nonzero(numpy.repeat(ok, lens))[0]
    return ok, post.cpu().numpy()[rows], numpy.cumsum([0] + lens[ok].tolist(), dtype=numpy.int64)
