"""``estimate_allele_fractions_batch`` — per reference position and per base other than the reference's, "which
share of the reads that cover this position carry this base?", by maximum likelihood over a two-component mixture.

``estimate_snps_batch`` adds the reads' normalised log-likelihood ratios per position and so asks whether ALL reads
carry a base: at a heterozygous site, in a heteroplasmic or viral population or in a pooled sample the reads that do
not carry it outvote the ones that do.  This workflow keeps the per-read ratios ``d_i`` and maximises
``L(f) = sum_i log((1 - f) + f exp(d_i))`` over the mixing fraction f per (position, base) — the contract is in
include/nadavca_hip.h (nvk_allele_rows_dev), the kernels in csrc/kernels_allele.hip.  Single process only: a mixture
needs every read's own value at a site, not a sum that ranks could exchange."""
import os

import numpy as np

from . import defaults


class AlleleFractionBatch:
    """What ``estimate_allele_fractions_batch`` returns.  Row arrays, one row per kept (position, alternative base),
    ascending in (global position, base): ``contig`` (an index into ``contig_names`` for a ``refset.ReferenceSet``; 0
    and None otherwise), ``position`` (forward, contig-local), ``ref_base``, ``alt_base`` (codes 0..3), ``coverage``
    (reads with status OK over the position), ``fraction`` (the estimate f^), ``lrt`` (2 L(f^): twice the
    log-likelihood gained over "no read carries it"), ``ll_half`` (L(1/2)), ``ll_full`` (L(1): the sum of the reads'
    ratios, the consensus sum at the consensus scale), ``genotype`` (0 / 1 / 2: the largest of (0, ll_half, ll_full),
    the first on ties), ``shadowed`` (some OTHER position within k - 1 bases, in the same contig, holds a larger lrt:
    a substitution changes the k-mers of its neighbours too, so the neighbours of a real variant score as well) and
    ``called`` (lrt >= threshold, fraction >= min_fraction and coverage >= min_coverage; all False without a
    threshold).  ``position_coverage``: the coverage of every position of the reference (of the concatenation for a
    ReferenceSet)."""

    FIELDS = ('contig', 'position', 'ref_base', 'alt_base', 'coverage', 'fraction', 'lrt', 'll_half', 'll_full',
              'genotype', 'shadowed', 'called')

    def __init__(self, contig, position, ref_base, alt_base, coverage, fraction, lrt, ll_half, ll_full, genotype,
                 shadowed, called, position_coverage, threshold=None, contig_names=None):
        self.contig, self.position, self.ref_base, self.alt_base = contig, position, ref_base, alt_base
        self.coverage, self.fraction, self.lrt, self.ll_half, self.ll_full = coverage, fraction, lrt, ll_half, ll_full
        self.genotype, self.shadowed, self.called = genotype, shadowed, called
        self.position_coverage, self.threshold, self.contig_names = position_coverage, threshold, contig_names

    @classmethod
    def empty(cls, ref_len, threshold=None, contig_names=None):
        z = lambda dt: np.zeros(0, dtype=dt)
        return cls(z(np.int32), z(np.int64), z(np.int8), z(np.int8), z(np.int64), z(np.float64), z(np.float64),
                   z(np.float64), z(np.float64), z(np.int8), z(bool), z(bool), np.zeros(int(ref_len), dtype=np.int64),
                   threshold, contig_names)

    def __len__(self):
        return int(self.position.size)

    def write_tsv(self, file):
        """Header, then one tab-separated row per kept (position, base): contig (by name where the
        batch has names), position, ref, alt, coverage, fraction, lrt, ll_half, ll_full (floats as ``repr`` gives
        them), genotype, shadowed and called (0 / 1), to ``file``, a path or a text file."""
        out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
        label = (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])
        try:
            out.write('contig\tposition\tref\talt\tcoverage\tfraction\tlrt\tll_half\tll_full\tgenotype\tshadowed\t'
                      'called\n')
            out.writelines('%s\t%d\t%s\t%s\t%d\t%r\t%r\t%r\t%r\t%d\t%d\t%d\n'
                           % (label(int(self.contig[t])), self.position[t], 'ACGT'[self.ref_base[t]],
                              'ACGT'[self.alt_base[t]], self.coverage[t], float(self.fraction[t]), float(self.lrt[t]),
                              float(self.ll_half[t]), float(self.ll_full[t]), self.genotype[t], self.shadowed[t],
                              self.called[t]) for t in range(len(self)))
        finally:
            if out is not file:
                out.close()


def neighbour_max(best, contig, reach):
    """Per position the largest ``best`` among the OTHER positions within ``reach`` of it that lie in the same contig
    (-inf where there is none).  ``best`` f64 (L,), ``contig`` int (L,) or None: torch tensors on one device."""
    import torch
    L = int(best.numel())
    out = torch.full_like(best, float('-inf'))
    ninf = best.new_full((), float('-inf'))
    for q in range(1, min(int(reach), L - 1) + 1):   # (the shifts, not the positions)
        left, right = best[:-q], best[q:]
        if contig is not None:
            same = contig[q:] == contig[:-q]
            left, right = torch.where(same, left, ninf), torch.where(same, right, ninf)
        out[q:] = torch.maximum(out[q:], left)
        out[:-q] = torch.maximum(out[:-q], right)
    return out


def estimate_allele_fractions_batch(reference_num, read_batch, config=defaults.CONFIG_FILE,
                                    kmer_model=defaults.KMER_MODEL_FILE, aligner=None, event_length=1.0,
                                    min_coverage=1, min_fraction=0.0, threshold=None, keep='positive'):
    """Per reference position and base other than the reference's: the fraction of the covering reads that carry it.
    The front end is ``estimate_snps_batch``'s — ONE median / MAD over all reads, approximate alignment, the spline
    tweak when configured, the per-read log-likelihood rows (``batchflow.device_stage`` 'pooled' and
    ``batchflow.likelihood_rows``) — then, instead of the per-position sum, ONE ``device.allele_fractions_dev`` call
    (normalise and strand-correct the rows, stable sort by position, per-position mixture solve: no float atomics,
    two runs give the same bits) and one copy to the host.
    ``reference_num``: base codes, or a ``refset.ReferenceSet`` holding the aligner's ``reference_num`` as its
    concatenation (rows are then contig-local and named).  ``aligner``: as for ``estimate_snps_batch``.
    ``event_length``: the divisor of the ratios.  1.0 (default) is the untempered likelihood, the one under which the
    estimate is a fraction of reads; the configuration's ``normalization_event_length`` (10) gives the consensus
    scale, at which ``ll_full`` is the consensus sum but the estimate is biased low.  ``threshold`` has NO calibrated
    default: it applies to 2 L(f^) in nats over however many reads cover the site, and only synthetic levels have
    been scored with it; None leaves ``called`` all False.  ``keep``: 'positive' keeps the rows with fraction > 0,
    'all' every (position, base != reference) with coverage >= ``min_coverage``.
    Alphabet 4 only; single process only (no ``distributed``).  -> AlleleFractionBatch."""
    if keep not in ('positive', 'all'):
        raise ValueError("estimate_allele_fractions_batch: keep %r is not 'positive' or 'all'" % (keep,))
    event_length = float(event_length)
    if not 0.0 < event_length < float('inf'):
        raise ValueError('estimate_allele_fractions_batch: event_length %r is not a positive finite number'
                         % (event_length,))
    min_fraction = float(min_fraction)
    if not 0.0 <= min_fraction <= 1.0:
        raise ValueError('estimate_allele_fractions_batch: min_fraction %r outside 0 .. 1' % (min_fraction,))
    if int(min_coverage) != min_coverage or min_coverage < 0:
        raise ValueError('estimate_allele_fractions_batch: min_coverage %r is not an integer >= 0' % (min_coverage,))
    if threshold is not None:
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError('estimate_allele_fractions_batch: threshold is NaN')
    if aligner is None:
        raise ValueError('estimate_allele_fractions_batch needs a batch aligner (BWA has no batch adapter offline)')
    from .batchflow import device_stage, likelihood_rows, load_config, load_kmer_model
    config, kmer_model = load_config(config), load_kmer_model(kmer_model)
    if kmer_model.alphabet_size != 4:
        raise ValueError('estimate_allele_fractions_batch: alphabet %d (the strand flip and the rows are those of ACGT)'
                         % kmer_model.alphabet_size)
    from .refset import ReferenceSet
    min_coverage = int(min_coverage)
    refset = reference_num if isinstance(reference_num, ReferenceSet) else None
    if refset is not None:
        if not np.array_equal(refset.codes, np.asarray(aligner.reference_num).reshape(-1)):
            raise ValueError("estimate_allele_fractions_batch: the ReferenceSet's concatenation differs from the "
                             "aligner's reference_num")
        reference_num = refset.codes
    reference_num = np.ascontiguousarray(reference_num, dtype=np.int32)
    L = reference_num.size
    stage = device_stage(read_batch, reference_num if refset is None else refset, config, kmer_model, aligner,
                         'pooled')
    if stage.n_live == 0 or L == 0:
        return AlleleFractionBatch.empty(L, threshold, None if refset is None else list(refset.names))
    ll, status, _ = likelihood_rows(stage, config, kmer_model)
    return allele_fractions_of_rows(stage, ll, status, reference_num, refset, kmer_model, event_length, min_coverage,
                                    min_fraction, threshold, keep)


def allele_fractions_of_rows(stage, ll, status, reference_num, refset, kmer_model, event_length=1.0, min_coverage=1,
                             min_fraction=0.0, threshold=None, keep='positive', sorted_rows=None):
    """The back half of ``estimate_allele_fractions_batch``, from the log-likelihood rows ``ll`` and the per-read
    ``status`` of a ``batchflow.DeviceStage`` with live reads (device tensors, as ``batchflow.likelihood_rows`` returns
    them): the ``device.allele_fractions_dev`` call, the row selection on the device and the one copy to the host.
    ``reference_num``: int32 base codes of the whole reference; ``refset``: its ReferenceSet or None; the other
    arguments as checked there.  ``sorted_rows``: (sorted_key, sorted_val) of ``device.allele_sorted_rows_dev`` for the
    same rows and ``event_length``, from a caller that needs the sorted rows itself (``phase.phase_of_rows``); the
    rows are then not made again.  -> AlleleFractionBatch."""
    import torch
    from .device import allele_fractions_dev, allele_solve_dev, to_host
    sa, context = stage.sa, kmer_model.context
    device = torch.device('cuda', context.device)
    L = reference_num.size
    names = None if refset is None else list(refset.names)
    codes = torch.from_numpy(reference_num).to(device)
    if sorted_rows is not None:
        fraction, lrt, half, full, cov = allele_solve_dev(context, sorted_rows[0], sorted_rows[1], codes)
    else:
        fraction, lrt, half, full, cov = allele_fractions_dev(context, stage.dbatch, ll, sa.ref_start.contiguous(),
                                                              sa.reverse.to(torch.int32), status, event_length, codes)
    # everything per (position, base) on the device; only the kept rows and the coverage cross to the host
    contig = None if refset is None else refset.locate(torch.arange(L, dtype=torch.int64, device=device))[0]
    near = neighbour_max(lrt.max(dim=1).values, contig, kmer_model.get_k() - 1)
    alt = torch.arange(4, device=device)[None, :] != codes[:, None]
    kept = (fraction > 0) if keep == 'positive' else alt & (cov >= min_coverage)[:, None]
    at = torch.nonzero(kept)            # row-major: ascending in (position, base)
    P, b = at[:, 0], at[:, 1]
    f_, lrt_, half_, full_ = fraction[P, b], lrt[P, b], half[P, b], full[P, b]
    zero = torch.zeros_like(half_)
    genotype = torch.where(full_ > torch.maximum(half_, zero), 2, torch.where(half_ > zero, 1, 0))
    table = torch.stack([P.double(), b.double(), cov[P].double(), f_, lrt_, half_, full_, genotype.double(),
                         (near[P] > lrt_).double()], 1)
    n_rows = int(P.numel())
    flat = to_host(torch.cat([table.reshape(-1), cov.double()]))   # (every integer here is exact in a double)
    table, position_coverage = flat[:n_rows * 9].reshape(n_rows, 9), flat[n_rows * 9:].astype(np.int64)
    position = table[:, 0].astype(np.int64)
    alt_base, coverage = table[:, 1].astype(np.int8), table[:, 2].astype(np.int64)
    ref_base = reference_num[position].astype(np.int8)
    row_contig = np.zeros(n_rows, dtype=np.int32)
    if refset is not None:
        c, position = refset.locate(position)
        row_contig = c.astype(np.int32)
    col = lambda j: np.ascontiguousarray(table[:, j])
    called = np.zeros(n_rows, dtype=bool) if threshold is None else \
        (col(4) >= threshold) & (col(3) >= min_fraction) & (coverage >= min_coverage)
    return AlleleFractionBatch(row_contig, position, ref_base, alt_base, coverage, col(3), col(4), col(5), col(6),
                               table[:, 7].astype(np.int8), table[:, 8].astype(bool), called, position_coverage,
                               threshold, names)
