"""``estimate_snps`` (mirrors /root/reference/nadavca/estimate_snps.py:13-70): SNP posteriors per
reference position, either a consensus over all reads or one Chunk per read (independent=True).
``aligner`` (optional, not in the reference signature) injects an approximate aligner."""
import os
import sys

from . import defaults
from .alignment import ApproximateAligner
from .batchflow import device_stage, likelihood_rows, load_config, load_kmer_model, seg_index
from .estimator import ProbabilityEstimator, Chunk, consensus_chunks, independent_posteriors  # noqa: F401
from .genome import Genome
from .read import Read


def estimate_snps(reference_filename, reads, reference=None, config=defaults.CONFIG_FILE,
                  kmer_model=defaults.KMER_MODEL_FILE, bwa_executable=defaults.BWA_EXECUTABLE,
                  independent=False, group_name=defaults.GROUP_NAME, aligner=None):
    try:
        config = load_config(config)
    except FileNotFoundError:
        sys.stderr.write('failed to load config: {} not found\n'.format(config))
        return None
    try:
        kmer_model = load_kmer_model(kmer_model)
    except FileNotFoundError:
        sys.stderr.write('failed to load k-mer model: {} not found\n'.format(kmer_model))
        return None
    if reference is None:
        try:
            reference = Genome.load_from_fasta(reference_filename)[0].bases
        except FileNotFoundError:
            sys.stderr.write("failed to process: reference {} doesn't exist\n".format(reference_filename))
            return None
    if aligner is None:
        aligner = ApproximateAligner(bwa_executable, reference, reference_filename)
    estimator = ProbabilityEstimator(kmer_model, aligner, config)

    if isinstance(reads, str):
        base = reads
        reads = [os.path.join(base, f) for f in os.listdir(base)
                 if f.endswith('.fast5') and not os.path.isdir(os.path.join(base, f))]
    reads = [Read.load_from_fast5(r, group_name) if isinstance(r, str) else r for r in reads]
    # ONE median/MAD over all reads (estimate_snps.py:61)
    Read.normalize_reads_device(reads, context=getattr(kmer_model, 'context', None))

    if independent:
        chunks = estimator.estimate_probabilities_independent(reference, reads)
        if any(c is None for c in chunks):
            # the reference indexes chunks[0] of an empty list here (estimate_snps.py:66-67)
            raise IndexError('a read produced no chunk (not aligned, or no valid path in the band)')
        return chunks
    return estimator.estimate_probabilities(reference, reads)


# what the last estimate_snps_batch call saw (bench.py reports it): reads in the batch, reads with an approximate
# alignment, reads whose log-likelihoods came back with status 0, reads the spline tweak fitted
last_batch_counts = {}


class IndependentChunks:
    """``estimate_snps(independent=True)`` for a batch: one chunk per read that produced one, as arrays —
    read ``reads[j]`` covers reference positions [start[j], end[j]) and has posterior rows
    values[row_off[j]:row_off[j+1]] (coverage is 1 everywhere, as in the reference's per-read call).  For a
    ``refset.ReferenceSet``: ``contig[j]`` (an index into ``contig_names``) is the read's contig and ``start`` / ``end``
    are positions inside it; for a plain array ``contig`` is None."""

    def __init__(self, reads, start, end, values, row_off, contig=None, contig_names=None):
        self.reads, self.start, self.end, self.values, self.row_off = reads, start, end, values, row_off
        self.contig, self.contig_names = contig, contig_names

    def __len__(self):
        return len(self.reads)

    def chunk(self, j):
        return Chunk(int(self.start[j]), int(self.end[j]), self.values[self.row_off[j]:self.row_off[j + 1]],
                     contig=None if self.contig is None else self.contig_names[int(self.contig[j])])


def estimate_snps_batch(reference_num, read_batch, config=defaults.CONFIG_FILE,
                        kmer_model=defaults.KMER_MODEL_FILE, independent=False, aligner=None, fit_workers=0,
                        group=None, distributed=None, dst=0, spline_fit='device'):
    """``estimate_snps`` for a struct-of-arrays ``ReadBatch`` (nadavca_amd/readbatch.py) without per-read
    Python: the steps of estimate_snps.py:57-70 and estimator.py:59-121,199-236 — ONE median/MAD over all
    reads, approximate alignment, the spline tweak (splinefit.tweak_signal_normalization: all on the device;
    ``spline_fit='host'`` sends its fit to scipy in ``fit_workers`` processes instead), log-likelihoods, normalise /
    strand-flip / per-position sum, grouping, posterior — with the signals, the sums and everything between them
    resident on the device.
    ``reference_num``: the reference as base codes, or a ``refset.ReferenceSet`` (it must hold the aligner's
    ``reference_num`` as its concatenation, else ValueError): the median / MAD and the consensus then run over all
    contigs at once, no chunk spans two contigs (touching chunks do not merge), and every Chunk carries its contig's
    name in ``.contig`` with ``start`` / ``end`` inside that contig.  ``aligner``: as for ``align_signal_batch``.
    -> list of Chunk (consensus) or IndependentChunks.

    Several GPUs (``distributed=True``, or a ``group``; default: whenever torch.distributed is initialised with
    more than one rank): every rank passes ITS shard of the reads as ``read_batch`` and the two exchange steps of
    the path run over torch.distributed (RCCL over xGMI with the nccl backend) — the pooled median / MAD of
    estimate_snps.py:61 as an exact distributed selection (256 counts per pass cross ranks, distributed.py:
    pooled_centre_scale), and for ``independent=False`` ONE reduce(sum) of the packed per-position sums plus a
    small all-gather of the chunk intervals.  The consensus Chunk list is returned on rank ``dst`` (None
    elsewhere); ``independent=True`` returns every rank's own IndependentChunks."""
    import numpy
    import torch
    from .device import consensus_accumulate_dev
    config, kmer_model = load_config(config), load_kmer_model(kmer_model)
    if aligner is None:
        raise ValueError('estimate_snps_batch needs a batch aligner (BWA has no batch adapter offline)')
    context = kmer_model.context
    device = torch.device('cuda', context.device)
    from .readbatch import contig_local_range
    from .refset import ReferenceSet
    refset = reference_num if isinstance(reference_num, ReferenceSet) else None
    if refset is not None:
        if not numpy.array_equal(refset.codes, numpy.asarray(aligner.reference_num).reshape(-1)):
            raise ValueError("estimate_snps_batch: the ReferenceSet's concatenation differs from the aligner's "
                             'reference_num')
        reference_num = refset.codes
    reference_num = numpy.ascontiguousarray(reference_num, dtype=numpy.int32)
    L = reference_num.size

    def localise(chunks):
        # consensus chunks in global positions -> inside their contig, named (every rank holds the same set)
        if refset is None or chunks is None:
            return chunks
        for ch in chunks:
            c, s = refset.locate(ch.start)
            ch.start, ch.end, ch.contig = int(s), int(s + (ch.end - ch.start)), refset.names[int(c)]
        return chunks
    if distributed is None:
        distributed = group is not None
        if not distributed:
            import torch.distributed as tdist
            distributed = tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1
    # all reads pooled, of ALL ranks when distributed (estimate_snps.py:61)
    stage = device_stage(read_batch, reference_num if refset is None else refset, config, kmer_model, aligner,
                         'ranks' if distributed else 'pooled', group)
    sa, dbatch, n_live = stage.sa, stage.dbatch, stage.n_live
    last_batch_counts.clear()
    last_batch_counts.update(reads=int(read_batch.n), reads_aligned=n_live, reads_ok=0, reads_fitted=None)
    if n_live == 0:
        if independent:
            return IndependentChunks(numpy.zeros(0, dtype=numpy.int64), *[numpy.zeros(0)] * 3,
                                     numpy.zeros(1, dtype=numpy.int64),
                                     None if refset is None else numpy.zeros(0, dtype=numpy.int32),
                                     None if refset is None else list(refset.names))
        if not distributed:
            return []
        # (a rank whose shard aligned nowhere still takes part in the exchange, with empty sums)
        acc = torch.zeros((L, kmer_model.alphabet_size), dtype=torch.float64, device=device)
        cov = torch.zeros(L, dtype=torch.int64, device=device)
        return localise(consensus_chunks(kmer_model, config['snp_prior_probability'], reference_num, acc, cov, [],
                                         True, group, dst))
    ll, status, last_batch_counts['reads_fitted'] = likelihood_rows(stage, config, kmer_model, fit_workers,
                                                                    spline_fit)
    rev32 = sa.reverse.to(torch.int32)
    nel, prior = config['normalization_event_length'], config['snp_prior_probability']
    ok = (status == 0)
    last_batch_counts['reads_ok'] = int(ok.sum())
    if independent:
        # the reference's base codes over every read's chunk, laid out as ll, gathered on the device
        owner, inner = seg_index(sa.ref_off, dbatch.total_ref)
        codes = torch.from_numpy(reference_num).to(device)[sa.ref_start[owner] + inner]
        okh, values, row_off = independent_posteriors(kmer_model, prior, nel, dbatch, ll, status, rev32, codes)
        start, end = contig_local_range(sa, reference_num if refset is None else refset)
        return IndependentChunks(sa.live.cpu().numpy()[okh], start.cpu().numpy()[okh], end.cpu().numpy()[okh], values,
                                 row_off, None if refset is None else sa.contig.cpu().numpy()[okh],
                                 None if refset is None else list(refset.names))
    acc, cov = consensus_accumulate_dev(context, dbatch, ll, sa.ref_start.contiguous(), rev32, status, nel, L)
    starts, ends = sa.ref_start[ok].cpu().numpy(), sa.ref_end[ok].cpu().numpy()
    return localise(consensus_chunks(kmer_model, prior, reference_num, acc, cov,
                                     list(zip(starts.tolist(), ends.tolist())), distributed, group, dst))
