"""``align_signal`` (mirrors /root/reference/nadavca/align_signal.py:13-81).

Generator of ``(read, (approximate_alignment, alignment))`` with ``alignment`` the (R, 3) int
array (reference position, event start, event end).  The per-read renormalise / re-align loop of
the reference (renorm_rounds, default 3: linear re-fit, re-align, linear re-fit) is kept, but every
round processes all reads in one batched GPU launch, and the signal stays on the device between the
rounds (per-event means, least-squares re-fit and rescale are kernels: include/nadavca_hip.h).
Extensions over the reference signature, both optional: ``reads`` may hold ``Read`` objects (not only
fast5 paths), and ``aligner`` injects an approximate aligner (BWA is not available offline)."""
import sys

import numpy

from . import defaults
from .alignment import ApproximateAligner
from .batchflow import align_batch, load_config, load_kmer_model, seg_index
from .estimator import ProbabilityEstimator
from .genome import Genome
from .read import Read

_load_config = load_config   # the name bench.py imports


def load_model_and_estimator(reference_filename, config=defaults.CONFIG_FILE, kmer_model=None,
                             bwa_executable=defaults.BWA_EXECUTABLE, aligner=None):
    if kmer_model is None:
        kmer_model = defaults.KMER_MODEL_FILE
    try:
        config = load_config(config)
    except FileNotFoundError:
        sys.stderr.write('failed to load config: {} not found\n'.format(config))
        return None
    kmer_model = load_kmer_model(kmer_model)
    if aligner is None:
        try:
            references = Genome.load_from_fasta(reference_filename)
        except FileNotFoundError:
            sys.stderr.write("failed to process: reference {} doesn't exist\n".format(reference_filename))
            return None
        references_dict = {r.description[1:]: r.bases for r in references}
        aligner = ApproximateAligner(bwa_executable, None, reference_filename, references_dict)
    return kmer_model, ProbabilityEstimator(kmer_model, aligner, config)


def align_signal(reference_filename, reads, config=defaults.CONFIG_FILE,
                 kmer_model=defaults.KMER_MODEL_FILE, bwa_executable=defaults.BWA_EXECUTABLE,
                 group_name=defaults.GROUP_NAME, renorm_rounds=defaults.RENORM_ROUNDS, aligner=None):
    loaded = load_model_and_estimator(reference_filename, config, kmer_model, bwa_executable, aligner)
    if loaded is None:
        return
    kmer_model, estimator = loaded
    loaded_reads = [Read.load_from_fast5(item, group_name) if isinstance(item, str) else item
                    for item in reads]
    # per-read normalisation (align_signal.py:54), all reads in one kernel
    Read.normalize_reads_device(loaded_reads, per_read=True, context=kmer_model.context)
    # align / re-fit / re-align / re-fit (align_signal.py:55-80), device-resident
    results = estimator.refine_and_renormalize(loaded_reads, renorm_rounds)
    for read, res in zip(loaded_reads, results):
        if res is None:
            # the reference raises TypeError here (it unpacks None, align_signal.py:55)
            raise TypeError('read could not be aligned (no approximate alignment or no path in the band)')
        yield read, res


class AlignedBatch:
    """What ``align_signal_batch`` returns: for the reads that aligned (``live``: their indices in the
    ReadBatch), the (reference position, event start, event end) rows of all reads end to end — read
    ``live[j]`` at rows [ref_off[j], ref_off[j+1]) — the approximate alignment they started from
    (``approximate``: a readbatch.SignalAlignmentBatch) and the per-round linear fits.  The reads' rescaled
    ``normalized_signal`` stays on the device (``normalized``) until ``normalized_signal(j)`` asks for it.
    With an aligner over a ``refset.ReferenceSet``: ``contig`` (int32 per live read, an index into ``contig_names``)
    and reference positions inside that contig; otherwise ``contig`` is 0 and ``contig_names`` None."""

    def __init__(self, live, status, alignment, ref_off, approximate, fits, normalized, sig_off, contig=None,
                 contig_names=None):
        self.live, self.status, self.alignment, self.ref_off = live, status, alignment, ref_off
        self.contig = numpy.zeros(len(live), dtype=numpy.int32) if contig is None else contig
        self.contig_names = contig_names
        self.approximate, self.fits, self.normalized, self.sig_off = approximate, fits, normalized, sig_off
        self.n_aligned = int((status == 0).sum())

    def alignment_of(self, j):
        """(R, 3) int64 rows of live read j, or None where the band held no path."""
        if self.status[j] != 0:
            return None
        return self.alignment[self.ref_off[j]:self.ref_off[j + 1]]

    def normalized_signal(self, read_index):
        lo, hi = int(self.sig_off[read_index]), int(self.sig_off[read_index + 1])
        return self.normalized[lo:hi].cpu().numpy()


def align_signal_batch(reference_filename, read_batch, config=defaults.CONFIG_FILE,
                       kmer_model=defaults.KMER_MODEL_FILE, renorm_rounds=defaults.RENORM_ROUNDS, aligner=None):
    """``align_signal`` for a struct-of-arrays ``ReadBatch`` (nadavca_amd/readbatch.py): the same steps per read
    as the reference's loop (align_signal.py:52-81) — per-read median/MAD normalisation, approximate
    alignment, banded alignment, linear re-fit, re-alignment, linear re-fit — with no per-read Python: the raw
    signals and the flat tables cross PCIe once in their native dtypes, the approximate-alignment stage and
    the window cutting are tensor operations on the device, and everything between stays there.  ``aligner``: an object with
    ``get_base_alignments(read_batch) -> BaseAlignmentBatch`` and ``reference_num`` (the reference as base
    codes).  -> AlignedBatch."""
    import torch
    from .device import to_host
    from .readbatch import contig_local_range
    rb = read_batch
    res = align_batch(rb, load_config(config), load_kmer_model(kmer_model), renorm_rounds, aligner)
    sa, norm, events, status, fits = res.stage.sa, res.stage.norm, res.events, res.status, res.fits
    names = res.stage.contig_names()
    if res.stage.n_live == 0:
        return AlignedBatch(numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0, dtype=numpy.int32),
                            numpy.zeros((0, 3), dtype=numpy.int64), numpy.zeros(1, dtype=numpy.int64), sa, [],
                            norm, rb.sig_off, contig_names=names)
    device = norm.device
    # the same linear maps for the samples outside the windows (the reference rescales the whole read,
    # align_signal.py:73): per read (x - intercept) / slope, fit after fit, on the device
    total = int(rb.sig_off[-1])
    lens = res.stage.group_off[1:] - res.stage.group_off[:-1]   # (normalised per read: the groups are the reads)
    okay = (status == 0)
    for f in fits:
        slope = torch.ones(rb.n, dtype=torch.float64, device=device)
        icpt = torch.zeros(rb.n, dtype=torch.float64, device=device)
        slope[sa.live] = torch.where(okay, f[:, 0], torch.ones_like(f[:, 0]))
        icpt[sa.live] = torch.where(okay, f[:, 1], torch.zeros_like(f[:, 1]))
        norm -= torch.repeat_interleave(icpt, lens, output_size=total)
        norm /= torch.repeat_interleave(slope, lens, output_size=total)
    # (R, 3) rows: reference position (descending on the reverse strand), events in read coordinates
    n_rows = res.stage.dbatch.total_ref
    owner, inner = seg_index(sa.ref_off, n_rows)
    rows = torch.empty((n_rows, 3), dtype=torch.int64, device=device)
    ref_start, ref_end = contig_local_range(sa, res.stage.reference)
    rows[:, 0] = torch.where(sa.reverse[owner], ref_end[owner] - inner - 1, ref_start[owner] + inner)
    start = sa.slice_start[owner]
    rows[:, 1] = events[:, 0] + start
    rows[:, 2] = events[:, 1] + start
    rb.normalized = norm
    return AlignedBatch(sa.live.cpu().numpy(), status.cpu().numpy(), to_host(rows), sa.ref_off.cpu().numpy(),
                        sa, [f.cpu().numpy() for f in fits], norm, rb.sig_off, sa.contig.cpu().numpy(), names)
