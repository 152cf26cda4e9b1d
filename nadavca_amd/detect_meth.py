"""``detect_meth`` — per-event deviation scores around every occurrence of a sequence pattern (mirrors
/root/reference/nadavca/detect_meth.py:21-120; a consumer of the alignments).

The alignment itself — normalise, align, linear re-fit, re-align, linear re-fit — is ``align_signal`` (the
reference repeats that loop inline, detect_meth.py:75-106; it is the same arithmetic, and here the same
kernels).  What this module adds is the scoring: for an occurrence of ``pattern`` at reference-part position
p, the 11 events p-5 .. p+5 are each scored by how far their mean level is from the model's expected level,
    z = |mean(event) - expected| / 0.35287208,   score = -log(max(1e-50, 2 * Phi(-z))),
an occurrence counts only when all 11 events exist and are non-empty, and its aggregate is the largest sum of
three consecutive scores.  All events of a read are scored at once (segment sums instead of a Python loop per
event)."""
import csv
import os
import sys

import numpy as np
from scipy.special import ndtr

from . import defaults
from .align_signal import align_signal, load_model_and_estimator
from .genome import Genome

SMALLEST_PVAL = 1e-50
LEVEL_SD = 0.35287208     # detect_meth.py:24
FLANK = 5                 # events on each side of the pattern's first base


def cdf_scoring(raw, exp):
    """Score of one event (detect_meth.py:23-26)."""
    z = np.abs(np.mean(raw) - exp) / LEVEL_SD
    return -np.log(max(SMALLEST_PVAL, ndtr(-z) * 2.0))


def event_scores(signal_cut, alignment, expected):
    """Scores of all events of one read: ``alignment`` (R, 3) rows (position, start, end) in read coordinates,
    ``signal_cut`` = normalized_signal[alignment[0][1] : alignment[-1][2]].  An empty event scores NaN."""
    alignment = np.asarray(alignment)
    start = alignment[:, 1] - alignment[0][1]
    end = alignment[:, 2] - alignment[0][1]
    padded = np.append(np.asarray(signal_cut, dtype=float), 0.0)
    cuts = np.empty(2 * len(start), dtype=np.intp)
    cuts[0::2], cuts[1::2] = start, np.maximum(end, start)
    sums = np.add.reduceat(padded, cuts)[0::2]
    n = end - start
    with np.errstate(invalid='ignore', divide='ignore'):
        means = np.where(n > 0, sums / np.maximum(n, 1), np.nan)
        z = np.abs(means - np.asarray(expected, dtype=float)[:len(means)]) / LEVEL_SD
        return -np.log(np.maximum(SMALLEST_PVAL, ndtr(-z) * 2.0))


def calculate_meth_scores(signal_cut, alignment, apx_alignment, pattern, kmer_model):
    """-> [(position, sequence context, [11 scores])] for every scorable occurrence of ``pattern`` in the
    aligned reference part (detect_meth.py:28-60)."""
    bases = apx_alignment.reference_part
    expected = np.asarray(kmer_model.get_expected_signal(Genome.to_numerical(bases), [], []))
    seq = ''.join(np.asarray(bases).tolist())
    scores = event_scores(signal_cut, alignment, expected)
    n = len(alignment)
    features, pos = [], seq.find(pattern)
    while pos != -1:
        lo, hi = pos - FLANK, pos + FLANK + 1
        if lo >= 0 and hi <= n:
            window = scores[lo:hi]
            if not np.isnan(window).any():
                features.append((pos, seq[lo:hi], window.tolist()))
        pos = seq.find(pattern, pos + 1)
    return features


def maxs3(values):
    """Largest sum of three consecutive scores (detect_meth.py:63-65)."""
    v = np.asarray(values, dtype=float)
    return float(np.max(v[:-2] + v[1:-1] + v[2:]))


def detect_meth(reference_filename, reads, pattern, output, config=defaults.CONFIG_FILE,
                kmer_model=defaults.KMER_MODEL_FILE, bwa_executable=defaults.BWA_EXECUTABLE,
                group_name=defaults.GROUP_NAME, renorm_rounds=defaults.RENORM_ROUNDS, aligner=None):
    """CSV of (Filename, Position, Sequence context, Position scores, Aggregated score) rows, one per scorable
    pattern occurrence per read, to ``output`` (a path) or stdout.  ``reads``: fast5 paths or ``Read``
    objects; ``aligner``: optional approximate aligner (extension, as in ``align_signal``)."""
    loaded = load_model_and_estimator(reference_filename, config, kmer_model, bwa_executable, aligner)
    if loaded is None:
        return
    model = loaded[0]
    out = open(output, 'w', newline='') if output is not None else sys.stdout
    try:
        writer = csv.writer(out)
        writer.writerow(('Filename', 'Position', 'Sequence context', 'Position scores', 'Aggregated score'))
        names = [r if isinstance(r, str) else getattr(r, 'name', 'read%d' % i) for i, r in enumerate(reads)]
        results = align_signal(reference_filename, reads, config=config, kmer_model=model,
                               bwa_executable=bwa_executable, group_name=group_name,
                               renorm_rounds=renorm_rounds, aligner=aligner)
        for name, (read, (apx, alignment)) in zip(names, results):
            cut = read.normalized_signal[alignment[0][1]:alignment[-1][2]]
            for pos, context, scores in calculate_meth_scores(cut, alignment, apx, pattern, model):
                writer.writerow((name, pos, context, ','.join(map(str, scores)), maxs3(scores)))
    finally:
        if output is not None:
            out.close()


_PATTERN_CODES = {'A': 0, 'C': 1, 'G': 2, 'T': 3}
_LETTERS = np.frombuffer(b'ACGT', dtype=np.uint8)


def pattern_codes(pattern):
    """``pattern`` as int32 base codes; a character outside ``ACGT`` (lowercase included) becomes -1, which never
    matches, as ``str.find`` on an upper-case ACGT sequence never finds it."""
    return np.array([_PATTERN_CODES.get(c, -1) for c in pattern], dtype=np.int32)


def contexts_from_codes(codes):
    """(n, 11) base codes -> n strings of 11 letters (``seq[p-5:p+6]`` of the occurrences), vectorised."""
    codes = np.asarray(codes).reshape(-1, 2 * FLANK + 1)
    return _LETTERS[codes].view('S%d' % (2 * FLANK + 1)).reshape(-1).astype('U%d' % (2 * FLANK + 1))


class MethBatch:
    """What ``detect_meth_batch`` returns: one row per scorable pattern occurrence of every read, in read order and
    ascending position — the rows ``detect_meth`` writes — as flat arrays: ``read`` (index in the ReadBatch),
    ``position`` (in the read's reference part), ``context`` (``seq[p-5:p+6]``), ``scores`` (n, 11), ``aggregate``
    (the largest sum of three consecutive scores); and per aligned read (``live``: its index in the ReadBatch) its
    ``status`` (``_lib.READ_*``; a read with status != 0 has no rows), as in ``AlignedBatch``.  ``contig`` (int32 per
    row): the contig of the row's read, an index into ``contig_names`` with an aligner over a ``refset.ReferenceSet``
    (0 and None otherwise); ``position`` is relative to the read's reference part either way, and ``write_csv`` keeps
    ``detect_meth``'s columns."""

    def __init__(self, read, position, context, scores, aggregate, status, live, contig=None, contig_names=None):
        self.read, self.position, self.context = read, position, context
        self.contig = np.zeros(len(read), dtype=np.int32) if contig is None else contig
        self.contig_names = contig_names
        self.scores, self.aggregate, self.status, self.live = scores, aggregate, status, live

    @classmethod
    def empty(cls, status=None, live=None, contig_names=None):
        z = lambda dt: np.zeros(0, dtype=dt)
        return cls(z(np.int64), z(np.int64), z('U%d' % (2 * FLANK + 1)), np.zeros((0, 2 * FLANK + 1)), z(np.float64),
                   z(np.int32) if status is None else status, z(np.int64) if live is None else live,
                   contig_names=contig_names)

    def __len__(self):
        return int(self.position.size)

    def write_csv(self, file, names=None):
        """The CSV ``detect_meth`` writes (header, then one row per occurrence: name, position, context, the 11
        scores joined by commas, aggregate; floats as ``str`` gives them) to ``file``, a path or a text file.
        ``names[i]``: the name of ReadBatch read i (default ``'read%d' % i``, as ``detect_meth`` names reads without
        one)."""
        out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
        try:
            writer = csv.writer(out)
            writer.writerow(('Filename', 'Position', 'Sequence context', 'Position scores', 'Aggregated score'))
            name = (lambda i: 'read%d' % i) if names is None else (lambda i: names[i])
            writer.writerows((name(i), p, c, ','.join(map(str, sc)), a) for i, p, c, sc, a in zip(
                self.read.tolist(), self.position.tolist(), self.context.tolist(), self.scores.tolist(),
                self.aggregate.tolist()))
        finally:
            if out is not file:
                out.close()


def detect_meth_batch(reference_filename, read_batch, pattern, config=defaults.CONFIG_FILE,
                      kmer_model=defaults.KMER_MODEL_FILE, renorm_rounds=defaults.RENORM_ROUNDS, aligner=None):
    """``detect_meth`` for a struct-of-arrays ``ReadBatch`` with no per-read Python: the alignment of
    ``align_signal_batch`` (the same kernels, the same ``aligner`` contract), then on the device the event means over
    the signal after the last rescale, the expected levels without contexts and the occurrence scores
    (include/nadavca_hip.h: nvk_meth_count_dev / nvk_meth_scores_dev), and one copy of the rows to the host.  Reads
    that did not align produce no rows (``detect_meth`` raises on them) and show in ``status`` / ``live``.
    -> MethBatch (``write_csv`` gives ``detect_meth``'s CSV)."""
    import torch
    from .batchflow import align_batch, load_config, load_kmer_model, seg_index
    from .device import event_means_dev, expected_levels_dev, meth_scores_dev, to_host
    kmer_model = load_kmer_model(kmer_model)
    res = align_batch(read_batch, load_config(config), kmer_model, renorm_rounds, aligner)
    names = res.stage.contig_names()
    if res.stage.n_live == 0:
        return MethBatch.empty(contig_names=names)
    sa, dbatch, events, status = res.stage.sa, res.stage.dbatch, res.events, res.status
    context = kmer_model.context
    live = sa.live.cpu().numpy()
    # the loop's own means were taken before its last rescale: these are over the final signal (detect_meth.py:106)
    means = event_means_dev(dbatch, context, events, status)
    expected = expected_levels_dev(dbatch, kmer_model, with_contexts=False)
    occ_off, pos, scores, agg = meth_scores_dev(context, dbatch.reference, dbatch.ref_off, means, expected, status,
                                                pattern_codes(pattern))
    n_occ = int(pos.numel())
    if n_occ == 0:
        return MethBatch.empty(status.cpu().numpy(), live, names)
    dev = pos.device
    owner, _ = seg_index(occ_off, n_occ)
    # the 11 bases around each occurrence, 2 bits each in one integer (exact in a double: 22 bits)
    first = dbatch.ref_off[:-1][owner] + pos - FLANK
    shifts = 2 * torch.arange(2 * FLANK, -1, -1, dtype=torch.int64, device=dev)
    packed = (dbatch.reference[first[:, None] + torch.arange(2 * FLANK + 1, device=dev)].to(torch.int64)
              << shifts).sum(1)
    # one device-to-host copy: scores, aggregate, position, read index, packed context as the columns of one table
    table = to_host(torch.cat([scores, agg[:, None], pos[:, None].double(), sa.live[owner][:, None].double(),
                               packed[:, None].double()], 1))
    W = 2 * FLANK + 1
    codes = (table[:, W + 3].astype(np.int64)[:, None] >> np.arange(2 * (W - 1), -1, -2)) & 3
    return MethBatch(table[:, W + 2].astype(np.int64), table[:, W + 1].astype(np.int64), contexts_from_codes(codes),
                     np.ascontiguousarray(table[:, :W]), np.ascontiguousarray(table[:, W]), status.cpu().numpy(), live,
                     sa.contig[owner].cpu().numpy(), names)


def detect_meth_command(args):
    reads = [os.path.join(args.read_basedir, fn) for fn in os.listdir(args.read_basedir) if fn.endswith('.fast5')]
    detect_meth(args.reference, reads, args.pattern, args.output, args.configuration, args.kmer_model,
                args.bwa_executable, args.group_name, args.renorm_rounds)
