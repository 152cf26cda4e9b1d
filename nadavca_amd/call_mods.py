"""``call_mods_batch`` — per read and per site, "is this base modified?" as a log-likelihood ratio under the HMM.

With a table whose alphabet holds a modified base beside ``ACGT`` (code 4, ``M``; ``kmer_train.extend_kmer_model``
makes one from a canonical table and known levels) and the canonical reference, the entry ``[p, 4]`` of
``estimate_log_likelihoods`` minus the entry ``[p, reference[p]]`` is the log-likelihood ratio of "base p is ``M``"
against "base p is what the reference says" (dtw.cpp:93-129 and 83-85, wobble rows and both quirks included).  The
full matrix scores every base of a read against every letter; a caller wants one letter at the positions where a
pattern occurs.  This workflow aligns a ``ReadBatch`` (``batchflow.align_batch``, the alignment of
``align_signal_batch``), finds the pattern's occurrences in every read's reference part on the device and scores
only those (``device.estimate_hypotheses_dev``).

One substitution per hypothesis: a site is scored against an otherwise canonical reference.  Two sites closer than
k bases share a k-mer and are each scored with the other assumed unmodified; such rows carry ``crowded``."""
import os

import numpy as np

from . import defaults, _lib
from .detect_meth import pattern_codes


def find_sites(reference, ref_off, start, end, reverse, pattern, mod_offset, k, keep=None, total_ref=None):
    """The occurrences of ``pattern`` (int base codes; a code outside 0..3 matches nothing) in the reference parts
    ``reference`` / ``ref_off`` of a batch (int32 / int64 tensors, any device; a part is in its READ's orientation,
    overlapping occurrences all count).  ``start`` / ``end``: the forward range of every part (int64 per read),
    ``reverse``: bool per read; ``keep``: bool per read or None, reads without it have no sites; ``total_ref``:
    ``ref_off[-1]`` where the caller holds it.  Index plumbing with torch operations — no loop over reads.
    -> (site_off int64 (n+1,), owner int64, pos int32, forward int64, crowded bool): read j's sites are
    [site_off[j], site_off[j+1]), ascending in ``pos`` = q + mod_offset, the position of the substituted base in the
    part for an occurrence at q; ``forward`` its forward coordinate (``start + pos``, reverse: ``end - 1 - pos``);
    ``crowded``: another site of the same read lies within k - 1 bases, so the two share a k-mer."""
    import torch
    from .batchflow import seg_index
    dev = ref_off.device
    pat = torch.as_tensor(np.asarray(pattern, dtype=np.int64).reshape(-1)).to(dev)
    m = int(pat.numel())
    if not 0 <= int(mod_offset) < max(m, 1) or m == 0:
        raise ValueError('find_sites: mod_offset %r outside the pattern (length %d)' % (mod_offset, m))
    n = int(ref_off.numel()) - 1
    total = int(ref_off[-1]) if total_ref is None else int(total_ref)
    owner, inner = seg_index(ref_off, total)
    length = (ref_off[1:] - ref_off[:-1])[owner]
    hit = inner + m <= length
    if keep is not None:
        hit &= keep.to(dev)[owner]
    if bool(((pat < 0) | (pat > 3)).any()):
        hit &= False
    flat = torch.arange(total, dtype=torch.int64, device=dev)
    ref = reference[:total]
    for t in range(m):   # (the pattern's letters, not the reads)
        hit &= ref[torch.clamp(flat + t, max=max(total - 1, 0))] == pat[t]
    at = torch.nonzero(hit).reshape(-1)
    owner, pos = owner[at], inner[at] + int(mod_offset)
    site_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(owner, minlength=n), 0, out=site_off[1:])
    forward = torch.where(reverse.to(dev)[owner], end.to(dev)[owner] - 1 - pos, start.to(dev)[owner] + pos)
    # rows are in read order and ascending position: a close neighbour is the row before or the row after
    near = (owner[1:] == owner[:-1]) & (pos[1:] - pos[:-1] <= int(k) - 1)
    crowded = torch.zeros(at.numel(), dtype=torch.bool, device=dev)
    crowded[1:] |= near
    crowded[:-1] |= near
    return site_off, owner, pos.to(torch.int32), forward, crowded


class ModCallBatch:
    """What ``call_mods_batch`` returns: one row per occurrence of the pattern in the reference part of every read
    that aligned, in read order and ascending position within the read's orientation, as flat arrays: ``read``
    (index in the ReadBatch), ``contig`` (an index into ``contig_names`` with an aligner over a
    ``refset.ReferenceSet``; 0 and None otherwise), ``position`` (forward, contig-local coordinate of the substituted
    base), ``strand`` (0 forward, 1 reverse: the site is then the complementary base of the reverse strand), ``llr``
    (log-likelihood of the read with the modified base at the site minus that with the reference's base) and
    ``crowded`` (another site of the read within k - 1 bases: the two share a k-mer and each was scored with the other
    assumed unmodified).  Per aligned read (``live``: its index in the ReadBatch): ``status`` (``_lib.READ_*``; a read
    with status != 0 has no rows) and ``total`` (its log-likelihood without a substitution, NaN where it did not
    run)."""

    def __init__(self, read, contig, position, strand, llr, crowded, status, live, total, contig_names=None):
        self.read, self.contig, self.position, self.strand = read, contig, position, strand
        self.llr, self.crowded = llr, crowded
        self.status, self.live, self.total = status, live, total
        self.contig_names = contig_names

    @classmethod
    def empty(cls, status=None, live=None, total=None, contig_names=None):
        z = lambda dt: np.zeros(0, dtype=dt)
        return cls(z(np.int64), z(np.int32), z(np.int64), z(np.int8), z(np.float64), z(bool),
                   z(np.int32) if status is None else status, z(np.int64) if live is None else live,
                   z(np.float64) if total is None else total, contig_names)

    def __len__(self):
        return int(self.position.size)

    def _contig_label(self):
        return (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])

    def write_tsv(self, file, names=None):
        """Header, then one tab-separated row per site: read, contig, position, strand (``+`` / ``-``), llr (as
        ``repr`` gives it), crowded (0 / 1), to ``file``, a path or a text file.  ``names[i]``: the name of ReadBatch
        read i (default ``'read%d' % i``); the contig by name where the batch has names, by index otherwise."""
        out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
        try:
            out.write('read\tcontig\tposition\tstrand\tllr\tcrowded\n')
            name = (lambda i: 'read%d' % i) if names is None else (lambda i: names[i])
            label = self._contig_label()
            out.writelines('%s\t%s\t%d\t%s\t%r\t%d\n' % (name(i), label(c), p, '-' if s else '+', v, w)
                           for i, c, p, s, v, w in zip(self.read.tolist(), self.contig.tolist(),
                                                       self.position.tolist(), self.strand.tolist(),
                                                       self.llr.tolist(), self.crowded.tolist()))
        finally:
            if out is not file:
                out.close()

    def site_table(self, threshold=2.0):
        """The rows per site: a dict of arrays, one entry per distinct (contig, position, strand), sorted by them:
        ``contig``, ``position``, ``strand``, ``reads`` (rows), ``modified`` (llr >= threshold), ``unmodified``
        (llr <= -threshold), ``ambiguous`` (the rest) and ``frequency`` = modified / (modified + unmodified), NaN
        when both are 0.  ``threshold``: the caller's; the default is the customary one of nanopolish, not a claim
        about calibration."""
        key = np.stack([self.contig.astype(np.int64), self.position.astype(np.int64),
                        self.strand.astype(np.int64)], 1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True) if len(self) else (key, np.zeros(0, dtype=np.int64))
        inv = np.asarray(inv).reshape(-1)
        count = lambda mask: np.bincount(inv[mask], minlength=len(uniq)).astype(np.int64)
        reads = count(np.ones(len(self), dtype=bool))
        mod, unmod = count(self.llr >= threshold), count(self.llr <= -threshold)
        with np.errstate(invalid='ignore', divide='ignore'):
            freq = np.where(mod + unmod > 0, mod / np.maximum(mod + unmod, 1), np.nan)
        return dict(contig=uniq[:, 0].astype(np.int32), position=uniq[:, 1], strand=uniq[:, 2].astype(np.int8),
                    reads=reads, modified=mod, unmodified=unmod, ambiguous=reads - mod - unmod, frequency=freq)


def call_mods_batch(read_batch, aligner, kmer_model, pattern='CG', mod_offset=0, mod_code=4,
                    config=defaults.CONFIG_FILE, renorm_rounds=defaults.RENORM_ROUNDS):
    """Per read and per occurrence of ``pattern`` (over ``ACGT``, matched literally) in the read's reference part: the
    log-likelihood ratio of ``mod_code`` against the reference's base at ``pattern[mod_offset]``.  ``kmer_model``: a
    KmerModel (or a file) whose alphabet holds ``mod_code`` — a 4-letter table is refused.  The alignment of
    ``align_signal_batch`` (the same kernels, the same ``aligner`` contract; contexts and reference stay canonical),
    then on the rescaled signal the occurrences (``find_sites``) and ONE call that scores exactly those hypotheses
    (include/nadavca_hip.h: nvk_estimate_hypotheses_batch_dev) with ``config['model_wobbling']``, and one copy to
    the host.  A reverse read's part is the reverse strand: its sites are that strand's.  -> ModCallBatch."""
    import torch
    from .batchflow import align_batch, check_status, load_config, load_kmer_model
    from .device import estimate_hypotheses_dev, to_host
    from .readbatch import contig_local_range
    from .refset import ReferenceSet
    kmer_model = load_kmer_model(kmer_model)
    config = load_config(config)
    alphabet = kmer_model.get_alphabet_size()
    if int(mod_code) != mod_code or not 4 <= mod_code < alphabet:
        raise ValueError('call_mods_batch: the k-mer table has %d letters and no modified base with code %r '
                         '(kmer_train.extend_kmer_model makes a 5-letter table from a canonical one)'
                         % (alphabet, mod_code))
    codes = pattern_codes(pattern)
    if not 0 <= int(mod_offset) < len(codes):
        raise ValueError('call_mods_batch: mod_offset %r outside the pattern %r' % (mod_offset, pattern))
    res = align_batch(read_batch, config, kmer_model, renorm_rounds, aligner)
    stage = res.stage
    names = list(stage.reference.names) if isinstance(stage.reference, ReferenceSet) else None
    if stage.n_live == 0:
        return ModCallBatch.empty(contig_names=names)
    sa, dbatch = stage.sa, stage.dbatch
    start, end = contig_local_range(sa, stage.reference)
    site_off, owner, pos, forward, crowded = find_sites(
        dbatch.reference, dbatch.ref_off, start, end, sa.reverse, codes, mod_offset, kmer_model.get_k(),
        keep=res.status == _lib.READ_OK, total_ref=dbatch.total_ref)
    total, hyp, status = estimate_hypotheses_dev(
        dbatch, config['bandwidth'], config['min_event_length'], kmer_model, config['model_wobbling'], site_off, pos,
        torch.full_like(pos, int(mod_code)))
    status = torch.where(res.status != _lib.READ_OK, res.status, status)   # a read that did not align stays that
    check_status('estimate_hypotheses', status, sa.live, too_wide='skip')
    live = sa.live.cpu().numpy()
    ok = (status == _lib.READ_OK)[owner]
    owner = owner[ok]
    if int(owner.numel()) == 0:
        return ModCallBatch.empty(status.cpu().numpy(), live, total.cpu().numpy(), names)
    # one device-to-host copy: the rows as the columns of one table (every integer is exact in a double)
    table = to_host(torch.stack([(hyp[ok] - total[owner]), sa.live[owner].double(), forward[ok].double(),
                                 sa.reverse[owner].double(), sa.contig[owner].double(), crowded[ok].double()], 1))
    return ModCallBatch(table[:, 1].astype(np.int64), table[:, 4].astype(np.int32), table[:, 2].astype(np.int64),
                        table[:, 3].astype(np.int8), np.ascontiguousarray(table[:, 0]), table[:, 5] != 0,
                        status.cpu().numpy(), live, total.cpu().numpy(), names)
