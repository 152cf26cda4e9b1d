"""``call_indels_batch`` — per read and per candidate, "does this read carry a one-base insertion or a short deletion
against the reference here?" as a log-likelihood ratio under the HMM.

An edit ``(p, d, s)`` of a reference part deletes ``ref[p .. p+d)`` and puts the letters ``s`` in its place.  The
operator behind this workflow (include/nadavca_hip.h: nvk_estimate_edit_hypotheses_batch_dev) gives the read's
likelihood under the edited part; minus the read's total that is the ratio.  The workflow aligns a ``ReadBatch``
(``batchflow.align_batch``, the alignment of ``align_signal_batch``), enumerates on the device every left-aligned
candidate of every aligned read, scores them in ONE call and sums the ratios per site.

The host helpers of this module (``apply_edit``, ``mapped_bands``, ``canonical_candidates``, ``to_read_frame``) are
plain numpy and need no GPU: they state what the kernel and the enumeration compute."""
import os

import numpy as np

from . import defaults, _lib

MAX_ROWS = 14        # rows one edit hypothesis re-runs at most (a group of 16 lanes, two of which are not rows)
MAX_DEL = 8          # deleted bases per candidate this workflow enumerates at most (the operator takes up to 255)


def apply_edit(ref, anchors, p, d, s):
    """The edit ``(p, d, s)`` applied to a reference part and its anchors.  ``ref``: base codes; ``anchors``: (A, 2)
    rows of (signal index, reference index).  -> (ref', anchors', clean): ``ref' = ref[:p] + s + ref[p+d:]``; the
    anchors behind the edit shifted by ``len(s) - d``, those on a deleted base dropped; ``clean``: no anchor sat on a
    deleted base (then ``mapped_bands`` equals the bands the reference computes for ``(ref', anchors')``)."""
    ref = np.asarray(ref)
    s = np.asarray(s, dtype=ref.dtype).reshape(-1)
    p, d = int(p), int(d)
    anchors = np.asarray(anchors).reshape(-1, 2)
    at = anchors[:, 1]
    gone = (at >= p) & (at < p + d)
    out = anchors[~gone].copy()
    out[out[:, 1] >= p + d, 1] += s.size - d
    return np.concatenate([ref[:p], s, ref[p + d:]]), out, not bool(gone.any())


def mapped_bands(bs, be, R, p, d, i):
    """The bands of the edited part from the read's own ``bs`` / ``be`` (R + 1 boundary rows), the operator's
    definition: row r' of the R' + 1 = R - d + i + 1 rows has the band (bs[r'], be[r']) for r' < p, (bs[p-1], be[p+d])
    for the inserted rows p <= r' < p + i, and (bs[r'-i+d], be[r'-i+d]) behind them.  -> (bs', be')."""
    bs, be = np.asarray(bs), np.asarray(be)
    r = np.arange(R - d + i + 1)
    inserted = (r >= p) & (r < p + i)
    src = np.where(r < p, r, r - i + d)
    return (np.where(inserted, bs[p - 1], bs[np.clip(src, 0, R)]),
            np.where(inserted, be[min(p + d, R)], be[np.clip(src, 0, R)]))


def canonical_candidates(fwd, start, end, max_del=1, trim=5):
    """The candidate edits of the forward range [start, end) of ``fwd`` (base codes 0..3), left-aligned as a VCF has
    them so that every distinct edited sequence is listed once: a deletion of [x, x+d), d = 1 .. max_del, only if
    ``fwd[x-1] != fwd[x+d-1]`` (else deleting [x-1, x+d-1) gives the same sequence), an insertion of the letter s
    before x only if ``fwd[x-1] != s``; x = 0 has nothing to its left and always counts.  Positions keep ``trim``
    bases from either end of the range: start + trim <= x and x + d <= end - trim.
    -> (x int64, d int64, letter int64): forward positions, deleted bases (0 for an insertion) and the inserted
    letter (-1 for a deletion), ascending in x, deletions by d before insertions by letter."""
    fwd = np.asarray(fwd, dtype=np.int64)
    start, end, max_del, trim = int(start), int(end), int(max_del), int(trim)
    xs = np.arange(start + trim, end - trim + 1, dtype=np.int64)
    left = np.where(xs > 0, fwd[np.clip(xs - 1, 0, max(fwd.size - 1, 0))] if fwd.size else -2, -2)
    rows = []
    for d in range(1, max_del + 1):
        ok = xs + d <= end - trim
        ok &= left != fwd[np.clip(xs + d - 1, 0, max(fwd.size - 1, 0))] if fwd.size else False
        rows.append((xs[ok], np.full(int(ok.sum()), d), np.full(int(ok.sum()), -1), np.full(int(ok.sum()), d - 1)))
    for s in range(4):
        ok = left != s
        rows.append((xs[ok], np.zeros(int(ok.sum()), dtype=np.int64), np.full(int(ok.sum()), s),
                     np.full(int(ok.sum()), max_del + s)))
    x, d, letter, kind = (np.concatenate([r[c] for r in rows]).astype(np.int64) for c in range(4))
    order = np.lexsort((kind, x))
    return x[order], d[order], letter[order]


def to_read_frame(x, d, letter, start, end, reverse):
    """A forward-frame edit (delete [x, x+d), insert ``letter`` before it; -1: no letter) as the edit of the reference
    part of a read that covers the forward range [start, end): a forward read's part is ``fwd[start:end]``, a reverse
    read's its reverse complement, where the same edit deletes [end - x - d, end - x) and inserts the complementary
    letter.  Scalars or arrays.  -> (p, d, letter) in the part's frame."""
    x, d, letter = np.asarray(x), np.asarray(d), np.asarray(letter)
    reverse = np.asarray(reverse, dtype=bool)
    p = np.where(reverse, end - x - d, x - start)
    return p, d, np.where(reverse & (letter >= 0), 3 - letter, letter)


class IndelCallBatch:
    """What ``call_indels_batch`` returns.  The site table, one entry per distinct candidate ``(contig, position,
    del_len, ins_letter)`` that a read with status OK scored, sorted by them: ``contig`` (an index into
    ``contig_names`` with an aligner over a ``refset.ReferenceSet``; 0 and None otherwise), ``position`` (forward,
    contig-local and left-aligned: the first deleted base, or the base an inserted letter goes in front of),
    ``del_len`` (0 for an insertion), ``ins_letter`` (0..3, -1 for a deletion; a forward-strand letter), ``reads``
    (reads that scored the site), ``llr`` (their summed log-likelihood ratios) and ``support`` (reads with a ratio
    above 0).  ``called``: the indices of the sites whose ``llr`` exceeds ``threshold``.  Per-read rows, flat arrays in
    site order: ``row_site`` (index into the site table), ``row_read`` (index in the ReadBatch), ``row_strand``
    (0 forward, 1 reverse) and ``row_llr`` — of the called sites (``keep_rows='called'``), of every site ('all') or
    empty (None).  Per aligned read (``live``: its index in the ReadBatch): ``status`` (``_lib.READ_*``), ``total``
    (its log-likelihood without an edit, NaN where it did not run) and ``candidates`` (edits scored for it)."""

    def __init__(self, contig, position, del_len, ins_letter, reads, llr, support, threshold, row_site, row_read,
                 row_strand, row_llr, status, live, total, candidates, contig_names=None):
        self.contig, self.position, self.del_len, self.ins_letter = contig, position, del_len, ins_letter
        self.reads, self.llr, self.support, self.threshold = reads, llr, support, threshold
        self.called = np.nonzero(llr > threshold)[0]
        self.row_site, self.row_read, self.row_strand, self.row_llr = row_site, row_read, row_strand, row_llr
        self.status, self.live, self.total, self.candidates = status, live, total, candidates
        self.contig_names = contig_names

    @classmethod
    def empty(cls, threshold, status=None, live=None, total=None, contig_names=None):
        z = lambda dt: np.zeros(0, dtype=dt)
        n = 0 if live is None else len(live)
        return cls(z(np.int32), z(np.int64), z(np.int32), z(np.int8), z(np.int64), z(np.float64), z(np.int64),
                   threshold, z(np.int64), z(np.int64), z(np.int8), z(np.float64),
                   z(np.int32) if status is None else status, z(np.int64) if live is None else live,
                   z(np.float64) if total is None else total, np.zeros(n, dtype=np.int64), contig_names)

    def __len__(self):
        return int(self.position.size)

    def write_tsv(self, file, called_only=True):
        """Header, then one tab-separated row per site (the called ones, or all): contig (by name where the batch has
        names), position, del_len, ins (the letter, ``.`` for a deletion), reads, support and llr (as ``repr`` gives
        it), to ``file``, a path or a text file."""
        out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
        label = (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])
        rows = self.called if called_only else np.arange(len(self))
        try:
            out.write('contig\tposition\tdel_len\tins\treads\tsupport\tllr\n')
            out.writelines('%s\t%d\t%d\t%s\t%d\t%d\t%r\n'
                           % (label(int(self.contig[t])), self.position[t], self.del_len[t],
                              'ACGT'[self.ins_letter[t]] if self.ins_letter[t] >= 0 else '.', self.reads[t],
                              self.support[t], float(self.llr[t])) for t in rows.tolist())
        finally:
            if out is not file:
                out.close()


def enumerate_candidates(reference, ref_off, reverse, keep, max_del, trim, total_ref=None):
    """``canonical_candidates`` + ``to_read_frame`` for every reference part of a batch at once (int32 / int64 / bool
    tensors, any device; a part is in its READ's orientation and covers its read's whole forward range), with torch
    index operations — no loop over reads.  ``keep``: bool per read, reads without it get no candidates.
    -> (hyp_off int64 (n+1,), owner int64, local int64, edit_pos int32, edit_del int32, letter int64, ins_off int64,
    ins_base int32): candidate h of read ``owner[h]`` edits the forward position ``local[h]`` of the read's range
    (deleting ``edit_del[h]`` bases or inserting the forward letter ``letter[h]``, -1 for a deletion); ``edit_pos``,
    ``edit_del``, ``ins_off`` and ``ins_base`` are the lists of ``device.estimate_edit_hypotheses_dev`` in the parts'
    own frames."""
    import torch
    from .batchflow import seg_index
    dev = ref_off.device
    n = int(ref_off.numel()) - 1
    total = int(ref_off[-1]) if total_ref is None else int(total_ref)
    owner, inner = seg_index(ref_off, total)          # inner: the forward position x of the read's range
    length = (ref_off[1:] - ref_off[:-1])[owner]
    rev = reverse.to(dev)[owner]
    first = ref_off[:-1][owner]
    ref = reference[:total].to(torch.int64)

    def fwd_at(x):   # the forward-frame letter at position x of the owner's range (x clamped into it)
        x = torch.minimum(torch.clamp(x, min=0), length - 1)
        return torch.where(rev, 3 - ref[first + length - 1 - x], ref[first + x])
    left = fwd_at(inner - 1)
    inside = (inner >= trim) & keep.to(dev)[owner]
    masks, dels, letters = [], [], []
    for d in range(1, max_del + 1):   # (the kinds of candidate, not the reads)
        masks.append(inside & (inner + d <= length - trim) & (left != fwd_at(inner + d - 1)))
        dels.append(d)
        letters.append(-1)
    for s in range(4):
        masks.append(inside & (inner <= length - trim) & (left != s))
        dels.append(0)
        letters.append(s)
    at = torch.nonzero(torch.stack(masks, 1))         # row-major: by read, position, kind
    flat, kind = at[:, 0], at[:, 1]
    owner, local = owner[flat], inner[flat]
    d = torch.tensor(dels, dtype=torch.int64, device=dev)[kind]
    letter = torch.tensor(letters, dtype=torch.int64, device=dev)[kind]
    rev, length = rev[flat], length[flat]
    hyp_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(owner, minlength=n), 0, out=hyp_off[1:])
    edit_pos = torch.where(rev, length - local - d, local)
    is_ins = letter >= 0
    ins_off = torch.zeros(int(flat.numel()) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(is_ins.to(torch.int64), 0, out=ins_off[1:])
    ins_base = torch.where(rev, 3 - letter, letter)[is_ins]
    return (hyp_off, owner, local, edit_pos.to(torch.int32), d.to(torch.int32), letter, ins_off,
            ins_base.to(torch.int32))


def call_indels_batch(read_batch, aligner, kmer_model, max_del=1, trim=5, threshold=0.0, config=defaults.CONFIG_FILE,
                      renorm_rounds=defaults.RENORM_ROUNDS, keep_rows='called'):
    """Per read and per candidate edit of the read's reference part — deletions of 1 .. ``max_del`` bases and
    insertions of one letter of ``ACGT``, at least ``trim`` bases (>= 1) from either end of the part, left-aligned in
    the forward frame (``canonical_candidates``) — the log-likelihood ratio of the read under the edited part against
    the part as the reference has it, summed per site over the reads.  The alignment of ``align_signal_batch`` (the
    same kernels, the same ``aligner`` contract), then on the rescaled signal the enumeration
    (``enumerate_candidates``), ONE call that scores exactly those hypotheses (include/nadavca_hip.h:
    nvk_estimate_edit_hypotheses_batch_dev) with ``config['model_wobbling']``, a stable sort of the rows by site and a
    segmented sum on the device (no float atomics: two runs give the same bits), and one copy to the host.  A reverse
    read scores the same forward-frame edits mapped to its strand (``to_read_frame``).
    ``threshold``: a site is ``called`` when its summed ratio exceeds it.  There is NO calibrated default: the value
    is applied to a sum of nats over however many reads cover the site, and nothing but synthetic levels has been
    scored with it — 0.0 merely means "the reads together prefer the edit".  ``keep_rows``: 'called', 'all' or None
    (``IndelCallBatch``).  -> IndelCallBatch."""
    if int(max_del) != max_del or not 0 <= max_del <= MAX_DEL:
        raise ValueError('call_indels_batch: max_del %r outside 0 .. %d' % (max_del, MAX_DEL))
    if int(trim) != trim or trim < 1:
        raise ValueError('call_indels_batch: trim %r is not an integer >= 1 (an edit keeps one base of the part on '
                         'either side)' % (trim,))
    if keep_rows not in ('called', 'all', None):
        raise ValueError("call_indels_batch: keep_rows %r is not 'called', 'all' or None" % (keep_rows,))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError('call_indels_batch: threshold is NaN')
    import torch
    from .batchflow import align_batch, hypothesis_rows, load_config, load_kmer_model
    from .device import estimate_edit_hypotheses_dev, kmer_reduce_dev, to_host
    from .readbatch import contig_local_range
    kmer_model = load_kmer_model(kmer_model)
    config = load_config(config)
    max_del, trim = int(max_del), int(trim)
    k, central = kmer_model.get_k(), kmer_model.get_central_position()
    if (k if central == k - 1 else k - 1) + 1 > MAX_ROWS:   # (k - 1 + i rows; k + i where no base behind p is read)
        raise ValueError('call_indels_batch: a one-base insertion re-runs more than %d rows with k = %d'
                         % (MAX_ROWS, k))
    res = align_batch(read_batch, config, kmer_model, renorm_rounds, aligner)
    stage = res.stage
    names = stage.contig_names()
    if stage.n_live == 0:
        return IndelCallBatch.empty(threshold, contig_names=names)
    sa, dbatch = stage.sa, stage.dbatch
    start, _ = contig_local_range(sa, stage.reference)
    hyp_off, owner, local, edit_pos, edit_del, letter, ins_off, ins_base = enumerate_candidates(
        dbatch.reference, dbatch.ref_off, sa.reverse, res.status == _lib.READ_OK, max_del, trim, dbatch.total_ref)
    total, hyp, status = estimate_edit_hypotheses_dev(
        dbatch, config['bandwidth'], config['min_event_length'], kmer_model, config['model_wobbling'], hyp_off,
        edit_pos, edit_del, ins_off, ins_base)
    status, live, ok = hypothesis_rows('estimate_edit_hypotheses', res, status, owner)
    per_read = (hyp_off[1:] - hyp_off[:-1]).cpu().numpy()
    owner = owner[ok]
    if int(owner.numel()) == 0:
        return IndelCallBatch.empty(threshold, status.cpu().numpy(), live, total.cpu().numpy(), names)
    llr = hyp[ok] - total[owner]
    position = start.to(device=owner.device, dtype=torch.int64)[owner] + local[ok]
    # the site key (contig, position, del_len, letter) as one integer; a STABLE sort keeps the reads of a site in
    # batch order, so the segmented sum below adds them in the same order on every run
    span = int(position.max()) + 1
    kinds = 5 * (max_del + 1)                # del_len * 5 + letter + 1
    key = (sa.contig.to(torch.int64)[owner] * span + position) * kinds + edit_del[ok].to(torch.int64) * 5 \
        + letter[ok] + 1
    key, order = torch.sort(key, stable=True)
    llr, owner = llr[order], owner[order]
    site_key, site = torch.unique_consecutive(key, return_inverse=True)
    n_sites = int(site_key.numel())
    site_llr, site_support, site_reads = kmer_reduce_dev(kmer_model.context, site, llr.contiguous(),
                                                         (llr > 0).to(torch.int64), n_sites)
    keep = torch.ones_like(site, dtype=torch.bool) if keep_rows == 'all' else \
        (site_llr > threshold)[site] if keep_rows == 'called' else torch.zeros_like(site, dtype=torch.bool)
    # two device-to-host copies: the sites and the kept rows, each as one table (every integer is exact in a double)
    sites = to_host(torch.stack([site_key.double(), site_reads.double(), site_llr, site_support.double()], 1))
    rows = to_host(torch.stack([site[keep].double(), sa.live[owner[keep]].double(),
                                sa.reverse[owner[keep]].double(), llr[keep]], 1))
    skey = sites[:, 0].astype(np.int64)
    kind = skey % kinds
    return IndelCallBatch((skey // (kinds * span)).astype(np.int32), skey // kinds % span,
                          (kind // 5).astype(np.int32), (kind % 5 - 1).astype(np.int8),
                          sites[:, 1].astype(np.int64), np.ascontiguousarray(sites[:, 2]),
                          sites[:, 3].astype(np.int64), threshold, rows[:, 0].astype(np.int64),
                          rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int8), np.ascontiguousarray(rows[:, 3]),
                          status.cpu().numpy(), live, total.cpu().numpy(), per_read, names)
