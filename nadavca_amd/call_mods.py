"""``call_mods_batch`` — per read and per site, "is this base modified?" as a log-likelihood ratio under the HMM.

With a table whose alphabet holds a modified base beside ``ACGT`` (code 4, ``M``; ``kmer_train.extend_kmer_model``
makes one from a canonical table and known levels) and the canonical reference, the entry ``[p, 4]`` of
``estimate_log_likelihoods`` minus the entry ``[p, reference[p]]`` is the log-likelihood ratio of "base p is ``M``"
against "base p is what the reference says" (dtw.cpp:93-129 and 83-85, wobble rows and both quirks included).  The
full matrix scores every base of a read against every letter; a caller wants one letter at the positions where a
pattern occurs.  This workflow aligns a ``ReadBatch`` (``batchflow.align_batch``, the alignment of
``align_signal_batch``), finds the pattern's occurrences in every read's reference part on the device and scores
only those (``device.estimate_hypotheses_dev``).

One substitution per hypothesis by default: a site is scored against an otherwise canonical reference.  Two sites
closer than k bases share a k-mer and are each scored with the other assumed unmodified; such rows carry ``crowded``.
With ``joint=True`` neighbouring sites are grouped into clusters (``cluster_sites``), every non-empty subset of a
cluster is scored as ONE hypothesis that carries all its substitutions (``device.estimate_joint_hypotheses_dev``), and
a site's ratio is the marginal over its neighbours' states (``marginal_llr``)."""
import math
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


MAX_JOINT = 8   # sites per cluster at most: 2^m - 1 hypotheses each


def cluster_sites(owner, pos, k, max_joint):
    """Groups the sites of ``find_sites`` (``owner`` int64, ``pos`` ascending within a read; any device) into
    clusters that one joint hypothesis can hold.  Walking a read's sites in ascending position, a site joins the open
    cluster if it lies within k - 1 of the previous site (the two share a k-mer), within 14 - k of the cluster's
    first site (the re-run of first - back .. last + fwd then fits the 14 rows of a 16-lane hypothesis group; a read's
    end only shortens it) and the cluster holds fewer than ``max_joint`` sites; otherwise it opens a new one.  Torch
    index operations: the walk is the orbit of "next cluster start" from every start of a run of close sites, marked
    by pointer doubling — no loop over reads or sites.
    -> (cluster int64 per site: its cluster, numbered in row order; first int64 per cluster: its first row; size
    int64 per cluster; cut bool per site: a site within k - 1 bases lies in ANOTHER cluster)."""
    import torch
    dev = pos.device
    n = int(pos.numel())
    z = torch.zeros(0, dtype=torch.int64, device=dev)
    if n == 0:
        return z, z, z, torch.zeros(0, dtype=torch.bool, device=dev)
    k, max_joint = int(k), int(max_joint)
    p64 = pos.to(torch.int64)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    near = torch.zeros(n, dtype=torch.bool, device=dev)      # close to the row before
    near[1:] = (owner[1:] == owner[:-1]) & (p64[1:] - p64[:-1] <= k - 1)
    run_first = torch.nonzero(~near).reshape(-1)
    run_end = torch.cat([run_first[1:], torch.full((1,), n, dtype=torch.int64, device=dev)])
    end_of = run_end[torch.cumsum((~near).to(torch.int64), 0) - 1]
    # the first row after s that cannot share s's cluster: beyond the span, beyond max_joint rows, or in another run
    span = max(14 - k, 0)
    key = owner.to(torch.int64) * (int(p64.max()) + span + 2) + p64
    nxt = torch.minimum(torch.minimum(torch.searchsorted(key, key + span, right=True), idx + max_joint), end_of)
    jump = torch.cat([torch.where(nxt >= end_of, torch.full_like(nxt, n), nxt),
                      torch.full((1,), n, dtype=torch.int64, device=dev)])     # row n: the end of every walk
    mark = torch.cat([~near, torch.zeros(1, dtype=torch.bool, device=dev)])
    count = int(mark.sum())
    while True:   # round t marks the starts 2^t .. 2^(t+1) - 1 steps along every walk
        mark[jump[torch.nonzero(mark).reshape(-1)]] = True
        mark[n] = False
        jump = jump[jump]
        now = int(mark.sum())
        if now == count:
            break
        count = now
    start = mark[:n]
    cluster = torch.cumsum(start.to(torch.int64), 0) - 1
    first = torch.nonzero(start).reshape(-1)
    size = torch.bincount(cluster, minlength=int(first.numel()))
    # clusters are runs of rows: the nearest sites outside one are the row before its first and the row after its last
    before, after = first[cluster] - 1, (first + size)[cluster]
    b, a = before.clamp(min=0), after.clamp(max=n - 1)
    cut = ((before >= 0) & (owner[b] == owner) & (p64 - p64[b] <= k - 1)) | \
          ((after < n) & (owner[a] == owner) & (p64[a] - p64 <= k - 1))
    return cluster, first, size, cut


def marginal_llr(values, size, site_prior=0.5):
    """Per-site log-likelihood ratios from the joint log-likelihoods of a cluster's subsets.  ``values``: (C, 2^J)
    f64 tensor, column ``mask`` = the log-likelihood with exactly the sites of ``mask`` modified (bit j: the cluster's
    j-th site; column 0: none, the read's total; columns >= 2^size are ignored); ``size``: int64 (C,).
    -> (C, J) f64: entry [c, j] = logsumexp over the subsets WITH site j minus logsumexp over those without it, every
    subset weighted by ``site_prior`` / ``1 - site_prior`` for each OTHER site of the cluster that it holds / does not
    hold — the site's own prior is not in it, so the value stays a likelihood ratio (entries with j >= size: -inf)."""
    import torch
    n_mask = int(values.shape[1])
    J = n_mask.bit_length() - 1
    if n_mask != 1 << J:
        raise ValueError('marginal_llr: %d columns are not a power of two' % n_mask)
    dev = values.device
    masks = torch.arange(n_mask, dtype=torch.int64, device=dev)
    valid = masks[None, :] < torch.bitwise_left_shift(torch.ones_like(size), size)[:, None]
    minus = torch.full_like(values, -math.inf)
    lp, lq = math.log(site_prior), math.log1p(-site_prior)
    out = torch.empty((int(values.shape[0]), J), dtype=values.dtype, device=dev)
    for j in range(J):   # (the sites of a cluster, not the clusters)
        others = masks & ~(1 << j)
        held = sum(((others >> t) & 1) for t in range(J)).to(values.dtype)
        weight = held[None, :] * lp + (size.to(values.dtype)[:, None] - 1.0 - held[None, :]) * lq
        a = torch.where(valid, values + weight, minus)
        has = ((masks >> j) & 1).bool()[None, :]
        out[:, j] = torch.logsumexp(torch.where(has, a, minus), 1) - torch.logsumexp(torch.where(has, minus, a), 1)
    return out


def joint_lists(owner, pos, n_reads, first, size, mod_code):
    """The two-level hypothesis list of ``device.estimate_joint_hypotheses_dev`` for the clusters of
    ``cluster_sites``: cluster c contributes its 2^size - 1 non-empty subsets in ascending ``mask`` (bit j: its j-th
    site), each with its sites' positions and ``mod_code``.
    -> (hyp_off (n_reads+1,), sub_off, sub_pos int32, sub_base int32, hyp_cluster, hyp_mask): the cluster and the mask
    of every hypothesis."""
    import torch
    from .batchflow import seg_index
    dev = pos.device
    n_hyp_c = torch.bitwise_left_shift(torch.ones_like(size), size) - 1
    c_off = torch.zeros(int(size.numel()) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_hyp_c, 0, out=c_off[1:])
    n_hyp = int(c_off[-1])
    hyp_cluster, inner = seg_index(c_off, n_hyp)
    hyp_mask = inner + 1
    hyp_off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    per_read = torch.zeros(n_reads, dtype=torch.int64, device=dev)
    per_read.index_add_(0, owner[first], n_hyp_c)
    torch.cumsum(per_read, 0, out=hyp_off[1:])
    J = int(size.max()) if int(size.numel()) else 1
    bits = ((hyp_mask[:, None] >> torch.arange(J, dtype=torch.int64, device=dev)[None, :]) & 1).bool()
    sub_off = torch.zeros(n_hyp + 1, dtype=torch.int64, device=dev)
    torch.cumsum(bits.sum(1), 0, out=sub_off[1:])
    at = torch.nonzero(bits)   # row-major: ascending site, so ascending position, within a hypothesis
    sub_pos = pos[first[hyp_cluster[at[:, 0]]] + at[:, 1]].to(torch.int32)
    return hyp_off, sub_off, sub_pos, torch.full_like(sub_pos, int(mod_code)), hyp_cluster, hyp_mask


class SiteScores:
    """What ``score_sites`` returns, device tensors unless noted.  Per site of ``find_sites`` (read order, ascending
    position): ``owner`` (its live read), ``pos``, ``forward``, ``crowded`` (with ``joint``: a site within k - 1 bases
    lies in ANOTHER cluster), ``hyp`` (the log-likelihood with the site alone modified), ``llr`` (with ``joint``: the
    marginal ratio; else ``hyp - total[owner]``), ``cluster_size`` (None without ``joint``) and ``ok`` (its read is
    READ_OK after the scoring; the rows of ``call_mods_batch`` are the sites with it).  Per live read: ``site_off``
    (n_live + 1,), ``total`` (the log-likelihood without a substitution) and ``status``; ``live``: a numpy array."""
    __slots__ = ('site_off', 'owner', 'pos', 'forward', 'crowded', 'total', 'hyp', 'llr', 'cluster_size', 'status',
                 'live', 'ok')


def score_sites(res, config, kmer_model, codes, mod_offset, mod_code, joint, max_joint, site_prior):
    """The part of ``call_mods_batch`` behind ``align_batch``, which ``mod_train.estimate_mod_model`` shares: the
    pattern's occurrences in the reads of the BatchAlignment ``res`` that aligned (``find_sites``) and their ratios
    from ONE call of the listed or the joint operator, on the device.  ``res.stage.n_live > 0``; ``config`` loaded,
    ``kmer_model`` a KmerModel holding ``mod_code``, ``codes`` the pattern's base codes.  -> SiteScores."""
    import torch
    from .batchflow import hypothesis_rows
    from .device import estimate_hypotheses_dev, estimate_joint_hypotheses_dev
    from .readbatch import contig_local_range
    stage = res.stage
    sa, dbatch = stage.sa, stage.dbatch
    start, end = contig_local_range(sa, stage.reference)
    site_off, owner, pos, forward, crowded = find_sites(
        dbatch.reference, dbatch.ref_off, start, end, sa.reverse, codes, mod_offset, kmer_model.get_k(),
        keep=res.status == _lib.READ_OK, total_ref=dbatch.total_ref)
    hyp_args = (dbatch, config['bandwidth'], config['min_event_length'], kmer_model, config['model_wobbling'])
    llr = cluster_size = None
    if joint:
        cluster, first, size, cut = cluster_sites(owner, pos, kmer_model.get_k(), max_joint)
        hyp_off, sub_off, sub_pos, sub_base, hyp_cluster, hyp_mask = joint_lists(owner, pos, stage.n_live, first, size,
                                                                                 mod_code)
        total, joint_ll, status = estimate_joint_hypotheses_dev(*hyp_args, hyp_off, sub_off, sub_pos, sub_base)
        # the clusters' subsets as a dense table (column: mask; column 0: no site, the read's total)
        values = torch.full((int(first.numel()), 1 << (int(size.max()) if int(size.numel()) else 0)), -math.inf,
                            dtype=torch.float64, device=pos.device)
        values[:, 0] = total[owner[first]]
        values[hyp_cluster, hyp_mask] = joint_ll
        rank = torch.arange(int(pos.numel()), dtype=torch.int64, device=pos.device) - first[cluster]
        hyp = values[cluster, torch.bitwise_left_shift(torch.ones_like(rank), rank)]      # the singleton subsets
        cluster_size = size[cluster]
        llr = torch.where(cluster_size > 1, marginal_llr(values, size, float(site_prior))[cluster, rank],
                          hyp - total[owner]) if int(pos.numel()) else hyp
        crowded = cut
    else:
        total, hyp, status = estimate_hypotheses_dev(*hyp_args, site_off, pos, torch.full_like(pos, int(mod_code)))
        llr = hyp - total[owner]
    status, live, ok = hypothesis_rows('estimate_joint_hypotheses' if joint else 'estimate_hypotheses', res, status,
                                       owner)
    sc = SiteScores()
    sc.site_off, sc.owner, sc.pos, sc.forward, sc.crowded = site_off, owner, pos, forward, crowded
    sc.total, sc.hyp, sc.llr, sc.cluster_size = total, hyp, llr, cluster_size
    sc.status, sc.live, sc.ok = status, live, ok
    return sc


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
    run).
    A batch made with ``joint=True`` also has ``cluster`` (int32: the sites of the row's cluster, 1 for a site scored
    alone) and ``llr_single`` (the one-substitution ratio, what ``llr`` is without ``joint``); both are None
    otherwise.  ``llr`` is then the marginal over the states of the cluster's other sites, and ``crowded`` is true
    only where a site within k - 1 bases lies OUTSIDE the row's cluster (a cluster had to be cut): ``llr`` there is
    conditional on that neighbour being canonical."""

    def __init__(self, read, contig, position, strand, llr, crowded, status, live, total, contig_names=None,
                 cluster=None, llr_single=None):
        self.read, self.contig, self.position, self.strand = read, contig, position, strand
        self.llr, self.crowded = llr, crowded
        self.status, self.live, self.total = status, live, total
        self.contig_names = contig_names
        self.cluster, self.llr_single = cluster, llr_single

    @classmethod
    def empty(cls, status=None, live=None, total=None, contig_names=None, joint=False):
        z = lambda dt: np.zeros(0, dtype=dt)
        return cls(z(np.int64), z(np.int32), z(np.int64), z(np.int8), z(np.float64), z(bool),
                   z(np.int32) if status is None else status, z(np.int64) if live is None else live,
                   z(np.float64) if total is None else total, contig_names,
                   z(np.int32) if joint else None, z(np.float64) if joint else None)

    def __len__(self):
        return int(self.position.size)

    def _contig_label(self):
        return (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])

    def write_tsv(self, file, names=None):
        """Header, then one tab-separated row per site: read, contig, position, strand (``+`` / ``-``), llr (as
        ``repr`` gives it), crowded (0 / 1), to ``file``, a path or a text file; a batch made with ``joint=True``
        appends the columns cluster and llr_single.  ``names[i]``: the name of ReadBatch read i (default
        ``'read%d' % i``); the contig by name where the batch has names, by index otherwise."""
        out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
        joint = self.cluster is not None
        try:
            out.write('read\tcontig\tposition\tstrand\tllr\tcrowded%s\n' % ('\tcluster\tllr_single' if joint else ''))
            name = (lambda i: 'read%d' % i) if names is None else (lambda i: names[i])
            label = self._contig_label()
            more = (['\t%d\t%r' % (m, v) for m, v in zip(self.cluster.tolist(), self.llr_single.tolist())] if joint
                    else [''] * len(self))
            out.writelines('%s\t%s\t%d\t%s\t%r\t%d%s\n' % (name(i), label(c), p, '-' if s else '+', v, w, x)
                           for i, c, p, s, v, w, x in zip(self.read.tolist(), self.contig.tolist(),
                                                          self.position.tolist(), self.strand.tolist(),
                                                          self.llr.tolist(), self.crowded.tolist(), more))
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
                    config=defaults.CONFIG_FILE, renorm_rounds=defaults.RENORM_ROUNDS, joint=False, max_joint=4,
                    site_prior=0.5):
    """Per read and per occurrence of ``pattern`` (over ``ACGT``, matched literally) in the read's reference part: the
    log-likelihood ratio of ``mod_code`` against the reference's base at ``pattern[mod_offset]``.  ``kmer_model``: a
    KmerModel (or a file) whose alphabet holds ``mod_code`` — a 4-letter table is refused.  The alignment of
    ``align_signal_batch`` (the same kernels, the same ``aligner`` contract; contexts and reference stay canonical),
    then on the rescaled signal the occurrences (``find_sites``) and ONE call that scores exactly those hypotheses
    (include/nadavca_hip.h: nvk_estimate_hypotheses_batch_dev) with ``config['model_wobbling']``, and one copy to
    the host.  A reverse read's part is the reverse strand: its sites are that strand's.
    ``joint=True``: sites that share a k-mer are scored jointly.  ``cluster_sites`` groups them (at most ``max_joint``
    per cluster, 1 .. 8), ONE call scores every non-empty subset of every cluster as a hypothesis with all its
    substitutions (include/nadavca_hip.h: nvk_estimate_joint_hypotheses_batch_dev; a cluster of one is the single
    hypothesis of ``joint=False``, bit for bit), and ``llr`` is the site's marginal ratio (``marginal_llr``; every
    other site of the cluster modified with probability ``site_prior``, in the open interval (0, 1)).  The rows, their
    order and coordinates are those of ``joint=False``; ``cluster``, ``llr_single`` and the narrower meaning of
    ``crowded`` are described at ``ModCallBatch``.  Where k leaves no room for two sites in 14 rows, every cluster is
    one site and ``llr`` equals that of ``joint=False``.  -> ModCallBatch."""
    if int(max_joint) != max_joint or not 1 <= max_joint <= MAX_JOINT:
        raise ValueError('call_mods_batch: max_joint %r outside 1 .. %d' % (max_joint, MAX_JOINT))
    if not 0.0 < float(site_prior) < 1.0:
        raise ValueError('call_mods_batch: site_prior %r outside the open interval (0, 1)' % (site_prior,))
    import torch
    from .batchflow import align_batch, load_config, load_kmer_model
    from .device import to_host
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
    names = stage.contig_names()
    if stage.n_live == 0:
        return ModCallBatch.empty(contig_names=names, joint=joint)
    sa = stage.sa
    sc = score_sites(res, config, kmer_model, codes, mod_offset, mod_code, joint, max_joint, site_prior)
    owner, forward, crowded, total, hyp, status, live, ok = (sc.owner, sc.forward, sc.crowded, sc.total, sc.hyp,
                                                             sc.status, sc.live, sc.ok)
    llr, cluster_size = sc.llr, sc.cluster_size
    owner = owner[ok]
    if int(owner.numel()) == 0:
        return ModCallBatch.empty(status.cpu().numpy(), live, total.cpu().numpy(), names, joint=joint)
    # one device-to-host copy: the rows as the columns of one table (every integer is exact in a double)
    single = hyp[ok] - total[owner]
    columns = [single, sa.live[owner].double(), forward[ok].double(), sa.reverse[owner].double(),
               sa.contig[owner].double(), crowded[ok].double()]
    if joint:
        columns += [llr[ok], cluster_size[ok].double()]
    table = to_host(torch.stack(columns, 1))
    more = (table[:, 7].astype(np.int32), np.ascontiguousarray(table[:, 0])) if joint else ()
    return ModCallBatch(table[:, 1].astype(np.int64), table[:, 4].astype(np.int32), table[:, 2].astype(np.int64),
                        table[:, 3].astype(np.int8), np.ascontiguousarray(table[:, 6 if joint else 0]),
                        table[:, 5] != 0, status.cpu().numpy(), live, total.cpu().numpy(), names, *more)
