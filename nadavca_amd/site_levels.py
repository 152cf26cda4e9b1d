"""``site_levels_batch`` and ``compare_site_levels`` — model-free site tests: the pile-up of the reads' event levels per
reference position and strand, and a two-sample test between two such pile-ups.

Every other per-site workflow needs a k-mer table that already knows the answer (``call_mods_batch`` a 5-letter one).
The usual way around a missing model is a native sample against an unmodified control: both are aligned against the SAME
canonical table, so their event levels are comparable, and a site whose levels differ between the samples is a candidate
(Tombo's sample compare, nanocompore and xPore work this way, on nanopolish ``eventalign``-style tables).  The device
part is the pile-up — per (read, base) the event's mean, standard deviation, length and distance from the expected
level; a stable sort by (position, strand); per site the count, the means and the sums of squared deviations — with the
contract in include/nadavca_hip.h (nvk_site_level_rows_dev) and the kernels in csrc/kernels_sitelevels.hip.  The
statistics are numpy on the host, from moments that can be saved, merged (``SiteLevelBatch.merge``: the hook for several
batches or ranks) and reused: a control sample is summarised once.  Single process only."""
import numpy as np

from . import defaults
from .site_tests import SiteTable, _open, _same_reference, _site_key, check_site_test, contig_label, site_coordinates

COLUMNS = ('level', 'stdv', 'dwell', 'resid')
EVENT_COLUMNS = ('read', 'contig', 'position', 'strand', 'level', 'stdv', 'dwell', 'expected')


class SiteLevelBatch:
    """What ``site_levels_batch`` returns.  Row arrays, one row per (position, strand) that at least one event covers,
    ascending in (global position, strand): ``contig`` (an index into ``contig_names`` with an aligner over a
    ``refset.ReferenceSet``; 0 and None otherwise), ``position`` (forward, contig-local), ``strand`` (0 forward, 1
    reverse), ``ref_base`` (the FORWARD reference's base code at the position, on either strand), ``count`` (events),
    ``mean`` and ``m2`` (n, 4): per column of ``COLUMNS`` = (level, stdv, dwell, resid) the mean over the site's events
    and the sum of their squared deviations from it.  ``ref_len``: bases of the whole reference (of the concatenation
    for a ReferenceSet).  Per aligned read (``live``: its index in the ReadBatch) its ``status`` (``_lib.READ_*``; a
    read with status != 0 adds nothing).  ``events``: None, or with ``rows=True`` the per-read table, a dict of arrays
    over the counted events in read order with the keys ``EVENT_COLUMNS`` (``expected``: the table's level of the
    base's k-mer, so that resid = level - expected)."""

    COLUMNS = COLUMNS

    def __init__(self, contig, position, strand, ref_base, count, mean, m2, ref_len, contig_names=None, status=None,
                 live=None, events=None):
        self.contig, self.position, self.strand, self.ref_base = contig, position, strand, ref_base
        self.count, self.mean, self.m2 = count, mean, m2
        self.ref_len, self.contig_names = int(ref_len), contig_names
        self.status = np.zeros(0, dtype=np.int32) if status is None else status
        self.live = np.zeros(0, dtype=np.int64) if live is None else live
        self.events = events

    @classmethod
    def empty(cls, ref_len, contig_names=None, status=None, live=None, rows=False):
        z = lambda dt: np.zeros(0, dtype=dt)
        events = None
        if rows:
            events = {c: z(np.float64 if c in ('level', 'stdv', 'dwell', 'expected') else np.int64)
                      for c in EVENT_COLUMNS}
        return cls(z(np.int32), z(np.int64), z(np.int8), z(np.int8), z(np.int64), np.zeros((0, len(COLUMNS))),
                   np.zeros((0, len(COLUMNS))), ref_len, contig_names, status, live, events)

    def __len__(self):
        return int(self.position.size)

    @staticmethod
    def column_index(column):
        if column not in COLUMNS:
            raise ValueError('column %r is not one of %s' % (column, ', '.join(COLUMNS)))
        return COLUMNS.index(column)

    def sd(self, column):
        """The sample standard deviation sqrt(m2 / (count - 1)) of ``column`` per row; NaN where count < 2."""
        j = self.column_index(column)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(self.count >= 2, np.sqrt(self.m2[:, j] / np.maximum(self.count - 1, 1)), np.nan)

    def write_tsv(self, file):
        """Header, then one tab-separated row per site: contig (by name where the batch has names), position, strand
        (+ / -), ref, count, then mean and sd of every column (floats as ``repr`` gives them), to ``file``, a path or
        a text file."""
        label, sds = contig_label(self.contig_names), [self.sd(c) for c in COLUMNS]
        with _open(file) as out:
            out.write('contig\tposition\tstrand\tref\tcount\t'
                      + '\t'.join('%s_mean\t%s_sd' % (c, c) for c in COLUMNS) + '\n')
            for t in range(len(self)):
                stats = '\t'.join('%r\t%r' % (float(self.mean[t, j]), float(sds[j][t])) for j in range(len(COLUMNS)))
                out.write('%s\t%d\t%s\t%s\t%d\t%s\n' % (label(int(self.contig[t])), self.position[t],
                                                        '+-'[self.strand[t]], 'ACGT'[self.ref_base[t]],
                                                        self.count[t], stats))

    def write_events_tsv(self, file, names=None):
        """The per-read event table of a ``rows=True`` batch in the style of nanopolish ``eventalign``: header, then
        one row per counted event in read order: read, contig, position, strand, level, stdv, dwell (samples),
        expected.  ``names[i]``: the name of ReadBatch read i (default ``'read%d' % i``)."""
        if self.events is None:
            raise ValueError('write_events_tsv: the batch carries no event table (site_levels_batch(rows=True))')
        label, ev = contig_label(self.contig_names), self.events
        name = (lambda i: 'read%d' % i) if names is None else (lambda i: names[i])
        with _open(file) as out:
            out.write('\t'.join(EVENT_COLUMNS) + '\n')
            out.writelines('%s\t%s\t%d\t%s\t%r\t%r\t%d\t%r\n'
                           % (name(int(ev['read'][t])), label(int(ev['contig'][t])), ev['position'][t],
                              '+-'[ev['strand'][t]], float(ev['level'][t]), float(ev['stdv'][t]), ev['dwell'][t],
                              float(ev['expected'][t])) for t in range(int(ev['read'].size)))

    def save(self, path):
        """Everything into one ``.npz`` (``load`` reads it back): a control sample is summarised once."""
        names = self.contig_names
        data = dict(contig=self.contig, position=self.position, strand=self.strand, ref_base=self.ref_base,
                    count=self.count, mean=self.mean, m2=self.m2, ref_len=np.int64(self.ref_len),
                    has_names=np.bool_(names is not None), contig_names=np.array(names or [], dtype=np.str_),
                    status=self.status, live=self.live, has_events=np.bool_(self.events is not None))
        if self.events is not None:
            data.update({'events_' + c: self.events[c] for c in EVENT_COLUMNS})
        with open(path, 'wb') as f:      # (np.savez would add '.npz' to a path without it)
            np.savez(f, **data)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            names = [str(x) for x in z['contig_names']] if bool(z['has_names']) else None
            events = {c: z['events_' + c] for c in EVENT_COLUMNS} if bool(z['has_events']) else None
            return cls(z['contig'], z['position'], z['strand'], z['ref_base'], z['count'], z['mean'], z['m2'],
                       int(z['ref_len']), names, z['status'], z['live'], events)

    def merge(self, other):
        """Pools two batches over the same reference (more reads of one sample, another batch or another rank's share):
        per site Chan's pairwise update on the host, n = na + nb, d = mean_b - mean_a, mean = mean_a + d nb / n,
        m2 = m2_a + m2_b + d^2 na nb / n; a site that only one batch holds is copied.  ``status`` and ``live`` are
        those of this batch followed by the other's; the event tables are not carried over (their read indices belong
        to two ReadBatches).  Different ``ref_len`` or ``contig_names``: ValueError.  -> SiteLevelBatch."""
        _same_reference('SiteLevelBatch.merge', self, other)
        ka = _site_key(self.contig, self.position, self.strand, self.ref_len)
        kb = _site_key(other.contig, other.position, other.strand, other.ref_len)
        keys = np.union1d(ka, kb)
        n, V = keys.size, len(COLUMNS)
        ia, ib = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
        na, nb = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        ma, mb, qa, qb = (np.zeros((n, V)) for _ in range(4))
        na[ia], ma[ia], qa[ia] = self.count, self.mean, self.m2
        nb[ib], mb[ib], qb[ib] = other.count, other.mean, other.m2
        tot = na + nb
        fa, fb, ft = na.astype(np.float64)[:, None], nb.astype(np.float64)[:, None], tot.astype(np.float64)[:, None]
        with np.errstate(invalid='ignore'):
            d = mb - ma
            mean = np.where(fb == 0, ma, np.where(fa == 0, mb, ma + d * fb / ft))
            m2 = np.where(fb == 0, qa, np.where(fa == 0, qb, qa + qb + d * d * fa * fb / ft))
        first = np.unique(np.concatenate([ka, kb]), return_index=True)[1]    # a row of either batch per merged site
        pick = lambda xa, xb, dt: np.concatenate([xa, xb])[first].astype(dt)
        return SiteLevelBatch(pick(self.contig, other.contig, np.int32), pick(self.position, other.position, np.int64),
                              pick(self.strand, other.strand, np.int8), pick(self.ref_base, other.ref_base, np.int8),
                              tot, mean, m2, self.ref_len, self.contig_names,
                              np.concatenate([self.status, other.status]), np.concatenate([self.live, other.live]))


def site_levels_batch(read_batch, aligner, kmer_model=defaults.KMER_MODEL_FILE, config=defaults.CONFIG_FILE,
                      renorm_rounds=defaults.RENORM_ROUNDS, trim=5, rows=False):
    """The pile-up of the reads' event levels per reference position and strand.  The front end is
    ``align_signal_batch``'s (``batchflow.align_batch``: per-read normalisation, approximate alignment, the
    renormalise / re-align loop); then on the device the expected levels with contexts and ONE
    ``device.site_levels_dev`` call over the final events and the signal after the last rescale (per-event values,
    stable sort by (position, strand), per-site moments: no float atomics, two runs give the same bits), and one copy
    of the covered sites to the host.  Two samples aligned against the same ``kmer_model`` have comparable levels:
    ``compare_site_levels``.
    ``aligner``: a batch aligner, as for ``align_signal_batch``; with one over a ``refset.ReferenceSet`` the rows are
    contig-local and named.  ``trim``: events this close to either end of a read's aligned part are not counted (the
    alignment is least certain there).  ``rows``: also keep the per-read event table (``SiteLevelBatch.events``,
    ``write_events_tsv``).  Reads that did not align show in ``status`` / ``live`` and add nothing; a band wider than
    the kernels serve is skipped with a note, as elsewhere.  Single process only (no ``distributed``; ``merge`` pools
    results).  -> SiteLevelBatch."""
    if int(trim) != trim or trim < 0:
        raise ValueError('site_levels_batch: trim %r is not an integer >= 0' % (trim,))
    import torch
    from .batchflow import align_batch, load_config, load_kmer_model, seg_index
    from .device import expected_levels_dev, site_levels_dev, to_host
    from .refset import ReferenceSet
    kmer_model = load_kmer_model(kmer_model)
    res = align_batch(read_batch, load_config(config), kmer_model, renorm_rounds, aligner)
    stage = res.stage
    refset = stage.reference if isinstance(stage.reference, ReferenceSet) else None
    names = stage.contig_names()
    reference_num = np.ascontiguousarray(aligner.reference_num, dtype=np.int32).reshape(-1)
    L = reference_num.size
    if stage.n_live == 0 or L == 0:
        return SiteLevelBatch.empty(L, names, rows=rows)
    sa, dbatch, context = stage.sa, stage.dbatch, kmer_model.context
    expected = expected_levels_dev(dbatch, kmer_model, with_contexts=True)
    count, mean, m2, key, val = site_levels_dev(context, dbatch, res.events, expected, sa.ref_start.contiguous(),
                                                sa.reverse.to(torch.int32), res.status, int(trim), L)
    # everything per key on the device; only the covered sites (and the counted events) cross to the host, as the
    # columns of tables of doubles (every integer here is exact in one: keys are below 2^53)
    q = torch.nonzero(count > 0).reshape(-1)
    parts = [torch.cat([q.double()[:, None], count[q].double()[:, None], mean[q], m2[q]], 1).reshape(-1)]
    n_sites, n_events, V = int(q.numel()), 0, len(COLUMNS)
    if rows:
        at = torch.nonzero(key >= 0).reshape(-1)
        n_events = int(at.numel())
        owner = seg_index(dbatch.ref_off, dbatch.total_ref)[0][at]
        parts.append(torch.stack([sa.live[owner].double(), key[at].double(), val[at, 0], val[at, 1], val[at, 2],
                                  expected[at]], 1).reshape(-1))
    parts.append(res.status.double())
    flat = to_host(torch.cat(parts))
    table = flat[:n_sites * (2 + 2 * V)].reshape(n_sites, 2 + 2 * V)
    rest = flat[table.size:]
    site_key = table[:, 0].astype(np.int64)
    contig, position, strand = site_coordinates(site_key, refset)
    events = None
    if rows:
        et = rest[:n_events * 6].reshape(n_events, 6)
        e_contig, e_position, e_strand = site_coordinates(et[:, 1].astype(np.int64), refset)
        col = lambda j: np.ascontiguousarray(et[:, j])
        events = dict(read=et[:, 0].astype(np.int64), contig=e_contig, position=e_position, strand=e_strand,
                      level=col(2), stdv=col(3), dwell=et[:, 4].astype(np.int64), expected=col(5))
    status = rest[n_events * 6 if rows else 0:].astype(np.int32)
    return SiteLevelBatch(contig, position, strand, reference_num[site_key >> 1].astype(np.int8),
                          table[:, 1].astype(np.int64), np.ascontiguousarray(table[:, 2:2 + V]),
                          np.ascontiguousarray(table[:, 2 + V:]), L, names, status, sa.live.cpu().numpy(), events)


class SiteComparison(SiteTable):
    """What ``compare_site_levels`` returns.  Row arrays, one row per (contig, position, strand) that both batches
    hold with count >= min_coverage, in the batches' order: ``contig``, ``position``, ``strand``, ``ref_base``,
    ``n_a``, ``n_b``, ``mean_a``, ``mean_b``, ``delta`` = mean_b - mean_a, Welch's ``t``, its Welch-Satterthwaite
    ``df``, the two-sided ``p`` and ``peak``; ``column``: what was compared; ``contig_names`` as the batches'."""

    _FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'mean_a', 'mean_b', 'delta', 't', 'df', 'p',
               'peak')
    _INTS = ('n_a', 'n_b', 'peak')

    def __init__(self, contig, position, strand, ref_base, n_a, n_b, mean_a, mean_b, delta, t, df, p, peak, column,
                 contig_names=None):
        super().__init__(column, contig_names, **dict(zip(self._FIELDS, (
            contig, position, strand, ref_base, n_a, n_b, mean_a, mean_b, delta, t, df, p, peak))))


def local_peaks(score, contig, position, strand, reach):
    """Per row: no OTHER row of the same contig and strand within ``reach`` positions has a larger ``score`` (a NaN
    score is never a peak and outranks nothing).  Rows ascending in (contig, position, strand), at most one per
    (contig, position, strand)."""
    score = np.asarray(score, dtype=np.float64)
    peak = ~np.isnan(score)
    reach = int(reach)
    for s in (0, 1):
        rows = np.nonzero(np.asarray(strand) == s)[0]
        sc, c, p = np.where(np.isnan(score[rows]), -np.inf, score[rows]), contig[rows], position[rows]
        best = np.full(rows.size, -np.inf)
        # (positions of one strand and contig are distinct and ascending: a row within `reach` positions is within
        # `reach` rows)
        for j in range(1, min(reach, rows.size - 1) + 1):
            near = (c[j:] == c[:-j]) & (p[j:] - p[:-j] <= reach)
            best[j:] = np.maximum(best[j:], np.where(near, sc[:-j], -np.inf))
            best[:-j] = np.maximum(best[:-j], np.where(near, sc[j:], -np.inf))
        peak[rows] &= ~(best > sc)
    return peak


def compare_site_levels(a, b, column='level', min_coverage=5, reach=5):
    """Two-sample test per site between two ``SiteLevelBatch``es over the same reference (``a`` the control, ``b`` the
    sample, by convention), numpy on the host.  Rows: the (contig, position, strand) present in both with count >=
    ``min_coverage`` in each.  Welch's unequal-variance t test of ``column`` (one of ``SiteLevelBatch.COLUMNS``): with
    v = m2 / (n - 1), t = (mean_b - mean_a) / sqrt(va / na + vb / nb), df by Welch-Satterthwaite,
    p = 2 * scipy.special.stdtr(df, -|t|); all three NaN where a count is below 2 or the denominator is 0.  ``peak``:
    no other kept row of the same contig and strand within ``reach`` positions has a larger |t| (a changed base moves
    the levels of every k-mer that holds it, so its neighbours score too; reach = k - 1 = 5 for a 6-mer pore model).
    There is NO calibrated threshold and no default call: |t| depends on coverage, on the size of the level shift and
    on how well both samples aligned, and only synthetic levels have been scored with it; the events of one read are
    treated as independent of each other.  Different ``ref_len`` or ``contig_names``: ValueError.
    -> SiteComparison."""
    from scipy.special import stdtr
    _same_reference('compare_site_levels', a, b)
    j = check_site_test('compare_site_levels', column, min_coverage, reach)
    ka = _site_key(a.contig, a.position, a.strand, a.ref_len)
    kb = _site_key(b.contig, b.position, b.strand, b.ref_len)
    _, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    keep = (a.count[ia] >= min_coverage) & (b.count[ib] >= min_coverage)
    ia, ib = ia[keep], ib[keep]
    na, nb = a.count[ia].astype(np.int64), b.count[ib].astype(np.int64)
    mean_a, mean_b = a.mean[ia, j], b.mean[ib, j]
    delta = mean_b - mean_a
    with np.errstate(invalid='ignore', divide='ignore'):
        fa, fb = na.astype(np.float64), nb.astype(np.float64)
        vna, vnb = a.m2[ia, j] / (fa - 1.0) / fa, b.m2[ib, j] / (fb - 1.0) / fb
        denom = np.sqrt(vna + vnb)
        ok = (na >= 2) & (nb >= 2) & (denom > 0)
        t = np.where(ok, delta / denom, np.nan)
        df = np.where(ok, (vna + vnb) ** 2 / (vna ** 2 / (fa - 1.0) + vnb ** 2 / (fb - 1.0)), np.nan)
        p = np.where(ok, 2.0 * stdtr(np.where(ok, df, 1.0), -np.abs(np.where(ok, t, 0.0))), np.nan)
    contig, position, strand = a.contig[ia], a.position[ia], a.strand[ia]
    peak = local_peaks(np.abs(t), contig, position, strand, reach)
    return SiteComparison(contig, position, strand, a.ref_base[ia], na, nb, mean_a, mean_b, delta, t, df, p, peak,
                          column, a.contig_names)
