"""``compare_site_ranks`` and ``site_rank_tests_batch`` — per-site rank tests between two samples: the two-sample
Kolmogorov-Smirnov test and the Mann-Whitney U test on the pile-ups of one event column per reference position and
strand (what nanocompore and Tombo's sample compare offer beside a test of the means).

``compare_site_levels`` tests the means from moments; a rank test needs the rows.  Its p-value holds under the null
hypothesis whatever the distribution of the levels, and it sees a change of shape (a part-modified site is bimodal)
that a difference of means dilutes.  The device part is one kernel over the listed sites (contract: include/nadavca_hip.h,
nvk_site_rank_tests_dev; csrc/kernels_siteranks.hip): per site the exact integers of both statistics and the exact
two-sided KS p-value by the lattice-path recurrence, which the asymptotic formula cannot replace at sequencing coverage
(n = m = 5 with D = 1 gives p = 0 there, 2 / 252 exactly).  Dropping, sorting and listing the sites is torch on the
device (``device.site_rank_tests_dev``); the p-values of the Mann-Whitney statistic, the asymptotic KS p-value of the
sites too large for the exact one, and the peaks are numpy and scipy on the host.  Single process only."""
import numpy as np

from . import defaults
from .site_levels import SiteLevelBatch, _open, _same_reference, _site_key, local_peaks

_FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'ks', 'ks_plus', 'ks_minus', 'ks_p', 'ks_exact',
           'u', 'auc', 'mw_z', 'mw_p', 'ks_peak', 'mw_peak')


class SiteRankComparison:
    """What ``compare_site_ranks`` and ``site_rank_tests_batch`` return.  Row arrays, one row per (contig, position,
    strand) with at least ``min_coverage`` events in both samples, ascending in (contig, position, strand):
    ``contig``, ``position``, ``strand``, ``ref_base``, ``n_a``, ``n_b``;
    ``ks`` = max(``ks_plus``, ``ks_minus``): the two-sided and the two one-sided Kolmogorov-Smirnov statistics
    (``ks_plus``: how far A's empirical distribution function rises above B's, scipy's alternative='greater');
    ``ks_p``: its two-sided p-value, exact (ties ignored, as scipy's method='exact') where ``ks_exact``, else
    ``scipy.stats.kstwo.sf(ks, round(n m / (n + m)))`` (scipy's method='asymp');
    ``u``: the Mann-Whitney U of A (the number of pairs with a > b, ties counting half); ``auc`` = 1 - u / (n m): the
    chance that a level of B exceeds one of A; ``mw_z`` and ``mw_p``: the normal approximation with tie and continuity
    corrections, two-sided (scipy's method='asymptotic'), NaN where every value of the site is the same;
    ``ks_peak`` / ``mw_peak``: no other row of the same contig and strand within ``reach`` positions has a larger
    -log ks_p / |mw_z|.  ``column``: what was compared; ``contig_names`` as the batches'."""

    def __init__(self, column, contig_names=None, **rows):
        for f in _FIELDS:
            setattr(self, f, rows[f])
        self.column, self.contig_names = column, contig_names

    def __len__(self):
        return int(self.position.size)

    def write_tsv(self, file):
        """Header, then one tab-separated row per site: contig, position, strand (+ / -), ref, n_a, n_b, ks, ks_plus,
        ks_minus, ks_p, ks_exact (0 / 1), u, auc, mw_z, mw_p (floats as ``repr`` gives them), ks_peak, mw_peak
        (0 / 1), to ``file``, a path or a text file."""
        out = _open(file)
        label = (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])
        try:
            out.write('contig\tposition\tstrand\tref\tn_a\tn_b\tks\tks_plus\tks_minus\tks_p\tks_exact\tu\tauc\tmw_z\t'
                      'mw_p\tks_peak\tmw_peak\n')
            out.writelines('%s\t%d\t%s\t%s\t%d\t%d\t%r\t%r\t%r\t%r\t%d\t%r\t%r\t%r\t%r\t%d\t%d\n'
                           % (label(int(self.contig[i])), self.position[i], '+-'[self.strand[i]],
                              'ACGT'[self.ref_base[i]], self.n_a[i], self.n_b[i], float(self.ks[i]),
                              float(self.ks_plus[i]), float(self.ks_minus[i]), float(self.ks_p[i]), self.ks_exact[i],
                              float(self.u[i]), float(self.auc[i]), float(self.mw_z[i]), float(self.mw_p[i]),
                              self.ks_peak[i], self.mw_peak[i]) for i in range(len(self)))
        finally:
            if out is not file:
                out.close()


def _check(what, column, min_coverage, reach, exact_cells):
    j = SiteLevelBatch.column_index(column)
    if int(min_coverage) != min_coverage or min_coverage < 1:
        raise ValueError('%s: min_coverage %r is not an integer >= 1' % (what, min_coverage))
    if int(reach) != reach or reach < 0:
        raise ValueError('%s: reach %r is not an integer >= 0' % (what, reach))
    if int(exact_cells) != exact_cells or exact_cells < 0:
        raise ValueError('%s: exact_cells %r is not an integer >= 0' % (what, exact_cells))
    return j


def _statistics(n_a, n_b, ks_plus, ks_minus, u2, tie, ks_p):
    """The host half: the kernel's integers and exact p-values as the float columns of a SiteRankComparison."""
    from scipy.special import ndtr
    from scipy.stats import kstwo
    n, m = n_a.astype(np.float64), n_b.astype(np.float64)
    nm, N = n * m, n + m
    exact = ~np.isnan(ks_p)
    ks = np.maximum(ks_plus, ks_minus) / nm
    p = ks_p.copy()
    if not exact.all():
        rest = ~exact
        p[rest] = np.clip(kstwo.sf(ks[rest], np.round(nm[rest] / N[rest])), 0.0, 1.0)
    u = u2 / 2.0
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.sqrt(nm / 12.0 * ((N + 1.0) - tie / (N * (N - 1.0))))
        d = nm / 2.0 - u
        ok = s > 0
        z = np.where(ok, np.sign(d) * np.maximum(np.abs(d) - 0.5, 0.0) / s, np.nan)
        mw_p = np.where(ok, np.minimum(1.0, 2.0 * ndtr(-(np.abs(d) - 0.5) / s)), np.nan)
    return dict(ks=ks, ks_plus=ks_plus / nm, ks_minus=ks_minus / nm, ks_p=p, ks_exact=exact, u=u, auc=1.0 - u / nm,
                mw_z=z, mw_p=mw_p)


def _comparison(column, contig_names, contig, position, strand, ref_base, reach, n_a, n_b, ks_plus, ks_minus, u2, tie,
                ks_p):
    rows = _statistics(n_a, n_b, ks_plus, ks_minus, u2, tie, ks_p)
    with np.errstate(divide='ignore'):
        rows['ks_peak'] = local_peaks(-np.log(rows['ks_p']), contig, position, strand, reach)
    rows['mw_peak'] = local_peaks(np.abs(rows['mw_z']), contig, position, strand, reach)
    return SiteRankComparison(column, contig_names, contig=contig, position=position, strand=strand,
                              ref_base=ref_base, n_a=n_a, n_b=n_b, **rows)


def _empty(column, contig_names):
    z = lambda dt: np.zeros(0, dtype=dt)
    return _comparison(column, contig_names, z(np.int32), z(np.int64), z(np.int8), z(np.int8), 0, z(np.int64),
                       z(np.int64), z(np.int64), z(np.int64), z(np.int64), z(np.int64), z(np.float64))


def _on_device(context, key_a, val_a, key_b, val_b, min_coverage, exact_cells):
    """One ``device.site_rank_tests_dev`` call over device tensors and one copy back: -> (site_key, n_a, n_b, ks_plus,
    ks_minus, u2, tie int64, ks_p f64) numpy arrays.  (ks_p crosses as its bits beside the integers: 64 B per site.)"""
    import torch
    from .device import site_rank_tests_dev, to_host
    out = site_rank_tests_dev(context, key_a, val_a, key_b, val_b, min_coverage, exact_cells)
    flat = to_host(torch.cat([t.view(torch.int64) for t in out]))
    table = flat.reshape(len(out), int(out[0].numel()))
    return tuple(np.ascontiguousarray(table[i]) for i in range(len(out) - 1)) + \
        (np.ascontiguousarray(table[-1]).view(np.float64),)


def _upload_and_test(key_a, val_a, key_b, val_b, min_coverage, exact_cells):
    """Host rows (key int64, one f64 column) of the two samples to the default context's GPU, then ``_on_device``."""
    import torch
    from . import _lib
    context = _lib.default_context()
    dev = torch.device('cuda', context.device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    return _on_device(context, up(key_a, np.int64), up(val_a, np.float64), up(key_b, np.int64), up(val_b, np.float64),
                      min_coverage, exact_cells)


def _event_column(batch, column):
    ev = batch.events
    if column == 'resid':
        return np.asarray(ev['level'], dtype=np.float64) - np.asarray(ev['expected'], dtype=np.float64)
    return np.asarray(ev[column], dtype=np.float64)


def compare_site_ranks(a, b, column='level', min_coverage=5, reach=5, exact_cells=16384):
    """Rank tests per site between two ``SiteLevelBatch``es made with ``rows=True`` over the same reference (``a`` the
    control, ``b`` the sample, by convention; either may come from ``SiteLevelBatch.load``: a control is summarised
    once).  The rows of ``column`` (one of ``SiteLevelBatch.COLUMNS``; resid = level - expected) of both event tables
    are uploaded, ONE ``device.site_rank_tests_dev`` call tests every (contig, position, strand) with at least
    ``min_coverage`` events in each sample, and one copy brings the integers back; the rest is numpy on the host.
    ``exact_cells``: the exact KS p-value is computed for a site of n and m events where min(n, m) <= 255 and
    n m <= exact_cells (the recurrence visits about n m cells), the asymptotic one elsewhere.  ``reach``: as for
    ``compare_site_levels``.
    There is NO default call: the p-values are per site and not corrected for the number of sites tested.  The exact KS
    p-value ignores ties (as scipy's): with many equal values, such as dwell times, it is conservative.  The
    Mann-Whitney p-value is a normal approximation, rough at n = 10 in the tails.  The events of one read are treated as
    independent of each other.  A batch without an event table, different ``ref_len`` or ``contig_names``, a column that
    is not one, min_coverage < 1, reach < 0 or exact_cells < 0: ValueError.  -> SiteRankComparison."""
    what = 'compare_site_ranks'
    for x in (a, b):
        if x.events is None:
            raise ValueError('%s: a batch carries no event table (site_levels_batch(rows=True))' % what)
    _same_reference(what, a, b)
    _check(what, column, min_coverage, reach, exact_cells)
    if a.events['read'].size == 0 or b.events['read'].size == 0:
        return _empty(column, a.contig_names)
    key = lambda x: _site_key(x.events['contig'], x.events['position'], x.events['strand'], x.ref_len)
    site_key, *stats = _upload_and_test(key(a), _event_column(a, column), key(b), _event_column(b, column),
                                        int(min_coverage), int(exact_cells))
    L = max(a.ref_len, 1)
    contig, position, strand = ((site_key >> 1) // L).astype(np.int32), (site_key >> 1) % L, \
        (site_key & 1).astype(np.int8)
    rows_key = _site_key(a.contig, a.position, a.strand, a.ref_len)
    order = np.argsort(rows_key, kind='stable')
    at = np.minimum(np.searchsorted(rows_key[order], site_key), max(rows_key.size - 1, 0))
    if site_key.size and (rows_key.size == 0 or not np.array_equal(rows_key[order][at], site_key)):
        raise ValueError('%s: the event table of the first batch holds sites that its rows do not' % what)
    ref_base = a.ref_base[order][at].astype(np.int8) if site_key.size else np.zeros(0, dtype=np.int8)
    return _comparison(column, a.contig_names, contig, position.astype(np.int64), strand, ref_base, int(reach), *stats)


def _sample_rows(read_batch, aligner, kmer_model, config, renorm_rounds, trim, j):
    """The front end of ``site_levels_batch`` for one sample, keeping 16 B per base on the device: -> (key int64, one
    f64 column, the alignment stage): device tensors, None twice where nothing aligned."""
    import torch
    from .batchflow import align_batch
    from .device import expected_levels_dev, site_level_rows_dev
    res = align_batch(read_batch, config, kmer_model, renorm_rounds, aligner)
    stage = res.stage
    L = np.asarray(aligner.reference_num).size
    if stage.n_live == 0 or L == 0:
        return None, None, stage
    sa, dbatch = stage.sa, stage.dbatch
    expected = expected_levels_dev(dbatch, kmer_model, with_contexts=True)
    key, val = site_level_rows_dev(kmer_model.context, dbatch, res.events, expected, sa.ref_start.contiguous(),
                                   sa.reverse.to(torch.int32), res.status, int(trim), L)
    return key, val[:, j].contiguous(), stage


def site_rank_tests_batch(read_batch_a, read_batch_b, aligner, kmer_model=defaults.KMER_MODEL_FILE,
                          config=defaults.CONFIG_FILE, renorm_rounds=defaults.RENORM_ROUNDS, trim=5, column='level',
                          min_coverage=5, reach=5, exact_cells=16384):
    """``compare_site_ranks`` of two ReadBatches without the event tables ever leaving the device.  Per sample the
    front end of ``site_levels_batch`` (``batchflow.align_batch``, the expected levels, ``device.site_level_rows_dev``),
    of which only the key and ``column`` stay, 16 B per base; then ONE ``device.site_rank_tests_dev`` call over both
    samples and one copy of the tested sites.  ``aligner``: a batch aligner that serves both samples, or a pair of
    aligners over the SAME reference, one per sample (different ``reference_num``: ValueError); with one over a
    ``refset.ReferenceSet`` the rows are contig-local and named, as ``site_levels_batch``'s.  ``trim``: as there.  The
    rows equal those of ``compare_site_ranks(site_levels_batch(a, rows=True), site_levels_batch(b, rows=True))``; what
    its docstring says about calls, ties, the normal approximation and independence holds here too.
    -> SiteRankComparison."""
    what = 'site_rank_tests_batch'
    if int(trim) != trim or trim < 0:
        raise ValueError('%s: trim %r is not an integer >= 0' % (what, trim))
    j = _check(what, column, min_coverage, reach, exact_cells)
    from .batchflow import load_config, load_kmer_model
    from .refset import ReferenceSet
    aligner_a, aligner_b = aligner if isinstance(aligner, (tuple, list)) and len(aligner) == 2 else (aligner, aligner)
    reference_num = np.ascontiguousarray(aligner_a.reference_num, dtype=np.int32).reshape(-1)
    if aligner_b is not aligner_a and not np.array_equal(reference_num, np.asarray(aligner_b.reference_num).reshape(-1)):
        raise ValueError('%s: the two aligners are over different references' % what)
    kmer_model, config = load_kmer_model(kmer_model), load_config(config)
    key_a, val_a, stage_a = _sample_rows(read_batch_a, aligner_a, kmer_model, config, renorm_rounds, trim, j)
    key_b, val_b, stage = _sample_rows(read_batch_b, aligner_b, kmer_model, config, renorm_rounds, trim, j)
    names = stage.contig_names()
    if stage_a.contig_names() != names:
        raise ValueError('%s: the two aligners are over different references (contig names %r / %r)'
                         % (what, stage_a.contig_names(), names))
    del stage_a
    if key_a is None or key_b is None:
        return _empty(column, names)
    refset = stage.reference if isinstance(stage.reference, ReferenceSet) else None
    del stage
    site_key, *stats = _on_device(kmer_model.context, key_a, val_a, key_b, val_b, int(min_coverage), int(exact_cells))
    position = site_key >> 1
    contig = np.zeros(position.size, dtype=np.int32)
    if refset is not None:
        c, position = refset.locate(position)
        contig = c.astype(np.int32)
    return _comparison(column, names, contig, position.astype(np.int64), (site_key & 1).astype(np.int8),
                       reference_num[site_key >> 1].astype(np.int8), int(reach), *stats)
