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
import sys

import numpy as np

from . import defaults
from .site_levels import local_peaks
from .site_tests import SiteTable, copy_back, host_table_tests, resident_tests, upload_rows

_THIS = sys.modules[__name__]        # what the shared layer takes as ``op``


class SiteRankComparison(SiteTable):
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

    _FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'ks', 'ks_plus', 'ks_minus', 'ks_p',
               'ks_exact', 'u', 'auc', 'mw_z', 'mw_p', 'ks_peak', 'mw_peak')
    _INTS = ('n_a', 'n_b', 'ks_exact', 'ks_peak', 'mw_peak')


def _check(what, exact_cells):
    if int(exact_cells) != exact_cells or exact_cells < 0:
        raise ValueError('%s: exact_cells %r is not an integer >= 0' % (what, exact_cells))
    return (int(exact_cells),)


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
    from .device import site_rank_tests_dev
    return copy_back(site_rank_tests_dev(context, key_a, val_a, key_b, val_b, min_coverage, exact_cells))


def _upload_and_test(key_a, val_a, key_b, val_b, min_coverage, exact_cells):
    """Host rows (key int64, one f64 column) of the two samples to the default context's GPU, then ``_on_device``."""
    return _on_device(*upload_rows(key_a, val_a, key_b, val_b), min_coverage, exact_cells)


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
    return host_table_tests(_THIS, 'compare_site_ranks', a, b, column, min_coverage, reach, exact_cells)


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
    return resident_tests(_THIS, 'site_rank_tests_batch', read_batch_a, read_batch_b, aligner, kmer_model, config,
                          renorm_rounds, trim, column, min_coverage, reach, exact_cells)
