"""``compare_site_mixtures`` and ``site_mixture_tests_batch`` — per-site stoichiometry between two samples: a
two-component Gaussian mixture over the pooled pile-ups of one event column per reference position and strand, the two
components shared by the samples and one mixing weight per sample (what xPore and nanocompore's GMM mode fit when they
compare a native sample with a control at signal level).

``compare_site_levels`` and ``compare_site_ranks`` say whether the two pile-ups differ; this says WHAT SHARE of the
reads sits in the second component in each sample.  The device part is one kernel over the listed sites (contract:
include/nadavca_hip.h, nvk_site_mixture_tests_dev; csrc/kernels_sitemix.hip): EM with one weight for all rows, which
never sees the labels, then from its solution EM with one weight per sample.  Dropping, sorting and listing the sites
is torch on the device (``device.site_mixture_tests_dev``); the component labels, the test and the peaks are numpy and
scipy on the host.  Single process only.

The test is a permutation score test.  The responsibilities r of the label-free fit are fixed scores; if the labels are
exchangeable (the null hypothesis), the sum of r over sample B has mean n_b rbar and variance n_a n_b Q / (N (N - 1)),
Q = sum (r - rbar)^2: ``z`` is the standardised sum and ``p`` = 2 ndtr(-|z|).  It is valid whatever the fit looks
like.  NO p-value is offered for ``lrt`` = 2 (ll_free - ll_shared): under a one-component null the mixture's
likelihood ratio does not follow chi^2_1.  Measured with the numpy restatement (tests/site_mixtures_ref.py, both
samples N(0, 0.35^2), 3 000 sites per coverage, iterations 32): the chi^2_1 p-value of ``lrt`` is below 0.01 on 0.035
to 0.062 of the null sites, 3 to 6 times the nominal level, where the score test gives p <= 0.01 on 0.0077 to 0.0083
of them at 10, 20 and 40 events per sample (p <= 0.05 on 0.045 to 0.055, p <= 0.001 on at most 0.0007)."""
import sys

import numpy as np

from . import defaults
from .device import SITE_MIX_COUNTS, SITE_MIX_FIT
from .site_levels import local_peaks
from .site_tests import SiteTable, copy_back, host_table_tests, resident_tests, upload_rows

_THIS = sys.modules[__name__]        # what the shared layer takes as ``op``


class SiteMixtureComparison(SiteTable):
    """What ``compare_site_mixtures`` and ``site_mixture_tests_batch`` return.  Row arrays, one row per (contig,
    position, strand) with at least ``min_coverage`` finite events in both samples, ascending in (contig, position,
    strand): ``contig``, ``position``, ``strand``, ``ref_base``, ``n_a``, ``n_b``;
    ``fitted``: the site has a spread and values on both sides of its mean; elsewhere every float but the three
    log-likelihoods (all equal to ``ll_one``) is NaN;
    ``mean_0``, ``sd_0``, ``mean_1``, ``sd_1``: the two components of the fit with one weight per sample, component 0
    being the one that holds most of the control ``a``; ``rate_a``, ``rate_b``: the share of component 1 in each sample
    (``rate_a`` <= 0.5), ``delta_rate`` = rate_b - rate_a;
    ``ll_one``, ``ll_shared``, ``ll_free``: the log-likelihoods of one Gaussian, of the mixture with one weight and of
    the mixture with two; ``lrt`` = 2 (ll_free - ll_shared), a statistic without a p-value (see the module);
    ``z``, ``p``: the permutation score test of the label-free fit's responsibilities, two-sided normal approximation;
    z > 0: sample B holds more of component 1; NaN where the responsibilities are all the same;
    ``peak``: no other row of the same contig and strand within ``reach`` positions has a larger |z|.
    ``steps_shared``, ``steps_free``: the EM steps run.  ``column``: what was compared; ``contig_names`` as the
    batches'."""

    _FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'fitted', 'mean_0', 'sd_0', 'mean_1', 'sd_1',
               'rate_a', 'rate_b', 'delta_rate', 'll_one', 'll_shared', 'll_free', 'lrt', 'z', 'p', 'peak')
    _INTS = ('n_a', 'n_b', 'fitted', 'peak')

    def __init__(self, column, contig_names=None, steps_shared=None, steps_free=None, **rows):
        super().__init__(column, contig_names, **rows)
        self.steps_shared, self.steps_free = steps_shared, steps_free


def _check(what, iterations, min_sd_ratio):
    if int(iterations) != iterations or not 1 <= iterations <= 1024:
        raise ValueError('%s: iterations %r is not an integer in 1 .. 1024' % (what, iterations))
    if not 0.0 < min_sd_ratio <= 1.0:
        raise ValueError('%s: min_sd_ratio %r is not in (0, 1]' % (what, min_sd_ratio))
    return int(iterations), float(min_sd_ratio)


def _statistics(counts, fit):
    """The host half: the kernel's two tables (sites, 5) and (sites, 17) as the columns of a SiteMixtureComparison."""
    from scipy.special import ndtr
    n_a, n_b, fitted = counts[:, 0].copy(), counts[:, 1].copy(), counts[:, 2] != 0
    n, m = n_a.astype(np.float64), n_b.astype(np.float64)
    N = n + m
    ra, rb, q = fit[:, 7], fit[:, 8], fit[:, 9]
    wa, wb = fit[:, 14], fit[:, 15]
    swap = wa > 0.5                                    # component 0 holds most of the control
    pick = lambda x, y: np.where(swap, y, x)
    with np.errstate(invalid='ignore', divide='ignore'):
        var = n * m * q / (N * (N - 1.0))
        z = np.where(var > 0, (rb - m * ((ra + rb) / N)) / np.sqrt(var), np.nan)
        z = np.where(swap, -z, z)
        p = 2.0 * ndtr(-np.abs(z))
        lrt = 2.0 * (fit[:, 16] - fit[:, 6])
    rate_a, rate_b = pick(wa, 1.0 - wa), pick(wb, 1.0 - wb)
    return dict(n_a=n_a, n_b=n_b, fitted=fitted, mean_0=pick(fit[:, 10], fit[:, 12]), sd_0=pick(fit[:, 11], fit[:, 13]),
                mean_1=pick(fit[:, 12], fit[:, 10]), sd_1=pick(fit[:, 13], fit[:, 11]), rate_a=rate_a, rate_b=rate_b,
                delta_rate=rate_b - rate_a, ll_one=fit[:, 0].copy(), ll_shared=fit[:, 6].copy(),
                ll_free=fit[:, 16].copy(), lrt=lrt, z=z, p=p,
                steps_shared=counts[:, 3].copy(), steps_free=counts[:, 4].copy())


def _comparison(column, contig_names, contig, position, strand, ref_base, reach, counts, fit):
    rows = _statistics(counts, fit)
    rows['peak'] = local_peaks(np.abs(rows['z']), contig, position, strand, reach)
    return SiteMixtureComparison(column, contig_names, contig=contig, position=position, strand=strand,
                                 ref_base=ref_base, **rows)


def _empty(column, contig_names):
    z = lambda dt: np.zeros(0, dtype=dt)
    return _comparison(column, contig_names, z(np.int32), z(np.int64), z(np.int8), z(np.int8), 0,
                       np.zeros((0, SITE_MIX_COUNTS), dtype=np.int64), np.zeros((0, SITE_MIX_FIT)))


def _on_device(context, key_a, val_a, key_b, val_b, min_coverage, iterations, min_sd_ratio):
    """One ``device.site_mixture_tests_dev`` call over device tensors and one copy back: -> (site_key int64 (sites,),
    counts int64 (sites, 5), fit f64 (sites, 17)) numpy arrays (the floats cross as their bits beside the integers:
    184 B per site)."""
    from .device import site_mixture_tests_dev
    return copy_back(site_mixture_tests_dev(context, key_a, val_a, key_b, val_b, min_coverage, iterations,
                                            min_sd_ratio))


def _upload_and_test(key_a, val_a, key_b, val_b, min_coverage, iterations, min_sd_ratio):
    """Host rows (key int64, one f64 column) of the two samples to the default context's GPU, then ``_on_device``."""
    return _on_device(*upload_rows(key_a, val_a, key_b, val_b), min_coverage, iterations, min_sd_ratio)


def compare_site_mixtures(a, b, column='level', min_coverage=5, reach=5, iterations=32, min_sd_ratio=0.1):
    """Mixture fits per site between two ``SiteLevelBatch``es made with ``rows=True`` over the same reference (``a`` the
    control, ``b`` the sample; either may come from ``SiteLevelBatch.load``).  The rows of ``column`` (one of
    ``SiteLevelBatch.COLUMNS``; resid = level - expected) of both event tables are uploaded, ONE
    ``device.site_mixture_tests_dev`` call fits every (contig, position, strand) with at least ``min_coverage`` finite
    events in each sample, and one copy brings the two tables back; labels, test and peaks are numpy on the host.
    ``iterations``: EM steps per stage (1 .. 1024); ``min_sd_ratio``: a component's standard deviation is kept at or
    above this share of the site's own (in (0, 1]).  Both are regularisation defaults, not calibrated values; 64
    iterations gave the same calibration and recovery figures as 32.  ``reach``: as for ``compare_site_levels``.
    There is NO default call: ``p`` is per site and not corrected for the number of sites tested, and it is a normal
    approximation, rough in the tails at n = 10.  ``lrt`` has no p-value (see the module).  The events of one read are
    treated as independent of each other.  Stoichiometry needs coverage: with half of B shifted by 4.3 standard
    deviations, 40 events per sample give p <= 1e-3 on 0.99 of the sites, 10 give p <= 1e-2 on about a third.  A batch
    without an event table, different ``ref_len`` or ``contig_names``, a column that is not one, min_coverage < 1,
    reach < 0, iterations or min_sd_ratio outside their ranges: ValueError.  -> SiteMixtureComparison."""
    return host_table_tests(_THIS, 'compare_site_mixtures', a, b, column, min_coverage, reach, iterations,
                            min_sd_ratio)


def site_mixture_tests_batch(read_batch_a, read_batch_b, aligner, kmer_model=defaults.KMER_MODEL_FILE,
                             config=defaults.CONFIG_FILE, renorm_rounds=defaults.RENORM_ROUNDS, trim=5, column='level',
                             min_coverage=5, reach=5, iterations=32, min_sd_ratio=0.1):
    """``compare_site_mixtures`` of two ReadBatches without the event tables ever leaving the device.  Per sample the
    front end of ``site_levels_batch`` as ``site_rank_tests_batch`` runs it (16 B per base stay on the device); then
    ONE ``device.site_mixture_tests_dev`` call over both samples and one copy of the tested sites.  ``aligner``: a
    batch aligner that serves both samples, or a pair of aligners over the SAME reference, one per sample (different
    ``reference_num``: ValueError); with one over a ``refset.ReferenceSet`` the rows are contig-local and named.
    ``trim``: as for ``site_levels_batch``.  The rows equal those of ``compare_site_mixtures(site_levels_batch(a,
    rows=True), site_levels_batch(b, rows=True))``; what its docstring says about calls, the normal approximation,
    ``lrt``, coverage and independence holds here too.  -> SiteMixtureComparison."""
    return resident_tests(_THIS, 'site_mixture_tests_batch', read_batch_a, read_batch_b, aligner, kmer_model, config,
                          renorm_rounds, trim, column, min_coverage, reach, iterations, min_sd_ratio)
