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
import numpy as np

from . import defaults
from .site_levels import SiteLevelBatch, _open, _same_reference, _site_key, local_peaks
from .site_ranks import _event_column, _sample_rows

_FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'fitted', 'mean_0', 'sd_0', 'mean_1', 'sd_1',
           'rate_a', 'rate_b', 'delta_rate', 'll_one', 'll_shared', 'll_free', 'lrt', 'z', 'p', 'peak')
N_COUNTS, N_FIT = 5, 17


class SiteMixtureComparison:
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

    def __init__(self, column, contig_names=None, steps_shared=None, steps_free=None, **rows):
        for f in _FIELDS:
            setattr(self, f, rows[f])
        self.column, self.contig_names = column, contig_names
        self.steps_shared, self.steps_free = steps_shared, steps_free

    def __len__(self):
        return int(self.position.size)

    def write_tsv(self, file):
        """Header, then one tab-separated row per site: contig, position, strand (+ / -), ref, n_a, n_b, fitted
        (0 / 1), mean_0, sd_0, mean_1, sd_1, rate_a, rate_b, delta_rate, ll_one, ll_shared, ll_free, lrt, z, p (floats
        as ``repr`` gives them), peak (0 / 1), to ``file``, a path or a text file."""
        out = _open(file)
        label = (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])
        floats = _FIELDS[7:20]
        try:
            out.write('contig\tposition\tstrand\tref\tn_a\tn_b\tfitted\t' + '\t'.join(floats) + '\tpeak\n')
            out.writelines('%s\t%d\t%s\t%s\t%d\t%d\t%d\t%s\t%d\n'
                           % (label(int(self.contig[i])), self.position[i], '+-'[self.strand[i]],
                              'ACGT'[self.ref_base[i]], self.n_a[i], self.n_b[i], self.fitted[i],
                              '\t'.join(repr(float(getattr(self, f)[i])) for f in floats), self.peak[i])
                           for i in range(len(self)))
        finally:
            if out is not file:
                out.close()


def _check(what, column, min_coverage, reach, iterations, min_sd_ratio):
    j = SiteLevelBatch.column_index(column)
    if int(min_coverage) != min_coverage or min_coverage < 1:
        raise ValueError('%s: min_coverage %r is not an integer >= 1' % (what, min_coverage))
    if int(reach) != reach or reach < 0:
        raise ValueError('%s: reach %r is not an integer >= 0' % (what, reach))
    if int(iterations) != iterations or not 1 <= iterations <= 1024:
        raise ValueError('%s: iterations %r is not an integer in 1 .. 1024' % (what, iterations))
    if not 0.0 < min_sd_ratio <= 1.0:
        raise ValueError('%s: min_sd_ratio %r is not in (0, 1]' % (what, min_sd_ratio))
    return j


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
                       np.zeros((0, N_COUNTS), dtype=np.int64), np.zeros((0, N_FIT)))


def _on_device(context, key_a, val_a, key_b, val_b, min_coverage, iterations, min_sd_ratio):
    """One ``device.site_mixture_tests_dev`` call over device tensors and one copy back: -> (site_key int64 (sites,),
    counts int64 (sites, 5), fit f64 (sites, 17)) numpy arrays (the floats cross as their bits beside the integers:
    184 B per site)."""
    import torch
    from .device import site_mixture_tests_dev, to_host
    site_key, counts, fit = site_mixture_tests_dev(context, key_a, val_a, key_b, val_b, min_coverage, iterations,
                                                   min_sd_ratio)
    n = int(site_key.numel())
    flat = to_host(torch.cat([site_key, counts.reshape(-1), fit.reshape(-1).view(torch.int64)]))
    return (np.ascontiguousarray(flat[:n]), np.ascontiguousarray(flat[n:n + N_COUNTS * n]).reshape(n, N_COUNTS),
            np.ascontiguousarray(flat[n + N_COUNTS * n:]).view(np.float64).reshape(n, N_FIT))


def _upload_and_test(key_a, val_a, key_b, val_b, min_coverage, iterations, min_sd_ratio):
    """Host rows (key int64, one f64 column) of the two samples to the default context's GPU, then ``_on_device``."""
    import torch
    from . import _lib
    context = _lib.default_context()
    dev = torch.device('cuda', context.device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    return _on_device(context, up(key_a, np.int64), up(val_a, np.float64), up(key_b, np.int64), up(val_b, np.float64),
                      min_coverage, iterations, min_sd_ratio)


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
    what = 'compare_site_mixtures'
    for x in (a, b):
        if x.events is None:
            raise ValueError('%s: a batch carries no event table (site_levels_batch(rows=True))' % what)
    _same_reference(what, a, b)
    _check(what, column, min_coverage, reach, iterations, min_sd_ratio)
    if a.events['read'].size == 0 or b.events['read'].size == 0:
        return _empty(column, a.contig_names)
    key = lambda x: _site_key(x.events['contig'], x.events['position'], x.events['strand'], x.ref_len)
    site_key, counts, fit = _upload_and_test(key(a), _event_column(a, column), key(b), _event_column(b, column),
                                             int(min_coverage), int(iterations), float(min_sd_ratio))
    L = max(a.ref_len, 1)
    contig, position, strand = ((site_key >> 1) // L).astype(np.int32), (site_key >> 1) % L, \
        (site_key & 1).astype(np.int8)
    rows_key = _site_key(a.contig, a.position, a.strand, a.ref_len)
    order = np.argsort(rows_key, kind='stable')
    at = np.minimum(np.searchsorted(rows_key[order], site_key), max(rows_key.size - 1, 0))
    if site_key.size and (rows_key.size == 0 or not np.array_equal(rows_key[order][at], site_key)):
        raise ValueError('%s: the event table of the first batch holds sites that its rows do not' % what)
    ref_base = a.ref_base[order][at].astype(np.int8) if site_key.size else np.zeros(0, dtype=np.int8)
    return _comparison(column, a.contig_names, contig, position.astype(np.int64), strand, ref_base, int(reach), counts,
                       fit)


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
    what = 'site_mixture_tests_batch'
    if int(trim) != trim or trim < 0:
        raise ValueError('%s: trim %r is not an integer >= 0' % (what, trim))
    j = _check(what, column, min_coverage, reach, iterations, min_sd_ratio)
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
    site_key, counts, fit = _on_device(kmer_model.context, key_a, val_a, key_b, val_b, int(min_coverage),
                                       int(iterations), float(min_sd_ratio))
    position = site_key >> 1
    contig = np.zeros(position.size, dtype=np.int32)
    if refset is not None:
        c, position = refset.locate(position)
        contig = c.astype(np.int32)
    return _comparison(column, names, contig, position.astype(np.int64), (site_key & 1).astype(np.int8),
                       reference_num[site_key >> 1].astype(np.int8), int(reach), counts, fit)
