"""CPU-only tests of ``compare_site_mixtures`` / ``site_mixture_tests_batch``: the numpy restatement of the kernel's
contract (tests/site_mixtures_ref.py) against scipy and against brute-force enumeration, EM's monotone likelihood, the
calibration of the score test under the null hypothesis and the recovery of a planted stoichiometry, the degenerate
pile-ups, and the package's host half (labels, test, TSV, guards) with the restatement in place of the device call."""
import io
import itertools
import os

import numpy as np
import pytest

import site_mixtures_ref as ref
from test_site_ranks_cpu import hand_made

F = {name: i for i, name in enumerate(ref.FIT_NAMES)}


def test_one_component_against_scipy():
    from scipy.stats import norm
    rng = np.random.default_rng(3)
    for n, m, centre in ((2, 2, 0.0), (7, 12, 1e3), (64, 64, -5.0), (70, 200, 0.3)):
        A, B = rng.normal(centre, 1.0, n), rng.normal(centre + 0.5, 2.0, m)
        counts, fit = ref.one_site(A, B)
        x = np.concatenate([A, B])
        want = norm.logpdf(x, x.mean(), x.std()).sum()
        assert counts[:3].tolist() == [n, m, 1]
        assert abs(fit[F['ll_one']] - want) <= 1e-9 * abs(want), (n, m)     # (the mean of 1e3 + N(0, 1) costs digits)
        # the mixture of the start already beats one component; EM only adds to that
        assert fit[F['ll_shared']] >= fit[F['ll_one']] and fit[F['ll_free']] >= fit[F['ll_one']]


def test_permutation_moments_against_every_label_assignment():
    """A site of N = 10 rows, n_b = 4: the label-free fit gives every assignment of the labels the same scores, so the
    sum of the scores over B, taken over all C(10, 4) = 210 assignments, has exactly the mean and variance the host
    half uses: n_b rbar and n_a n_b Q / (N (N - 1))."""
    from nadavca_amd.site_mixtures import _statistics
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.normal(0.0, 0.3, 6), rng.normal(1.2, 0.3, 4)])
    runs = []
    for b in itertools.combinations(range(10), 4):
        mask = np.zeros(10, dtype=bool)
        mask[list(b)] = True
        runs.append((np.sort(x[~mask]), np.sort(x[mask])))
    assert len(runs) == 210
    counts, fit = ref.fit_runs(runs, 32, 0.1)
    assert (counts[:, 2] == 1).all()
    # label-free: the same fit whatever the labels (the rows only change places in the sums)
    for f in ('mean0_shared', 'sd0_shared', 'mean1_shared', 'sd1_shared', 'w_shared', 'll_shared', 'q'):
        assert np.abs(fit[:, F[f]] - fit[0, F[f]]).max() <= 1e-12, f
    total = fit[:, F['ra']] + fit[:, F['rb']]
    assert np.abs(total - total[0]).max() <= 1e-12
    rb = fit[:, F['rb']]
    mean = 4.0 * (total[0] / 10.0)
    var = 6.0 * 4.0 * fit[0, F['q']] / (10.0 * 9.0)
    assert abs(rb.mean() - mean) <= 1e-12 and abs(((rb - mean) ** 2).mean() - var) <= 1e-12 and var > 0.1
    # the package's z is the standardised sum (sign: the label swap)
    rows = _statistics(counts, fit)
    sign = np.where(fit[:, F['wa']] > 0.5, -1.0, 1.0)
    assert np.abs(rows['z'] - sign * (rb - mean) / np.sqrt(var)).max() <= 1e-9


def test_likelihood_rises_step_by_step():
    """EM never lowers the likelihood of the model it fits: along stage 0, and along stage 1, which starts from stage
    0's solution, so that ll_free >= ll_shared.  The floor on the standard deviations is outside that argument: the
    steps whose parameters sit on it are left out.  Rounding: 1e-9 of the magnitude."""
    rng = np.random.default_rng(12)
    runs = []
    for t in range(400):
        n, m = int(rng.integers(5, 60)), int(rng.integers(5, 60))
        B = rng.normal(0.0, 0.35, m)
        B[rng.random(m) < 0.5 * (t % 2)] += 1.5
        runs.append((np.sort(rng.normal(0.0, 0.35, n)), np.sort(B)))
    trace = []
    counts, fit = ref.fit_sites(*ref.pack(runs), 32, 0.1, trace=trace)
    assert len(trace) == 64 and [t[0] for t in trace] == [0] * 32 + [1] * 32
    ll = np.stack([t[1] for t in trace] + [fit[:, F['ll_free']]])
    sd_min = 0.1 * np.array([np.concatenate(r).std() for r in runs]) * (1.0 + 1e-12)
    at_end = (fit[:, F['sd0']] <= sd_min) | (fit[:, F['sd1']] <= sd_min)
    free_of_floor = ~(np.stack([t[3] for t in trace]).any(axis=0) | at_end)
    assert free_of_floor.sum() >= 300
    step = ll[1:] - ll[:-1]
    slack = 1e-9 * (1.0 + np.abs(ll[:-1]))
    assert (step[:, free_of_floor] >= -slack[:, free_of_floor]).all()
    # stage 1 starts where stage 0 ended: its first likelihood is ll_shared
    assert np.abs(ll[32] - fit[:, F['ll_shared']]).max() <= 1e-9
    assert (fit[free_of_floor, F['ll_free']] >= fit[free_of_floor, F['ll_shared']] - slack[0, free_of_floor]).all()
    assert (counts[:, 3] == 32).all() and (counts[:, 4] == 32).all()


@pytest.mark.parametrize('coverage', [10, 20, 40])
def test_null_calibration(coverage):
    """Both samples N(0, 0.35^2), 3 000 seeded sites, iterations 32: the share of sites with p <= 0.01 is at most
    0.019 = 0.01 + 5 sqrt(0.01 0.99 / 3000), the nominal level and five binomial standard deviations.  Seen: 0.0080,
    0.0083, 0.0077 at 10, 20, 40 events per sample (p <= 0.05: 0.051, 0.055, 0.045; p <= 0.001: 0.0007, 0, 0.0007);
    the chi^2_1 p-value of lrt, which the package does not offer, is below 0.01 on 0.062, 0.049, 0.035 of them."""
    from scipy.stats import chi2
    from nadavca_amd.site_mixtures import _statistics
    rng = np.random.default_rng(1000 + coverage)
    runs = [(np.sort(rng.normal(0.0, 0.35, coverage)), np.sort(rng.normal(0.0, 0.35, coverage))) for _ in range(3000)]
    rows = _statistics(*ref.fit_runs(runs, 32, 0.1))
    p = rows['p']
    assert rows['fitted'].all() and not np.isnan(p).any()
    print('coverage %d: p <= 0.05 on %.4f, <= 0.01 on %.4f, <= 0.001 on %.4f; chi2 p of lrt <= 0.01 on %.4f'
          % (coverage, (p <= 0.05).mean(), (p <= 0.01).mean(), (p <= 0.001).mean(),
             (chi2.sf(rows['lrt'], 1) <= 0.01).mean()))
    assert (p <= 0.01).mean() <= 0.019


def test_planted_stoichiometry_is_recovered():
    """40 events per sample, noise 0.35, each event of B shifted by 1.5 (4.3 standard deviations) with chance 0.5;
    2 000 seeded sites.  The restatement gave: p <= 1e-3 on 0.990 of the sites; |delta_rate - the realised share of
    shifted events| has median 0.0138 and 90th percentile 0.0475.  Asserted at twice those: 0.0276 and 0.095."""
    from nadavca_amd.site_mixtures import _statistics
    rng = np.random.default_rng(77)
    runs, share = [], []
    for _ in range(2000):
        A, B = rng.normal(0.0, 0.35, 40), rng.normal(0.0, 0.35, 40)
        shifted = rng.random(40) < 0.5
        B[shifted] += 1.5
        runs.append((np.sort(A), np.sort(B)))
        share.append(shifted.mean())
    rows = _statistics(*ref.fit_runs(runs, 32, 0.1))
    err = np.abs(rows['delta_rate'] - np.array(share))
    print('p <= 1e-3 on %.3f of the sites; |delta_rate - share|: median %.4f, 90th percentile %.4f'
          % ((rows['p'] <= 1e-3).mean(), np.median(err), np.quantile(err, 0.9)))
    assert np.median(err) <= 0.0276 and np.quantile(err, 0.9) <= 0.095
    assert (rows['rate_a'] <= 0.5).all() and (rows['mean_1'] > rows['mean_0']).mean() > 0.99
    assert np.median(rows['z']) > 3.0


def test_degenerate_sites():
    from nadavca_amd.site_mixtures import _statistics
    # every value the same: no spread, not fitted; the one-component likelihood is unbounded
    counts, fit = ref.one_site(np.full(7, 2.5), np.full(9, 2.5))
    assert counts.tolist() == [7, 9, 0, 0, 0]
    others = [i for i in range(17) if i not in (F['ll_one'], F['ll_shared'], F['ll_free'])]
    assert fit[F['ll_one']] == np.inf == fit[F['ll_shared']] == fit[F['ll_free']] and np.isnan(fit[others]).all()
    rows = _statistics(counts[None], fit[None])
    assert not rows['fitted'][0] and np.isnan(rows['z'][0]) and np.isnan(rows['p'][0]) and np.isnan(rows['rate_b'][0])
    assert np.isnan(rows['lrt'][0]) or rows['lrt'][0] == 0.0
    # one-sided: the rounded mean is the largest value
    counts, fit = ref.one_site([1.0 - 2.0 ** -53], [1.0, 1.0, 1.0])
    assert counts.tolist() == [1, 3, 0, 0, 0] and np.isfinite(fit[F['ll_one']]) and np.isnan(fit[others]).all()
    assert fit[F['ll_shared']] == fit[F['ll_one']] == fit[F['ll_free']]
    # two distinct values, one per sample: both components sit on the floor, the weights reach 0 and 1
    counts, fit = ref.one_site(np.full(6, 1.0), np.full(4, 2.0))
    assert counts.tolist() == [6, 4, 1, 32, 32]
    assert fit[F['sd0']] == fit[F['sd1']] == 0.1 * np.sqrt(0.24) and (fit[F['mean0']], fit[F['mean1']]) == (1.0, 2.0)
    assert (fit[F['wa']], fit[F['wb']]) == (0.0, 1.0) and abs(fit[F['w_shared']] - 0.4) <= 1e-15
    rows = _statistics(counts[None], fit[None])
    assert rows['delta_rate'][0] == 1.0 and abs(rows['z'][0] - 3.0) <= 1e-9       # sqrt(N - 1): the largest |z| there is
    # two distinct values mixed over both samples
    counts, fit = ref.one_site([1.0, 1.0, 2.0], [1.0, 2.0, 2.0, 2.0])
    assert counts[2] == 1 and abs(fit[F['wa']] - 1 / 3) <= 1e-12 and abs(fit[F['wb']] - 0.75) <= 1e-12
    # a listed key that a sample lacks; the device layer drops keys < 0 and values that are not finite
    counts, fit = ref.mixture_tests([4, 4, 9], [1.0, 2.0, 0.5], [9, 9, 7], [0.1, 0.9, 1.0], [4, 7, 8, 9], 32, 0.1)
    assert counts.tolist() == [[2, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 2, 1, 32, 32]]
    assert np.isnan(fit[:3]).all() and np.isfinite(fit[3]).all()
    site = ref.device_layer(np.array([4, 4, -1, 4, 4, 9]), np.array([1.0, np.nan, 5.0, 2.0, np.inf, 1.0]),
                            np.array([4, 4, 4, 9, -3]), np.array([0.0, 3.0, -np.inf, 1.0, 1.0]), 2, 32, 0.1)
    assert site[0].tolist() == [4] and site[1][0, :3].tolist() == [2, 2, 1]


def test_component_0_is_the_controls():
    """Mirroring the values swaps the kernel's components (0 is the lower one at the start); the host half names them
    by the control, so rates, z and p stay and the means change sign."""
    from nadavca_amd.site_mixtures import _statistics
    rng = np.random.default_rng(31)
    runs = []
    for _ in range(50):
        B = rng.normal(0.0, 0.35, 30)
        B[rng.random(30) < 0.4] += 1.5
        runs.append((rng.normal(0.0, 0.35, 25), B))
    up = ref.fit_runs([(np.sort(a), np.sort(b)) for a, b in runs], 32, 0.1)
    down = ref.fit_runs([(np.sort(-a), np.sort(-b)) for a, b in runs], 32, 0.1)
    assert (up[1][:, F['wa']] < 0.5).all() and (down[1][:, F['wa']] > 0.5).all()
    x, y = _statistics(*up), _statistics(*down)
    for f in ('rate_a', 'rate_b', 'delta_rate', 'sd_0', 'sd_1', 'z', 'p', 'lrt'):
        assert np.allclose(x[f], y[f], rtol=1e-7, atol=1e-9), f
    assert np.allclose(x['mean_0'], -y['mean_0'], atol=1e-9) and np.allclose(x['mean_1'], -y['mean_1'], atol=1e-9)
    assert (x['rate_a'] <= 0.5).all() and (x['z'] > 0).all() and (x['mean_1'] > x['mean_0']).all()
    # the host half row by row
    for stats in (up, down):
        want = ref.host_columns(*stats)
        got = _statistics(*stats)
        for f, w in want.items():
            assert np.allclose(got[f], w, rtol=1e-13, atol=0, equal_nan=True), f


@pytest.fixture
def restated_device(monkeypatch):
    """``compare_site_mixtures`` with tests/site_mixtures_ref.py's device layer in place of the upload and the kernel."""
    from nadavca_amd import site_mixtures
    monkeypatch.setattr(site_mixtures, '_upload_and_test', ref.device_layer)


FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'fitted', 'mean_0', 'sd_0', 'mean_1', 'sd_1',
          'rate_a', 'rate_b', 'delta_rate', 'll_one', 'll_shared', 'll_free', 'lrt', 'z', 'p', 'peak')


def test_compare_site_mixtures_on_hand_made_batches(restated_device, tmp_path):
    from nadavca_amd import SiteLevelBatch, SiteMixtureComparison, compare_site_mixtures
    from nadavca_amd.site_levels import local_peaks
    (a, ref_codes), (b, _) = hand_made(11, 0.0), hand_made(12, 1.2)
    path = os.path.join(str(tmp_path), 'control.npz')
    a.save(path)
    loaded = SiteLevelBatch.load(path)
    for column, min_cov in (('level', 3), ('resid', 5), ('dwell', 4)):
        cmp = compare_site_mixtures(a, b, column=column, min_coverage=min_cov)
        assert isinstance(cmp, SiteMixtureComparison) and cmp.column == column
        assert cmp.contig_names == ['chrA', 'chrB']
        value = lambda x: x.events['level'] - x.events['expected'] if column == 'resid' else x.events[column]
        where, runs = [], []
        for c, p, s in sorted(set(zip(a.events['contig'].tolist(), a.events['position'].tolist(),
                                      a.events['strand'].tolist()))):
            sel = lambda x: (x.events['contig'] == c) & (x.events['position'] == p) & (x.events['strand'] == s)
            A, B = value(a)[sel(a)].astype(float), value(b)[sel(b)].astype(float)
            if A.size >= min_cov and B.size >= min_cov:
                where.append((c, p, s))
                runs.append((np.sort(A), np.sort(B)))
        assert len(runs) >= 8 and len(cmp) == len(runs)
        counts, fit = ref.fit_runs(runs, 32, 0.1)
        for f, w in zip(('contig', 'position', 'strand'), zip(*where)):
            assert np.array_equal(getattr(cmp, f), w), f
        assert cmp.contig.dtype == np.int32 and cmp.position.dtype == np.int64 and cmp.strand.dtype == np.int8
        assert np.array_equal(cmp.ref_base, ref_codes[cmp.contig * 20 + cmp.position])
        assert np.array_equal(cmp.n_a, counts[:, 0]) and np.array_equal(cmp.n_b, counts[:, 1])
        assert np.array_equal(cmp.fitted, counts[:, 2] != 0) and cmp.fitted.dtype == bool and cmp.fitted.all()
        assert np.array_equal(cmp.steps_shared, counts[:, 3]) and np.array_equal(cmp.steps_free, counts[:, 4])
        for f, w in ref.host_columns(counts, fit).items():
            assert np.allclose(getattr(cmp, f), w, rtol=1e-13, atol=0, equal_nan=True), f
        assert np.array_equal(cmp.lrt, 2.0 * (cmp.ll_free - cmp.ll_shared))
        assert np.array_equal(cmp.delta_rate, cmp.rate_b - cmp.rate_a) and (cmp.rate_a <= 0.5).all()
        assert np.array_equal(cmp.peak, local_peaks(np.abs(cmp.z), cmp.contig, cmp.position, cmp.strand, 5))
        again = compare_site_mixtures(loaded, b, column=column, min_coverage=min_cov)
        for f in FIELDS:
            assert np.array_equal(getattr(again, f), getattr(cmp, f), equal_nan=True), f
    cmp = compare_site_mixtures(a, b, min_coverage=3)
    shifted = (cmp.contig == 0) & (cmp.position == 5) | (cmp.contig == 1) & (cmp.position == 3)
    assert shifted.sum() == 3 and (cmp.delta_rate[shifted] > 0.7).all() and (cmp.z[shifted] > 2.0).all()
    assert compare_site_mixtures(a, b, min_coverage=3, reach=0).peak.all()
    fewer = compare_site_mixtures(a, b, min_coverage=3, iterations=2, min_sd_ratio=0.5)
    assert (fewer.steps_shared == 2).all() and not np.array_equal(fewer.ll_free, cmp.ll_free)
    assert np.array_equal(fewer.ll_one, cmp.ll_one)
    # the TSV
    buf = io.StringIO(newline='')
    cmp.write_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0].split('\t') == ['contig', 'position', 'strand', 'ref', 'n_a', 'n_b', 'fitted', 'mean_0', 'sd_0',
                                    'mean_1', 'sd_1', 'rate_a', 'rate_b', 'delta_rate', 'll_one', 'll_shared',
                                    'll_free', 'lrt', 'z', 'p', 'peak']
    i = len(cmp) - 1
    assert cmp.contig[i] == 1 and lines[i + 1] == 'chrB\t%d\t+\t%s\t%d\t%d\t1\t%s\t%d' % (
        cmp.position[i], 'ACGT'[cmp.ref_base[i]], cmp.n_a[i], cmp.n_b[i],
        '\t'.join(repr(float(getattr(cmp, f)[i])) for f in FIELDS[7:20]), cmp.peak[i])
    assert len(lines) == len(cmp) + 2 and lines[-1] == '' and lines[1].startswith('chrA\t2\t+\t')
    tsv = os.path.join(str(tmp_path), 'r.tsv')
    cmp.write_tsv(tsv)
    assert open(tsv).read() == buf.getvalue()


def test_guards_and_empty_batches():
    """Every ValueError comes before any device call, and so does the result for a batch without events."""
    from nadavca_amd import SiteLevelBatch, compare_site_mixtures, site_mixture_tests_batch
    a, _ = hand_made(11, 0.0)
    b, _ = hand_made(12, 1.0)
    no_table = SiteLevelBatch(a.contig, a.position, a.strand, a.ref_base, a.count, a.mean, a.m2, a.ref_len,
                              a.contig_names)
    other_len, _ = hand_made(12, 1.0)
    other_len.ref_len = 21
    other_names, _ = hand_made(12, 1.0)
    other_names.contig_names = ['chrA', 'chrC']
    for bad in (no_table, other_len, other_names):
        with pytest.raises(ValueError):
            compare_site_mixtures(a, bad)
        with pytest.raises(ValueError):
            compare_site_mixtures(bad, a)
    for kw in (dict(column='mean'), dict(min_coverage=0), dict(min_coverage=2.5), dict(reach=-1), dict(reach=1.5),
               dict(iterations=0), dict(iterations=1025), dict(iterations=2.5), dict(min_sd_ratio=0.0),
               dict(min_sd_ratio=1.5), dict(min_sd_ratio=float('nan'))):
        with pytest.raises(ValueError):
            compare_site_mixtures(a, b, **kw)
        with pytest.raises(ValueError):
            site_mixture_tests_batch(None, None, None, **kw)
    for trim in (-1, 2.5):
        with pytest.raises(ValueError):
            site_mixture_tests_batch(None, None, None, trim=trim)
    z = SiteLevelBatch.empty(20, ['chrA', 'chrB'], rows=True)
    for x, y in ((z, z), (a, z), (z, a)):
        cmp = compare_site_mixtures(x, y, column='dwell')
        assert len(cmp) == 0 and cmp.column == 'dwell' and cmp.contig_names == ['chrA', 'chrB']
        assert cmp.p.dtype == np.float64 and cmp.fitted.dtype == bool and cmp.peak.dtype == bool
        assert cmp.n_a.dtype == np.int64 and cmp.z.size == 0 and cmp.delta_rate.size == 0
        buf = io.StringIO(newline='')
        cmp.write_tsv(buf)
        assert buf.getvalue().count('\n') == 1


def test_new_entry_declared_bound_and_exported():
    from conftest import ROOT
    import nadavca_amd
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    lib = _lib.load()
    name = 'nvk_site_mixture_tests_dev'
    assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES[name][1]) == 13
    assert callable(device.site_mixture_tests_dev) and (device.SITE_MIX_COUNTS, device.SITE_MIX_FIT) == (5, 17)
    assert len(ref.FIT_NAMES) == 17
    for f in ('compare_site_mixtures', 'site_mixture_tests_batch', 'SiteMixtureComparison'):
        assert f in nadavca_amd.__all__ and hasattr(nadavca_amd, f)
