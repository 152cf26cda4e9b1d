"""CPU-only tests of ``compare_site_ranks`` / ``site_rank_tests_batch``: the numpy restatement of the kernel's contract
(tests/site_ranks_ref.py) and the package's host formulas against scipy, the edge pile-ups, ``compare_site_ranks`` on
hand-made batches with the restatement in place of the device call, the new entry of the C-ABI, and the planted-site
experiment through the CPU oracle."""
import io
import os
import warnings

import numpy as np
import pytest

import site_levels_ref
import site_ranks_ref


def random_pairs(count, seed):
    """Pairs of samples with n, m in 2 .. 70: continuous values, and integers 0 .. 5 (heavy ties) for every third."""
    rng = np.random.default_rng(seed)
    for t in range(count):
        n, m = int(rng.integers(2, 71)), int(rng.integers(2, 71))
        if t % 3 == 2:
            yield rng.integers(0, 6, n).astype(float), rng.integers(0, 6, m).astype(float), True
        else:
            shift = rng.choice([0.0, 0.5, 1.5])
            yield rng.normal(0.0, 1.0, n), rng.normal(shift, rng.choice([1.0, 2.0]), m), False


def test_restatement_and_host_formulas_against_scipy():
    """ks_p: all terms of the recurrence are positive, so its relative error is bounded by about 3 (n + m) 2^-53 =
    5e-14 at n + m = 140; scipy's own exact method has an error of the same kind: 1e-10 leaves room for both.
    The asymptotic p-value: the statistic h / (n m) and scipy's difference of two quotients may differ by the 1e-15
    allowed above, and p ~ 2 exp(-2 en D^2) moves by the relative 4 en D times that, at most 140e-15 with en = n m /
    (n + m) <= 35 and D <= 1: 1e-12; on top of that scipy's ``kstwo.sf`` itself jumps by up to 4e-12 relative between
    neighbouring doubles of its argument (seen at n, m = 42, 45), so the reference's own step at the statistic is
    allowed twice."""
    from scipy import stats
    from nadavca_amd.site_ranks import _statistics
    checked_exact = checked_mw = tied = 0
    worst_p = worst_mw = worst_asymp = 0.0
    for A, B, ties in random_pairs(330, 7):
        n, m = A.size, B.size
        na, nb, kp, km, u2, tie, p = site_ranks_ref.one_site(A, B, 70 * 70)
        assert (na, nb) == (n, m) and kp >= 0 and km >= 0 and not np.isnan(p)
        for got, alt in ((kp, 'greater'), (km, 'less'), (max(kp, km), 'two-sided')):
            want = stats.ks_2samp(A, B, alternative=alt, method='asymp').statistic
            assert abs(got / (n * m) - want) <= 1e-15, (alt, n, m)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            want_p = stats.ks_2samp(A, B, method='exact').pvalue
        if not caught:
            assert abs(p - want_p) <= 1e-10 * want_p, (n, m, p, want_p)
            worst_p = max(worst_p, abs(p - want_p) / want_p)
            checked_exact += 1
        assert u2 / 2.0 == stats.mannwhitneyu(A, B, method='asymptotic').statistic
        pooled_counts = np.unique(np.concatenate([A, B]), return_counts=True)[1]
        assert tie == int((pooled_counts ** 3 - pooled_counts).sum()) and (tie > 0) == bool((pooled_counts > 1).any())
        tied += tie > 0
        # the package's host half, for this one row, with the exact p-value and without it
        arr = lambda v, dt=np.int64: np.array([v], dtype=dt)
        rows = _statistics(arr(n), arr(m), arr(kp), arr(km), arr(u2), arr(tie), arr(p, np.float64))
        assert rows['ks_exact'][0] and rows['ks_p'][0] == p and rows['u'][0] == u2 / 2.0
        assert rows['ks'][0] == max(kp, km) / (n * m) and rows['auc'][0] == 1.0 - u2 / 2.0 / (n * m)
        ref = site_ranks_ref.host_columns(arr(n), arr(m), arr(kp), arr(km), arr(u2), arr(tie), arr(p, np.float64))
        s = np.sqrt(n * m / 12.0 * ((n + m + 1.0) - tie / ((n + m) * (n + m - 1.0))))
        if s > 0:
            want_mw = stats.mannwhitneyu(A, B, method='asymptotic', use_continuity=True).pvalue
            assert abs(rows['mw_p'][0] - want_mw) <= 1e-14, (n, m, rows['mw_p'][0], want_mw)
            assert abs(ref['mw_p'][0] - want_mw) <= 1e-14
            worst_mw = max(worst_mw, abs(rows['mw_p'][0] - want_mw))
            d = n * m / 2.0 - u2 / 2.0
            assert rows['mw_z'][0] == np.sign(d) * max(abs(d) - 0.5, 0.0) / s
            checked_mw += 1
        else:
            assert np.isnan(rows['mw_p'][0]) and np.isnan(rows['mw_z'][0])
        rows = _statistics(arr(n), arr(m), arr(kp), arr(km), arr(u2), arr(tie), arr(np.nan, np.float64))
        res = stats.ks_2samp(A, B, method='asymp')
        want_asymp = res.pvalue
        # (scipy's kstwo.sf is not smooth in the last bits of its argument: what one step of the statistic does to it)
        near = [stats.kstwo.sf(np.nextafter(res.statistic, side), np.round(n * m / (n + m))) for side in (0.0, 1.0)]
        tol_asymp = 1e-12 * want_asymp + 2.0 * max(abs(x - want_asymp) for x in near)
        worst_asymp = max(worst_asymp, abs(rows['ks_p'][0] - want_asymp) / max(want_asymp, 1e-300))
        assert not rows['ks_exact'][0] and abs(rows['ks_p'][0] - want_asymp) <= tol_asymp
        ref = site_ranks_ref.host_columns(arr(n), arr(m), arr(kp), arr(km), arr(u2), arr(tie), arr(np.nan, np.float64))
        assert abs(ref['ks_p'][0] - want_asymp) <= tol_asymp and not ref['ks_exact'][0]
    print('%d pairs against the exact method (largest relative difference %.2g), %d against Mann-Whitney (largest '
          'difference %.2g), %d with ties; asymptotic KS p: largest relative difference %.2g'
          % (checked_exact, worst_p, checked_mw, worst_mw, tied, worst_asymp))
    assert checked_exact >= 300 and checked_mw >= 300 and tied >= 100


def test_edge_pile_ups():
    from nadavca_amd.site_ranks import _statistics
    one = site_ranks_ref.one_site
    # all values equal
    n, m, kp, km, u2, tie, p = one(np.full(7, 2.5), np.full(9, 2.5), 1000)
    assert (kp, km, p, tie, u2) == (0, 0, 1.0, 16 ** 3 - 16, 7 * 9)
    arr = lambda v, dt=np.int64: np.array([v], dtype=dt)
    rows = _statistics(arr(n), arr(m), arr(kp), arr(km), arr(u2), arr(tie), arr(p, np.float64))
    assert np.isnan(rows['mw_z'][0]) and np.isnan(rows['mw_p'][0]) and rows['ks'][0] == 0.0 and rows['auc'][0] == 0.5
    # A wholly below B
    n, m, kp, km, u2, tie, p = one([1, 2, 3, 4, 5], [6, 7, 8, 9, 10], 25)
    assert (kp, km, u2, tie) == (25, 0, 0, 0) and p == 2.0 / 252.0
    rows = _statistics(arr(n), arr(m), arr(kp), arr(km), arr(u2), arr(tie), arr(p, np.float64))
    assert rows['ks'][0] == 1.0 and rows['u'][0] == 0.0 and rows['auc'][0] == 1.0 and rows['mw_z'][0] > 0
    n, m, kp, km, u2, tie, p = one([6, 7, 8, 9, 10], [1, 2, 3, 4, 5], 25)
    assert (kp, km, u2) == (0, 25, 50) and p == 2.0 / 252.0
    # +-inf and the two zeros
    n, m, kp, km, u2, tie, p = one([-np.inf, -0.0, 1.0, np.inf], [0.0, np.inf, np.inf], 12)
    assert (kp, km, u2, tie) == (5, 0, 0 + 1 + 2 + 4, (2 ** 3 - 2) + (3 ** 3 - 3))
    # a listed key with an empty run; exact_cells = 0
    key_a, val_a = np.array([4, 4, 4, 9]), np.array([1.0, 2.0, 3.0, 0.5])
    key_b, val_b = np.array([9, 9, 4, 4, 7]), np.array([0.1, 0.9, 2.5, 0.5, 1.0])
    out = site_ranks_ref.rank_tests(key_a, val_a, key_b, val_b, [4, 7, 8, 9], 100)
    assert out[0].tolist() == [3, 0, 0, 1] and out[1].tolist() == [2, 1, 0, 2]
    assert all(o[1:3].tolist() == [0, 0] for o in out[2:6]) and np.isnan(out[6]).tolist() == [False, True, True, False]
    assert out[2].tolist()[0] == 1 and out[3].tolist()[0] == 3             # key 4: A = 1 2 3, B = 0.5 2.5
    out0 = site_ranks_ref.rank_tests(key_a, val_a, key_b, val_b, [4, 7, 8, 9], 0)
    assert np.isnan(out0[6]).all() and all(np.array_equal(x, y) for x, y in zip(out[:6], out0[:6]))
    # the exact p-value is served up to min(n, m) = 255
    rng = np.random.default_rng(5)
    assert not np.isnan(one(rng.normal(size=255), rng.normal(size=3), 1 << 20)[6])
    assert not np.isnan(one(rng.normal(size=3), rng.normal(size=255), 1 << 20)[6])
    assert np.isnan(one(rng.normal(size=256), rng.normal(size=256), 1 << 20)[6])
    assert not np.isnan(one(rng.normal(size=256), rng.normal(size=3), 1 << 20)[6])   # (min is 3)
    assert np.isnan(one(rng.normal(size=20), rng.normal(size=20), 399)[6])
    assert not np.isnan(one(rng.normal(size=20), rng.normal(size=20), 400)[6])
    # the device layer drops keys < 0 and NaN values, and lists the keys with the coverage in both
    site = site_ranks_ref.device_layer(np.array([4, 4, -1, 4, 9]), np.array([1.0, np.nan, 5.0, 2.0, 1.0]),
                                       np.array([4, 4, 9, -3]), np.array([0.0, 3.0, 1.0, 1.0]), 2, 100)
    assert site[0].tolist() == [4] and site[1].tolist() == [2] and site[2].tolist() == [2]


def batch_from_events(events, ref_len, names, ref_codes):
    """A ``rows=True`` SiteLevelBatch around a hand-made event table (the moments are not what is tested: zeros)."""
    from nadavca_amd.site_levels import SiteLevelBatch, _site_key
    key = _site_key(events['contig'], events['position'], events['strand'], ref_len)
    q, count = np.unique(key, return_counts=True)
    g = q >> 1
    return SiteLevelBatch((g // ref_len).astype(np.int32), (g % ref_len).astype(np.int64), (q & 1).astype(np.int8),
                          np.asarray(ref_codes)[g].astype(np.int8), count.astype(np.int64), np.zeros((q.size, 4)),
                          np.zeros((q.size, 4)), ref_len, names, events=events)


def hand_made(seed, shift):
    """Two contigs of 12 and 8 bases (ref_len 20): positions 2 .. 9 of contig 0 on both strands and 1 .. 5 of contig 1
    on the forward strand, 3 .. 9 events each, levels shifted by ``shift`` at contig 0 position 5 and contig 1 position
    3."""
    rng = np.random.default_rng(seed)
    cols = {c: [] for c in ('read', 'contig', 'position', 'strand', 'level', 'stdv', 'dwell', 'expected')}
    sites = [(0, p, s) for p in range(2, 10) for s in (0, 1)] + [(1, p, 0) for p in range(1, 6)]
    for c, p, s in sites:
        cov = int(rng.integers(3, 10))
        centre = 0.1 * p + (shift if (c, p) in ((0, 5), (1, 3)) else 0.0)
        cols['read'] += rng.integers(0, 30, cov).tolist()
        cols['contig'] += [c] * cov
        cols['position'] += [p] * cov
        cols['strand'] += [s] * cov
        cols['level'] += rng.normal(centre, 0.3, cov).tolist()
        cols['stdv'] += np.abs(rng.normal(0.3, 0.05, cov)).tolist()
        cols['dwell'] += rng.integers(3, 9, cov).tolist()
        cols['expected'] += [0.1 * p] * cov
    order = rng.permutation(len(cols['read']))
    dt = dict(read=np.int64, contig=np.int32, position=np.int64, strand=np.int8, dwell=np.int64)
    events = {c: np.array(v, dtype=dt.get(c, np.float64))[order] for c, v in cols.items()}
    ref_codes = np.random.default_rng(1).integers(0, 4, 40)          # by contig * ref_len + position
    return batch_from_events(events, 20, ['chrA', 'chrB'], ref_codes), ref_codes


@pytest.fixture
def restated_device(monkeypatch):
    """``compare_site_ranks`` with tests/site_ranks_ref.py's device layer in place of the upload and the kernel."""
    from nadavca_amd import site_ranks
    monkeypatch.setattr(site_ranks, '_upload_and_test', site_ranks_ref.device_layer)


def test_compare_site_ranks_on_hand_made_batches(restated_device, tmp_path):
    from nadavca_amd import SiteLevelBatch, SiteRankComparison, compare_site_ranks
    from nadavca_amd.site_levels import local_peaks
    (a, ref_codes), (b, _) = hand_made(11, 0.0), hand_made(12, 1.2)
    path = os.path.join(str(tmp_path), 'control.npz')
    a.save(path)
    loaded = SiteLevelBatch.load(path)
    for column, min_cov in (('level', 3), ('resid', 5), ('dwell', 4)):
        cmp = compare_site_ranks(a, b, column=column, min_coverage=min_cov)
        assert isinstance(cmp, SiteRankComparison) and cmp.column == column and cmp.contig_names == ['chrA', 'chrB']
        # the rows: by a loop over the sites
        value = lambda x: x.events['level'] - x.events['expected'] if column == 'resid' else x.events[column]
        want = []
        for c, p, s in sorted(set(zip(a.events['contig'].tolist(), a.events['position'].tolist(),
                                      a.events['strand'].tolist()))):
            sel = lambda x: (x.events['contig'] == c) & (x.events['position'] == p) & (x.events['strand'] == s)
            A, B = value(a)[sel(a)].astype(float), value(b)[sel(b)].astype(float)
            if A.size >= min_cov and B.size >= min_cov:
                want.append((c, p, s) + site_ranks_ref.one_site(A, B, 16384))
        assert len(want) >= 8 and len(cmp) == len(want)
        cols = [np.array(c) for c in zip(*want)]
        for f, w in zip(('contig', 'position', 'strand', 'n_a', 'n_b'), cols[:5]):
            assert np.array_equal(getattr(cmp, f), w), f
        assert cmp.contig.dtype == np.int32 and cmp.position.dtype == np.int64 and cmp.strand.dtype == np.int8
        assert set(cmp.contig) == {0, 1} and np.array_equal(cmp.ref_base, ref_codes[cmp.contig * 20 + cmp.position])
        ref = site_ranks_ref.host_columns(*cols[3:])
        for f in ('ks', 'ks_plus', 'ks_minus', 'u', 'auc', 'ks_exact'):
            assert np.array_equal(getattr(cmp, f), ref[f]), f
        assert site_ranks_ref.same_bits(cmp.ks_p, ref['ks_p']) and cmp.ks_exact.all()
        for f in ('mw_z', 'mw_p'):
            assert np.allclose(getattr(cmp, f), ref[f], rtol=1e-13, atol=0, equal_nan=True), f
        # peaks respect contigs and strands
        with np.errstate(divide='ignore'):
            assert np.array_equal(cmp.ks_peak, local_peaks(-np.log(cmp.ks_p), cmp.contig, cmp.position, cmp.strand, 5))
        assert np.array_equal(cmp.mw_peak, local_peaks(np.abs(cmp.mw_z), cmp.contig, cmp.position, cmp.strand, 5))
        for c, s in ((0, 0), (0, 1), (1, 0)):
            sel = (cmp.contig == c) & (cmp.strand == s)
            assert cmp.mw_peak[sel].any() and cmp.ks_peak[sel].any()
        # a control that was saved and loaded gives the same rows
        again = compare_site_ranks(loaded, b, column=column, min_coverage=min_cov)
        for f in ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'ks', 'ks_plus', 'ks_minus', 'ks_p',
                  'ks_exact', 'u', 'auc', 'mw_z', 'mw_p', 'ks_peak', 'mw_peak'):
            assert np.array_equal(getattr(again, f), getattr(cmp, f), equal_nan=True), f
    cmp = compare_site_ranks(a, b, min_coverage=3)
    shifted = (cmp.contig == 0) & (cmp.position == 5) | (cmp.contig == 1) & (cmp.position == 3)
    assert shifted.sum() == 3 and cmp.ks[shifted].min() > np.median(cmp.ks) and (cmp.auc[shifted] > 0.8).all()
    # reach 0: every row is a peak; exact_cells 0: no exact p-value, the asymptotic one instead
    assert compare_site_ranks(a, b, min_coverage=3, reach=0).ks_peak.all()
    rough = compare_site_ranks(a, b, min_coverage=3, exact_cells=0)
    assert not rough.ks_exact.any() and np.array_equal(rough.ks, cmp.ks) and not np.array_equal(rough.ks_p, cmp.ks_p)
    assert np.isfinite(rough.ks_p).all() and np.array_equal(rough.mw_p, cmp.mw_p)
    # the TSV
    buf = io.StringIO(newline='')
    cmp.write_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0].split('\t') == ['contig', 'position', 'strand', 'ref', 'n_a', 'n_b', 'ks', 'ks_plus', 'ks_minus',
                                    'ks_p', 'ks_exact', 'u', 'auc', 'mw_z', 'mw_p', 'ks_peak', 'mw_peak']
    i = len(cmp) - 1
    assert cmp.contig[i] == 1 and lines[i + 1] == 'chrB\t%d\t+\t%s\t%d\t%d\t%r\t%r\t%r\t%r\t1\t%r\t%r\t%r\t%r\t%d\t%d' % (
        cmp.position[i], 'ACGT'[cmp.ref_base[i]], cmp.n_a[i], cmp.n_b[i], float(cmp.ks[i]), float(cmp.ks_plus[i]),
        float(cmp.ks_minus[i]), float(cmp.ks_p[i]), float(cmp.u[i]), float(cmp.auc[i]), float(cmp.mw_z[i]),
        float(cmp.mw_p[i]), cmp.ks_peak[i], cmp.mw_peak[i])
    assert len(lines) == len(cmp) + 2 and lines[-1] == '' and lines[1].startswith('chrA\t2\t+\t')
    tsv = os.path.join(str(tmp_path), 'r.tsv')
    cmp.write_tsv(tsv)
    assert open(tsv).read() == buf.getvalue()


def test_guards_and_empty_batches():
    """Every ValueError comes before any device call, and so does the result for a batch without events."""
    from nadavca_amd import SiteLevelBatch, compare_site_ranks, site_rank_tests_batch
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
            compare_site_ranks(a, bad)
        with pytest.raises(ValueError):
            compare_site_ranks(bad, a)
    for kw in (dict(column='mean'), dict(column='count'), dict(min_coverage=0), dict(min_coverage=2.5), dict(reach=-1),
               dict(reach=1.5), dict(exact_cells=-1), dict(exact_cells=0.5)):
        with pytest.raises(ValueError):
            compare_site_ranks(a, b, **kw)
        with pytest.raises(ValueError):
            site_rank_tests_batch(None, None, None, **kw)
    for trim in (-1, 2.5):
        with pytest.raises(ValueError):
            site_rank_tests_batch(None, None, None, trim=trim)
    z = SiteLevelBatch.empty(20, ['chrA', 'chrB'], rows=True)
    for x, y in ((z, z), (a, z), (z, a)):
        cmp = compare_site_ranks(x, y, column='dwell')
        assert len(cmp) == 0 and cmp.column == 'dwell' and cmp.contig_names == ['chrA', 'chrB']
        assert cmp.ks_p.dtype == np.float64 and cmp.ks_exact.dtype == bool and cmp.ks_peak.dtype == bool
        assert cmp.n_a.dtype == np.int64 and cmp.ks.size == 0 and cmp.mw_p.size == 0
        buf = io.StringIO(newline='')
        cmp.write_tsv(buf)
        assert buf.getvalue().count('\n') == 1


def test_new_entry_declared_bound_and_exported():
    from conftest import ROOT
    import nadavca_amd
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    lib = _lib.load()
    name = 'nvk_site_rank_tests_dev'
    assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES[name][1]) == 17
    assert _lib.K_SITE == 12 and 'NVK_K_SITE = 12' in header and 'NVK_K_COUNT = 13' in header
    assert len(_lib.KERNEL_NAMES) == 13
    assert callable(device.site_rank_tests_dev)
    for f in ('compare_site_ranks', 'site_rank_tests_batch', 'SiteRankComparison'):
        assert f in nadavca_amd.__all__ and hasattr(nadavca_amd, f)


@pytest.mark.parametrize('seed,read_seeds', [(4, (104, 204)), (5, (105, 205))])
def test_planted_sites_on_the_oracle(oracle_port, seed, read_seeds):
    """The two-sample experiment of tests/test_site_levels_cpu.py (600 bases, 120 reads of 120 bases per sample,
    bandwidth 40, trim 5) with the rank tests on column 'level', min_coverage 5, the restatement in place of the kernel.
    Conditions, with 'nearby' and 'far' as ``site_levels_ref.detection_shares`` has them: KS, exact p: (a) at least 0.8
    of the modified sites have a row with p <= 1e-3 nearby, (b) at most 0.005 of the far rows have one; Mann-Whitney:
    (a) at least 0.9 at p <= 1e-2, (b) at most 0.03.  The (b) bounds are 5 and 3 times the nominal level, far outside
    the Poisson spread of a valid test on 500 rows.  A numpy run before the kernel existed gave, for seed 4: KS (a)
    0.867 of 15 sites, (b) 0 of 637 rows, MW (a) 1.0, (b) 0.0063; for seed 5: KS (a) 0.893 of 28, (b) 0 of 503, MW (a)
    1.0, (b) 0.0139.  The figures of a run are printed."""
    from nadavca_amd import synthetic
    from nadavca_amd.site_levels import SiteLevelBatch
    from nadavca_amd.site_ranks import _comparison
    model, model5 = synthetic.load_model_arrays(), site_levels_ref.model5()
    rows, truths = [], []
    for fraction, read_seed in zip((0.0, 0.3), read_seeds):
        rb, aligner, genome, truth = synthetic.make_modified_read_batch(
            120, model5, seed=seed, modified_fraction=fraction, genome_length=600, length=120, spread=0,
            read_seed=read_seed)
        sa, signal, sig_off, events, expected, status = site_levels_ref.oracle_front(
            oracle_port, rb, aligner.get_base_alignments(rb), genome, model, 40)
        assert sa.live.size == 120 and (status == 0).all()
        key, val = site_levels_ref.rows(signal, sig_off, events, sa.ref_off, expected, sa.ref_start, sa.reverse,
                                        status, 5, genome.size)
        rows.append((key, val[:, SiteLevelBatch.COLUMNS.index('level')]))
        truths.append(truth)
    assert not truths[0]['forward'].any() and not truths[0]['reverse'].any()
    site_key, *stats = site_ranks_ref.device_layer(*rows[0], *rows[1], 5, 16384)
    position = site_key >> 1
    cmp = _comparison('level', None, np.zeros(position.size, np.int32), position, (site_key & 1).astype(np.int8),
                      genome[position].astype(np.int8), 5, *stats)
    assert cmp.ks_exact.all()
    site_ranks_ref.check_detection(cmp, truths[1], model[0], min_sites=8, min_far=200)
