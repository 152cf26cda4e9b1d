"""CPU-only tests of ``site_levels_batch`` / ``compare_site_levels``: the numpy restatement of the kernels' contract
(tests/site_levels_ref.py) against plain numpy, Welch's test against scipy, ``merge`` against one pooled batch, the
round trips and guards, the new entries of the C-ABI, ``read_seed`` of the synthetic reads, and the planted-site
experiment through the CPU oracle."""
import io
import os

import numpy as np
import pytest

import site_levels_ref


def pile_ups(seed, n_sites, cov_lo, cov_hi, shift_share=0.3):
    """Random rows of 4 columns over ``n_sites`` positions and both strands: -> (key, val) in random row order, with
    coverage cov_lo .. cov_hi - 1 per key and a shifted level at some sites."""
    rng = np.random.default_rng(seed)
    keys, vals = [], []
    for q in range(2 * n_sites):
        c = int(rng.integers(cov_lo, cov_hi))
        centre = rng.normal(0.0, 1.0) + (rng.normal(0.0, 0.8) if rng.random() < shift_share else 0.0)
        keys.append(np.full(c, q))
        vals.append(np.stack([rng.normal(centre, 0.3, c), np.abs(rng.normal(0.3, 0.05, c)),
                              rng.integers(3, 18, c).astype(float), rng.normal(0.0, 0.3, c)], 1))
    key, val = np.concatenate(keys), np.concatenate(vals)
    order = rng.permutation(key.size)
    return key[order], val[order]


def test_restatement_against_plain_numpy():
    """At most 130 rows per key: about n 2^-53 = 3e-14 of rounding; the tolerance is about 30 times that."""
    rng = np.random.default_rng(3)
    counts = [0, 1, 2, 63, 64, 65, 130, 7, 0, 40]
    key = np.concatenate([np.full(c, q) for q, c in enumerate(counts)] + [np.full(5, -1), np.full(4, len(counts))])
    val = rng.normal(1.0, 2.0, (key.size, 4))
    val[:, 2] = rng.integers(1, 300, key.size)
    order = rng.permutation(key.size)
    key, val = key[order], val[order]
    count, mean, m2 = site_levels_ref.site_levels(key, val, len(counts))
    assert count.tolist() == counts
    for q, c in enumerate(counts):
        v = val[key == q]
        if c == 0:
            assert (mean[q] == 0).all() and (m2[q] == 0).all()
            continue
        want_mean = np.mean(v, axis=0)
        want_m2 = np.sum((v - want_mean) ** 2, axis=0)
        assert np.all(np.abs(mean[q] - want_mean) <= 1e-12 * np.abs(want_mean)), (q, mean[q], want_mean)
        assert np.all(np.abs(m2[q] - want_m2) <= 1e-12 * np.abs(want_m2) + 1e-12 * np.max(np.abs(v), axis=0) ** 2)
    assert (m2[1] == 0).all() and np.array_equal(mean[1], val[key == 1][0])
    # a NaN stays inside its own column
    val2 = val.copy()
    val2[np.nonzero(key == 6)[0][70], 1] = np.nan
    _, mean2, m22 = site_levels_ref.site_levels(key, val2, len(counts))
    assert np.isnan(mean2[6, 1]) and np.isnan(m22[6, 1])
    keep = np.ones_like(mean, dtype=bool)
    keep[6, 1] = False
    assert np.array_equal(mean2[keep], mean[keep]) and np.array_equal(m22[keep], m2[keep])


def test_rows_restatement_on_a_tiny_read():
    x = np.arange(20, dtype=float) ** 1.5
    events = np.array([[0, 2], [2, 2], [2, 9], [9, 25], [-3, 1], [12, 14]], dtype=np.int32)
    expected = np.linspace(-1, 1, 6)
    for rev in (0, 1):
        key, val = site_levels_ref.rows(x, [0, 20], events, [0, 6], expected, [7], [rev], None, 0, 12)
        pos = [7 + (5 - g if rev else g) for g in range(6)]
        inside = lambda g: 2 * pos[g] + rev if pos[g] < 12 else -1       # (forward: base 5, reverse: base 0 lies past)
        assert key.tolist() == [inside(0), -1, inside(2), inside(3), inside(4), inside(5)] and sum(key < 0) == 2
        assert val[1].tolist() == [0.0] * 4
        assert val[3].tolist() == [np.mean(x[9:20]), np.std(x[9:20]), 11.0, np.mean(x[9:20]) - expected[3]]
        assert val[4].tolist() == [0.0, 0.0, 1.0, 0.0 - expected[4]]
    key, _ = site_levels_ref.rows(x, [0, 20], events, [0, 6], expected, [7], [0], [1], 0, 12)
    assert (key == -1).all()
    key, _ = site_levels_ref.rows(x, [0, 20], events, [0, 6], expected, [7], [0], [0], 2, 12)
    assert (key >= 0).tolist() == [False, False, True, True, False, False]


def test_compare_site_levels_against_scipy():
    from scipy import stats
    from nadavca_amd import compare_site_levels
    n_sites = 40
    ref = np.random.default_rng(1).integers(0, 4, n_sites)
    ka, va = pile_ups(21, n_sites, 0, 30)
    kb, vb = pile_ups(22, n_sites, 0, 30)
    a = site_levels_ref.batch_from_moments(*site_levels_ref.site_levels(ka, va, 2 * n_sites), ref)
    b = site_levels_ref.batch_from_moments(*site_levels_ref.site_levels(kb, vb, 2 * n_sites), ref)
    for column, min_cov in (('level', 5), ('resid', 2), ('dwell', 1), ('stdv', 12)):
        j = a.COLUMNS.index(column)
        cmp = compare_site_levels(a, b, column=column, min_coverage=min_cov)
        want = [q for q in range(2 * n_sites) if (ka == q).sum() >= min_cov and (kb == q).sum() >= min_cov]
        assert (2 * cmp.position + cmp.strand).tolist() == want and len(want) > 10
        assert cmp.column == column and np.array_equal(cmp.ref_base, ref[cmp.position])
        checked = 0
        for i, q in enumerate(want):
            xa, xb = va[ka == q, j], vb[kb == q, j]
            assert cmp.n_a[i] == xa.size and cmp.n_b[i] == xb.size
            assert cmp.delta[i] == cmp.mean_b[i] - cmp.mean_a[i]
            if xa.size < 2 or xb.size < 2:
                assert np.isnan(cmp.t[i]) and np.isnan(cmp.df[i]) and np.isnan(cmp.p[i]) and not cmp.peak[i]
                continue
            res = stats.ttest_ind(xb, xa, equal_var=False)
            assert abs(cmp.t[i] - res.statistic) <= 1e-12 * abs(res.statistic), (column, q)
            assert abs(cmp.df[i] - res.df) <= 1e-12 * res.df
            if res.pvalue > 1e-300:
                assert abs(cmp.p[i] - res.pvalue) <= 1e-9 * res.pvalue
            checked += 1
        assert checked > 10
        # peak against a loop
        at = np.abs(cmp.t)
        for i in range(len(cmp)):
            others = [at[m] for m in range(len(cmp)) if m != i and cmp.strand[m] == cmp.strand[i]
                      and abs(cmp.position[m] - cmp.position[i]) <= 5 and not np.isnan(at[m])]
            assert cmp.peak[i] == (not np.isnan(at[i]) and not any(o > at[i] for o in others)), i
        assert cmp.peak.any() and not cmp.peak.all()
    assert np.isnan(compare_site_levels(a, b, column='dwell', min_coverage=1).t).any()
    # a denominator of 0: both pile-ups constant
    const = lambda v: site_levels_ref.batch_from_moments(
        *site_levels_ref.site_levels(np.zeros(6, np.int64), np.full((6, 4), v), 2 * n_sites), ref)
    z = compare_site_levels(const(1.0), const(2.0))
    assert len(z) == 1 and z.delta[0] == 1.0 and np.isnan(z.t[0]) and np.isnan(z.df[0]) and np.isnan(z.p[0])
    # reach: with reach 0 every row with a t is a peak
    assert compare_site_levels(a, b, reach=0).peak.all()


def test_peak_respects_contigs():
    from nadavca_amd.site_levels import local_peaks
    score = np.array([1.0, 3.0, 2.0, np.nan, 5.0, 4.0])
    contig = np.array([0, 0, 0, 1, 1, 1])
    position = np.array([10, 12, 30, 0, 2, 3])
    strand = np.zeros(6, dtype=np.int8)
    assert local_peaks(score, contig, position, strand, 5).tolist() == [False, True, True, False, True, False]
    assert local_peaks(score, np.zeros(6, int), np.array([0, 1, 2, 3, 4, 5]), strand, 5).tolist() == \
        [False, False, False, False, True, False]
    assert local_peaks(score, contig, position, np.array([0, 1, 0, 1, 0, 1]), 5).tolist() == \
        [True, True, True, False, True, True]


def test_merge_against_one_batch():
    """Chan's update adds a few roundings per merge and coverage stays below 10^3: 1e-10 relative."""
    from nadavca_amd.site_levels import SiteLevelBatch
    n_sites = 30
    ref = np.random.default_rng(2).integers(0, 4, n_sites)
    parts = [pile_ups(31 + i, n_sites, 0, 200) for i in range(3)]
    # key 3 only in the first part, key 7 only in the last
    drop = lambda part, keys: tuple(x[~np.isin(part[0], keys)] for x in part)
    parts = [drop(parts[0], [7]), drop(parts[1], [3, 7]), drop(parts[2], [3])]
    batches = [site_levels_ref.batch_from_moments(*site_levels_ref.site_levels(k, v, 2 * n_sites), ref,
                                                  status=np.array([0, i], np.int32), live=np.array([0, 1]))
               for i, (k, v) in enumerate(parts)]
    only_first = batches[0]
    merged = batches[0].merge(batches[1]).merge(batches[2])
    key = np.concatenate([k for k, _ in parts])
    val = np.concatenate([v for _, v in parts])
    pooled = site_levels_ref.batch_from_moments(*site_levels_ref.site_levels(key, val, 2 * n_sites), ref)
    for f in ('contig', 'position', 'strand', 'ref_base', 'count'):
        assert np.array_equal(getattr(merged, f), getattr(pooled, f)), f
        assert getattr(merged, f).dtype == getattr(only_first, f).dtype
    assert np.all(np.abs(merged.mean - pooled.mean) <= 1e-10 * np.abs(pooled.mean))
    assert np.all(np.abs(merged.m2 - pooled.m2) <= 1e-10 * np.abs(pooled.m2))
    assert merged.count.max() < 1000 and merged.status.tolist() == [0, 0, 0, 1, 0, 2] and merged.events is None
    assert len(merged) > max(len(x) for x in batches)
    # merging with an empty batch changes nothing
    same = batches[0].merge(SiteLevelBatch.empty(n_sites))
    assert np.array_equal(same.mean, batches[0].mean) and np.array_equal(same.m2, batches[0].m2)
    assert np.array_equal(same.count, batches[0].count) and np.array_equal(same.position, batches[0].position)
    # sd
    sd = pooled.sd('level')
    for i in range(len(pooled)):
        v = val[key == 2 * pooled.position[i] + pooled.strand[i], 0]
        if v.size < 2:
            assert np.isnan(sd[i])
        else:
            assert abs(sd[i] - np.std(v, ddof=1)) <= 1e-10 * np.std(v, ddof=1)


def _tiny_batch(rows=True):
    from nadavca_amd.site_levels import SiteLevelBatch
    events = None
    if rows:
        events = dict(read=np.array([3, 3, 7]), contig=np.array([0, 1, 1], np.int32), position=np.array([5, 2, 2]),
                      strand=np.array([0, 1, 1], np.int8), level=np.array([0.5, -1.25, -0.75]),
                      stdv=np.array([0.25, 0.5, 0.125]), dwell=np.array([4, 9, 3]), expected=np.array([0.25, -1.0, -1.0]))
    return SiteLevelBatch(np.array([0, 1], np.int32), np.array([5, 2]), np.array([0, 1], np.int8),
                          np.array([2, 3], np.int8), np.array([1, 2]),
                          np.array([[0.5, 0.25, 4.0, 0.25], [-1.0, 0.3125, 6.0, 0.0]]),
                          np.array([[0.0, 0.0, 0.0, 0.0], [0.125, 0.0703125, 18.0, 0.125]]), 9, ['chrA', 'chrB'],
                          np.array([0, 1, 0], np.int32), np.array([3, 5, 7]), events)


def test_round_trips_and_guards(tmp_path):
    from nadavca_amd import SiteLevelBatch, compare_site_levels, site_levels_batch
    b = _tiny_batch()
    path = os.path.join(str(tmp_path), 'control.npz')
    b.save(path)
    again = SiteLevelBatch.load(path)
    for f in ('contig', 'position', 'strand', 'ref_base', 'count', 'mean', 'm2', 'status', 'live'):
        assert np.array_equal(getattr(again, f), getattr(b, f)) and getattr(again, f).dtype == getattr(b, f).dtype, f
    assert again.ref_len == 9 and again.contig_names == ['chrA', 'chrB']
    assert all(np.array_equal(again.events[c], b.events[c]) for c in b.events)
    plain = _tiny_batch(rows=False)
    plain.contig_names = None
    plain.save(path)
    again = SiteLevelBatch.load(path)
    assert again.contig_names is None and again.events is None

    buf = io.StringIO(newline='')
    b.write_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0].split('\t') == ['contig', 'position', 'strand', 'ref', 'count', 'level_mean', 'level_sd',
                                    'stdv_mean', 'stdv_sd', 'dwell_mean', 'dwell_sd', 'resid_mean', 'resid_sd']
    assert lines[1] == 'chrA\t5\t+\tG\t1\t0.5\tnan\t0.25\tnan\t4.0\tnan\t0.25\tnan'
    assert lines[2].startswith('chrB\t2\t-\tT\t2\t-1.0\t%r\t' % float(np.sqrt(0.125))) and lines[3] == ''
    tsv = os.path.join(str(tmp_path), 's.tsv')
    b.write_tsv(tsv)
    assert open(tsv).read() == buf.getvalue()
    buf = io.StringIO(newline='')
    b.write_events_tsv(buf, names={3: 'r3', 7: 'r7'})
    assert buf.getvalue().split('\n') == ['read\tcontig\tposition\tstrand\tlevel\tstdv\tdwell\texpected',
                                          'r3\tchrA\t5\t+\t0.5\t0.25\t4\t0.25', 'r3\tchrB\t2\t-\t-1.25\t0.5\t9\t-1.0',
                                          'r7\tchrB\t2\t-\t-0.75\t0.125\t3\t-1.0', '']
    buf = io.StringIO(newline='')
    b.write_events_tsv(buf)
    assert buf.getvalue().split('\n')[1].startswith('read3\t')
    with pytest.raises(ValueError):
        plain.write_events_tsv(io.StringIO())
    cmp = compare_site_levels(b, b, min_coverage=1)
    buf = io.StringIO(newline='')
    cmp.write_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0].split('\t') == ['contig', 'position', 'strand', 'ref', 'n_a', 'n_b', 'mean_a', 'mean_b', 'delta',
                                    't', 'df', 'p', 'peak']
    assert lines[1] == 'chrA\t5\t+\tG\t1\t1\t0.5\t0.5\t0.0\tnan\tnan\tnan\t0'
    assert lines[2] == 'chrB\t2\t-\tT\t2\t2\t-1.0\t-1.0\t0.0\t0.0\t2.0\t1.0\t1' and lines[3] == ''

    other = _tiny_batch()
    other.ref_len = 10
    named = _tiny_batch()
    named.contig_names = ['chrA', 'chrC']
    for bad in (other, named, plain):
        with pytest.raises(ValueError):
            b.merge(bad)
        with pytest.raises(ValueError):
            compare_site_levels(b, bad)
    for kw in (dict(column='mean'), dict(min_coverage=0), dict(min_coverage=2.5), dict(reach=-1)):
        with pytest.raises(ValueError):
            compare_site_levels(b, b, **kw)
    with pytest.raises(ValueError):
        b.sd('count')
    for trim in (-1, 2.5):
        with pytest.raises(ValueError):          # (before any device call)
            site_levels_batch(None, None, trim=trim)
    z = SiteLevelBatch.empty(7, ['a'], rows=True)
    assert len(z) == 0 and z.mean.shape == (0, 4) and z.events['read'].size == 0 and z.sd('level').size == 0
    assert len(compare_site_levels(z, z)) == 0


def test_new_entries_declared_bound_and_exported():
    from conftest import ROOT
    import nadavca_amd
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    lib = _lib.load()
    for name in ('nvk_site_level_rows_dev', 'nvk_site_moments_dev'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'NVK_K_SITE = %d' % _lib.K_SITE in header and _lib.KERNEL_NAMES[_lib.K_SITE] == 'site'
    assert _lib.K_SITE == 12 and 'NVK_K_COUNT = %d' % len(_lib.KERNEL_NAMES) in header and len(_lib.KERNEL_NAMES) == 13
    for f in ('site_level_rows_dev', 'site_moments_dev', 'site_levels_dev'):
        assert callable(getattr(device, f))
    for f in ('site_levels_batch', 'compare_site_levels', 'SiteLevelBatch', 'SiteComparison'):
        assert f in nadavca_amd.__all__ and hasattr(nadavca_amd, f)


def test_read_seed_of_the_modified_reads():
    from nadavca_amd import synthetic
    model5 = site_levels_ref.model5()
    kw = dict(seed=8, genome_length=800, length=100, spread=10, modified_fraction=0.3)
    rb0, al0, genome0, truth0 = synthetic.make_modified_read_batch(6, model5, **kw)
    rb1, al1, genome1, truth1 = synthetic.make_modified_read_batch(6, model5, read_seed=None, **kw)
    fields = ('raw_signal', 'sig_off', 'sequence', 'seq_off', 'map_base', 'map_sig', 'map_off')
    for f in fields:
        assert np.array_equal(getattr(rb0, f), getattr(rb1, f)), f
    rb2, al2, genome2, truth2 = synthetic.make_modified_read_batch(6, model5, read_seed=99, **kw)
    assert np.array_equal(genome0, genome2) and np.array_equal(al0.reference_num, al2.reference_num)
    assert np.array_equal(truth0['forward'], truth2['forward']) and np.array_equal(truth0['reverse'], truth2['reverse'])
    assert truth0['forward'].any() and truth0['reverse'].any()
    assert rb2.raw_signal.size != rb0.raw_signal.size or not np.array_equal(rb2.raw_signal, rb0.raw_signal)
    rb3 = synthetic.make_modified_read_batch(6, model5, read_seed=99, **kw)[0]
    assert np.array_equal(rb3.raw_signal, rb2.raw_signal)
    # read_seed equal to seed draws the reads that no read_seed draws
    rb4 = synthetic.make_modified_read_batch(6, model5, read_seed=8, **kw)[0]
    assert np.array_equal(rb4.raw_signal, rb0.raw_signal)


def test_planted_sites_on_the_oracle(oracle_port):
    """The two-sample experiment through the CPU oracle, with the restatement in place of the kernels: the levels of
    ``_model5`` (an M k-mer = its C k-mer + N(0, 0.6^2)), a 600-base genome, sample A unmodified and sample B with 0.3
    of the CG sites of each strand modified (the same ``seed``, another ``read_seed``), 120 reads of 120 bases per
    sample, alignment against the canonical packaged table, bandwidth 40, three renormalisation rounds, trim 5,
    min_coverage 5.  Conditions: (a) at least 0.8 of the modified sites have a row with |t| >= 6 among the bases whose
    6-mer holds the site; (b) at most 0.02 of the rows more than 12 positions from every modified site of their strand
    have |t| >= 6.
    Observed with seed 4 (read seeds 104 / 204), column 'level': 980 rows; (a) 0.800 of the 15 modified sites with a
    row of their own (12 of 15; 19 sites in all); (b) 0.0 of 637 far rows, largest far |t| 3.94; 12 peak rows with
    |t| >= 6, all within 3 positions of a modified site.  'resid' gives the same shares (both samples share the
    expected levels), 'dwell' (a) 0.133.  Seed 5 (read seeds 105 / 205) gave (a) 0.893 of 28 and (b) 0.0 of 503, largest
    far |t| 3.75.  The sites that are missed have small level shifts in all six k-mers (largest |t| 4.5 .. 5.7): the
    alignment against the canonical table moves event boundaries towards the expected levels, which the idealised
    simulation behind the two bounds does not do."""
    from nadavca_amd import compare_site_levels, synthetic
    model, model5 = synthetic.load_model_arrays(), site_levels_ref.model5()
    seed, samples = 4, []
    for fraction, read_seed in ((0.0, 104), (0.3, 204)):
        rb, aligner, genome, truth = synthetic.make_modified_read_batch(
            120, model5, seed=seed, modified_fraction=fraction, genome_length=600, length=120, spread=0,
            read_seed=read_seed)
        sa, signal, sig_off, events, expected, status = site_levels_ref.oracle_front(
            oracle_port, rb, aligner.get_base_alignments(rb), genome, model, 40)
        assert sa.live.size == 120 and (status == 0).all()
        key, val = site_levels_ref.rows(signal, sig_off, events, sa.ref_off, expected, sa.ref_start, sa.reverse,
                                        status, 5, genome.size)
        samples.append((site_levels_ref.batch_from_moments(*site_levels_ref.site_levels(key, val, 2 * genome.size),
                                                           genome), truth))
    (a, truth_a), (b, truth_b) = samples
    assert not truth_a['forward'].any() and not truth_a['reverse'].any()
    n_mod = int(truth_b['forward'].sum() + truth_b['reverse'].sum())
    for column in ('level', 'resid', 'dwell'):
        cmp = compare_site_levels(a, b, column=column, min_coverage=5)
        share_a, sites, share_b, far_rows, far_max, peak_dist = site_levels_ref.detection_shares(cmp, truth_b, model[0])
        print('%s: %d rows; (a) %.3f of %d modified sites (of %d) have |t| >= 6 nearby; (b) %.4f of %d far rows have '
              '|t| >= 6, largest far |t| %.2f; %d peak rows with |t| >= 6, %d of them on a modified site, %d within 3'
              % (column, len(cmp), share_a, sites, n_mod, share_b, far_rows, far_max, peak_dist.size,
                 int((peak_dist == 0).sum()), int((peak_dist <= 3).sum())))
        if column == 'level':
            assert sites >= 8 and far_rows >= 200
            assert share_a >= 0.8, share_a
            assert share_b <= 0.02, share_b
