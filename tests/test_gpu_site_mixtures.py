"""``compare_site_mixtures`` and ``site_mixture_tests_batch`` on the GPU, on two samples over the genome of
tests/test_gpu_site_ranks.py: every array against the numpy restatement (tests/site_mixtures_ref.py) run on the host
copies of the event tables; the resident path against the host-table path; two contigs through a ``ReferenceSet``; and
the detection conditions of a planted stoichiometry of about one half."""
import numpy as np
import pytest

import site_levels_ref
import site_mixtures_ref as ref

pytestmark = pytest.mark.gpu

SEED, GENOME, TRIM = 4, 3000, 5
FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'fitted', 'mean_0', 'sd_0', 'mean_1', 'sd_1',
          'rate_a', 'rate_b', 'delta_rate', 'll_one', 'll_shared', 'll_free', 'lrt', 'z', 'p', 'peak', 'steps_shared',
          'steps_free')


def make_samples(model5):
    """Sample A: 1 200 unmodified reads.  Sample B: 600 reads with 0.3 of the CG sites of each strand modified and 600
    unmodified reads: a modified site holds the modification in about half of B's reads.
    -> ((ReadBatch A, its synthetic aligner), (ReadBatch B, the two parts' synthetic aligners), genome, truth)"""
    from contig_fixture import concat_batches
    from nadavca_amd import synthetic
    make = lambda n, fraction, read_seed: synthetic.make_modified_read_batch(
        n, model5, seed=SEED, modified_fraction=fraction, genome_length=GENOME, length=200, spread=20,
        read_seed=read_seed)
    a = make(1200, 0.0, 104)
    b_mod, b_plain = make(600, 0.3, 204), make(600, 0.0, 304)
    assert np.array_equal(a[2], b_mod[2]) and np.array_equal(a[2], b_plain[2])
    assert not a[3]['forward'].any() and not a[3]['reverse'].any() and not b_plain[3]['forward'].any()
    return (a[0], a[1]), (concat_batches([b_mod[0], b_plain[0]]), (b_mod[1], b_plain[1])), a[2], b_mod[3]


@pytest.fixture(scope='module')
def world():
    from nadavca_amd import SeedAligner, defaults, dtw, site_levels_batch, synthetic
    from nadavca_amd.batchflow import load_config
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    km = dtw.KmerModel(*synthetic.load_model_arrays())
    (rb_a, _), (rb_b, _), genome, truth = make_samples(site_levels_ref.model5())
    aligner = SeedAligner(genome)
    out = dict(config=config, km=km, aligner=aligner, genome=genome, truth=truth, rb=(rb_a, rb_b))
    out['got'] = tuple(site_levels_batch(rb, aligner, km, config, trim=TRIM, rows=True) for rb in (rb_a, rb_b))
    return out


@pytest.fixture(scope='module')
def compared(world):
    from nadavca_amd import compare_site_mixtures
    return compare_site_mixtures(*world['got'], column='level', min_coverage=5)


def test_every_array_equals_the_restatement(world, compared):
    from nadavca_amd.site_levels import local_peaks
    a, b = world['got']
    cmp, genome = compared, world['genome']
    key = lambda x: 2 * x.events['position'] + x.events['strand']
    site_key, counts, fit = ref.device_layer(key(a), a.events['level'].astype(np.float64), key(b),
                                             b.events['level'].astype(np.float64), 5, 32, 0.1)
    assert site_key.size > 4000 and len(cmp) == site_key.size and np.median(counts[:, 0]) >= 30
    assert np.array_equal(cmp.position, site_key >> 1) and np.array_equal(cmp.strand, site_key & 1)
    assert (cmp.contig == 0).all() and np.array_equal(cmp.ref_base, genome[site_key >> 1])
    assert cmp.contig_names is None and cmp.column == 'level'
    # the kernel's two tables as the package brings them back, against the restatement: the kernel's tolerance
    from nadavca_amd import site_mixtures
    got_key, got_counts, got_fit = site_mixtures._upload_and_test(
        key(a), a.events['level'].astype(np.float64), key(b), b.events['level'].astype(np.float64), 5, 32, 0.1)
    assert np.array_equal(got_key, site_key)
    worst = ref.check_against(got_counts, got_fit, counts, fit)
    print('largest |difference| / (1 + |value|) over %d sites: %.3g' % (len(cmp), worst))
    # the rows: the host half on those tables, row by row with Python floats
    assert np.array_equal(np.stack([cmp.n_a, cmp.n_b, cmp.fitted.astype(np.int64), cmp.steps_shared, cmp.steps_free],
                                   axis=1), got_counts) and cmp.fitted.all()
    for f, w in ref.host_columns(got_counts, got_fit).items():
        assert np.allclose(getattr(cmp, f), w, rtol=1e-13, atol=0, equal_nan=True), f
    assert (cmp.rate_a <= 0.5).all() and np.array_equal(cmp.delta_rate, cmp.rate_b - cmp.rate_a)
    assert np.array_equal(cmp.lrt, 2.0 * (cmp.ll_free - cmp.ll_shared))
    assert np.array_equal(cmp.peak, local_peaks(np.abs(cmp.z), cmp.contig, cmp.position, cmp.strand, 5))


def equal_rows(x, y):
    for f in FIELDS:
        gx, gy = getattr(x, f), getattr(y, f)
        assert gx.dtype == gy.dtype and np.array_equal(gx, gy, equal_nan=True), f
    assert x.column == y.column and x.contig_names == y.contig_names


def test_the_resident_path_equals_the_host_tables(world, compared):
    from nadavca_amd import compare_site_mixtures, site_mixture_tests_batch
    got = site_mixture_tests_batch(*world['rb'], world['aligner'], world['km'], world['config'], trim=TRIM,
                                   column='level', min_coverage=5)
    equal_rows(got, compared)
    # a second call gives equal arrays; other parameters give another fit of the same sites
    equal_rows(compare_site_mixtures(*world['got'], column='level', min_coverage=5), compared)
    other = compare_site_mixtures(*world['got'], column='level', min_coverage=5, iterations=4, min_sd_ratio=0.5)
    assert np.array_equal(other.position, compared.position) and np.array_equal(other.ll_one, compared.ll_one)
    assert (other.steps_free == 4).all() and not np.array_equal(other.rate_b, compared.rate_b)


def test_planted_stoichiometry_is_found(world, compared):
    """Sample A unmodified; in sample B half of the reads carry the modification at 0.3 of the CG sites of each strand.
    Over the (site, strand) with coverage >= 5 in both samples, column 'level', 'nearby' and 'far' as
    ``site_levels_ref.detection_shares`` has them: (a) the share of the modified sites with a row of p <= 1e-3 nearby
    is at least 0.851, and the median ``delta_rate`` of the rows with p <= 1e-3 near a modified site is within 0.1 of
    0.523 (the measured figures below, minus 0.1 and +- 0.1); (b) at most 0.03 of the far rows have p <= 1e-2, 3 times
    the nominal level, as for the Mann-Whitney test.  The level shifts of the sites are N(0, 0.6^2) at a noise of 0.35,
    so many are small and (a) is not derivable: it was measured with the same reads through the CPU oracle (each part
    under its synthetic aligner) and the numpy restatement: 5 861 rows, median coverage 38 / 38, (a) 0.951 of 102
    modified sites, median delta_rate of the 315 such rows 0.523, (b) 0.0093 of 3 641 far rows (smallest far p 1.7e-4).
    One MI355X gave the same: 5 861 rows, (a) 0.951 of 102, median delta_rate 0.523 over 315 rows, (b) 0.0093 of 3 641.
    The figures of a run are printed."""
    share_a, sites, median, hits, share_b, far_rows = ref.detection(compared, world['truth'], 6)
    assert sites >= 50 and far_rows >= 1000 and hits >= 50
    assert share_b <= 0.03
    assert share_a >= 0.951 - 0.1 and abs(median - 0.523) <= 0.1


def test_two_contigs_with_one_seed_aligner(world):
    """Both samples through ONE ``SeedAligner`` over a ``ReferenceSet`` of two contigs: named, contig-local rows, and
    the resident path equal to the host-table path in every array."""
    from contig_fixture import two_contig_samples
    from nadavca_amd import compare_site_mixtures, site_levels_batch, site_mixture_tests_batch
    samples, contigs, names, aligner = two_contig_samples(site_levels_ref.model5())
    km, config = world['km'], world['config']
    got = site_mixture_tests_batch(samples[0], samples[1], aligner, km, config, trim=TRIM, column='resid',
                                   min_coverage=5)
    a, b = (site_levels_batch(rb, aligner, km, config, trim=TRIM, rows=True) for rb in samples)
    equal_rows(got, compare_site_mixtures(a, b, column='resid', min_coverage=5))
    assert got.contig_names == names and got.column == 'resid' and len(got) > 1500
    assert set(got.contig.tolist()) == {0, 1} and (np.diff(got.contig) >= 0).all()
    for c, genome in enumerate(contigs):
        sel = got.contig == c
        assert sel.sum() > 400 and got.position[sel].max() < genome.size
        assert np.array_equal(got.ref_base[sel], genome[got.position[sel]])
        assert (np.diff(2 * got.position[sel] + got.strand[sel]) > 0).all()
    assert (got.n_a >= 5).all() and (got.n_b >= 5).all() and got.fitted.all() and (got.rate_a <= 0.5).all()
