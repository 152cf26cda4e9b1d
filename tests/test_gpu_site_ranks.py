"""``compare_site_ranks`` and ``site_rank_tests_batch`` on the GPU, on the two samples of tests/test_gpu_site_levels.py:
every array against the numpy restatement (tests/site_ranks_ref.py) run on the host copies of the event tables, the
integers equal and the exact p-value bit for bit; the resident path against the host-table path; and the four detection
conditions of the planted-site experiment."""
import numpy as np
import pytest

import site_levels_ref
import site_ranks_ref

pytestmark = pytest.mark.gpu

SEED, N_READS, GENOME, TRIM = 4, 300, 3000, 5
SAMPLES = (('A', 0.0, 104), ('B', 0.3, 204))         # name, modified fraction of the CG sites, read seed
FIELDS = ('contig', 'position', 'strand', 'ref_base', 'n_a', 'n_b', 'ks', 'ks_plus', 'ks_minus', 'ks_p', 'ks_exact',
          'u', 'auc', 'mw_z', 'mw_p', 'ks_peak', 'mw_peak')


@pytest.fixture(scope='module')
def world():
    from nadavca_amd import defaults, dtw, site_levels_batch, synthetic
    from nadavca_amd.batchflow import load_config
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    km = dtw.KmerModel(*synthetic.load_model_arrays())
    model5 = site_levels_ref.model5()
    out = dict(config=config, km=km)
    for name, fraction, read_seed in SAMPLES:
        rb, aligner, genome, truth = synthetic.make_modified_read_batch(
            N_READS, model5, seed=SEED, modified_fraction=fraction, genome_length=GENOME, length=200, spread=20,
            read_seed=read_seed)
        out[name] = dict(rb=rb, aligner=aligner, genome=genome, truth=truth,
                         got=site_levels_batch(rb, aligner, km, config, trim=TRIM, rows=True))
    return out


@pytest.fixture(scope='module')
def compared(world):
    from nadavca_amd import compare_site_ranks
    a, b = world['A']['got'], world['B']['got']
    return {column: compare_site_ranks(a, b, column=column, min_coverage=5) for column in ('level', 'dwell')}


@pytest.mark.parametrize('column', ['level', 'dwell'])
def test_every_array_equals_the_restatement(world, compared, column):
    from nadavca_amd.site_levels import local_peaks
    a, b, genome = world['A']['got'], world['B']['got'], world['A']['genome']
    cmp = compared[column]
    key = lambda x: 2 * x.events['position'] + x.events['strand']
    site_key, *stats = site_ranks_ref.device_layer(key(a), a.events[column].astype(np.float64), key(b),
                                                   b.events[column].astype(np.float64), 5, 16384)
    assert site_key.size > 4000 and len(cmp) == site_key.size and np.median(stats[0]) >= 8
    assert np.array_equal(cmp.position, site_key >> 1) and np.array_equal(cmp.strand, site_key & 1)
    assert (cmp.contig == 0).all() and np.array_equal(cmp.ref_base, genome[site_key >> 1])
    assert cmp.contig_names is None and cmp.column == column
    assert np.array_equal(cmp.n_a, stats[0]) and np.array_equal(cmp.n_b, stats[1])
    ref = site_ranks_ref.host_columns(*stats)
    for f in ('ks', 'ks_plus', 'ks_minus', 'u', 'auc', 'ks_exact'):
        assert np.array_equal(getattr(cmp, f), ref[f]), f
    assert cmp.ks_exact.all() and site_ranks_ref.same_bits(cmp.ks_p, stats[6])
    # (mw_z and mw_p: a square root, a division and scipy's ndtr on equal inputs, row by row there and as arrays here)
    for f in ('mw_z', 'mw_p'):
        assert np.allclose(getattr(cmp, f), ref[f], rtol=1e-13, atol=0, equal_nan=True), f
    with np.errstate(divide='ignore'):
        assert np.array_equal(cmp.ks_peak, local_peaks(-np.log(cmp.ks_p), cmp.contig, cmp.position, cmp.strand, 5))
    assert np.array_equal(cmp.mw_peak, local_peaks(np.abs(cmp.mw_z), cmp.contig, cmp.position, cmp.strand, 5))
    if column == 'dwell':
        tie = stats[5]
        assert (tie > 0).mean() > 0.9                                   # dwell times are small integers


def equal_rows(x, y):
    for f in FIELDS:
        gx, gy = getattr(x, f), getattr(y, f)
        assert gx.dtype == gy.dtype and np.array_equal(gx, gy, equal_nan=True), f
    assert x.column == y.column and x.contig_names == y.contig_names


@pytest.mark.parametrize('column', ['level', 'dwell'])
def test_the_resident_path_equals_the_host_tables(world, compared, column):
    from nadavca_amd import site_rank_tests_batch
    got = site_rank_tests_batch(world['A']['rb'], world['B']['rb'], (world['A']['aligner'], world['B']['aligner']),
                                world['km'], world['config'], trim=TRIM, column=column, min_coverage=5)
    equal_rows(got, compared[column])


def test_a_second_call_gives_equal_arrays(world, compared):
    from nadavca_amd import compare_site_ranks
    equal_rows(compare_site_ranks(world['A']['got'], world['B']['got'], column='level', min_coverage=5),
               compared['level'])
    # a smaller exact_cells: the integers stay, the sites above it get the asymptotic p-value
    rough = compare_site_ranks(world['A']['got'], world['B']['got'], column='level', min_coverage=5, exact_cells=100)
    cmp = compared['level']
    small = cmp.n_a * cmp.n_b <= 100
    assert small.any() and not small.all() and np.array_equal(rough.ks_exact, small)
    assert np.array_equal(rough.ks_p[small], cmp.ks_p[small]) and np.array_equal(rough.u, cmp.u)
    assert np.isfinite(rough.ks_p).all() and not np.array_equal(rough.ks_p[~small], cmp.ks_p[~small])


def test_planted_sites_are_found(world, compared):
    """Sample A unmodified, sample B with 0.3 of the CG sites of each strand modified: the input of
    tests/test_gpu_site_levels.py.  Over the (site, strand) with coverage >= 5 in both samples, column 'level', 'nearby'
    and 'far' as ``site_levels_ref.detection_shares`` has them: KS, exact p: (a) at least 0.8 of the modified sites have
    a row with p <= 1e-3 nearby, (b) at most 0.005 of the far rows have one; Mann-Whitney: (a) at least 0.9 at
    p <= 1e-2, (b) at most 0.03.  The (b) bounds are 5 and 3 times the nominal level, far outside the Poisson spread of
    a valid test on 3 000 rows.  The same input through the CPU oracle and a numpy restatement gave 5 107 rows, median
    coverage 10 / 10, 87 modified sites with a row, 3 181 far rows; KS (a) 0.931, (b) 0.0013 (smallest far p 8.3e-5);
    MW (a) 0.989, (b) 0.0094.  One MI355X gave the same: 5 107 rows, KS (a) 0.931 of 87, (b) 0.0013 of 3 181 (smallest far
    p 8.4e-5), MW (a) 0.989, (b) 0.0094.  The figures of a run are printed."""
    assert not world['A']['truth']['forward'].any() and not world['A']['truth']['reverse'].any()
    site_ranks_ref.check_detection(compared['level'], world['B']['truth'], 6, min_sites=50, min_far=1000)


def test_two_contigs_with_one_seed_aligner(world):
    """Both samples through ONE ``SeedAligner`` over a ``ReferenceSet`` of two contigs: named, contig-local rows, and
    the resident path equal to the host-table path in every array."""
    from contig_fixture import two_contig_samples
    from nadavca_amd import compare_site_ranks, site_levels_batch, site_rank_tests_batch
    samples, contigs, names, aligner = two_contig_samples(site_levels_ref.model5())
    km, config = world['km'], world['config']
    got = site_rank_tests_batch(samples[0], samples[1], aligner, km, config, trim=TRIM, column='resid', min_coverage=5)
    a, b = (site_levels_batch(rb, aligner, km, config, trim=TRIM, rows=True) for rb in samples)
    equal_rows(got, compare_site_ranks(a, b, column='resid', min_coverage=5))
    assert got.contig_names == names and got.column == 'resid' and len(got) > 1500
    assert set(got.contig.tolist()) == {0, 1} and (np.diff(got.contig) >= 0).all()
    for c, genome in enumerate(contigs):
        sel = got.contig == c
        assert sel.sum() > 400 and got.position[sel].max() < genome.size
        assert np.array_equal(got.ref_base[sel], genome[got.position[sel]])
        key = 2 * got.position[sel] + got.strand[sel]
        assert (np.diff(key) > 0).all()
    assert got.ks_exact.all() and (got.n_a >= 5).all() and (got.n_b >= 5).all()
