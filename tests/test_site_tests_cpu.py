"""The layer the per-site two-sample operators share (nadavca_amd/site_tests.py), without a GPU: the one TSV writer
under the three result classes against lines written out here, the one copy back on CPU tensors, and the shared check
of ``column``, ``min_coverage``, ``reach`` and ``trim``."""
import io
import os

import numpy as np
import pytest

NAN, INF = float('nan'), float('inf')
LABELS = {None: ['0', '0', '1', '1'], 'named': ['chrA', 'chrA', 'chrB', 'chrB']}
COMMON = ['3\t+\tA', '3\t-\tC', '0\t+\tG', '17\t-\tT']            # position, strand, ref of the four rows

LEVELS_HEADER = 'contig\tposition\tstrand\tref\tn_a\tn_b\tmean_a\tmean_b\tdelta\tt\tdf\tp\tpeak'
LEVELS_ROWS = ['5\t9\t0.5\t1.5\t1.0\t2.5\t8.0\t0.03125\t1',
               '6\t10\t-1.25\t-1.0\t0.25\t1e-300\t9.5\t1.0\t0',
               '7\t11\t0.1\t0.30000000000000004\t0.2\t-0.0\t16.0\t1.0\t1',
               '8\t12\t100.0\tnan\tnan\tnan\tnan\tnan\t0']
RANKS_HEADER = 'contig\tposition\tstrand\tref\tn_a\tn_b\tks\tks_plus\tks_minus\tks_p\tks_exact\tu\tauc\tmw_z\tmw_p\t' \
               'ks_peak\tmw_peak'
RANKS_ROWS = ['5\t9\t0.5\t0.5\t0.25\t0.125\t1\t10.0\t0.75\t-1.5\t0.0625\t1\t0',
              '6\t10\t1.0\t0.0\t1.0\t2e-05\t0\t0.0\t1.0\tinf\t0.0\t0\t1',
              '7\t11\t0.2\t0.1\t0.2\t1.0\t1\t38.5\t0.5\tnan\tnan\t1\t0',
              '8\t12\t0.75\t0.75\t0.0\t1.5e-10\t0\t96.0\t0.0\t-0.0\t1.0\t0\t0']
MIX_HEADER = 'contig\tposition\tstrand\tref\tn_a\tn_b\tfitted\tmean_0\tsd_0\tmean_1\tsd_1\trate_a\trate_b\t' \
             'delta_rate\tll_one\tll_shared\tll_free\tlrt\tz\tp\tpeak'
MIX_ROWS = ['5\t9\t1\t0.0\t1.0\t2.5\t0.5\t0.25\t0.75\t0.5\t-10.5\t-9.0\t-8.5\t1.0\t3.0\t0.002\t1',
            '6\t10\t0\tnan\tnan\tnan\tnan\tnan\tnan\tnan\t-20.0\t-20.0\t-20.0\tnan\tnan\tnan\t0',
            '7\t11\t1\t-1.5\t0.125\t1.5\t0.125\t0.0\t1.0\t1.0\t-1e+22\t-5.5\t-5.5\t0.0\t-0.0\t1.0\t1',
            '8\t12\t1\t0.1\t0.2\t0.7\t0.30000000000000004\t0.5\t0.25\t-0.25\t-3.0\t-2.0\t-1.0\t2.0\t-inf\t0.0\t0']


def hand_made(names):
    """One result of each class with the four rows above -> ((result, header, rows), ...)."""
    from nadavca_amd import SiteComparison, SiteMixtureComparison, SiteRankComparison
    f, flag = (lambda *x: np.array(x, dtype=np.float64)), (lambda *x: np.array(x, dtype=bool))
    common = dict(contig=np.array([0, 0, 1, 1], dtype=np.int32), position=np.array([3, 3, 0, 17], dtype=np.int64),
                  strand=np.array([0, 1, 0, 1], dtype=np.int8), ref_base=np.array([0, 1, 2, 3], dtype=np.int8),
                  n_a=np.array([5, 6, 7, 8], dtype=np.int64), n_b=np.array([9, 10, 11, 12], dtype=np.int64))
    levels = SiteComparison(*common.values(), f(0.5, -1.25, 0.1, 100.0), f(1.5, -1.0, 0.1 + 0.2, NAN),
                            f(1.0, 0.25, 0.2, NAN), f(2.5, 1e-300, -0.0, NAN), f(8.0, 9.5, 16.0, NAN),
                            f(0.03125, 1.0, 1.0, NAN), flag(1, 0, 1, 0), 'level', names)
    ranks = SiteRankComparison(
        'dwell', names, **common, ks=f(0.5, 1.0, 0.2, 0.75), ks_plus=f(0.5, 0.0, 0.1, 0.75),
        ks_minus=f(0.25, 1.0, 0.2, 0.0), ks_p=f(0.125, 2e-5, 1.0, 1.5e-10), ks_exact=flag(1, 0, 1, 0),
        u=f(10.0, 0.0, 38.5, 96.0), auc=f(0.75, 1.0, 0.5, 0.0), mw_z=f(-1.5, INF, NAN, -0.0),
        mw_p=f(0.0625, 0.0, NAN, 1.0), ks_peak=flag(1, 0, 1, 0), mw_peak=flag(0, 1, 0, 0))
    steps = np.array([32, 0, 7, 32], dtype=np.int64)
    mixtures = SiteMixtureComparison(
        'resid', names, steps, steps, **common, fitted=flag(1, 0, 1, 1), mean_0=f(0.0, NAN, -1.5, 0.1),
        sd_0=f(1.0, NAN, 0.125, 0.2), mean_1=f(2.5, NAN, 1.5, 0.7), sd_1=f(0.5, NAN, 0.125, 0.1 + 0.2),
        rate_a=f(0.25, NAN, 0.0, 0.5), rate_b=f(0.75, NAN, 1.0, 0.25), delta_rate=f(0.5, NAN, 1.0, -0.25),
        ll_one=f(-10.5, -20.0, -1e22, -3.0), ll_shared=f(-9.0, -20.0, -5.5, -2.0), ll_free=f(-8.5, -20.0, -5.5, -1.0),
        lrt=f(1.0, NAN, 0.0, 2.0), z=f(3.0, NAN, -0.0, -INF), p=f(0.002, NAN, 1.0, 0.0), peak=flag(1, 0, 1, 0))
    return (levels, LEVELS_HEADER, LEVELS_ROWS), (ranks, RANKS_HEADER, RANKS_ROWS), (mixtures, MIX_HEADER, MIX_ROWS)


@pytest.mark.parametrize('names', [None, 'named'])
def test_one_writer_prints_the_three_tables(names, tmp_path):
    from nadavca_amd.site_tests import SiteTable
    for result, header, rows in hand_made(None if names is None else ['chrA', 'chrB']):
        assert isinstance(result, SiteTable) and len(result) == 4
        buf = io.StringIO(newline='')
        result.write_tsv(buf)
        lines = buf.getvalue().split('\n')
        assert lines[0] == header and lines[-1] == '' and len(lines) == 6
        for line, label, common, row in zip(lines[1:5], LABELS[names], COMMON, rows):
            assert line == label + '\t' + common + '\t' + row
        path = os.path.join(str(tmp_path), type(result).__name__ + '.tsv')
        result.write_tsv(path)
        with open(path, newline='') as fh:
            assert fh.read() == buf.getvalue()
        assert not buf.closed                       # a file that was handed in stays open


@pytest.mark.parametrize('sites', [0, 3])
def test_copy_back_restores_dtype_shape_and_bits(sites):
    import torch
    from nadavca_amd.site_tests import copy_back
    rng = np.random.default_rng(sites)
    key = rng.integers(-2 ** 62, 2 ** 62, sites)
    counts = rng.integers(-5, 2 ** 40, (sites, 5))
    fit = rng.normal(size=(sites, 17))
    vec = rng.normal(size=sites)
    if sites:
        fit[0, :4] = [np.nan, -0.0, np.inf, -np.inf]
        fit[2, 16] = np.nan
        vec[:3] = [-0.0, np.nan, np.inf]
    want = (key, counts, fit, vec)
    got = copy_back(tuple(torch.from_numpy(x.copy()) for x in want))
    assert isinstance(got, tuple) and len(got) == 4
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(np.ascontiguousarray(g).view(np.int64), w.view(np.int64))
    assert got[0].dtype == np.int64 and got[1].shape == (sites, 5) and got[2].dtype == np.float64
    assert got[2].shape == (sites, 17) and got[3].shape == (sites,)


def test_the_shared_check():
    from nadavca_amd.site_tests import check_site_test
    assert [check_site_test('w', c, 1, 0) for c in ('level', 'stdv', 'dwell', 'resid')] == [0, 1, 2, 3]
    assert check_site_test('w', 'dwell', 5.0, 5.0, trim=0) == 2 and check_site_test('w', 'level', 1, 0, 7) == 0
    for what in ('compare_site_levels', 'site_rank_tests_batch'):
        for kw in (dict(min_coverage=0), dict(min_coverage=-3), dict(min_coverage=2.5), dict(reach=-1),
                   dict(reach=1.5), dict(trim=-1), dict(trim=2.5)):
            args = dict(dict(column='level', min_coverage=5, reach=5, trim=5), **kw)
            with pytest.raises(ValueError) as e:
                check_site_test(what, **args)
            (name, value), = kw.items()
            assert str(e.value).startswith('%s: %s %r is not an integer >= ' % (what, name, value))
        # a column that is not one: ``SiteLevelBatch.column_index``'s message, which has never named the caller
        for column in ('mean', 'count', None, 0):
            with pytest.raises(ValueError) as e:
                check_site_test(what, column, 5, 5)
            assert str(e.value) == 'column %r is not one of level, stdv, dwell, resid' % (column,)
