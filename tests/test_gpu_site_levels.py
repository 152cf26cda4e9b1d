"""``site_levels_batch`` and ``compare_site_levels`` on the GPU: every row of two samples over one genome against the
numpy restatement of the kernels' contract (tests/site_levels_ref.py) on the host copies of the same alignment stage,
bit for bit; and the two detection conditions of the planted-site experiment."""
import numpy as np
import pytest

import site_levels_ref

pytestmark = pytest.mark.gpu

SEED, N_READS, GENOME, TRIM = 4, 300, 3000, 5
SAMPLES = (('A', 0.0, 104), ('B', 0.3, 204))         # name, modified fraction of the CG sites, read seed


@pytest.fixture(scope='module')
def world():
    """Per sample: the reads, the workflow's result with the event table, and the restatement on the host copies of
    the stage ``batchflow.align_batch`` leaves for the same input (the front end of ``site_levels_batch``)."""
    from nadavca_amd import defaults, dtw, site_levels_batch, synthetic
    from nadavca_amd.batchflow import align_batch, load_config
    from nadavca_amd.device import expected_levels_dev
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    km = dtw.KmerModel(*synthetic.load_model_arrays())
    model5 = site_levels_ref.model5()
    out = dict(config=config, km=km)
    for name, fraction, read_seed in SAMPLES:
        rb, aligner, genome, truth = synthetic.make_modified_read_batch(
            N_READS, model5, seed=SEED, modified_fraction=fraction, genome_length=GENOME, length=200, spread=20,
            read_seed=read_seed)
        got = site_levels_batch(rb, aligner, km, config, trim=TRIM, rows=True)
        res = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
        sa, db = res.stage.sa, res.stage.dbatch
        host = lambda t: t.cpu().numpy()
        expected = host(expected_levels_dev(db, km, with_contexts=True))
        status = host(res.status)
        key, val = site_levels_ref.rows(host(db.signal), host(db.sig_off), host(res.events), host(db.ref_off), expected,
                                        host(sa.ref_start), host(sa.reverse), status, TRIM, genome.size)
        out[name] = dict(rb=rb, aligner=aligner, genome=genome, truth=truth, got=got, key=key, val=val,
                         expected=expected, status=status, live=host(sa.live), ref_off=host(db.ref_off))
    return out


@pytest.mark.parametrize('name', ['A', 'B'])
def test_every_row_equals_the_restatement(world, name):
    w = world[name]
    got, genome = w['got'], w['genome']
    want = site_levels_ref.batch_from_moments(*site_levels_ref.site_levels(w['key'], w['val'], 2 * genome.size), genome)
    assert len(want) > 1.5 * GENOME and want.count.max() >= 10
    for f in ('contig', 'position', 'strand', 'ref_base', 'count'):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
        assert getattr(got, f).dtype == getattr(want, f).dtype, f
    assert np.array_equal(got.mean.view(np.int64), want.mean.view(np.int64))
    assert np.array_equal(got.m2.view(np.int64), want.m2.view(np.int64))
    assert got.ref_len == genome.size and got.contig_names is None
    assert np.array_equal(got.status, w['status']) and np.array_equal(got.live, w['live'])
    assert (got.status == 0).sum() > 0.9 * N_READS
    # the event table: the counted rows in read order
    at = np.nonzero(w['key'] >= 0)[0]
    owner = np.searchsorted(w['ref_off'], at, side='right') - 1
    ev = got.events
    assert np.array_equal(ev['read'], w['live'][owner]) and (ev['contig'] == 0).all()
    assert np.array_equal(ev['position'], w['key'][at] >> 1) and np.array_equal(ev['strand'], w['key'][at] & 1)
    for c, j in (('level', 0), ('stdv', 1)):
        assert np.array_equal(ev[c].view(np.int64), w['val'][at, j].view(np.int64)), c
    assert np.array_equal(ev['dwell'], w['val'][at, 2].astype(np.int64))
    assert np.array_equal(ev['expected'], w['expected'][at])
    assert np.array_equal(ev['level'] - ev['expected'], w['val'][at, 3])


def test_a_second_call_gives_equal_arrays(world):
    from nadavca_amd import site_levels_batch
    w = world['B']
    again = site_levels_batch(w['rb'], w['aligner'], world['km'], world['config'], trim=TRIM)
    assert again.events is None
    for f in ('contig', 'position', 'strand', 'ref_base', 'count', 'mean', 'm2', 'status', 'live'):
        assert np.array_equal(getattr(again, f), getattr(w['got'], f)), f


def test_planted_sites_are_found(world):
    """Sample A unmodified, sample B with 0.3 of the CG sites of each strand modified (levels of ``_model5``), 300 reads
    of about 200 bases each over 3 000 bases, both aligned against the canonical packaged table, bandwidth 40: about 10
    reads per strand per sample.  Over the (site, strand) with coverage >= 5 in both samples: (a) at least 0.8 of the
    truly modified sites have a row with |t| >= 6 among the bases whose 6-mer holds the site; (b) at most 0.02 of the
    rows more than 12 positions from every modified site of their strand have |t| >= 6.  The conditions come from an
    idealised simulation (0.988 .. 1.0 and 0.0); the same input through the CPU oracle and the restatement (seed 4,
    read seeds 104 / 204) gave (a) 0.897 of 87 sites and (b) 0.0 of 3 181 rows, largest far |t| 5.36; seeds 5, 6, 7 gave
    (a) 0.868, 0.889, 0.840 and (b) 0.0, 0.0003, 0.0.  One MI355X gave the oracle's figures for seed 4: 5 107 rows, (a) 0.897
    of 87, (b) 0.0 of 3 181, largest far |t| 5.36; 'dwell': (a) 0.299, (b) 0.0003.  The figures of a run are printed."""
    from nadavca_amd import compare_site_levels
    a, b, truth = world['A']['got'], world['B']['got'], world['B']['truth']
    assert not world['A']['truth']['forward'].any() and not world['A']['truth']['reverse'].any()
    for column in ('level', 'resid', 'dwell'):
        cmp = compare_site_levels(a, b, column=column, min_coverage=5)
        share_a, sites, share_b, far_rows, far_max, peak_dist = site_levels_ref.detection_shares(cmp, truth, 6)
        print('%s: %d rows; (a) %.3f of %d modified sites have |t| >= 6 nearby; (b) %.4f of %d far rows have |t| >= 6, '
              'largest far |t| %.2f; %d peak rows with |t| >= 6: %d on a modified site, %d within 3, %d beyond 12'
              % (column, len(cmp), share_a, sites, share_b, far_rows, far_max, peak_dist.size,
                 int((peak_dist == 0).sum()), int((peak_dist <= 3).sum()), int((peak_dist > 12).sum())))
        if column == 'level':
            assert sites >= 50 and far_rows >= 1000
            assert share_a >= 0.8, share_a
            assert share_b <= 0.02, share_b
