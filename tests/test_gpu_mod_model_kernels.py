"""The two kernels of modified-base table training on the GPU (nadavca_amd/csrc/kernels_modstats.hip) against the numpy
restatement (tests/mod_model_ref.py), bit for bit (int64 views), two calls giving the same bits:

* a constructed batch of a dozen reads: lengths 5, 63, 64, 65 and 150, windows with 0 .. 5 (and 6) sites, sites at the
  first and the last base, empty and one-base contexts, reads with status 1 and -1, an empty, a clamped and a
  300-sample event, gamma from {0, 1, random}; six window shapes, two alphabets, trim 0 and 5;
* the reduction on hand-made sorted rows: runs of 1, 63, 64, 65, 200 and 10 000 rows behind leading key -1 rows, and
  no run at all;
* with every gamma 1, the existing k-mer statistics on a copy of the batch whose reference carries the modified base;
* bad arguments, and a row_off that disagrees with the kernel's own counts."""
import copy
import ctypes as C

import numpy as np
import pytest

import read_rows_case
from mod_model_ref import mod_reduce, mod_rows_of, mod_stats

pytestmark = pytest.mark.gpu

LENGTHS = [5, 63, 64, 65, 150, 150, 150, 40, 150, 64, 33, 150]
CONTEXTS = [(0, 0), (1, 0), (2, 3), (0, 1), (6, 6), (3, 3), (3, 3), (6, 6), (0, 0), (6, 6), (1, 1), (6, 6)]
STATUS = [0, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 0]
GAMMA_MODE = ['random', 'one', 'random', 'zero', 'mixed', 'random', 'random', 'mixed', 'one', 'random', 'zero', 'mixed']


def _constructed():
    """-> (synthetic.Batch, events (sum R, 2) int32, status, site_off, site_pos, site_gamma): host arrays."""
    from nadavca_amd import synthetic
    rng = np.random.default_rng(41)
    cases, sites, gammas = [], [], []
    for j, (R, (nb, na), mode) in enumerate(zip(LENGTHS, CONTEXTS, GAMMA_MODE)):
        lens = rng.integers(1, 12, R)
        if j == 4:
            lens[12] = 300                              # one long event, in the middle of a run of sites
        starts = np.concatenate([[0], np.cumsum(lens)])
        ev = np.stack([starts[:-1], starts[1:]], 1).astype(np.int32)
        if R > 30:
            ev[10] = (ev[10][1], ev[10][0])            # empty
            ev[11, 1] = starts[-1] + 50                # clamped
        cases.append(dict(signal=rng.normal(0.0, 1.0, int(starts[-1])),
                          reference=rng.integers(0, 4, R).astype(np.int32),
                          context_before=rng.integers(0, 4, nb).astype(np.int32),
                          context_after=rng.integers(0, 4, na).astype(np.int32),
                          approximate_alignment=np.zeros((1, 2), np.int32), events=ev))
        # the first and the last base, six neighbours in a row (windows of k = 6 hold 5 of them, of k = 8 all 6), then
        # pairs and triples at growing distances, then singles
        want = [0, R - 1] + list(range(9, 15)) + [20, 22, 27, 30, 33, 41, 45, 49, 53, 70, 90, 91, 120]
        if R == 5:
            want = [0, 2, 4]
        pos = np.array(sorted(set(p for p in want if 0 <= p < R)), dtype=np.int32)
        g = {'one': np.ones(pos.size), 'zero': np.zeros(pos.size), 'random': rng.random(pos.size),
             'mixed': rng.choice([0.0, 1.0, 0.37], pos.size)}[mode]
        sites.append(pos)
        gammas.append(g)
    batch = synthetic.Batch(cases)
    site_off = np.concatenate([[0], np.cumsum([s.size for s in sites])]).astype(np.int64)
    return (batch, np.concatenate([c['events'] for c in cases]), np.array(STATUS, dtype=np.int32), site_off,
            np.concatenate(sites), np.concatenate(gammas))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope='module')
def constructed(ctx):
    import torch
    from nadavca_amd.device import DeviceBatch
    batch, events, status, site_off, site_pos, site_gamma = _constructed()
    dbatch = DeviceBatch(batch, 'cuda:%d' % ctx.device)
    up = lambda a: torch.from_numpy(a).to(dbatch.device)
    return dict(batch=batch, dbatch=dbatch, events=events, status=status, site_off=site_off, site_pos=site_pos,
                site_gamma=site_gamma, d_events=up(events), d_status=up(status), d_site_off=up(site_off),
                d_site_pos=up(site_pos), d_site_gamma=up(site_gamma))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize('alphabet', [5, 6])
@pytest.mark.parametrize('k,central', [(6, 2), (3, 1), (1, 0), (6, 0), (6, 5), (8, 3)])
def test_rows_equal_the_restatement_on_the_constructed_batch(ctx, constructed, k, central, alphabet):
    import torch
    from nadavca_amd.device import mod_kmer_rows_dev, mod_kmer_stats_dev
    c = constructed
    mod_code = alphabet - 1
    level = np.random.default_rng(100 * k + alphabet).normal(0.0, 1.0, alphabet ** k)
    d_level = torch.from_numpy(level).to(c['dbatch'].device)
    seen = set()
    for trim in (0, 5):
        args = (c['dbatch'], ctx, c['d_events'], c['d_status'], k, central, alphabet, trim, c['d_site_off'],
                c['d_site_pos'], c['d_site_gamma'], mod_code, d_level)
        key, val, row_off, skipped = mod_kmer_rows_dev(*args)
        exp_count, exp_key, exp_val, exp_skipped = mod_rows_of(c['batch'], c['events'], c['status'], k, central,
                                                               alphabet, trim, c['site_off'], c['site_pos'],
                                                               c['site_gamma'], mod_code, level)
        key, val, row_off = key.cpu().numpy(), val.cpu().numpy(), row_off.cpu().numpy()
        assert np.array_equal(np.diff(row_off), exp_count)
        assert skipped == exp_skipped and (skipped > 0) == (k >= 5)
        assert np.array_equal(key, exp_key)
        assert np.array_equal(_bits(val), _bits(exp_val))
        assert (key >= 0).sum() > 0 and (key < 0).sum() > 0
        seen |= set(np.unique(exp_count).tolist())
        key2, val2, _, skipped2 = mod_kmer_rows_dev(*args)
        assert np.array_equal(key2.cpu().numpy(), key) and np.array_equal(_bits(val2.cpu().numpy()), _bits(val))
        assert skipped2 == skipped
        # sort, gather, runs and the reduction behind the rows
        stats = mod_kmer_stats_dev(ctx, *args[:1], *args[2:])
        ukey, sums, rows = mod_stats(exp_key, exp_val)
        assert np.array_equal(stats['key'].cpu().numpy(), ukey) and np.array_equal(stats['count'].cpu().numpy(), rows)
        assert np.array_equal(_bits(stats['sums'].cpu().numpy()), _bits(sums))
        assert stats['rows'] == exp_key.size and stats['windows_skipped'] == exp_skipped
    # every width the window's shape allows came up
    assert seen == {0} | {(1 << m) - 1 for m in range(1, min(k, 4) + 1)}
    # status NULL: every read counts
    key, val, _, _ = mod_kmer_rows_dev(c['dbatch'], ctx, c['d_events'], None, k, central, alphabet, 0, c['d_site_off'],
                                       c['d_site_pos'], c['d_site_gamma'], mod_code, d_level)
    _, exp_key, exp_val, _ = mod_rows_of(c['batch'], c['events'], None, k, central, alphabet, 0, c['site_off'],
                                         c['site_pos'], c['site_gamma'], mod_code, level)
    assert np.array_equal(key.cpu().numpy(), exp_key) and np.array_equal(_bits(val.cpu().numpy()), _bits(exp_val))
    torch.cuda.synchronize()


@pytest.mark.parametrize('k,central', [(6, 2), (3, 1)])
def test_rows_on_the_read_view_shapes(ctx, k, central):
    """The batch of read_rows_case.py: reads without bases or samples, a dead read between live ones (its rows are
    written with key -1), trim beyond half a read, every clamp of an event, events around 128 samples, a read count
    that leaves a block part empty."""
    import torch
    from nadavca_amd import synthetic
    from nadavca_amd.device import DeviceBatch, mod_kmer_rows_dev
    case = read_rows_case.build()
    batch = synthetic.Batch(case['cases'])
    dbatch = DeviceBatch(batch, 'cuda:%d' % ctx.device)
    up = lambda a: torch.from_numpy(a).to(dbatch.device)
    level = np.random.default_rng(7 * k).normal(0.0, 1.0, 5 ** k)
    for trim in (0, read_rows_case.TRIM):
        for status in (case['status'], None):
            key, val, row_off, skipped = mod_kmer_rows_dev(dbatch, ctx, up(case['events']),
                                                           None if status is None else up(status), k, central, 5, trim,
                                                           up(case['site_off']), up(case['site_pos']),
                                                           up(case['site_gamma']), 4, up(level))
            exp_count, exp_key, exp_val, exp_skipped = mod_rows_of(batch, case['events'], status, k, central, 5, trim,
                                                                   case['site_off'], case['site_pos'],
                                                                   case['site_gamma'], 4, level)
            row_off = row_off.cpu().numpy()
            assert np.array_equal(np.diff(row_off), exp_count) and skipped == exp_skipped
            assert np.array_equal(key.cpu().numpy(), exp_key)
            assert np.array_equal(_bits(val.cpu().numpy()), _bits(exp_val))
            # the dead read between two live ones has rows, and they count only without a status
            off = case['ref_off']
            dead = key.cpu().numpy()[row_off[off[1]]:row_off[off[2]]]
            assert dead.size > 0 and (dead >= 0).any() == (status is None)
            assert (exp_key >= 0).sum() > 20


def test_reduction_on_hand_made_rows(ctx):
    import torch
    from nadavca_amd.device import mod_kmer_reduce_dev
    rng = np.random.default_rng(9)
    runs = [1, 63, 64, 65, 200, 10000]
    n_neg = 7
    n = n_neg + sum(runs)
    val = np.stack([rng.random(n), rng.integers(1, 300, n).astype(np.float64), rng.normal(0.0, 40.0, n),
                    rng.random(n) * 900.0], 1)
    val[:n_neg] = 0.0
    val[n_neg + 1 + 5, 0] = 0.0                         # weights of exactly 0 and 1 among the others
    val[n_neg + 1 + 6, 0] = 1.0
    run_off = (n_neg + np.concatenate([[0], np.cumsum(runs)])).astype(np.int64)
    dev = 'cuda:%d' % ctx.device
    d_val, d_off = torch.from_numpy(val).to(dev), torch.from_numpy(run_off).to(dev)
    exp_sums, exp_rows = mod_reduce(val, run_off)
    for _ in range(2):
        sums, rows = mod_kmer_reduce_dev(ctx, d_val, d_off)
        assert np.array_equal(rows.cpu().numpy(), exp_rows) and exp_rows.tolist() == runs
        assert np.array_equal(_bits(sums.cpu().numpy()), _bits(exp_sums))
    # no run at all: the rows all carry key -1, or there are none
    for rows_val, off in ((d_val[:n_neg], [n_neg]), (d_val[:0], [0])):
        sums, rows = mod_kmer_reduce_dev(ctx, rows_val, torch.tensor(off, dtype=torch.int64, device=dev))
        assert tuple(sums.shape) == (0, 4) and int(rows.numel()) == 0


def test_every_gamma_one_equals_the_kmer_statistics_of_a_modified_reference(ctx):
    """40 aligned reads of both strands, gamma = 1 at every CG: the full mask of every window has weight 1, so the
    weighted statistics of the k-mers holding M are the plain statistics of a batch whose reference carries M at the
    sites.  Sample counts and event counts exactly; means and variances within 1e-10: the two sides sum the same
    samples in different orders, |x| <= about 6 after normalisation and at most 1e5 samples per k-mer, so either sum
    of n terms carries a relative rounding error of at most n * 2^-53 = 1e-11 on means and variances of order 1."""
    import torch
    from nadavca_amd import defaults, dtw, kmer_train, synthetic
    from nadavca_amd.batchflow import align_batch, load_config
    from nadavca_amd.call_mods import find_sites
    from nadavca_amd.device import mod_kmer_stats_dev
    from nadavca_amd.kmer_train import kmer_stats_dev
    from nadavca_amd.mod_train import holds_code
    from nadavca_amd.readbatch import contig_local_range
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    model5 = (k, central, 5, mean5, sigma5)
    km5 = dtw.KmerModel(*model5)
    rb, aligner, _, _ = synthetic.make_modified_read_batch(40, model5, seed=61, genome_length=3000, length=200,
                                                           spread=20, modified_fraction=1.0)
    res = align_batch(rb, load_config(defaults.CONFIG_FILE), km5, defaults.RENORM_ROUNDS, aligner)
    sa, dbatch = res.stage.sa, res.stage.dbatch
    assert bool(sa.reverse.any()) and not bool(sa.reverse.all())
    start, end = contig_local_range(sa, res.stage.reference)
    site_off, owner, pos, _, _ = find_sites(dbatch.reference, dbatch.ref_off, start, end, sa.reverse, [1, 2], 0, k,
                                            keep=res.status == 0, total_ref=dbatch.total_ref)
    assert int(pos.numel()) > 200
    gamma = torch.ones(int(pos.numel()), dtype=torch.float64, device=pos.device)
    context = km5.context
    stats = mod_kmer_stats_dev(context, dbatch, res.events, res.status, k, central, 5, 5, site_off, pos, gamma, 4,
                               torch.from_numpy(mean5).to(dbatch.device))
    assert stats['windows_skipped'] == 0 and stats['rows'] > 0      # (a 6-mer holds three CGs at most)
    key, sums = stats['key'].cpu().numpy(), stats['sums'].cpu().numpy()
    # the same batch with M written into the reference part
    marked = copy.copy(dbatch)
    marked.reference = dbatch.reference.clone()
    marked.reference[dbatch.ref_off[owner] + pos.to(torch.int64)] = 4
    S, N, e = (t.cpu().numpy() for t in kmer_stats_dev(context, marked, res.events, res.status, k, central, 5, 5))
    m = np.where(N > 0, S / np.maximum(N, 1), 0.0)
    Q = kmer_stats_dev(context, marked, res.events, res.status, k, central, 5, 5, level=m)[0].cpu().numpy()
    has_m = holds_code(k, 5, 4)
    Nw = np.zeros(5 ** k)
    Nw[key] = sums[:, 1]
    assert (N[has_m] > 0).sum() > 100
    assert np.array_equal(Nw[has_m], N[has_m].astype(np.float64))
    W = np.zeros(5 ** k)
    W[key] = sums[:, 0]
    assert np.array_equal(W[has_m], e[has_m].astype(np.float64))
    sel = sums[:, 1] > 0
    shift = sums[sel, 2] / sums[sel, 1]
    got_mean = mean5[key[sel]] + shift
    got_var = sums[sel, 3] / sums[sel, 1] - shift * shift
    err_mean = np.abs(got_mean - m[key[sel]]).max()
    err_var = np.abs(got_var - Q[key[sel]] / N[key[sel]]).max()
    print('k-mers %d, largest mean difference %.3e, variance difference %.3e' % (int(sel.sum()), err_mean, err_var))
    assert err_mean <= 1e-10 and err_var <= 1e-10


def _rows_call(lib, ctx, c, level, **kw):
    """nvk_mod_kmer_rows_dev on the constructed batch through ctypes; keyword arguments replace single arguments."""
    db = c['dbatch']
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = dict(n_reads=db.n, total_ref=db.total_ref, sig_off=db.sig_off, ref_off=db.ref_off, k=6, central=2, alphabet=5,
             trim=0, n_sites=int(c['d_site_pos'].numel()), site_off=c['d_site_off'], site_pos=c['d_site_pos'],
             site_gamma=c['d_site_gamma'], mod_code=4, level=level, n_rows=0, row_off=None, out_count=None,
             out_key=None, out_val=None)
    a.update(kw)
    skipped = C.c_int64(-1)
    rc = lib.nvk_mod_kmer_rows_dev(ctx.handle, a['n_reads'], a['total_ref'], dp(db.signal), dp(a['sig_off']),
                                   dp(c['d_events']), dp(a['ref_off']), dp(db.reference), dp(db.context_before),
                                   dp(db.cb_off), dp(db.context_after), dp(db.ca_off), dp(c['d_status']), a['k'],
                                   a['central'], a['alphabet'], a['trim'], a['n_sites'], dp(a['site_off']),
                                   dp(a['site_pos']), dp(a['site_gamma']), a['mod_code'], dp(a['level']), a['n_rows'],
                                   dp(a['row_off']), dp(a['out_count']), dp(a['out_key']), dp(a['out_val']),
                                   C.byref(skipped))
    return rc, skipped.value


def test_bad_arguments(ctx, constructed):
    import torch
    from nadavca_amd import _lib
    from nadavca_amd.device import mod_kmer_reduce_dev, mod_kmer_rows_dev
    lib = _lib.load()
    c = constructed
    db = c['dbatch']
    dev = db.device
    level = torch.zeros(5 ** 6, dtype=torch.float64, device=dev)
    count = torch.zeros(db.total_ref, dtype=torch.int64, device=dev)
    rc, skipped = _rows_call(lib, ctx, c, level, out_count=count)
    assert rc == _lib.NVK_OK and skipped > 0 and int(count.sum()) > 0
    key = torch.zeros(int(count.sum()), dtype=torch.int64, device=dev)
    val = torch.zeros((int(count.sum()), 4), dtype=torch.float64, device=dev)
    bad_ref = db.ref_off.clone()
    bad_ref[2] = bad_ref[3] + 1
    bad_site = c['d_site_off'].clone()
    bad_site[3] = bad_site[4] + 1
    short_site = c['d_site_off'].clone()
    short_site[-1] -= 1
    for kw in (dict(k=0), dict(k=17), dict(central=6), dict(central=-1), dict(alphabet=0), dict(trim=-1),
               dict(mod_code=5), dict(mod_code=-1), dict(n_sites=-1), dict(n_reads=-1),
               dict(total_ref=db.total_ref + 1),
               dict(ref_off=bad_ref), dict(site_off=bad_site), dict(site_off=short_site), dict(site_off=None),
               dict(site_pos=None), dict(out_count=None),
               dict(out_key=key), dict(out_val=val), dict(out_key=key, out_val=val, n_rows=int(key.numel())),
               dict(out_key=key, out_val=val, row_off=count, n_rows=-1)):
        kw = dict(dict(out_count=count), **kw)
        assert _rows_call(lib, ctx, c, level, **kw)[0] == _lib.NVK_ERR_INVALID, kw
    dp = lambda t: C.c_void_p(t.data_ptr())
    rows_val = torch.ones((10, 4), dtype=torch.float64, device=dev)
    sums = torch.zeros((2, 4), dtype=torch.float64, device=dev)
    n_out = torch.zeros(2, dtype=torch.int64, device=dev)
    off = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)
    reduce = lambda n_rows, n_keys, v, o: lib.nvk_mod_kmer_reduce_dev(ctx.handle, n_rows, n_keys, v, o, dp(sums),
                                                                      dp(n_out))
    assert reduce(10, 2, dp(rows_val), dp(off(2, 6, 10))) == _lib.NVK_OK
    for n_rows, n_keys, v, o in ((10, -1, dp(rows_val), dp(off(2, 6, 10))), (-1, 2, dp(rows_val), dp(off(2, 6, 10))),
                                 (10, 2, dp(rows_val), None), (10, 2, None, dp(off(2, 6, 10))),
                                 (10, 2, dp(rows_val), dp(off(2, 6, 9))), (10, 2, dp(rows_val), dp(off(2, 6, 11))),
                                 (10, 2, dp(rows_val), dp(off(6, 2, 10))), (10, 2, dp(rows_val), dp(off(-1, 6, 10))),
                                 (10, 2, dp(rows_val), dp(off(11, 11, 11)))):
        assert reduce(n_rows, n_keys, v, o) == _lib.NVK_ERR_INVALID
    assert lib.nvk_mod_kmer_reduce_dev(ctx.handle, 10, 2, dp(rows_val), dp(off(2, 6, 10)), None, None) == \
        _lib.NVK_ERR_INVALID
    # the wrappers
    args = lambda **kw: dict(dict(site_off=c['d_site_off'], site_pos=c['d_site_pos'], site_gamma=c['d_site_gamma'],
                                  level=level), **kw)
    gamma = c['d_site_gamma'].clone()
    pos = c['d_site_pos'].clone()
    cases = []
    for bad in (1.5, -0.25, float('nan'), float('inf')):
        g = gamma.clone()
        g[4] = bad
        cases.append(args(site_gamma=g))
    p = pos.clone()
    p[[5, 6]] = p[[6, 5]]                      # read 1: unsorted
    cases.append(args(site_pos=p))
    p = pos.clone()
    p[6] = p[5]                                # not strictly ascending
    cases.append(args(site_pos=p))
    p = pos.clone()
    p[2] = 5                                   # read 0 has 5 bases
    cases.append(args(site_pos=p))
    p = pos.clone()
    p[0] = -1
    cases.append(args(site_pos=p))
    cases.append(args(level=level[:-1]))
    cases.append(args(site_off=bad_site))
    for kw in cases:
        with pytest.raises(ValueError):
            mod_kmer_rows_dev(db, ctx, c['d_events'], c['d_status'], 6, 2, 5, 0, kw['site_off'], kw['site_pos'],
                              kw['site_gamma'], 4, kw['level'])
    with pytest.raises(ValueError):
        mod_kmer_rows_dev(db, ctx, c['d_events'], c['d_status'], 6, 6, 5, 0, c['d_site_off'], pos, gamma, 4, level)
    with pytest.raises(ValueError):
        mod_kmer_reduce_dev(ctx, rows_val, off(6, 2, 10))
    with pytest.raises(ValueError):
        mod_kmer_reduce_dev(ctx, rows_val[:, :3], off(2, 6, 10))


def test_row_off_that_disagrees_writes_nothing_out_of_range(ctx, constructed):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    c = constructed
    db = c['dbatch']
    dev = db.device
    level = torch.from_numpy(np.random.default_rng(2).normal(0.0, 1.0, 5 ** 6)).to(dev)
    count = torch.zeros(db.total_ref, dtype=torch.int64, device=dev)
    assert _rows_call(lib, ctx, c, level, out_count=count)[0] == _lib.NVK_OK
    row_off = torch.zeros(db.total_ref + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=row_off[1:])
    n_rows = int(row_off[-1])
    GUARD_KEY, GUARD_VAL, PAD = -77, -12345.5, 64

    def fill(off, n, buffer_rows):
        key = torch.full((buffer_rows + PAD,), GUARD_KEY, dtype=torch.int64, device=dev)
        val = torch.full((buffer_rows + PAD, 4), GUARD_VAL, dtype=torch.float64, device=dev)
        rc, _ = _rows_call(lib, ctx, c, level, n_rows=n, row_off=off, out_key=key, out_val=val)
        return rc, key.cpu().numpy(), val.cpu().numpy()

    rc, key, val = fill(row_off, n_rows, n_rows)
    assert rc == _lib.NVK_OK and (key[:n_rows] != GUARD_KEY).all()
    assert (key[n_rows:] == GUARD_KEY).all() and (val[n_rows:] == GUARD_VAL).all()
    good_key, good_val = key[:n_rows], val[:n_rows]
    # one base is given a row too few: its rows are not written, every other base's are, nothing beyond the end
    base = int(torch.nonzero(count == 3)[0])
    narrow = count.clone()
    narrow[base] = 2
    off2 = torch.zeros_like(row_off)
    torch.cumsum(narrow, 0, out=off2[1:])
    rc, key, val = fill(off2, n_rows - 1, n_rows - 1)
    assert rc == _lib.NVK_ERR_INVALID and b'row_off' in lib.nvk_last_error()
    at = int(off2[base])
    assert (key[at:at + 2] == GUARD_KEY).all() and (val[at:at + 2] == GUARD_VAL).all()
    assert np.array_equal(key[:at], good_key[:at]) and np.array_equal(key[at + 2:n_rows - 1], good_key[at + 3:])
    assert np.array_equal(_bits(val[at + 2:n_rows - 1]), _bits(good_val[at + 3:]))
    assert (key[n_rows - 1:] == GUARD_KEY).all() and (val[n_rows - 1:] == GUARD_VAL).all()
    # offsets that run past n_rows: the last read's buffer ends early, nothing is written behind it
    cut = n_rows - int(count[db.total_ref - 60:].sum())
    assert 0 < cut < n_rows
    rc, key, val = fill(row_off, cut, cut)
    assert rc == _lib.NVK_ERR_INVALID
    assert np.array_equal(key[:cut], good_key[:cut]) and np.array_equal(_bits(val[:cut]), _bits(good_val[:cut]))
    assert (key[cut:] == GUARD_KEY).all() and (val[cut:] == GUARD_VAL).all()
    # negative offsets
    rc, key, val = fill(row_off - 5, n_rows, n_rows)
    assert rc == _lib.NVK_ERR_INVALID and (key[n_rows:] == GUARD_KEY).all()
    # and a later correct call is served as before
    rc, key, val = fill(row_off, n_rows, n_rows)
    assert rc == _lib.NVK_OK and np.array_equal(key[:n_rows], good_key) and np.array_equal(_bits(val[:n_rows]),
                                                                                          _bits(good_val))
