"""GPU tests of the site-level kernels (csrc/kernels_sitelevels.hip) on constructed reads, no DP: the keys and values of
nvk_site_level_rows_dev and the moments of nvk_site_moments_dev bit for bit against the numpy restatement
(tests/site_levels_ref.py), the same bits on a second call, and the invalid-argument returns."""
import ctypes as C
import types

import numpy as np
import pytest

import read_rows_case
import site_levels_ref

pytestmark = pytest.mark.gpu

REF_LEN = 150
EVENT_LENGTHS = (1, 7, 8, 9, 127, 128, 129, 300)     # 8 and 128 samples are numpy's block edges


def build_case(seed):
    """About 40 reads of 4 (shorter than 2 * trim), 5, 63, 64, 65 and 70 bases on both strands of a 150-base reference,
    two with status 1 and -3, one starting before position 0 and one running past the end.  Events are 2 .. 12 samples
    long, laid end to end from a random start; every read of 63 bases or more also holds an empty event, one starting
    below 0, one ending past the window, and events of every length of EVENT_LENGTHS."""
    rng = np.random.default_rng(seed)
    reads = []                                   # (start, bases, status)
    for R in (4, 5, 63, 64, 65, 70):
        for _ in range(6):
            reads.append((int(rng.integers(0, REF_LEN - R)), R, 0))
    reads += [(20, 64, 1), (40, 70, -3), (-3, 65, 0), (REF_LEN - 20, 63, 0)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    n = len(reads)
    start = np.array([r[0] for r in reads], dtype=np.int64)
    R = np.array([r[1] for r in reads], dtype=np.int64)
    status = np.array([r[2] for r in reads], dtype=np.int32)
    reverse = (np.arange(n) % 2).astype(np.int32)
    ref_off = np.concatenate([[0], np.cumsum(R)]).astype(np.int64)
    events, signals = [], []
    for j in range(n):
        length = rng.integers(2, 13, R[j])
        if R[j] >= 63:
            at = rng.permutation(np.arange(12, R[j] - 8))[:len(EVENT_LENGTHS)]
            length[at] = EVENT_LENGTHS
            length[8] = 0                         # an empty event
        first = int(rng.integers(0, 30))
        bounds = first + np.concatenate([[0], np.cumsum(length)])
        ev = np.stack([bounds[:-1], bounds[1:]], 1).astype(np.int32)
        N = int(bounds[-1]) + int(rng.integers(0, 20))
        if R[j] >= 63:
            ev[9] = (-5, ev[9][1])                # start < 0: clamped to 0 (a long event)
            ev[R[j] - 7] = (ev[R[j] - 7][0], N + 40)   # end > N: clamped to N
            ev[10] = (N + 3, N + 9)               # wholly past the window: empty after clamping
        events.append(ev)
        signals.append(rng.normal(0.0, 1.0, N) * rng.choice([1.0, 1e-3, 50.0]) + rng.normal(0.0, 2.0))
    sig_off = np.concatenate([[0], np.cumsum([s.size for s in signals])]).astype(np.int64)
    events = np.concatenate(events)
    return dict(n=n, total=int(ref_off[-1]), start=start, reverse=reverse, status=status, ref_off=ref_off,
                sig_off=sig_off, signal=np.concatenate(signals), events=events,
                expected=rng.normal(0.0, 1.0, int(ref_off[-1])))


def same_bits(a, b):
    """Equal bit for bit, the sign of a zero included; a NaN equals a NaN whatever its payload."""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope='module')
def case():
    return build_case(12)


def on_device(case, ctx):
    import torch
    dev = torch.device('cuda', ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dbatch = types.SimpleNamespace(torch=torch, device=dev, n=case['n'], total_ref=case['total'],
                                   signal=up(case['signal']), sig_off=up(case['sig_off']), ref_off=up(case['ref_off']))
    return dbatch, up(case['events']), up(case['expected']), up(case['start']), up(case['reverse']), up(case['status'])


def want_rows(case, status, trim):
    return site_levels_ref.rows(case['signal'], case['sig_off'], case['events'], case['ref_off'], case['expected'],
                                case['start'], case['reverse'], status, trim, REF_LEN)


@pytest.mark.parametrize('trim,with_status', [(0, True), (3, True), (3, False)])
def test_rows_against_the_restatement(ctx, case, trim, with_status):
    from nadavca_amd import device
    dbatch, events, expected, start, reverse, status = on_device(case, ctx)
    want_key, want_val = want_rows(case, case['status'] if with_status else None, trim)
    key, val = device.site_level_rows_dev(ctx, dbatch, events, expected, start, reverse,
                                          status if with_status else None, trim, REF_LEN)
    key, val = key.cpu().numpy(), val.cpu().numpy()
    assert np.array_equal(key, want_key)
    assert same_bits(val, want_val)
    # what the case is meant to hold is there
    counted = key >= 0
    dwell = val[counted, 2]
    for length in EVENT_LENGTHS:
        assert (dwell == length).any(), length
    assert dwell.max() >= 300 and set(key[counted] & 1) == {0, 1}
    assert key[counted].min() >= 0 and key[counted].max() < 2 * REF_LEN
    assert (val[~counted] == 0).all() and (~counted).sum() > (30 if trim == 0 else 100)
    R = np.diff(case['ref_off'])
    for j in np.nonzero(R < 2 * trim)[0]:
        assert not counted[case['ref_off'][j]:case['ref_off'][j + 1]].any()
    live = np.repeat(case['status'] == 0, R)
    assert counted[~live].any() == (not with_status)
    # level equals event_means_dev's bits wherever both are defined
    means = device.event_means_dev(dbatch, ctx, events, status if with_status else None).cpu().numpy()
    assert np.array_equal(val[counted, 0], means[counted]) and counted.sum() > 1000
    # a second call gives the same bits
    key2, val2 = device.site_level_rows_dev(ctx, dbatch, events, expected, start, reverse,
                                            status if with_status else None, trim, REF_LEN)
    assert np.array_equal(key2.cpu().numpy(), key) and same_bits(val2.cpu().numpy(), val)


@pytest.mark.parametrize('trim,with_status', [(0, True), (read_rows_case.TRIM, True), (0, False)])
def test_rows_on_the_read_view_shapes(ctx, trim, with_status):
    """The batch of read_rows_case.py: reads without bases or samples, a dead read between live ones, trim beyond half a
    read, every clamp of an event, events around 128 samples, a read count that leaves a block part empty."""
    from nadavca_amd import device
    case = read_rows_case.build()
    dbatch, events, expected, start, reverse, status = on_device(case, ctx)
    want_key, want_val = site_levels_ref.rows(case['signal'], case['sig_off'], case['events'], case['ref_off'],
                                              case['expected'], case['start'], case['reverse'],
                                              case['status'] if with_status else None, trim, read_rows_case.REF_LEN)
    key, val = device.site_level_rows_dev(ctx, dbatch, events, expected, start, reverse,
                                          status if with_status else None, trim, read_rows_case.REF_LEN)
    key, val = key.cpu().numpy(), val.cpu().numpy()
    assert np.array_equal(key, want_key)
    assert same_bits(val, want_val)
    counted = key >= 0
    for length in read_rows_case.EVENT_LENGTHS:
        assert (val[counted, 2] == length).any(), length
    off = case['ref_off']
    assert not counted[off[4]:off[5]].any()                              # the read without samples
    assert counted[off[1]:off[2]].any() == (not with_status)             # the dead read between two live ones
    assert counted[off[0]:off[1]].any() and counted[off[2]:off[3]].any()
    assert counted[off[5]:off[6]].any() == (trim == 0)


def test_site_levels_dev_is_rows_sort_moments(ctx, case):
    from nadavca_amd import device
    dbatch, events, expected, start, reverse, status = on_device(case, ctx)
    want_key, want_val = want_rows(case, case['status'], 3)
    want = site_levels_ref.site_levels(want_key, want_val, 2 * REF_LEN)
    count, mean, m2, key, val = device.site_levels_dev(ctx, dbatch, events, expected, start, reverse, status, 3,
                                                       REF_LEN)
    assert np.array_equal(key.cpu().numpy(), want_key) and np.array_equal(val.cpu().numpy(), want_val)
    for got, exp in zip((count, mean, m2), want):
        assert np.array_equal(got.cpu().numpy(), exp)
    assert want[0].max() >= 5 and (want[0] == 0).any()


def moment_rows(n_val, seed):
    """Keys with 0, 1, 2, 63, 64, 65 and 130 rows among others, negative keys and keys >= n_keys, a NaN in one column
    of the key with 130 rows (where n_val > 1; of the key with 65 rows otherwise), in random row order."""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, 63, 64, 65, 130, 0, 9, 200]
    key = np.concatenate([np.full(c, q) for q, c in enumerate(counts)]
                         + [np.full(6, -1), np.full(3, -7), np.full(5, len(counts)), np.full(2, len(counts) + 40)])
    val = rng.normal(0.5, 3.0, (key.size, n_val)) * rng.choice([1.0, 1e-6, 1e4], (1, n_val))
    order = rng.permutation(key.size)
    key, val = key[order], val[order]
    nan_key, nan_col = (6, 1) if n_val > 1 else (5, 0)
    val[np.nonzero(key == nan_key)[0][40], nan_col] = np.nan
    return key.astype(np.int64), val, counts, nan_key, nan_col


@pytest.mark.parametrize('n_val', [1, 4, 8])
def test_moments_against_the_restatement(ctx, n_val):
    import torch
    from nadavca_amd import device
    key, val, counts, nan_key, nan_col = moment_rows(n_val, 40 + n_val)
    dev = torch.device('cuda', ctx.device)
    order = np.argsort(key, kind='stable')
    skey, sval = torch.from_numpy(key[order]).to(dev), torch.from_numpy(val[order]).to(dev)
    want = site_levels_ref.moments(key[order], val[order], len(counts))
    got = [t.cpu().numpy() for t in device.site_moments_dev(ctx, skey, sval, len(counts))]
    assert got[0].tolist() == counts
    for g, w in zip(got[1:], want[1:]):
        assert g.shape == (len(counts), n_val)
        assert same_bits(g, w)
    nan = np.zeros((len(counts), n_val), dtype=bool)
    nan[nan_key, nan_col] = True
    assert np.array_equal(np.isnan(got[1]), nan) and np.array_equal(np.isnan(got[2]), nan)
    assert (got[1][[0, 7]] == 0).all() and (got[2][[0, 7]] == 0).all() and (got[2][1] == 0).all()
    again = [t.cpu().numpy() for t in device.site_moments_dev(ctx, skey, sval, len(counts))]
    for g, a in zip(got, again):
        assert np.array_equal(g, a, equal_nan=True)
    # fewer keys than the rows hold: the rest is skipped
    short = [t.cpu().numpy() for t in device.site_moments_dev(ctx, skey, sval, 5)]
    for g, s in zip(got, short):
        assert np.array_equal(g[:5], s, equal_nan=True)


def test_c_abi_rejects_bad_arguments(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    signal = torch.zeros(100, dtype=torch.float64, device=dev)
    sig_off = torch.tensor([0, 40, 100], dtype=torch.int64, device=dev)
    events = torch.zeros((30, 2), dtype=torch.int32, device=dev)
    off = torch.tensor([0, 10, 30], dtype=torch.int64, device=dev)
    expected = torch.zeros(30, dtype=torch.float64, device=dev)
    start = torch.zeros(2, dtype=torch.int64, device=dev)
    rev = torch.zeros(2, dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    key = torch.zeros(30, dtype=torch.int64, device=dev)
    val = torch.zeros((30, 4), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    bad = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)

    def rows(c=None, n=2, total=30, sig_=signal, so_=sig_off, ev_=events, off_=off, exp_=expected, start_=start,
             rev_=rev, st_=st, trim=0, ref_len=40, key_=key, val_=val):
        return lib.nvk_site_level_rows_dev(ctx.handle if c is None else c, n, total, p(sig_), p(so_), p(ev_), p(off_),
                                           p(exp_), p(start_), p(rev_), p(st_), trim, ref_len, p(key_), p(val_))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert rows() == _lib.NVK_OK and int((key >= 0).sum()) == 0          # every event is empty
    assert rows(st_=None) == _lib.NVK_OK
    assert rows(ref_len=0) == _lib.NVK_OK and rows(ref_len=1 << 61) == _lib.NVK_OK and rows(trim=1 << 20) == _lib.NVK_OK
    assert rows(sig_=None, so_=bad(0, 0, 0)) == _lib.NVK_OK              # no samples: the signal may be NULL
    assert rows(n=0, total=0, sig_=None, so_=None, ev_=None, off_=None, exp_=None, start_=None, rev_=None, key_=None,
                val_=None) == _lib.NVK_OK
    assert rows(total=0, off_=bad(0, 0, 0), ev_=None, exp_=None, key_=None, val_=None) == _lib.NVK_OK
    assert rows(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(trim=-1), dict(ref_len=-1), dict(ref_len=(1 << 61) + 1), dict(n=-1), dict(total=-1), dict(n=0),
               dict(total=29), dict(sig_=None), dict(so_=None), dict(ev_=None), dict(off_=None), dict(exp_=None),
               dict(start_=None), dict(rev_=None), dict(key_=None), dict(val_=None), dict(off_=bad(0, 31, 30)),
               dict(off_=bad(1, 10, 30)), dict(so_=bad(0, 101, 100)), dict(so_=bad(2, 40, 100))):
        assert invalid(rows(**kw)), kw
    count = torch.zeros(12, dtype=torch.int64, device=dev)
    mean = torch.zeros((12, 4), dtype=torch.float64, device=dev)
    m2 = torch.zeros((12, 4), dtype=torch.float64, device=dev)

    def moments(c=None, n_rows=30, n_keys=12, n_val=4, key_=key, val_=val, count_=count, mean_=mean, m2_=m2):
        return lib.nvk_site_moments_dev(ctx.handle if c is None else c, n_rows, n_keys, n_val, p(key_), p(val_),
                                        p(count_), p(mean_), p(m2_))

    assert moments() == _lib.NVK_OK and count.tolist() == [0] * 12       # (the rows call above wrote key = -1)
    assert moments(n_rows=0, key_=None, val_=None) == _lib.NVK_OK and int(count.sum()) == 0
    assert moments(n_keys=0, count_=None, mean_=None, m2_=None) == _lib.NVK_OK
    assert moments(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(n_val=0), dict(n_val=9), dict(n_rows=-1), dict(n_keys=-1), dict(key_=None), dict(val_=None),
               dict(count_=None), dict(mean_=None), dict(m2_=None)):
        assert invalid(moments(**kw)), kw
