"""GPU tests of the allele-mixture kernels (csrc/kernels_allele.hip) on random log-likelihood rows, no DP: the rows and
keys of nvk_allele_rows_dev bit for bit, the per-position solve of nvk_allele_solve_dev against the numpy restatement
(tests/allele_ref.py) with the tolerances of ``allele_ref.check_against``, the same bits on a second call, and the
invalid-argument returns."""
import ctypes as C
import types

import numpy as np
import pytest

import allele_ref
import read_rows_case

pytestmark = pytest.mark.gpu

REF_LEN = 120
CACHED_ROWS = 128     # positions of up to this many rows keep exp(-|d|) in registers (mix_mle.h: 64 * MIX_CACHE)


def build_case(alpha, seed):
    """About 330 reads of 5 .. 40 bases on a 120-base reference, both strands: positions 2 .. 4 and 30 .. 39 without a
    read, 5 .. 9 under one, 10 .. 14 under two, 15 .. 19 / 20 .. 24 / 25 .. 29 under 63 / 64 / 65, position 60 under
    more than 128; reads with status != 0, one with a shift that is not finite, one starting before the reference and
    one running past its end."""
    rng = np.random.default_rng(seed)
    ref_codes = rng.integers(0, alpha, REF_LEN).astype(np.int32)
    reads = []                                    # (start, length, status)
    for first, count in ((5, 1), (10, 2), (15, 63), (20, 64), (25, 65)):
        reads += [(first, 5, 0)] * count
    for _ in range(CACHED_ROWS + 7):
        length = int(rng.integers(5, 41))
        reads.append((int(rng.integers(max(40, 60 - length + 1), min(60, 95 - length) + 1)), length, 0))
    reads += [(15, 10, 1), (50, 30, -3), (8, 12, 1)]          # not OK: they count nowhere
    bad_shift = len(reads)
    reads.append((55, 12, 0))
    reads += [(-3, 5, 0), (110, 20, 0)]
    order = rng.permutation(len(reads))
    bad_shift = int(np.nonzero(order == bad_shift)[0][0])
    reads = [reads[i] for i in order]
    n = len(reads)
    start = np.array([r[0] for r in reads], dtype=np.int64)
    length = np.array([r[1] for r in reads], dtype=np.int64)
    status = np.array([r[2] for r in reads], dtype=np.int32)
    reverse = (rng.random(n) < 0.5).astype(np.int32)
    ref_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    total = int(ref_off[-1])
    reference = np.zeros(total, dtype=np.int32)
    ll = rng.normal(-30.0, 12.0, (total, alpha))
    for i in range(n):
        pos = np.clip(start[i] + np.arange(length[i]), 0, REF_LEN - 1)   # (outside: any base)
        part = ref_codes[pos]
        reference[ref_off[i]:ref_off[i + 1]] = (alpha - 1 - part)[::-1] if reverse[i] else part
    r0 = ref_off[bad_shift]
    ll[r0, reference[r0]] = -np.inf

    def set_column(P, b, values):
        """d of the covering reads of (P, forward base b), in read order, becomes ``values`` (before the division)."""
        j = 0
        for i in range(n):
            if not start[i] <= P < start[i] + length[i]:
                continue
            p = start[i] + length[i] - 1 - P if reverse[i] else P - start[i]
            c = alpha - 1 - b if reverse[i] else b
            a = ref_off[i]
            ll[a + p, c] = ll[a, reference[a]] + values[j % len(values)]
            j += 1

    alts = lambda P: [b for b in range(alpha) if b != ref_codes[P]]
    set_column(17, alts(17)[0], [-np.inf])
    set_column(17, alts(17)[1], [600.0, -600.0, 3.0, -np.inf])
    set_column(22, alts(22)[0], -np.abs(rng.normal(0, 8, 64)) - 1e-3)
    set_column(22, alts(22)[1], rng.normal(0, 1e-4, 64))
    set_column(27, alts(27)[0], np.abs(rng.normal(0, 8, 65)) + 1e-3)
    set_column(27, alts(27)[1], np.where(rng.random(65) < 0.3, 289.0, -35.0) + rng.normal(0, 2, 65))
    set_column(60, alts(60)[0], np.where(rng.random(200) < 0.4, 600.0, -600.0))
    set_column(60, alts(60)[1], np.abs(rng.normal(0, 5, 200)) + 1e-3)
    set_column(60, alts(60)[2], -np.abs(rng.normal(0, 5, 200)) - 1e-3)
    set_column(12, alts(12)[0], [600.0, -600.0])
    set_column(12, alts(12)[1], [-np.inf, 2.0])
    set_column(7, alts(7)[0], [4.0])
    set_column(7, alts(7)[1], [0.0])
    return dict(alpha=alpha, ref_codes=ref_codes, start=start, reverse=reverse, status=status, ref_off=ref_off,
                reference=reference, ll=ll, n=n, total=total)


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def on_device(case, ctx):
    import torch
    dev = torch.device('cuda', ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dbatch = types.SimpleNamespace(torch=torch, device=dev, n=case['n'], total_ref=case['total'],
                                   reference=up(case['reference']), ref_off=up(case['ref_off']))
    return dbatch, up(case['ll']), up(case['start']), up(case['reverse']), up(case['status']), up(case['ref_codes'])


@pytest.mark.parametrize('alpha,event_length', [(4, 1.0), (5, 2.5)])
def test_kernels_against_the_restatement(ctx, alpha, event_length):
    from nadavca_amd import device
    case = build_case(alpha, 100 + alpha)
    dbatch, ll, start, reverse, status, codes = on_device(case, ctx)
    want_key, want_val = allele_ref.rows(case['ll'], case['reference'], case['ref_off'], case['start'],
                                         case['reverse'], case['status'], event_length, REF_LEN)
    key, val = device.allele_rows_dev(ctx, dbatch, ll, start, reverse, status, event_length, REF_LEN)
    assert np.array_equal(key.cpu().numpy(), want_key)
    assert np.array_equal(val.cpu().numpy(), want_val)          # a rounded subtraction and division: the same bits
    P, b, D, valid, coverage = allele_ref.sites(want_key, want_val, case['ref_codes'])
    for c in (0, 1, 2, 63, 64, 65):
        assert (coverage == c).any(), c
    assert coverage[60] > CACHED_ROWS and coverage[2] == 0 and coverage[119] == 1 and coverage[0] == 1
    ref = allele_ref.solve(D, valid)
    got = [t.cpu().numpy() for t in device.allele_fractions_dev(ctx, dbatch, ll, start, reverse, status, event_length,
                                                                codes)]
    fraction, lrt, half, full, cov = got
    assert np.array_equal(cov, coverage)
    counts = allele_ref.check_against(ref, fraction[P, b], lrt[P, b], half[P, b], full[P, b], D, valid,
                                      'alphabet %d' % alpha)
    print('alphabet %d: %d (position, base) pairs; fraction surely 0 / 1 / inside: %d / %d / %d; sharp optima: %d'
          % ((alpha, P.size) + counts))
    assert min(counts) >= 3
    # the reference base's column and the positions without a read hold zeros
    rest = np.ones((REF_LEN, alpha), dtype=bool)
    rest[P, b] = False
    for a in (fraction, lrt, half, full):
        assert (a[rest] == 0).all()
    # the planted columns: all -inf and all negative -> 0, all positive -> 1 (the uncached path at position 60 too)
    alts = lambda p: [x for x in range(alpha) if x != case['ref_codes'][p]]
    assert fraction[17, alts(17)[0]] == 0 and full[17, alts(17)[0]] == -np.inf and lrt[17, alts(17)[0]] == 0
    assert fraction[22, alts(22)[0]] == 0 and fraction[27, alts(27)[0]] == 1
    assert fraction[60, alts(60)[1]] == 1 and fraction[60, alts(60)[2]] == 0
    assert 0.2 < fraction[60, alts(60)[0]] < 0.6 and 0.1 < fraction[27, alts(27)[1]] < 0.5
    assert fraction[7, alts(7)[0]] == 1 and abs(lrt[7, alts(7)[0]] - 2 * (4.0 / event_length)) < 1e-9
    assert fraction[7, alts(7)[1]] == 0
    # a second call returns the same bits
    again = [t.cpu().numpy() for t in device.allele_fractions_dev(ctx, dbatch, ll, start, reverse, status,
                                                                  event_length, codes)]
    for x, y in zip(got, again):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize('with_status', [True, False])
def test_rows_on_the_read_view_shapes(ctx, with_status):
    """The batch of read_rows_case.py: reads without bases (the last read among them), a dead read between live ones,
    reads off either end of the reference, a read count that leaves a block part empty."""
    from nadavca_amd import device
    case = read_rows_case.build()
    dbatch, ll, start, reverse, status, _ = on_device(case, ctx)
    st = case['status'] if with_status else None
    want_key, want_val = allele_ref.rows(case['ll'], case['reference'], case['ref_off'], case['start'],
                                         case['reverse'], st, 2.5, read_rows_case.REF_LEN)
    key, val = device.allele_rows_dev(ctx, dbatch, ll, start, reverse, status if with_status else None, 2.5,
                                      read_rows_case.REF_LEN)
    key = key.cpu().numpy()
    assert np.array_equal(key, want_key) and np.array_equal(val.cpu().numpy(), want_val)
    off = case['ref_off']
    assert (key[off[1]:off[2]] >= 0).any() == (not with_status)          # the dead read between two live ones
    assert (key[off[0]:off[1]] >= 0).all() and (key[off[2]:off[3]] >= 0).all()
    assert (key[off[6]:off[7]] < 0).sum() == 3 and (key[off[9]:off[10]] < 0).sum() == 50    # off either end


@pytest.mark.parametrize('alpha', [2, 4, 8])
def test_solve_at_the_edges_of_the_cached_rows(ctx, alpha):
    """Positions of 0, 1, 64, 128, 129 and 200 rows (64: one row per lane; 128: the last size whose rows stay in
    registers).  At every position the first alternative base has its maximum inside (0, 1), so it is bisected, while
    the others, all negative, end after the first sweep."""
    import torch
    from nadavca_amd import device
    rng = np.random.default_rng(60 + alpha)
    sizes = [0, 1, 64, CACHED_ROWS, CACHED_ROWS + 1, 200]
    key = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    ref_codes = rng.integers(0, alpha, len(sizes)).astype(np.int32)
    val = -np.abs(rng.normal(0.0, 6.0, (key.size, alpha))) - 1e-3
    first_alt = np.where(ref_codes == 0, 1, 0)
    sign = np.where(rng.random(key.size) < 0.4, 1.0, -1.0)
    val[np.arange(key.size), first_alt[key]] = sign * rng.normal(6.0, 2.0, key.size)
    val[0, first_alt[1]] = 4.0                                # the single row, of position 1: f^ = 1
    dev = torch.device('cuda', ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = [t.cpu().numpy() for t in device.allele_solve_dev(ctx, up(key), up(val), up(ref_codes))]
    fraction, lrt, half, full, cov = got
    assert cov.tolist() == sizes
    P, b, D, valid, coverage = allele_ref.sites(key, val, ref_codes)
    allele_ref.check_against(allele_ref.solve(D, valid), fraction[P, b], lrt[P, b], half[P, b], full[P, b], D, valid,
                             'alphabet %d, edge sizes' % alpha)
    for p in range(2, len(sizes)):
        assert 0.0 < fraction[p, first_alt[p]] < 1.0, p
        rest = [a for a in range(alpha) if a != ref_codes[p] and a != first_alt[p]]
        assert (fraction[p, rest] == 0).all() and (lrt[p, rest] == 0).all(), p
    assert fraction[1, first_alt[1]] == 1.0 and (fraction[0] == 0).all()
    again = [t.cpu().numpy() for t in device.allele_solve_dev(ctx, up(key), up(val), up(ref_codes))]
    for x, y in zip(got, again):
        assert np.array_equal(x, y, equal_nan=True)


def test_no_status_and_unsorted_tail(ctx):
    """status NULL counts every read; keys at or beyond ref_len and negative keys are skipped by the solve."""
    import torch
    from nadavca_amd import device
    case = build_case(4, 7)
    dbatch, ll, start, reverse, status, codes = on_device(case, ctx)
    key, val = device.allele_rows_dev(ctx, dbatch, ll, start, reverse, None, 1.0, REF_LEN)
    want_key, want_val = allele_ref.rows(case['ll'], case['reference'], case['ref_off'], case['start'],
                                         case['reverse'], None, 1.0, REF_LEN)
    assert np.array_equal(key.cpu().numpy(), want_key) and np.array_equal(val.cpu().numpy(), want_val)
    # the same rows solved against a SHORTER reference: the rows of positions >= 50 are skipped
    skey, order = torch.sort(key, stable=True)
    out = device.allele_solve_dev(ctx, skey, val[order], codes[:50].contiguous())
    full_out = device.allele_solve_dev(ctx, skey, val[order], codes)
    for a, b in zip(out, full_out):
        assert torch.equal(a, b[:50])


def test_c_abi_rejects_bad_arguments(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    ll = torch.zeros((30, 4), dtype=torch.float64, device=dev)
    reference = torch.zeros(30, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 10, 30], dtype=torch.int64, device=dev)
    start = torch.zeros(2, dtype=torch.int64, device=dev)
    rev = torch.zeros(2, dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    key = torch.zeros(30, dtype=torch.int64, device=dev)
    val = torch.zeros((30, 4), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def rows(c=None, n=2, total=30, alpha=4, ll_=ll, ref_=reference, off_=off, start_=start, rev_=rev, st_=st,
             el=1.0, ref_len=40, key_=key, val_=val):
        return lib.nvk_allele_rows_dev(ctx.handle if c is None else c, n, total, alpha, p(ll_), p(ref_), p(off_),
                                       p(start_), p(rev_), p(st_), el, ref_len, p(key_), p(val_))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert rows() == _lib.NVK_OK
    assert rows(st_=None) == _lib.NVK_OK
    assert rows(n=0, total=0, ll_=None, ref_=None, off_=None, key_=None, val_=None) == _lib.NVK_OK
    assert rows(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(alpha=1), dict(alpha=9), dict(el=0.0), dict(el=-1.0), dict(el=float('nan')),
               dict(el=float('inf')), dict(ref_len=-1), dict(n=-1), dict(total=-1), dict(n=0), dict(total=29),
               dict(ll_=None), dict(ref_=None), dict(off_=None), dict(start_=None), dict(rev_=None), dict(key_=None),
               dict(val_=None), dict(off_=torch.tensor([0, 31, 30], dtype=torch.int64, device=dev)),
               dict(off_=torch.tensor([1, 10, 30], dtype=torch.int64, device=dev))):
        assert invalid(rows(**kw)), kw
    codes = torch.zeros(40, dtype=torch.int32, device=dev)
    outs = [torch.zeros((40, 4), dtype=torch.float64, device=dev) for _ in range(4)]
    cov = torch.zeros(40, dtype=torch.int64, device=dev)

    def solve(c=None, n_rows=30, ref_len=40, alpha=4, key_=key, val_=val, codes_=codes, outs_=outs, cov_=cov):
        return lib.nvk_allele_solve_dev(ctx.handle if c is None else c, n_rows, ref_len, alpha, p(key_), p(val_),
                                        p(codes_), *[p(t) for t in outs_], p(cov_))

    assert solve() == _lib.NVK_OK
    assert solve(n_rows=0, key_=None, val_=None) == _lib.NVK_OK and int(cov.sum()) == 0
    assert solve(ref_len=0, codes_=None, outs_=[None] * 4, cov_=None) == _lib.NVK_OK
    assert solve(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(alpha=1), dict(alpha=9), dict(n_rows=-1), dict(ref_len=-1), dict(key_=None), dict(val_=None),
               dict(codes_=None), dict(cov_=None), dict(outs_=[None] + outs[1:]), dict(outs_=outs[:3] + [None])):
        assert invalid(solve(**kw)), kw
