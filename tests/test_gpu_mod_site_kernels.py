"""nvk_mod_site_solve_dev on the GPU against its numpy restatement (tests/mod_sites_ref.py), with the tolerances of
``allele_ref.check_against`` and the counts exact.  The sites have 0, 1, 2, 63, 64, 65, 128, 129, 130 and 300 rows: the
partial-sum boundary at 64 and the boundary of the rows the kernel keeps in registers, 64 * MIX_CACHE = 128, from both
sides."""
import ctypes as C

import numpy as np
import pytest

import allele_ref
import mod_sites_ref

pytestmark = pytest.mark.gpu

CLIP = 30.0
CACHED_ROWS = 128          # 64 * MIX_CACHE of csrc/mix_mle.h
SIZES = [0, 1, 2, 63, 64, 65, 128, 129, 130, 300, 40, 40, 12, 70, 200]
ALL_POSITIVE, ALL_NEGATIVE, SPECIAL, MIXED_LONG, SPECIAL_LONG = 10, 11, 12, 13, 14


def build_case(seed):
    """Rows of ratios +-N(6, 2.5^2) with a share of modified rows that differs per group, groups 0 .. 2 mixed with a
    few rows outside 0 .. 31; one site all positive, one all negative, two with the special values."""
    rng = np.random.default_rng(seed)
    lo = np.concatenate([[0], np.cumsum(SIZES)[:-1]]).astype(np.int64)
    hi = np.cumsum(SIZES).astype(np.int64)
    n = int(hi[-1])
    group = rng.choice([0, 1, 2], n, p=[0.3, 0.35, 0.35]).astype(np.int32)
    share = np.array([0.5, 0.85, 0.2])[group]
    val = np.where(rng.random(n) < share, 1.0, -1.0) * rng.normal(6.0, 2.5, n)
    odd = rng.random(n) < 0.03
    group[odd] = rng.choice([-1, 32, 33, -7, 1 << 20], int(odd.sum()))
    val[lo[ALL_POSITIVE]:hi[ALL_POSITIVE]] = np.abs(val[lo[ALL_POSITIVE]:hi[ALL_POSITIVE]]) + 0.5
    val[lo[ALL_NEGATIVE]:hi[ALL_NEGATIVE]] = -np.abs(val[lo[ALL_NEGATIVE]:hi[ALL_NEGATIVE]]) - 0.5
    special = np.array([0.0, -0.0, 1e-300, -1e-300, CLIP, -CLIP, np.inf, -np.inf, np.nan, 2.0 * CLIP, -2.0 * CLIP, 3.5])
    val[lo[SPECIAL]:hi[SPECIAL]] = special
    group[lo[SPECIAL]:hi[SPECIAL]] = [1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 0]
    at = lo[SPECIAL_LONG] + rng.choice(SIZES[SPECIAL_LONG], 5 * special.size, replace=False)   # beyond the registers
    val[at] = np.tile(special, 5)
    return lo, hi, val, group


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def on_device(ctx, *arrays):
    import torch
    dev = torch.device('cuda', ctx.device)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def solve_and_check(ctx, lo, hi, val, group, masks, label):
    from nadavca_amd import device
    d_lo, d_hi, d_val, d_group = on_device(ctx, lo, hi, val, group)
    got = [t.cpu().numpy() for t in device.mod_site_solve_dev(ctx, d_lo, d_hi, d_val, d_group, masks, CLIP)]
    count, fraction, ll = got
    assert count.shape == fraction.shape == ll.shape == (len(lo), len(masks))
    assert count.dtype == np.int64 and fraction.dtype == np.float64 and ll.dtype == np.float64
    r_count, r_fraction, r_ll, ref, D, valid = mod_sites_ref.solve(lo, hi, val, group, masks, CLIP, full=True)
    assert np.array_equal(count, r_count), label
    # ll_half and ll_full are not outputs of this operator: the restatement's own values stand in
    counts = allele_ref.check_against(ref, fraction.reshape(-1), 2.0 * ll.reshape(-1), ref['ll_half'], ref['ll_full'],
                                      D, valid, label)
    assert (ll[fraction == 0] == 0).all() and (ll[count == 0] == 0).all() and (fraction[count == 0] == 0).all()
    again = [t.cpu().numpy() for t in device.mod_site_solve_dev(ctx, d_lo, d_hi, d_val, d_group, masks, CLIP)]
    for a, b in zip(got, again):
        assert np.array_equal(a, b), label + ': a second call gave other bits'
    return count, fraction, ll, counts


def test_the_four_sets_against_the_restatement(ctx):
    lo, hi, val, group = build_case(41)
    count, fraction, ll, counts = solve_and_check(ctx, lo, hi, val, group, mod_sites_ref.MASKS, 'four sets')
    print('%d (site, set) pairs; fraction surely 0 / 1 / inside: %d / %d / %d; sharp optima: %d'
          % ((count.size,) + counts))
    assert min(counts) >= 3
    assert (hi - lo).tolist() == SIZES and max(SIZES) > CACHED_ROWS + 64
    # the empty site, and the sets "all" and "tagged" of the others
    assert (count[0] == 0).all() and (fraction[0] == 0).all() and (ll[0] == 0).all()
    assert np.array_equal(count[:, 3], count[:, 1] + count[:, 2]) and (count[:, 0] >= count[:, 3]).all()
    assert (count[:, 0] < hi - lo)[[9, 14]].all()              # rows with a group outside 0 .. 31 are in no set
    for q in range(4):
        assert fraction[ALL_POSITIVE, q] == 1.0 and fraction[ALL_NEGATIVE, q] == 0.0 and ll[ALL_NEGATIVE, q] == 0.0
    # the special values: NaN in no set, +-inf and +-2 clip clipped; haplotype 1 holds 0, 1e-300, clip, inf, -2 clip
    assert count[SPECIAL].tolist() == [11, 5, 5, 10]
    # the planted shares show: group 1 above group 2 at every large site
    big = [9, 13, 14]
    assert (fraction[big, 1] > 0.6).all() and (fraction[big, 2] < 0.4).all()


def test_one_set_bisected_beside_one_that_is_not(ctx):
    """Sites of 0, 1, 64, 128, 129 and 200 rows; group 1 mixes both signs, so its set has its maximum inside (0, 1) and
    is bisected; group 0 is all positive, so its set ends after the first sweep with f^ = 1; a third set is empty."""
    rng = np.random.default_rng(49)
    sizes = [0, 1, 64, CACHED_ROWS, CACHED_ROWS + 1, 200]
    lo = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    hi = np.cumsum(sizes).astype(np.int64)
    n = int(hi[-1])
    group = (np.arange(n) % 2).astype(np.int32)
    val = np.where(rng.random(n) < 0.4, 1.0, -1.0) * rng.normal(6.0, 2.0, n)
    val[group == 0] = np.abs(val[group == 0]) + 0.5
    count, fraction, ll, _ = solve_and_check(ctx, lo, hi, val, group, (0b010, 0b001, 0b100), 'edge sizes')
    assert np.array_equal(count.sum(1), sizes) and (count[:, 2] == 0).all()
    assert ((fraction[2:, 0] > 0) & (fraction[2:, 0] < 1)).all() and (fraction[1:, 1] == 1.0).all()
    assert (fraction[:, 2] == 0).all() and (fraction[0] == 0).all()


@pytest.mark.parametrize('n_sets', [1, 2, 3, 5, 6, 7, 8])
def test_every_number_of_sets(ctx, n_sets):
    lo, hi, val, group = build_case(43)
    masks = [0b111, 0b010, 0b100, 0b110, 0b001, 0, 0xffffffff, 0b101][:n_sets]
    if n_sets == 1:
        # one set, no groups: every row whose value is a number
        count, fraction, ll, _ = solve_and_check(ctx, lo, hi, val, None, (1,), 'no groups')
        assert np.array_equal(count[:, 0], [int((~np.isnan(val[a:b])).sum()) for a, b in zip(lo, hi)])
    count, fraction, ll, _ = solve_and_check(ctx, lo, hi, val, group, masks, '%d sets' % n_sets)
    if n_sets >= 7:
        assert (count[:, 5] == 0).all() and np.array_equal(count[:, 6], count[:, 0])
        assert np.array_equal(fraction[:, 6], fraction[:, 0]) and np.array_equal(ll[:, 6], ll[:, 0])


def test_sets_are_solved_alone_as_together_and_order_matters_not(ctx):
    """A set solved in a launch of its own gives the bits it has among the four: a row outside a set adds +0.0, so the
    partial sums are those of the launch with all sets; and the sites may come in any order."""
    from nadavca_amd import device
    lo, hi, val, group = build_case(47)
    d_lo, d_hi, d_val, d_group = on_device(ctx, lo, hi, val, group)
    four = [t.cpu().numpy() for t in device.mod_site_solve_dev(ctx, d_lo, d_hi, d_val, d_group, mod_sites_ref.MASKS,
                                                               CLIP)]
    for q, m in enumerate(mod_sites_ref.MASKS):
        one = [t.cpu().numpy() for t in device.mod_site_solve_dev(ctx, d_lo, d_hi, d_val, d_group, (m,), CLIP)]
        for a, b in zip(one, four):
            assert np.array_equal(a[:, 0], b[:, q]), q
    perm = np.random.default_rng(1).permutation(len(lo))
    p_lo, p_hi = on_device(ctx, lo[perm], hi[perm])
    shuffled = [t.cpu().numpy() for t in device.mod_site_solve_dev(ctx, p_lo, p_hi, d_val, d_group,
                                                                   mod_sites_ref.MASKS, CLIP)]
    for a, b in zip(shuffled, four):
        assert np.array_equal(a, b[perm])
    # a range that leaves 0 .. n_rows is cut to it
    w_lo, w_hi = on_device(ctx, np.array([-5, 0], dtype=np.int64), np.array([val.size + 7, val.size], dtype=np.int64))
    wide = [t.cpu().numpy() for t in device.mod_site_solve_dev(ctx, w_lo, w_hi, d_val, d_group, (0b111,), CLIP)]
    for a in wide:
        assert a[0, 0] == a[1, 0]
    assert wide[0][0, 0] == int((~np.isnan(val) & (group >= 0) & (group < 32)).sum())


def test_no_sites_and_no_rows(ctx):
    import torch
    from nadavca_amd import device
    dev = torch.device('cuda', ctx.device)
    z64 = torch.zeros(0, dtype=torch.int64, device=dev)
    val = torch.zeros(5, dtype=torch.float64, device=dev)
    out = device.mod_site_solve_dev(ctx, z64, z64, val, None, mod_sites_ref.MASKS, CLIP)
    assert [tuple(t.shape) for t in out] == [(0, 4)] * 3
    # sites without rows at all
    lo = torch.zeros(3, dtype=torch.int64, device=dev)
    out = device.mod_site_solve_dev(ctx, lo, lo, torch.zeros(0, dtype=torch.float64, device=dev), None, (1, 1), CLIP)
    assert all(int(t.abs().sum()) == 0 and tuple(t.shape) == (3, 2) for t in out)
    for masks in ((), (1,) * 9, (-1,), (1 << 32,)):
        with pytest.raises(ValueError):
            device.mod_site_solve_dev(ctx, lo, lo, val, None, masks, CLIP)
    with pytest.raises(ValueError):
        device.mod_site_solve_dev(ctx, lo, lo, val, None, (1,), 0.0)
    with pytest.raises(ValueError):
        device.mod_site_solve_dev(ctx, lo, lo, val, torch.zeros(4, dtype=torch.int32, device=dev), (1,), CLIP)


def test_c_abi_rejects_bad_arguments(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    lo = torch.tensor([0, 4], dtype=torch.int64, device=dev)
    hi = torch.tensor([4, 10], dtype=torch.int64, device=dev)
    val = torch.ones(10, dtype=torch.float64, device=dev)
    group = torch.zeros(10, dtype=torch.int32, device=dev)
    mask = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    count = torch.full((2, 2), -1, dtype=torch.int64, device=dev)
    fraction = torch.full((2, 2), -1.0, dtype=torch.float64, device=dev)
    ll = torch.full((2, 2), -1.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(c=None, n_sites=2, n_rows=10, lo_=lo, hi_=hi, val_=val, group_=group, n_sets=2, mask_=mask, clip=CLIP,
             count_=count, fraction_=fraction, ll_=ll):
        return lib.nvk_mod_site_solve_dev(ctx.handle if c is None else c, n_sites, n_rows, p(lo_), p(hi_), p(val_),
                                          p(group_), n_sets, p(mask_), clip, p(count_), p(fraction_), p(ll_))

    def invalid(rc):
        return rc == _lib.NVK_ERR_INVALID and lib.nvk_last_error()

    assert call() == _lib.NVK_OK
    assert count.cpu().tolist() == [[4, 4], [6, 6]] and fraction.cpu().tolist() == [[1.0, 1.0], [1.0, 1.0]]
    assert ll.cpu().tolist() == [[4.0, 4.0], [6.0, 6.0]]
    assert call(group_=None) == _lib.NVK_OK
    # n_sites == 0 launches nothing and writes nothing
    count.fill_(-1)
    assert call(n_sites=0, lo_=None, hi_=None, val_=None, mask_=None, count_=None, fraction_=None, ll_=None) \
        == _lib.NVK_OK
    assert call(n_sites=0) == _lib.NVK_OK and (count == -1).all()
    assert call(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
    for kw in (dict(n_sites=-1), dict(n_rows=-1), dict(n_sets=0), dict(n_sets=9), dict(clip=0.0), dict(clip=-1.0),
               dict(clip=float('nan')), dict(clip=float('inf')), dict(lo_=None), dict(hi_=None), dict(val_=None),
               dict(mask_=None), dict(count_=None), dict(fraction_=None), dict(ll_=None)):
        assert invalid(call(**kw)), kw
    # the timer of the allele family counts the launch
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        assert call() == _lib.NVK_OK
        assert ctx.timing_read()['allele'][1] == 1
    finally:
        ctx.timing_enable(False)
