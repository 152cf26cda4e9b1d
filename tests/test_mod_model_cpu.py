"""The modified-base statistics without a GPU: the numpy restatement (tests/mod_model_ref.py) against a brute-force
enumeration on tiny hand-made reads, the update rule of ``estimate_mod_model`` (``mod_train.update_mod_levels``) against
its one-k-mer-at-a-time restatement and on its edge cases, and the two C-ABI entries declared, bound and exported."""
import itertools
import os
import re

import numpy as np
import pytest

from mod_model_ref import mod_reduce, mod_rows, mod_stats, update_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(seed, R, sites, gammas, k, central, alphabet=5, ctx=(2, 3)):
    """One read of R bases with events of 1 .. 6 samples, contexts of ``ctx`` bases, the given sites."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 7, R)
    starts = np.concatenate([[0], np.cumsum(lens)])
    args = dict(signal=rng.normal(0.0, 1.0, int(starts[-1])), sig_off=np.array([0, starts[-1]]),
                events=np.stack([starts[:-1], starts[1:]], 1).astype(np.int32), ref_off=np.array([0, R]),
                reference=rng.integers(0, 4, R).astype(np.int32),
                ctx_before=rng.integers(0, 4, ctx[0]).astype(np.int32), cb_off=np.array([0, ctx[0]]),
                ctx_after=rng.integers(0, 4, ctx[1]).astype(np.int32), ca_off=np.array([0, ctx[1]]),
                status=np.zeros(1, np.int32), k=k, central=central, alphabet=alphabet, trim=0,
                site_off=np.array([0, len(sites)]), site_pos=np.array(sites, dtype=np.int32),
                site_gamma=np.array(gammas, dtype=np.float64), mod_code=alphabet - 1,
                level=rng.normal(0.0, 1.0, alphabet ** k))
    return args


def _brute(args):
    """Per base with 1 .. 4 sites in its window: every subset of them, the empty one included, as (base, mask, key,
    weight), the weight a plain product; and the event's samples."""
    k, central, A = args['k'], args['central'], args['alphabet']
    ext = np.concatenate([args['ctx_before'], args['reference'], args['ctx_after']]).astype(np.int64)
    nb, R = args['ctx_before'].size, args['reference'].size
    out = []
    for g in range(R):
        p0 = g - central
        if p0 < -nb or p0 + k > R + args['ctx_after'].size:
            continue
        inside = [(int(p), float(w)) for p, w in zip(args['site_pos'], args['site_gamma']) if p0 <= p < p0 + k]
        if not 1 <= len(inside) <= 4:
            continue
        s, e = args['events'][g]
        for states in itertools.product((0, 1), repeat=len(inside)):
            window = ext[p0 + nb:p0 + nb + k].copy()
            weight, mask = 1.0, 0
            for t, ((p, gam), on) in enumerate(zip(inside, states)):
                weight *= gam if on else 1.0 - gam
                if on:
                    window[p - p0] = args['mod_code']
                    mask |= 1 << t
            key = 0
            for v in window:
                key = key * A + int(v)
            out.append((g, mask, key, weight, args['signal'][s:e]))
    return out


@pytest.mark.parametrize('k,central,sites,gammas', [
    (6, 2, [0, 3, 4, 9, 10, 11, 12, 19], [0.3, 0.9, 0.5, 0.2, 0.7, 0.4, 0.6, 0.8]),
    (3, 1, [1, 2, 3, 7, 19], [0.25, 1.0, 0.0, 0.5, 0.1]),
    (1, 0, [0, 5, 19], [0.5, 0.3, 1.0]),
    (6, 5, [2, 4, 6, 8, 15], [0.6, 0.1, 0.9, 0.35, 0.45]),
])
def test_restatement_against_brute_force(k, central, sites, gammas):
    args = _tiny(11 + k, 20, sites, gammas, k, central)
    count, key, val, skipped = mod_rows(**args)
    assert skipped == 0 and count.sum() == key.size > 0
    row_off = np.concatenate([[0], np.cumsum(count)])
    brute = _brute(args)
    by_base = {}
    for g, mask, bkey, weight, x in brute:
        by_base.setdefault(g, []).append((mask, bkey, weight, x))
    checked = 0
    for g in range(20):
        rows = slice(row_off[g], row_off[g + 1])
        if count[g] == 0:
            continue
        if (key[rows] < 0).all():           # an edge window: not counted, zeros
            assert g not in by_base and not val[rows].any()
            continue
        subsets = sorted(by_base[g])
        assert [s[0] for s in subsets] == list(range(count[g] + 1))     # every mask, the empty one first
        assert key[rows].tolist() == [s[1] for s in subsets[1:]]
        w = val[rows, 0]
        assert np.allclose(w, [s[2] for s in subsets[1:]], rtol=0, atol=1e-15)
        # the weights of all subsets multiply out: the non-empty ones leave what the empty one takes
        m = int(count[g] + 1).bit_length() - 1
        gam = [gm for p, gm in zip(args['site_pos'], args['site_gamma']) if g - central <= p < g - central + k]
        assert len(gam) == m
        assert abs(w.sum() - (1.0 - np.prod([1.0 - v for v in gam]))) <= 1e-15
        x = subsets[0][3]
        assert (val[rows, 1] == x.size).all()
        assert np.allclose(args['level'][key[rows]] + val[rows, 2] / val[rows, 1], x.mean(), rtol=0, atol=1e-12)
        # and the squared deviations are those around the subset's own level
        for r, kk in zip(range(row_off[g], row_off[g + 1]), key[rows]):
            assert abs(val[r, 3] - np.sum((x - args['level'][kk]) ** 2)) <= 1e-11
        checked += 1
    assert checked >= 3


def test_every_gamma_one_leaves_the_full_mask():
    args = _tiny(3, 20, [2, 4, 5, 12], [1.0, 1.0, 1.0, 1.0], 6, 2)
    count, key, val, _ = mod_rows(**args)
    row_off = np.concatenate([[0], np.cumsum(count)])
    seen = 0
    for g in np.nonzero(count)[0]:
        rows = slice(row_off[g], row_off[g + 1])
        if (key[rows] < 0).all():
            continue
        w = val[rows, 0]
        assert w[-1] == 1.0 and (w[:-1] == 0.0).all()      # exactly
        seen += 1
    assert seen > 5


def test_more_than_four_sites_give_no_rows_and_are_counted():
    args = _tiny(5, 20, [6, 7, 8, 9, 10, 15], [0.5] * 6, 6, 2)
    count, key, val, skipped = mod_rows(**args)
    # the windows [g - 2, g + 4) holding all of 6 .. 10: g = 7 and 8
    assert skipped == 2 and count[7] == 0 and count[8] == 0 and count[6] == 15 and count[9] == 15


def test_reduction_restatement_is_the_plain_weighted_sum():
    rng = np.random.default_rng(8)
    key = np.repeat([-1, 3, 7, 7 + 5 ** 3], [4, 1, 65, 200])
    val = np.stack([rng.random(key.size), rng.integers(1, 12, key.size).astype(float), rng.normal(0, 3, key.size),
                    rng.random(key.size) * 9], 1)
    perm = rng.permutation(key.size)
    ukey, sums, rows = mod_stats(key[perm], val[perm])
    assert ukey.tolist() == [3, 7, 7 + 5 ** 3] and rows.tolist() == [1, 65, 200]
    for q, kk in enumerate(ukey):
        v = val[key == kk]
        plain = [v[:, 0].sum(), (v[:, 0] * v[:, 1]).sum(), (v[:, 0] * v[:, 2]).sum(), (v[:, 0] * v[:, 3]).sum()]
        assert np.allclose(sums[q], plain, rtol=1e-13, atol=1e-13)
    assert mod_reduce(val, np.array([key.size]))[0].shape == (0, 4)


def _ids(*kmers):
    return [int(sum(d * 5 ** (len(km) - 1 - i) for i, d in enumerate(km))) for km in kmers]


def test_update_rule():
    from nadavca_amd.mod_train import holds_code, update_mod_levels
    k, alphabet = 3, 5
    rng = np.random.default_rng(1)
    mean, sigma = rng.normal(0, 1, 125), 0.2 + rng.random(125)
    with_m = _ids((4, 0, 1), (1, 4, 4), (2, 3, 4), (4, 4, 4), (0, 4, 2))
    without = _ids((0, 1, 2), (3, 3, 3))
    key = np.array(sorted(with_m + without))
    sums = np.zeros((key.size, 4))
    for q, kk in enumerate(key):
        W = 20.0 + q
        Nw = W * 8.0
        sums[q] = (W, Nw, Nw * 0.25, Nw * (0.25 ** 2 + 0.3 ** 2))
    low = int(np.nonzero(key == with_m[0])[0][0])
    sums[low, 0] = 9.999                                              # below min_weight
    floor = int(np.nonzero(key == with_m[1])[0][0])
    sums[floor, 3] = sums[floor, 1] * (0.25 ** 2 + 0.01 ** 2)          # sigma 0.01: the floor applies
    neg = int(np.nonzero(key == with_m[2])[0][0])
    sums[neg, 3] = sums[neg, 1] * 0.25 ** 2 * (1 - 1e-12)              # a variance just below 0
    assert sums[neg, 3] / sums[neg, 1] - (sums[neg, 2] / sums[neg, 1]) ** 2 < 0
    new_mean, new_sigma, updated, weight, samples = update_mod_levels(mean, sigma, key, sums, k, alphabet, 4, 10.0,
                                                                      0.05)
    ref_mean, ref_sigma, ref_updated = update_rule(mean, sigma, key, sums, k, alphabet, 4, 10.0, 0.05)
    assert np.array_equal(new_mean.view(np.int64), ref_mean.view(np.int64))
    assert np.array_equal(new_sigma.view(np.int64), ref_sigma.view(np.int64))
    assert np.array_equal(updated, ref_updated)
    assert sorted(np.nonzero(updated)[0].tolist()) == sorted(with_m[1:])
    kept = ~updated
    assert np.array_equal(new_mean[kept].view(np.int64), mean[kept].view(np.int64))
    assert np.array_equal(new_sigma[kept].view(np.int64), sigma[kept].view(np.int64))
    assert not updated[without].any() and not updated[with_m[0]]
    assert new_sigma[with_m[1]] == 0.05 and new_sigma[with_m[2]] == 0.05          # the floor; the clamp to 0 first
    assert np.allclose(new_mean[with_m[3]], mean[with_m[3]] + 0.25, rtol=0, atol=1e-15)
    assert abs(new_sigma[with_m[3]] - 0.3) < 1e-12
    assert np.array_equal(weight[key], sums[:, 0]) and np.array_equal(samples[key], sums[:, 1])
    assert weight.sum() == sums[:, 0].sum()
    assert holds_code(3, 5, 4).sum() == 125 - 64
    # the inputs are not written to
    assert mean is not new_mean and not np.shares_memory(mean, new_mean)
    for bad in (dict(min_weight=0.0), dict(min_sigma=0.0)):
        kw = dict(min_weight=10.0, min_sigma=0.05)
        kw.update(bad)
        with pytest.raises(ValueError):
            update_mod_levels(mean, sigma, key, sums, k, alphabet, 4, **kw)
    with pytest.raises(ValueError):
        update_mod_levels(mean, sigma, np.array([1, 1]), sums[:2], k, alphabet, 4, 10.0, 0.05)
    with pytest.raises(ValueError):
        update_mod_levels(mean[:10], sigma, key, sums, k, alphabet, 4, 10.0, 0.05)


def test_new_entries_declared_bound_and_exported():
    import ctypes as C
    from nadavca_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    sizes = {'nvk_mod_kmer_rows_dev': 29, 'nvk_mod_kmer_reduce_dev': 7}
    params = {}
    for name, n_args in sizes.items():
        m = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert m, '%s is not declared' % name
        params[name] = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(params[name]) == len(args) == n_args
        for p, a in zip(params[name], args):
            want = C.c_void_p if '*' in p else C.c_int64 if p.startswith('int64_t') else C.c_int
            assert a is want, p
    # the rows entry starts with the arguments of nvk_kmer_event_stats_dev
    stats = re.search(r'int nvk_kmer_event_stats_dev\(([^;]*)\);', header).group(1)
    stats = [p.strip() for p in stats.replace('\n', ' ').split(',')]
    assert params['nvk_mod_kmer_rows_dev'][:17] == stats[:17]
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail('the library is not built: %s' % _lib.LIB_PATH)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in sizes:
        assert hasattr(lib, name)
    import nadavca_amd
    assert callable(nadavca_amd.estimate_mod_model) and 'estimate_mod_model' in nadavca_amd.__all__
    assert 'ModModelEstimate' in nadavca_amd.__all__
    srcs = re.search(r'^SRCS\s*:=(.*)$', open(os.path.join(ROOT, 'nadavca_amd', 'csrc', 'Makefile')).read(), re.M)
    assert 'kernels_modstats.hip' in srcs.group(1).split()


def test_refusals_that_need_no_gpu():
    """The argument checks in front of the first device call."""
    from nadavca_amd import estimate_mod_model
    km4 = None        # (not reached)
    for kw in (dict(labels='x'), dict(rounds=0), dict(min_weight=0.0), dict(min_weight=-1.0), dict(fraction=0.0),
               dict(fraction=1.0), dict(min_sigma=0.0), dict(trim=-1)):
        with pytest.raises(ValueError):
            estimate_mod_model(None, None, km4, **kw)
