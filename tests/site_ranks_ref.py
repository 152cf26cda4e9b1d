"""The rank-test contract of include/nadavca_hip.h (nvk_site_rank_tests_dev) restated in plain numpy and Python floats:
the counts by ``searchsorted``, the tie sum by ``np.unique``, the exact Kolmogorov-Smirnov p-value by filling the table
V cell by cell; then the device layer around it (drop, sort, list the sites) and the host formulas of
``SiteRankComparison``.  The yardstick of the CPU and the GPU tests of ``compare_site_ranks``; nothing here touches the
package's kernels."""
import numpy as np

import site_levels_ref


def exact_p(n, m, h):
    """V(n, m): V(i, j) = 1.0 where |i m - j n| >= h, else V(0, 0) = 0.0 and V(i, j) = (V(i-1, j) * i + V(i, j-1) * j)
    / (i + j), a missing neighbour being 0.0.  Python floats are IEEE doubles; every operation is rounded once."""
    n, m, h = int(n), int(m), int(h)
    above = [0.0] * (m + 1)                       # row i - 1
    for i in range(n + 1):
        row = [0.0] * (m + 1)
        for j in range(m + 1):
            if abs(i * m - j * n) >= h:
                row[j] = 1.0
            elif i == 0 and j == 0:
                row[j] = 0.0
            else:
                up = above[j] if i > 0 else 0.0
                left = row[j - 1] if j > 0 else 0.0
                row[j] = (up * float(i) + left * float(j)) / float(i + j)
        above = row
    return above[m]


def one_site(A, B, exact_cells):
    """The seven outputs for one listed key: A, B the values of its runs in the two samples (any order)."""
    A, B = np.sort(np.asarray(A, dtype=np.float64)), np.sort(np.asarray(B, dtype=np.float64))
    n, m = A.size, B.size
    if n == 0 or m == 0:
        return n, m, 0, 0, 0, 0, np.nan
    pooled = np.concatenate([A, B])
    a_le, b_le = np.searchsorted(A, pooled, 'right'), np.searchsorted(B, pooled, 'right')
    d = a_le.astype(np.int64) * m - b_le.astype(np.int64) * n
    ks_plus, ks_minus = int(d.max()), int((-d).max())
    u2 = int(np.searchsorted(B, A, 'left').sum() + np.searchsorted(B, A, 'right').sum())
    t = np.unique(pooled, return_counts=True)[1].astype(np.int64)
    tie = int((t ** 3 - t).sum())
    p = np.nan
    if min(n, m) <= 255 and n * m <= exact_cells:
        p = exact_p(n, m, max(ks_plus, ks_minus))
    return n, m, ks_plus, ks_minus, u2, tie, p


def rank_tests(key_a, val_a, key_b, val_b, site_key, exact_cells):
    """nvk_site_rank_tests_dev from host arrays (rows in any order): -> (n_a, n_b, ks_plus, ks_minus, u2, tie int64,
    ks_p f64), one entry per listed key."""
    key_a, key_b = np.asarray(key_a), np.asarray(key_b)
    val_a, val_b = np.asarray(val_a, dtype=np.float64), np.asarray(val_b, dtype=np.float64)
    oa, ob = np.argsort(key_a, kind='stable'), np.argsort(key_b, kind='stable')
    ka, kb, va, vb = key_a[oa], key_b[ob], val_a[oa], val_b[ob]
    out = [one_site(va[np.searchsorted(ka, q, 'left'):np.searchsorted(ka, q, 'right')],
                    vb[np.searchsorted(kb, q, 'left'):np.searchsorted(kb, q, 'right')], exact_cells)
           for q in np.asarray(site_key).tolist()]
    cols = list(zip(*out)) if out else [[]] * 7
    return tuple(np.array(c, dtype=np.int64) for c in cols[:6]) + (np.array(cols[6], dtype=np.float64),)


def device_layer(key_a, val_a, key_b, val_b, min_coverage, exact_cells):
    """``device.site_rank_tests_dev`` from host arrays: rows with key < 0 or a NaN value dropped, the sites with at
    least ``min_coverage`` rows in both samples, ascending, and the kernel's outputs for them: -> (site_key, n_a, n_b,
    ks_plus, ks_minus, u2, tie, ks_p)."""
    rows = []
    for key, val in ((key_a, val_a), (key_b, val_b)):
        key, val = np.asarray(key, dtype=np.int64), np.asarray(val, dtype=np.float64)
        keep = (key >= 0) & ~np.isnan(val)
        rows.append((key[keep], val[keep]))
    (ka, va), (kb, vb) = rows
    ua, ca = np.unique(ka, return_counts=True)
    ub, cb = np.unique(kb, return_counts=True)
    site_key = np.intersect1d(ua[ca >= min_coverage], ub[cb >= min_coverage]).astype(np.int64)
    return (site_key,) + rank_tests(ka, va, kb, vb, site_key, exact_cells)


def host_columns(n_a, n_b, ks_plus, ks_minus, u2, tie, ks_p):
    """The float columns of a SiteRankComparison from the kernel's outputs, row by row with scipy's own functions."""
    from scipy.special import ndtr
    from scipy.stats import kstwo
    out = {f: [] for f in ('ks', 'ks_plus', 'ks_minus', 'ks_p', 'ks_exact', 'u', 'auc', 'mw_z', 'mw_p')}
    for n, m, kp, km, u2_, t, p in zip(n_a.tolist(), n_b.tolist(), ks_plus.tolist(), ks_minus.tolist(), u2.tolist(),
                                       tie.tolist(), ks_p.tolist()):
        nm, N = float(n * m), float(n + m)
        ks = max(kp, km) / nm
        exact = not np.isnan(p)
        if not exact:
            p = float(min(max(kstwo.sf(ks, np.round(nm / N)), 0.0), 1.0))
        u = u2_ / 2.0
        var = nm / 12.0 * ((N + 1.0) - t / (N * (N - 1.0)))
        s = np.sqrt(var)
        d = nm / 2.0 - u
        if s > 0:
            z = float(np.sign(d)) * max(abs(d) - 0.5, 0.0) / s
            mw_p = min(1.0, 2.0 * float(ndtr(-(abs(d) - 0.5) / s)))
        else:
            z = mw_p = np.nan
        for f, v in (('ks', ks), ('ks_plus', kp / nm), ('ks_minus', km / nm), ('ks_p', p), ('ks_exact', exact),
                     ('u', u), ('auc', 1.0 - u / nm), ('mw_z', z), ('mw_p', mw_p)):
            out[f].append(v)
    return {f: np.array(v, dtype=bool if f == 'ks_exact' else np.float64) for f, v in out.items()}


def same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN whatever its payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


class AsT:
    """A row table with ``t`` = -log10 p and the fields ``site_levels_ref.detection_shares`` reads: a threshold
    p <= 10^-x is |t| >= x there."""

    def __init__(self, cmp, p):
        with np.errstate(divide='ignore'):
            self.t = -np.log10(p)
        self.strand, self.position = cmp.strand, cmp.position
        self.peak = np.zeros(self.t.size, dtype=bool)


def check_detection(cmp, truth, k, min_sites, min_far):
    """The four conditions of the planted-site experiment on a SiteRankComparison; prints the run's figures."""
    shares = {}
    for name, p, level in (('KS 1e-3', cmp.ks_p, 3.0), ('KS 1e-2', cmp.ks_p, 2.0), ('MW 1e-2', cmp.mw_p, 2.0),
                           ('MW 1e-3', cmp.mw_p, 3.0)):
        share_a, sites, share_b, far_rows, far_max, _ = site_levels_ref.detection_shares(
            AsT(cmp, p), truth, k, t_min=level)
        print('%s: %d rows, median coverage %d / %d; (a) %.3f of %d modified sites have such a row nearby; (b) %.4f '
              'of %d far rows; smallest far p %.2g' % (name, len(cmp), np.median(cmp.n_a), np.median(cmp.n_b), share_a,
                                                       sites, share_b, far_rows, 10.0 ** -far_max))
        assert sites >= min_sites and far_rows >= min_far
        shares[name] = (share_a, share_b)
    assert shares['KS 1e-3'][0] >= 0.8 and shares['KS 1e-3'][1] <= 0.005, shares['KS 1e-3']
    assert shares['MW 1e-2'][0] >= 0.9 and shares['MW 1e-2'][1] <= 0.03, shares['MW 1e-2']
