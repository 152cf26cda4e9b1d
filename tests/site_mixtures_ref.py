"""The mixture contract of include/nadavca_hip.h (nvk_site_mixture_tests_dev) restated in numpy: every sum as 64
lane-strided partial sums and the butterfly, every expression in the contract's order; many sites side by side (rows
that a site does not have add 0.0 to its sums, which changes no bit).  Then the device layer around it (drop, sort, list
the sites) and the host formulas of ``SiteMixtureComparison`` row by row.  The yardstick of the CPU and the GPU tests of
``compare_site_mixtures``; nothing here touches the package's kernels."""
import numpy as np

HALF_LOG_2PI = 0.9189385332046727
N_COUNTS, N_FIT = 5, 17
FIT_NAMES = ('ll_one', 'mean0_shared', 'sd0_shared', 'mean1_shared', 'sd1_shared', 'w_shared', 'll_shared', 'ra', 'rb',
             'q', 'mean0', 'sd0', 'mean1', 'sd1', 'wa', 'wb', 'll_free')


def wave_sum(t):
    """SUM of the contract per row of t (sites, 64 c): column i goes to partial sum i mod 64 in ascending i; then
    p[l] = p[l] + p[l xor d] for d = 32 .. 1."""
    t = t.reshape(t.shape[0], -1, 64)
    p = np.zeros((t.shape[0], 64))
    for c in range(t.shape[1]):
        p = p + t[:, c]
    # (lane 0's value: after the step of distance d the lanes l and l xor d hold the same bits, a + b being b + a, so
    # the lower half of the lanes is all that lane 0 ever reads)
    for d in (32, 16, 8, 4, 2, 1):
        p = p[:, :d] + p[:, d:]
    return p[:, 0].copy()


def _responsibility(y, w, m0, sd0, m1, sd1):
    """r(y, w) of the contract: -> (r, the row's log density without the constant).  y, w (sites, rows); the
    parameters (sites, 1)."""
    i0, i1, ls0, ls1 = 1.0 / sd0, 1.0 / sd1, np.log(sd0), np.log(sd1)
    z0, z1 = (y - m0) * i0, (y - m1) * i1
    l0, l1 = -0.5 * (z0 * z0) - ls0, -0.5 * (z1 * z1) - ls1
    q = l1 - l0
    pos = q > 0.0
    e = np.exp(-np.abs(q))
    u = 1.0 - w
    we = w * e
    num = np.where(pos, w, we)
    den = np.where(pos, w + u * e, we + u)
    r = np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), np.where(pos, 0.0, 1.0))
    return r, np.where(pos, l1, l0) + np.log(den)


def fit_sites(x, in_a, valid, iterations, min_sd_ratio, trace=None):
    """The contract for sites side by side: x (sites, 64 c) the pooled rows (A's, then B's, then padding), in_a and
    valid masks of the same shape; every site has rows of both samples.  -> (counts int64 (sites, 5), fit f64 (sites,
    17)).  ``trace``: a list that receives, per EM step and stage, (stage, the log-likelihood at the step's parameters
    BEFORE it, which sites took the step, where those parameters sit on the floor) — what the kernel does not compute,
    for the monotonicity test."""
    S = x.shape[0]
    col = lambda v: v[:, None]
    sel = lambda mask, t: np.where(mask & valid, t, 0.0)
    n, m = (in_a & valid).sum(axis=1), (~in_a & valid).sum(axis=1)
    fN, fn, fm = (n + m).astype(np.float64), n.astype(np.float64), m.astype(np.float64)
    counts = np.zeros((S, N_COUNTS), dtype=np.int64)
    fit = np.full((S, N_FIT), np.nan)
    counts[:, 0], counts[:, 1] = n, m
    with np.errstate(all='ignore'):
        mu = wave_sum(sel(valid, x)) / fN
        y = np.where(valid, x - col(mu), 0.0)
        hi = y > 0.0
        s = np.sqrt(wave_sum(sel(valid, y * y)) / fN)
        ll_one = -fN * (np.log(s) + (HALF_LOG_2PI + 0.5))
        c1 = wave_sum(sel(hi, np.ones_like(y)))
        c0 = fN - c1
        fitted = (s > 0.0) & (s < np.inf) & (c0 > 0.0) & (c1 > 0.0)
        sd_min = min_sd_ratio * s
        m0, m1 = wave_sum(sel(~hi, y)) / c0, wave_sum(sel(hi, y)) / c1
        d = y - np.where(hi, col(m1), col(m0))
        sd0 = np.maximum(np.sqrt(wave_sum(sel(~hi, d * d)) / c0), sd_min)
        sd1 = np.maximum(np.sqrt(wave_sum(sel(hi, d * d)) / c1), sd_min)
        wa = wb = c1 / fN
        fit[:, 0] = ll_one
        for stage in (0, 1):
            active = fitted.copy()
            steps = np.zeros(S, dtype=np.int64)
            weight = lambda: np.where(in_a, col(wa), col(wb))
            for _ in range(iterations):
                r, ld = _responsibility(y, weight(), col(m0), col(sd0), col(m1), col(sd1))
                ra, rb = wave_sum(sel(in_a, r)), wave_sum(sel(~in_a, r))
                r0 = wave_sum(sel(valid, 1.0 - r))
                t1, t0 = wave_sum(sel(valid, r * y)), wave_sum(sel(valid, (1.0 - r) * y))
                r1 = ra + rb
                active = active & (r1 > 0.0) & (r0 > 0.0)
                if trace is not None:
                    trace.append((stage, wave_sum(sel(valid, ld)) - fN * HALF_LOG_2PI, active.copy(),
                                  (sd0 <= sd_min) | (sd1 <= sd_min)))
                if not active.any():
                    break
                nm0, nm1 = t0 / r0, t1 / r1
                d0, d1 = y - col(nm0), y - col(nm1)
                v0, v1 = wave_sum(sel(valid, (1.0 - r) * (d0 * d0))), wave_sum(sel(valid, r * (d1 * d1)))
                keep = lambda new, old: np.where(active, new, old)
                m0, m1 = keep(nm0, m0), keep(nm1, m1)
                sd0 = keep(np.maximum(np.sqrt(v0 / r0), sd_min), sd0)
                sd1 = keep(np.maximum(np.sqrt(v1 / r1), sd_min), sd1)
                wa = keep(ra / fn if stage else r1 / fN, wa)
                wb = keep(rb / fm if stage else r1 / fN, wb)
                steps += active
            r, ld = _responsibility(y, weight(), col(m0), col(sd0), col(m1), col(sd1))
            ll = wave_sum(sel(valid, ld)) - fN * HALF_LOG_2PI
            counts[:, 3 + stage] = steps
            if stage == 0:
                ra, rb = wave_sum(sel(in_a, r)), wave_sum(sel(~in_a, r))
                dr = r - col((ra + rb) / fN)
                fit[:, 1:10] = np.stack([mu + m0, sd0, mu + m1, sd1, wa, ll, ra, rb, wave_sum(sel(valid, dr * dr))],
                                        axis=1)
            else:
                fit[:, 10:17] = np.stack([mu + m0, sd0, mu + m1, sd1, wa, wb, ll], axis=1)
    counts[:, 2] = fitted
    counts[~fitted, 3:] = 0
    fit[~fitted] = np.nan
    fit[~fitted, 0] = fit[~fitted, 6] = fit[~fitted, 16] = ll_one[~fitted]
    return counts, fit


def pack(runs):
    """[(A, B)] of non-empty value arrays -> (x, in_a, valid) padded to the same multiple of 64 columns."""
    width = 64 * max((a.size + b.size + 63) // 64 for a, b in runs)
    x = np.zeros((len(runs), width))
    in_a, valid = np.zeros(x.shape, dtype=bool), np.zeros(x.shape, dtype=bool)
    for i, (a, b) in enumerate(runs):
        x[i, :a.size], x[i, a.size:a.size + b.size] = a, b
        in_a[i, :a.size] = True
        valid[i, :a.size + b.size] = True
    return x, in_a, valid


def fit_runs(runs, iterations, min_sd_ratio):
    """The two output tables for [(A, B)], A and B the values of one listed key in the two samples in the kernel's
    order (ascending; the order within a run only changes which partial sum a value joins).  Sites are fitted side by
    side with those of the same number of 64-row chunks."""
    counts = np.zeros((len(runs), N_COUNTS), dtype=np.int64)
    fit = np.full((len(runs), N_FIT), np.nan)
    groups = {}
    for i, (a, b) in enumerate(runs):
        counts[i, :2] = a.size, b.size
        if a.size and b.size:
            groups.setdefault((a.size + b.size + 63) // 64, []).append(i)
    for rows in groups.values():
        c, f = fit_sites(*pack([runs[i] for i in rows]), iterations, min_sd_ratio)
        counts[rows], fit[rows] = c, f
    return counts, fit


def one_site(A, B, iterations=32, min_sd_ratio=0.1):
    """One listed key: -> (counts (5,), fit (17,)); A, B in any order (sorted here, as the device layer does)."""
    c, f = fit_runs([(np.sort(np.asarray(A, dtype=np.float64)), np.sort(np.asarray(B, dtype=np.float64)))],
                    iterations, min_sd_ratio)
    return c[0], f[0]


def mixture_tests(key_a, val_a, key_b, val_b, site_key, iterations, min_sd_ratio):
    """nvk_site_mixture_tests_dev from host arrays (rows in any order; sorted by (key, value) here): -> (counts, fit)."""
    key_a, key_b = np.asarray(key_a, dtype=np.int64), np.asarray(key_b, dtype=np.int64)
    val_a, val_b = np.asarray(val_a, dtype=np.float64), np.asarray(val_b, dtype=np.float64)
    oa, ob = np.lexsort((val_a, key_a)), np.lexsort((val_b, key_b))
    ka, kb, va, vb = key_a[oa], key_b[ob], val_a[oa], val_b[ob]
    site_key = np.asarray(site_key, dtype=np.int64)
    la, ha = np.searchsorted(ka, site_key, 'left'), np.searchsorted(ka, site_key, 'right')
    lb, hb = np.searchsorted(kb, site_key, 'left'), np.searchsorted(kb, site_key, 'right')
    return fit_runs([(va[la[i]:ha[i]], vb[lb[i]:hb[i]]) for i in range(site_key.size)], iterations, min_sd_ratio)


def device_layer(key_a, val_a, key_b, val_b, min_coverage, iterations, min_sd_ratio):
    """``device.site_mixture_tests_dev`` from host arrays: rows with key < 0 or a value that is not finite dropped,
    the sites with at least ``min_coverage`` rows in both samples, ascending, and the kernel's tables for them:
    -> (site_key, counts, fit)."""
    rows = []
    for key, val in ((key_a, val_a), (key_b, val_b)):
        key, val = np.asarray(key, dtype=np.int64), np.asarray(val, dtype=np.float64)
        keep = (key >= 0) & np.isfinite(val)
        rows.append((key[keep], val[keep]))
    (ka, va), (kb, vb) = rows
    ua, ca = np.unique(ka, return_counts=True)
    ub, cb = np.unique(kb, return_counts=True)
    site_key = np.intersect1d(ua[ca >= min_coverage], ub[cb >= min_coverage]).astype(np.int64)
    return (site_key,) + mixture_tests(ka, va, kb, vb, site_key, iterations, min_sd_ratio)


def host_columns(counts, fit):
    """The float columns of a SiteMixtureComparison from the kernel's tables, row by row with Python floats."""
    from scipy.special import ndtr
    names = ('mean_0', 'sd_0', 'mean_1', 'sd_1', 'rate_a', 'rate_b', 'delta_rate', 'll_one', 'll_shared', 'll_free',
             'lrt', 'z', 'p')
    out = {f: [] for f in names}
    for c, f in zip(counts.tolist(), fit.tolist()):
        n, m = float(c[0]), float(c[1])
        N = n + m
        v = dict(zip(FIT_NAMES, f))
        swap = v['wa'] > 0.5
        comp = [(v['mean0'], v['sd0']), (v['mean1'], v['sd1'])]
        rate_a, rate_b = v['wa'], v['wb']
        if swap:
            comp, rate_a, rate_b = comp[::-1], 1.0 - rate_a, 1.0 - rate_b
        var = n * m * v['q'] / (N * (N - 1.0))
        if var > 0:
            z = (v['rb'] - m * ((v['ra'] + v['rb']) / N)) / np.sqrt(var)
            z = -z if swap else z
            p = 2.0 * float(ndtr(-abs(z)))
        else:
            z = p = np.nan
        for name, value in zip(names, (comp[0][0], comp[0][1], comp[1][0], comp[1][1], rate_a, rate_b, rate_b - rate_a,
                                       v['ll_one'], v['ll_shared'], v['ll_free'], 2.0 * (v['ll_free'] - v['ll_shared']),
                                       z, p)):
            out[name].append(value)
    return {f: np.array(v, dtype=np.float64) for f, v in out.items()}


def check_against(got_counts, got_fit, want_counts, want_fit):
    """The integers equal, NaN and infinities in the same places, the finite floats within 1e-9 relative + 1e-9
    absolute (device exp / log against numpy's, as ``allele_ref.check_against``).  -> the largest |difference| /
    (1 + |value|) seen."""
    assert np.array_equal(got_counts, want_counts), np.nonzero((got_counts != want_counts).any(axis=1))[0][:10]
    assert got_fit.shape == want_fit.shape
    finite = np.isfinite(want_fit)
    assert np.array_equal(np.isnan(got_fit), np.isnan(want_fit))
    assert np.array_equal(got_fit[~finite & ~np.isnan(want_fit)], want_fit[~finite & ~np.isnan(want_fit)])
    diff = np.abs(got_fit[finite] - want_fit[finite])
    bad = diff > 1e-9 * np.abs(want_fit[finite]) + 1e-9
    assert not bad.any(), (int(bad.sum()), float(diff.max()))
    return float((diff / (1.0 + np.abs(want_fit[finite]))).max()) if diff.size else 0.0


class AsT:
    """A row table with ``t`` = -log10 p and the fields ``site_levels_ref.detection_shares`` reads."""

    def __init__(self, cmp, p):
        with np.errstate(divide='ignore'):
            self.t = np.where(np.isnan(p), 0.0, -np.log10(p))
        self.strand, self.position = cmp.strand, cmp.position
        self.peak = np.zeros(self.t.size, dtype=bool)


def detection(cmp, truth, k):
    """The planted-site experiment on a SiteMixtureComparison over one plain reference, 'nearby' and 'far' as
    ``site_levels_ref.detection_shares`` has them: -> (a) the share of the modified (site, strand) with a row of
    p <= 1e-3 nearby, the sites counted, the median ``delta_rate`` of the rows with p <= 1e-3 near a modified site and
    their number, (b) the share of the far rows with p <= 1e-2 and the far rows; prints them."""
    import site_levels_ref
    share_a, sites, _, far_rows, _, _ = site_levels_ref.detection_shares(AsT(cmp, cmp.p), truth, k, t_min=3.0)
    _, _, share_b, _, far_max, _ = site_levels_ref.detection_shares(AsT(cmp, cmp.p), truth, k, t_min=2.0)
    near = np.zeros(len(cmp), dtype=bool)
    for s, mask in ((0, truth['forward']), (1, truth['reverse'])):
        lo, hi = (3, 2) if s == 0 else (2, 3)              # the positions whose k-mer holds the site: p - lo .. p + hi
        cover = np.zeros(mask.size, dtype=bool)
        for p in np.nonzero(mask)[0]:
            cover[max(p - lo, 0):p + hi + 1] = True
        near |= (cmp.strand == s) & cover[cmp.position]
    hits = near & (cmp.p <= 1e-3)
    median = float(np.median(cmp.delta_rate[hits])) if hits.any() else np.nan
    print('%d rows, median coverage %d / %d; (a) %.3f of %d modified sites have a row of p <= 1e-3 nearby; median '
          'delta_rate of the %d such rows %.3f; (b) p <= 1e-2 on %.4f of %d far rows, smallest far p %.2g'
          % (len(cmp), np.median(cmp.n_a), np.median(cmp.n_b), share_a, sites, int(hits.sum()), median, share_b,
             far_rows, 10.0 ** -far_max))
    return share_a, sites, median, int(hits.sum()), share_b, far_rows
