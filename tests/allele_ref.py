"""The allele-mixture contract of include/nadavca_hip.h (nvk_allele_rows_dev / nvk_allele_solve_dev) restated in plain
numpy float64, every sum in read order (numpy.cumsum adds left to right).  The yardstick of the CPU and the GPU
tests of ``estimate_allele_fractions_batch``; nothing here touches the package's kernels."""
import numpy as np

BISECT = 52


def t_term(f, d):
    """t(f, d) = d + log(f + (1 - f) exp(-d)) for d > 0, else log((1 - f) + f exp(d)); f and d broadcast."""
    f, d = np.broadcast_arrays(np.asarray(f, dtype=np.float64), np.asarray(d, dtype=np.float64))
    pos = d > 0
    e = np.exp(-np.abs(d))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(pos, np.where(pos, d, 0.0) + np.log(f + (1.0 - f) * e), np.log((1.0 - f) + f * e))


def u_term(f, d):
    """u(f, d) = (1 - exp(-d)) / (exp(-d) (1 - f) + f) for d > 0, else (exp(d) - 1) / (1 + f (exp(d) - 1))."""
    f, d = np.broadcast_arrays(np.asarray(f, dtype=np.float64), np.asarray(d, dtype=np.float64))
    pos = d > 0
    e = np.exp(-np.abs(d))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(pos, 1.0 - e, e - 1.0) / np.where(pos, e * (1.0 - f) + f, 1.0 + f * (e - 1.0))


def _seq_sum(terms, valid):
    """Row sums left to right over the valid entries (a padded entry adds 0.0, which changes no bit)."""
    if terms.shape[1] == 0:
        return np.zeros(terms.shape[0])
    with np.errstate(invalid='ignore'):
        return np.cumsum(np.where(valid, terms, 0.0), axis=1)[:, -1]


def likelihood(f, D, valid):
    """L(f[m]) of every row m of the padded matrix D (M, C); valid: which entries are values."""
    return _seq_sum(t_term(np.asarray(f, dtype=np.float64)[:, None], np.where(valid, D, 0.0)), valid)


def derivative(f, D, valid):
    return _seq_sum(u_term(np.asarray(f, dtype=np.float64)[:, None], np.where(valid, D, 0.0)), valid)


def pad(vectors):
    """A list of 1-d arrays -> (D (M, C) padded with 0, valid (M, C))."""
    C = max([len(v) for v in vectors], default=0)
    D = np.zeros((len(vectors), C))
    valid = np.zeros((len(vectors), C), dtype=bool)
    for m, v in enumerate(vectors):
        D[m, :len(v)] = v
        valid[m, :len(v)] = True
    return D, valid


def solve(D, valid):
    """The estimate of every row of D: -> dict of (M,) arrays: fraction, lrt, ll_half, ll_full, and for the tests'
    conditioning g0, g1 (the derivative at 0 and 1), abs0, abs1 (the sums of |u| there) and curvature (-g'(f^) =
    the sum of u(f^, d)^2)."""
    M = D.shape[0]
    Dz = np.where(valid, D, 0.0)
    zero, one = np.zeros(M), np.ones(M)
    g0, g1 = derivative(zero, D, valid), derivative(one, D, valid)
    abs0 = _seq_sum(np.abs(u_term(zero[:, None], Dz)), valid)
    abs1 = _seq_sum(np.abs(u_term(one[:, None], Dz)), valid)
    at0 = ~(g0 > 0)
    at1 = ~at0 & (g1 >= 0)
    run = ~at0 & ~at1
    lo, hi = np.zeros(M), np.ones(M)
    for _ in range(BISECT):
        m = (lo + hi) / 2.0
        up = derivative(m, D, valid) > 0
        lo = np.where(run & up, m, lo)
        hi = np.where(run & ~up, m, hi)
    f = np.where(at0, 0.0, np.where(at1, 1.0, (lo + hi) / 2.0))
    lrt = np.where(f > 0, 2.0 * likelihood(f, D, valid), 0.0)
    with np.errstate(invalid='ignore', over='ignore'):
        curvature = _seq_sum(u_term(f[:, None], Dz) ** 2, valid)
    return dict(fraction=f, lrt=lrt, ll_half=likelihood(np.full(M, 0.5), D, valid), ll_full=_seq_sum(Dz, valid),
                g0=g0, g1=g1, abs0=abs0, abs1=abs1, curvature=curvature)


def rows(ll, reference, ref_off, chunk_start, reverse, status, event_length, ref_len):
    """nvk_allele_rows_dev: -> (key (sum R,), val (sum R, alphabet)) from host arrays."""
    ll = np.asarray(ll, dtype=np.float64)
    alpha = ll.shape[1]
    ref_off = np.asarray(ref_off, dtype=np.int64)
    n = ref_off.size - 1
    key = np.full(ll.shape[0], -1, dtype=np.int64)
    val = np.zeros_like(ll)
    for i in range(n):
        r0, r1 = int(ref_off[i]), int(ref_off[i + 1])
        R = r1 - r0
        if R == 0 or (status is not None and status[i] != 0):
            continue
        c0 = int(reference[r0])
        if not 0 <= c0 < alpha or not np.isfinite(ll[r0, c0]):
            continue
        with np.errstate(invalid='ignore'):
            d = (ll[r0:r1] - ll[r0, c0]) / event_length
        p = np.arange(R)
        if reverse[i]:
            pos, d = int(chunk_start[i]) + R - 1 - p, d[:, ::-1]
        else:
            pos = int(chunk_start[i]) + p
        ok = (pos >= 0) & (pos < ref_len)
        key[r0:r1] = np.where(ok, pos, -1)
        val[r0:r1] = np.where(ok[:, None], d, 0.0)
    return key, val


def sites(key, val, ref_codes):
    """The (P, b != r) pairs with coverage > 0 and their d vectors in read order: -> (P (M,), b (M,), D, valid,
    coverage (L,))."""
    ref_codes = np.asarray(ref_codes)
    L, alpha = ref_codes.size, val.shape[1]
    order = np.argsort(key, kind='stable')
    k, v = key[order], val[order]
    lo, hi = np.searchsorted(k, np.arange(L), 'left'), np.searchsorted(k, np.arange(L), 'right')
    coverage = (hi - lo).astype(np.int64)
    Ps, bs, vectors = [], [], []
    for P in np.nonzero(coverage)[0]:
        r = int(ref_codes[P])
        if not 0 <= r < alpha:
            continue
        for b in range(alpha):
            if b != r:
                Ps.append(P)
                bs.append(b)
                vectors.append(v[lo[P]:hi[P], b])
    D, valid = pad(vectors)
    return np.array(Ps, dtype=np.int64), np.array(bs, dtype=np.int64), D, valid, coverage


def check_against(ref, got_fraction, got_lrt, got_half, got_full, D, valid, label=''):
    """The tolerances of the allele kernels against ``solve``'s result ``ref`` for the same rows: ll_full, ll_half and
    lrt within 1e-9 relative + 1e-9 absolute; fraction exactly 0 / 1 where g(0) / g(1) are away from zero by more than
    1e-9 of their sums of |u|; elsewhere L(f_got) >= L(f_ref) - 1e-9 (1 + |L|), and |f_got - f_ref| <= 1e-6 where
    -g'(f_ref) >= 1."""
    def close(a, b, what):
        with np.errstate(invalid='ignore'):
            same = (a == b) | (np.abs(a - b) <= 1e-9 + 1e-9 * np.abs(b))
        assert same.all(), '%s %s: %r vs %r' % (label, what, a[~same][:4], b[~same][:4])
    close(got_full, ref['ll_full'], 'll_full')
    close(got_half, ref['ll_half'], 'll_half')
    close(got_lrt, ref['lrt'], 'lrt')
    f_ref = ref['fraction']
    sure0 = ref['g0'] < -1e-9 * ref['abs0']
    sure_pos = ref['g0'] > 1e-9 * ref['abs0']
    sure1 = sure_pos & (ref['g1'] > 1e-9 * ref['abs1'])
    sure_in = sure_pos & (ref['g1'] < -1e-9 * ref['abs1'])
    assert (got_fraction[sure0] == 0).all(), label + ' fraction not 0'
    assert (got_fraction[sure1] == 1).all(), label + ' fraction not 1'
    assert ((got_fraction[sure_in] > 0) & (got_fraction[sure_in] < 1)).all(), label + ' fraction not inside (0, 1)'
    assert ((got_fraction >= 0) & (got_fraction <= 1)).all()
    L_got, L_ref = likelihood(got_fraction, D, valid), likelihood(f_ref, D, valid)
    with np.errstate(invalid='ignore'):
        ok = (L_got == L_ref) | (L_got >= L_ref - 1e-9 * (1.0 + np.abs(L_ref)))
    assert ok.all(), '%s likelihood at the estimate: %r vs %r' % (label, L_got[~ok][:4], L_ref[~ok][:4])
    sharp = ref['curvature'] >= 1.0
    assert (np.abs(got_fraction - f_ref)[sharp] <= 1e-6).all(), label + ' fraction differs where the optimum is sharp'
    return int(sure0.sum()), int(sure1.sum()), int(sure_in.sum()), int(sharp.sum())


# ---- the front end of the workflow on the CPU oracle ----------------------------------------------------------------
def oracle_front(oracle, rb, ba, reference_num, model, bandwidth, min_event_length=2, wobbling=True,
                 normalise=True):
    """What ``estimate_allele_fractions_batch`` runs in front of its kernels, on the CPU (no spline tweak): ONE median /
    MAD over all reads (``normalise`` False: the raw signal is taken as normalised), ``readbatch.signal_alignments``
    with the base alignments ``ba``, and the oracle's ``estimate_log_likelihoods`` per live read.  ``model``: the tuple
    of ``synthetic.load_model_arrays``.  -> (ll (sum R, alphabet), sa): ``sa`` the SignalAlignmentBatch as numpy arrays.
    A read without a path has non-finite rows, which ``rows`` drops."""
    from nadavca_amd import readbatch
    raw = np.asarray(rb.raw_signal, dtype=np.float64)
    norm = raw
    if normalise:
        centre = np.median(raw)
        norm = np.clip((raw - centre) / np.median(np.abs(raw - centre)), -5, 5)
    sa = readbatch.signal_alignments(rb, ba, bandwidth, reference_num, model[0], model[1], device='cpu').host()
    mo = oracle.KmerModel(*model)
    ll = np.zeros((int(sa.ref_off[-1]), model[2]))
    for j in range(sa.live.size):
        seg = lambda a, off: a[off[j]:off[j + 1]]
        ll[sa.ref_off[j]:sa.ref_off[j + 1]] = oracle.estimate_log_likelihoods(
            norm[sa.win_start[j]:sa.win_start[j] + sa.win_len[j]], seg(sa.reference, sa.ref_off),
            seg(sa.context_before, sa.cb_off), seg(sa.context_after, sa.ca_off), seg(sa.anchors, sa.anc_off),
            bandwidth, min_event_length, mo, wobbling)
    return ll, sa


def planted_haplotypes(length, sites, seed):
    """A random genome of ``length`` bases and a second haplotype that differs from it at ``sites`` (each base replaced
    by another one): -> (reference codes, haplotype codes, planted alt bases)."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, length).astype(np.int32)
    hap = ref.copy()
    sites = np.asarray(sites, dtype=np.int64)
    hap[sites] = (ref[sites] + rng.integers(1, 4, sites.size)) % 4
    return ref, hap, hap[sites].astype(np.int64)


def realised_share(P, sa, status, haplotype_of_live):
    """The share of the reads with status 0 covering position P that came from haplotype 1, and their number."""
    cover = (np.asarray(status) == 0) & (sa.ref_start <= P) & (P < sa.ref_end)
    n = int(cover.sum())
    return (float((haplotype_of_live[cover] == 1).sum()) / n if n else 0.0), n


def planted_check(P_rows, b_rows, fraction, lrt, sites, alts, realised, k):
    """The quality claims of the planted-site experiment over the rows (P, b) of a keep='all' result: every planted
    (site, alt) row has |fraction - realised| <= 0.1 and an lrt above that of every row more than k - 1 positions
    from every planted site.  -> (largest |fraction - realised|, smallest planted lrt, largest far lrt)."""
    sites = np.asarray(sites, dtype=np.int64)
    far = np.abs(P_rows[:, None] - sites[None, :]).min(axis=1) > k - 1
    planted = np.array([int(np.nonzero((P_rows == s) & (b_rows == a))[0][0]) for s, a in zip(sites, alts)])
    err = np.abs(fraction[planted] - np.asarray(realised))
    worst, low, high = float(err.max()), float(lrt[planted].min()), float(lrt[far].max())
    print('planted sites: largest |fraction - realised| %.4f, smallest planted lrt %.1f, largest far lrt %.1f (%d far '
          'rows)' % (worst, low, high, int(far.sum())))
    assert far.sum() > 100
    assert worst <= 0.1, err
    assert low > high, (low, high)
    return worst, low, high
