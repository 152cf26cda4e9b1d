"""The site-level contract of include/nadavca_hip.h (nvk_site_level_rows_dev / nvk_site_moments_dev) restated in plain
numpy float64: an event's level and spread are ``np.mean`` and ``np.std`` themselves, a site's sums are 64 interleaved
partial sums and the fixed butterfly.  The yardstick of the CPU and the GPU tests of ``site_levels_batch``; nothing here
touches the package's kernels."""
import numpy as np

NCOL = 4
_LANES = np.arange(64)


def rows(signal, sig_off, events, ref_off, expected, chunk_start, reverse, status, trim, ref_len):
    """nvk_site_level_rows_dev from host arrays: -> (key (sum R,), val (sum R, 4))."""
    signal = np.asarray(signal, dtype=np.float64)
    events = np.asarray(events).reshape(-1, 2)
    total = int(ref_off[-1])
    key = np.full(total, -1, dtype=np.int64)
    val = np.zeros((total, NCOL))
    for j in range(len(ref_off) - 1):
        r0, R = int(ref_off[j]), int(ref_off[j + 1] - ref_off[j])
        if status is not None and status[j] != 0:
            continue
        x = signal[sig_off[j]:sig_off[j + 1]]
        N = x.size
        for g in range(max(int(trim), 0), R - int(trim)):
            a, b = (min(max(int(e), 0), N) for e in events[r0 + g])
            P = int(chunk_start[j]) + (R - 1 - g if reverse[j] else g)
            if not a < b or not 0 <= P < ref_len:
                continue
            level = np.mean(x[a:b])
            key[r0 + g] = 2 * P + (1 if reverse[j] else 0)
            val[r0 + g] = (level, np.std(x[a:b]), float(b - a), level - expected[r0 + g])
    return key, val


def wave_total(v):
    """The sum of the rows of v (c, V) per column as the kernel takes it: 64 partial sums from 0.0, row i into sum
    i mod 64 in ascending i, then the butterfly xor 32, 16, .., 1."""
    p = np.zeros((64, v.shape[1]))
    with np.errstate(invalid='ignore'):
        for i in range(0, v.shape[0], 64):
            blk = v[i:i + 64]
            p[:blk.shape[0]] = p[:blk.shape[0]] + blk
        for d in (32, 16, 8, 4, 2, 1):
            p = p + p[_LANES ^ d]
    return p[0]


def moments(key, val, n_keys):
    """nvk_site_moments_dev: ``key`` sorted ascending (stable), ``val`` (rows, V) gathered alike -> (count (n_keys,),
    mean (n_keys, V), m2 (n_keys, V))."""
    key, val = np.asarray(key), np.asarray(val, dtype=np.float64)
    val = val.reshape(key.size, -1)
    V = val.shape[1]
    q = np.arange(n_keys)
    lo, hi = np.searchsorted(key, q, 'left'), np.searchsorted(key, q, 'right')
    count = (hi - lo).astype(np.int64)
    mean, m2 = np.zeros((n_keys, V)), np.zeros((n_keys, V))
    with np.errstate(invalid='ignore'):
        for k in np.nonzero(count)[0]:
            v = val[lo[k]:hi[k]]
            mean[k] = wave_total(v) / float(count[k])
            d = v - mean[k]
            m2[k] = wave_total(d * d)
    return count, mean, m2


def site_levels(key, val, n_keys):
    """rows -> stable sort -> gather -> moments, as ``device.site_levels_dev``."""
    order = np.argsort(key, kind='stable')
    return moments(key[order], val[order], n_keys)


def batch_from_moments(count, mean, m2, ref_codes, **kw):
    """The moments of every key 2 P + strand over one plain reference as a SiteLevelBatch (the rows with count > 0)."""
    from nadavca_amd.site_levels import SiteLevelBatch
    q = np.nonzero(count)[0]
    P = q >> 1
    return SiteLevelBatch(np.zeros(q.size, np.int32), P.astype(np.int64), (q & 1).astype(np.int8),
                          np.asarray(ref_codes)[P].astype(np.int8), count[q].astype(np.int64), mean[q], m2[q],
                          len(ref_codes), **kw)


# ---- the planted-site experiment -------------------------------------------------------------------------------------
def model5(seed=5, sd=0.6):
    """The packaged 6-mer table extended to 5 letters: an M k-mer = its C k-mer's level + N(0, sd^2) (the levels of
    tests/test_gpu_call_mods.py's ``_model5``)."""
    from nadavca_amd import synthetic, kmer_train
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
    mean5 = mean5 + np.where(has_m, np.random.default_rng(seed).normal(0.0, sd, 5 ** k), 0.0)
    return k, central, 5, mean5, sigma5


# ---- the front end of the workflow on the CPU oracle ----------------------------------------------------------------
def oracle_front(oracle, rb, ba, reference_num, model, bandwidth, min_event_length=2, transitions=True,
                 renorm_rounds=3):
    """What ``site_levels_batch`` runs in front of its kernels, on the CPU: per-read median / MAD normalisation,
    ``readbatch.signal_alignments`` with the base alignments ``ba``, then per live read the oracle's
    ``refine_alignment`` and the renormalise / re-align loop of ``device.refine_renorm_loop_dev`` (least-squares line of
    the event means on the expected levels without contexts, rescale, align again).  ``model``: the tuple of
    ``synthetic.load_model_arrays``.  -> (sa as numpy arrays, signal of the windows end to end after the last rescale,
    sig_off, events (sum R, 2), expected levels with contexts, status)."""
    from scipy.stats import linregress
    from nadavca_amd import readbatch
    sa = readbatch.signal_alignments(rb, ba, bandwidth, reference_num, model[0], model[1], device='cpu').host()
    mo = oracle.KmerModel(*model)
    n = sa.live.size
    windows, events, expected, status = [], [], [], np.zeros(n, dtype=np.int32)
    for j in range(n):
        i = int(sa.live[j])
        raw = np.asarray(rb.raw_signal[rb.sig_off[i]:rb.sig_off[i + 1]], dtype=np.float64)
        centre = np.median(raw)
        norm = np.clip((raw - centre) / np.median(np.abs(raw - centre)), -5, 5)
        o = int(sa.win_start[j] - rb.sig_off[i])
        x = norm[o:o + int(sa.win_len[j])].copy()
        seg = lambda a, off: a[off[j]:off[j + 1]]
        ref, cb, ca = seg(sa.reference, sa.ref_off), seg(sa.context_before, sa.cb_off), seg(sa.context_after, sa.ca_off)
        align = lambda: np.asarray(oracle.refine_alignment(x, ref, cb, ca, seg(sa.anchors, sa.anc_off), bandwidth,
                                                           min_event_length, mo, transitions))
        plain = np.asarray(mo.get_expected_signal(ref, [], []))
        ev = align()
        for r in range(renorm_rounds):
            if ev.size == 0:
                break
            if r % 2 == 0:
                means = np.array([np.mean(x[a:b]) for a, b in ev])
                fit = linregress(plain, means)
                x = (x - fit.intercept) / fit.slope
            else:
                ev = align()
        if ev.size == 0:
            status[j], ev = 1, np.zeros((ref.size, 2), dtype=np.int32)
        windows.append(x)
        events.append(ev.reshape(-1, 2))
        expected.append(np.asarray(mo.get_expected_signal(ref, cb, ca)))
    sig_off = np.concatenate([[0], np.cumsum([w.size for w in windows])]).astype(np.int64)
    return sa, np.concatenate(windows), sig_off, np.concatenate(events), np.concatenate(expected), status


# ---- the two detection conditions -------------------------------------------------------------------------------------
def detection_shares(cmp, truth, k, t_min=6.0):
    """Over the rows of a SiteComparison on one plain reference, with ``truth`` = {'forward', 'reverse'} masks of the
    modified bases in FORWARD coordinates and a k-mer table of ``k`` letters whose events sit on the k-mer's base
    ``central`` = 2: (a) the share of the truly modified (site, strand) with a row of |t| >= t_min among the positions
    whose k-mer holds the site, p - 3 .. p + 2 in the strand's own direction, out of those whose own position has a row;
    (b) the share of the rows more than 2 k positions from every modified site of their strand with |t| >= t_min.
    -> (share a, sites counted, share b, far rows, largest far |t|, distances of the peak rows >= t_min to the nearest
    modified site of their strand)."""
    at = np.abs(cmp.t)
    hits = sites = 0
    far_rows, far_hits, far_max, peak_dist = 0, 0, 0.0, []
    for s, mask in ((0, truth['forward']), (1, truth['reverse'])):
        sel = cmp.strand == s
        pos, ts = cmp.position[sel], at[sel]
        mod = np.nonzero(mask)[0]
        big = np.zeros(mask.size, dtype=bool)
        big[pos[ts >= t_min]] = True
        have = np.zeros(mask.size, dtype=bool)
        have[pos] = True
        for p in mod:
            # the base at reference-part index g carries the k-mer g - 2 .. g + 3 of the read's own strand: on the
            # forward strand the positions p - 3 .. p + 2, mirrored on the reverse strand
            lo, hi = (p - 3, p + 2) if s == 0 else (p - 2, p + 3)
            lo, hi = max(lo, 0), min(hi, mask.size - 1)
            if have[p]:
                sites += 1
                hits += bool(big[lo:hi + 1].any())
        if mod.size:
            dist = np.abs(pos[:, None] - mod[None, :]).min(axis=1)
        else:
            dist = np.full(pos.size, mask.size)
        far = dist > 2 * k
        far_rows += int(far.sum())
        far_hits += int((ts[far] >= t_min).sum())
        if far.any() and np.isfinite(ts[far]).any():
            far_max = max(far_max, float(np.nanmax(ts[far])))
        peak_dist += dist[cmp.peak[sel] & (ts >= t_min)].tolist()
    return (hits / max(sites, 1), sites, far_hits / max(far_rows, 1), far_rows, far_max,
            np.array(peak_dist, dtype=np.int64))
