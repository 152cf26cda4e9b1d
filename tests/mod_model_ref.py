"""numpy restatement of the modified-base statistics contract (include/nadavca_hip.h, nvk_mod_kmer_rows_dev and
nvk_mod_kmer_reduce_dev) and of the update rule of ``estimate_mod_model``: the yardstick of tests/test_mod_model_cpu.py,
tests/test_gpu_mod_model_kernels.py and tests/test_gpu_mod_model.py.  Host arrays in the flat layout of the C-ABI.
Every floating-point expression is written in the contract's order; an ascending sum from 0.0 is ``np.cumsum`` over
the terms behind a leading 0.0."""
import numpy as np

from kmer_stats_ref import event_keys

MAX_SITES = 4


def ascending_sum(terms):
    """0.0 + t0 + t1 + ... left to right."""
    return float(np.cumsum(np.concatenate([[0.0], np.asarray(terms, dtype=np.float64)]))[-1])


def window_sites(site_pos_of_read, p0, k):
    """Indices (into the read's site list) of the sites inside [p0, p0 + k), ascending."""
    sp = np.asarray(site_pos_of_read, dtype=np.int64)
    return np.nonzero((sp >= p0) & (sp < p0 + k))[0]


def mod_rows(signal, sig_off, events, ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k, central,
             alphabet, trim, site_off, site_pos, site_gamma, mod_code, level):
    """-> (count int64 per base, key int64 per row, val f64 (rows, 4): w, n, sd, sq, windows_skipped)."""
    signal = np.asarray(signal, dtype=np.float64)
    level = np.asarray(level, dtype=np.float64)
    key0, a_, b_ = event_keys(sig_off, events, ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k,
                              central, alphabet, trim)
    total = int(ref_off[-1])
    count = np.zeros(total, dtype=np.int64)
    keys, vals = [], []
    skipped = 0
    for j in range(len(ref_off) - 1):
        r0, R = int(ref_off[j]), int(ref_off[j + 1] - ref_off[j])
        sp = np.asarray(site_pos[site_off[j]:site_off[j + 1]], dtype=np.int64)
        sg = np.asarray(site_gamma[site_off[j]:site_off[j + 1]], dtype=np.float64)
        x = signal[sig_off[j]:sig_off[j + 1]]
        for g in range(R):
            p0 = g - central
            at = window_sites(sp, p0, k)
            m = at.size
            if m > MAX_SITES:
                skipped += 1
            if m == 0 or m > MAX_SITES:
                continue
            count[r0 + g] = (1 << m) - 1
            k0 = int(key0[r0 + g])
            if k0 >= 0:
                c0 = level[k0]
                dv = x[a_[r0 + g]:b_[r0 + g]] - c0
                a, b = ascending_sum(dv), ascending_sum(dv * dv)
                n = float(b_[r0 + g] - a_[r0 + g])
            for mask in range(1, 1 << m):
                if k0 < 0:
                    keys.append(-1)
                    vals.append((0.0, 0.0, 0.0, 0.0))
                    continue
                key, w = k0, np.float64(1.0)
                for t in range(m):
                    if (mask >> t) & 1:
                        place = int(sp[at[t]]) - p0
                        key += (mod_code - int(reference[r0 + sp[at[t]]])) * alphabet ** (k - 1 - place)
                        w = w * sg[at[t]]
                    else:
                        w = w * (np.float64(1.0) - sg[at[t]])
                d = c0 - level[key]
                n_ = np.float64(n)
                sd = np.float64(a) + n_ * d
                sq = np.float64(b) + (np.float64(2.0) * d) * np.float64(a) + (n_ * d) * d
                keys.append(key)
                vals.append((float(w), n, float(sd), float(sq)))
    return (count, np.array(keys, dtype=np.int64), np.array(vals, dtype=np.float64).reshape(-1, 4), skipped)


def mod_rows_of(batch, events, status, k, central, alphabet, trim, site_off, site_pos, site_gamma, mod_code, level):
    """mod_rows for a flat batch object (synthetic.Batch / dtw.FlatBatch layout, host arrays)."""
    return mod_rows(batch.signal, batch.sig_off, events, batch.ref_off, batch.reference, batch.context_before,
                    batch.cb_off, batch.context_after, batch.ca_off, status, k, central, alphabet, trim, site_off,
                    site_pos, site_gamma, mod_code, level)


def wave_sum64(partials):
    """The butterfly p[l] = p[l] + p[l xor d], d = 32 .. 1, over axis 0 (64 entries).  -> entry 0 (all are equal)."""
    p = np.array(partials, dtype=np.float64)
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ d]
    return p[0]


def mod_reduce(val, run_off):
    """-> (sums f64 (n_keys, 4): W, Nw, Sd, Sq, rows int64 (n_keys,)) for the runs run_off[q] .. run_off[q + 1] of
    ``val`` (rows, 4) in stable key order."""
    val = np.asarray(val, dtype=np.float64).reshape(-1, 4)
    n_keys = len(run_off) - 1
    sums = np.zeros((n_keys, 4))
    rows = np.zeros(n_keys, dtype=np.int64)
    for q in range(n_keys):
        v = val[run_off[q]:run_off[q + 1]]
        c = v.shape[0]
        terms = np.stack([v[:, 0], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2], v[:, 0] * v[:, 3]], 1)
        # row i goes to partial i mod 64 in ascending i; a lane without a row in the last step adds nothing (padding
        # with +0.0 adds nothing to a partial that started at +0.0)
        pad = (-c) % 64
        terms = np.concatenate([terms, np.zeros((pad, 4))]).reshape(-1, 64, 4)
        p = np.zeros((64, 4))
        for step in terms:
            p = p + step
        sums[q] = wave_sum64(p)
        rows[q] = c
    return sums, rows


def mod_stats(key, val):
    """The caller's plumbing between the two kernels and the reduction: stable sort, gather, runs of the keys >= 0.
    -> (distinct keys ascending, sums (n_keys, 4), rows (n_keys,))."""
    order = np.argsort(key, kind='stable')
    skey, sval = key[order], val[order]
    n_neg = int((skey < 0).sum())
    ukey, counts = np.unique(skey[n_neg:], return_counts=True)
    run_off = np.concatenate([[n_neg], n_neg + np.cumsum(counts)]).astype(np.int64)
    sums, rows = mod_reduce(sval, run_off)
    return ukey, sums, rows


def holds_code(key, k, alphabet, code):
    return any((int(key) // alphabet ** m) % alphabet == code for m in range(k))


def update_rule(mean, sigma, key, sums, k, alphabet, mod_code, min_weight, min_sigma):
    """The update rule, one k-mer at a time.  -> (mean, sigma, updated)."""
    mean, sigma = np.array(mean, dtype=np.float64), np.array(sigma, dtype=np.float64)
    updated = np.zeros(mean.size, dtype=bool)
    for q, (W, Nw, Sd, Sq) in zip(np.asarray(key).tolist(), np.asarray(sums, dtype=np.float64)):
        if not holds_code(q, k, alphabet, mod_code) or not W >= min_weight:
            continue
        shift = Sd / Nw
        var = max(Sq / Nw - shift * shift, np.float64(0.0))
        mean[q] = mean[q] + shift
        sigma[q] = max(np.sqrt(var), np.float64(min_sigma))
        updated[q] = True
    return mean, sigma, updated
