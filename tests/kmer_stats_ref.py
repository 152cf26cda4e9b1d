"""numpy restatement of the k-mer statistics contract (include/nadavca_hip.h, nvk_kmer_event_stats_dev), the yardstick
of tests/test_kmer_train_cpu.py and tests/test_gpu_kmer_train.py.  Host arrays in the flat layout of the C-ABI; the
sums are numpy's own (np.sum), so agreeing with this is agreeing with numpy."""
import numpy as np


def event_keys(sig_off, events, ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k, central,
               alphabet, trim):
    """-> (key int64, a int64, b int64) per event: the k-mer key of a counted event (-1 otherwise) and its clamped
    sample range [a, b) in the read's slice."""
    events = np.asarray(events, dtype=np.int64).reshape(-1, 2)
    total = int(ref_off[-1])
    key = np.full(total, -1, dtype=np.int64)
    a = np.zeros(total, dtype=np.int64)
    b = np.zeros(total, dtype=np.int64)
    for j in range(len(ref_off) - 1):
        if status is not None and status[j] != 0:
            continue
        r0, R = int(ref_off[j]), int(ref_off[j + 1] - ref_off[j])
        N = int(sig_off[j + 1] - sig_off[j])
        cb = np.asarray(ctx_before[cb_off[j]:cb_off[j + 1]], dtype=np.int64)
        ca = np.asarray(ctx_after[ca_off[j]:ca_off[j + 1]], dtype=np.int64)
        ext = np.concatenate([cb, np.asarray(reference[r0:r0 + R], dtype=np.int64), ca])
        g = np.arange(R)
        s = np.clip(events[r0:r0 + R, 0], 0, N)
        e = np.clip(events[r0:r0 + R, 1], 0, N)
        p0 = g - central
        ok = (g >= trim) & (g < R - trim) & (e > s) & (p0 >= -cb.size) & (p0 + k - 1 < R + ca.size)
        kk = np.zeros(R, dtype=np.int64)
        for m in range(k):
            p = np.clip(p0 + m + cb.size, 0, max(ext.size - 1, 0))
            base = ext[p] if ext.size else np.zeros(R, dtype=np.int64)
            ok &= (base >= 0) & (base < alphabet)
            kk = kk * alphabet + base
        key[r0:r0 + R] = np.where(ok, kk, -1)
        a[r0:r0 + R] = s
        b[r0:r0 + R] = e
    return key, a, b


def kmer_stats(signal, sig_off, events, ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k, central,
               alphabet, trim):
    """Both passes of the contract.  -> dict of per-k-mer arrays S, N, e, m (NaN where N = 0), Q, sigma and the
    per-event key / s / q arrays."""
    signal = np.asarray(signal, dtype=np.float64)
    key, a, b = event_keys(sig_off, events, ref_off, reference, ctx_before, cb_off, ctx_after, ca_off, status, k,
                           central, alphabet, trim)
    owner = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    counted = np.nonzero(key >= 0)[0]
    n_kmers = alphabet ** k
    s = np.zeros(key.size)
    for i in counted:
        base = int(sig_off[owner[i]])
        s[i] = np.sum(signal[base + a[i]:base + b[i]])
    order = counted[np.argsort(key[counted], kind='stable')]
    ks = key[order]
    bounds = np.searchsorted(ks, np.arange(n_kmers + 1))
    S = np.zeros(n_kmers)
    N = np.zeros(n_kmers, dtype=np.int64)
    e = np.diff(bounds).astype(np.int64)
    lens = b - a
    for kid in np.nonzero(e)[0]:
        sel = order[bounds[kid]:bounds[kid + 1]]
        S[kid] = np.sum(s[sel])
        N[kid] = int(lens[sel].sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        m = S / N
    q = np.zeros(key.size)
    for i in counted:
        base = int(sig_off[owner[i]])
        d = signal[base + a[i]:base + b[i]] - m[key[i]]
        q[i] = np.sum(d * d)
    Q = np.zeros(n_kmers)
    for kid in np.nonzero(e)[0]:
        Q[kid] = np.sum(q[order[bounds[kid]:bounds[kid + 1]]])
    with np.errstate(invalid='ignore', divide='ignore'):
        sigma = np.sqrt(Q / N)
    return dict(S=S, N=N, e=e, m=m, Q=Q, sigma=sigma, key=key, s=s, q=q)


def kmer_stats_of(batch, events, status, k, central, alphabet, trim):
    """kmer_stats for a flat batch object (synthetic.Batch / dtw.FlatBatch layout, host arrays)."""
    return kmer_stats(batch.signal, batch.sig_off, events, batch.ref_off, batch.reference, batch.context_before,
                      batch.cb_off, batch.context_after, batch.ca_off, status, k, central, alphabet, trim)
