"""The CPU side of the signal_map tests: the restatements of tests/host_shims/events_host.cpp and eventalign_host.cpp
on numpy arrays, the stages of ``signal_map_batch`` between them in numpy (``cpu_signal_map``: what
nadavca_amd/signal_map.py does with the kernels, stage for stage), and the constructed cases both test files share."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_OK, MAP_NO_EVENTS, MAP_LOST = 0, 1, 2
TILE = 256   # samples per block of event_flags_kernel (csrc/kernels_events.hip)

_p = lambda x: x.ctypes.data
_a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)


class MapHost:
    def __init__(self, lib):
        self._flags = lib.event_flags_host
        self._flags.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
        self._flags.restype = None
        self._levels = lib.event_levels_host
        self._levels.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        self._levels.restype = None
        self._align = lib.event_align_host
        self._align.argtypes = [C.c_int64] + [C.c_void_p] * 9 + [C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 4
        self._align.restype = None

    def flags(self, signal, sig_off, window, threshold, var_floor):
        signal, sig_off = _a(signal, np.float64), _a(sig_off, np.int64)
        out = np.zeros(max(signal.size, 1), dtype=np.int32)
        self._flags(sig_off.size - 1, _p(signal), _p(sig_off), window, threshold, var_floor, _p(out))
        return out[:signal.size]

    def levels(self, signal, sig_off, ev_pos):
        """-> (start i32, length i32, level f64) per event; ``ev_pos``: the flat positions of the borders"""
        signal, sig_off, ev_pos = _a(signal, np.float64), _a(sig_off, np.int64), _a(ev_pos, np.int64)
        n = ev_pos.size
        start, length = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        level = np.zeros(max(n, 1), dtype=np.float64)
        self._levels(sig_off.size - 1, signal.size, _p(signal), _p(sig_off), n, _p(ev_pos), _p(start), _p(length),
                     _p(level))
        return start[:n], length[:n], level[:n]

    def align(self, level, ev_off, mu, ac, mc, base_off, l_stay, l_step, band, trim_cost, skip_cost, status_in=None,
              corners=False):
        """-> (hit (n, 4): status, events, first, last; score f64 (n,); base_event i32 (total bases,)) and, with
        ``corners`` (one read), the (E + K + 1, 2) corners (event, base) of its bands"""
        level, mu, ac, mc = (_a(x, np.float64) for x in (level, mu, ac, mc))
        ev_off, base_off = _a(ev_off, np.int64), _a(base_off, np.int64)
        l_stay, l_step = _a(l_stay, np.float64), _a(l_step, np.float64)
        n = ev_off.size - 1
        hit = np.zeros((n, 4), dtype=np.int32)
        score = np.zeros(n, dtype=np.float64)
        be = np.zeros(max(mu.size, 1), dtype=np.int32)
        st = None
        if status_in is not None:
            status_in = _a(status_in, np.int32)
            st = _p(status_in)
        corner = np.zeros((int(ev_off[-1] + base_off[-1]) + 1, 2), dtype=np.int32) if corners else None
        assert not corners or n == 1
        self._align(n, _p(level), _p(ev_off), _p(mu), _p(ac), _p(mc), _p(base_off), _p(l_stay), _p(l_step), st, band,
                    trim_cost, skip_cost, _p(hit), _p(score), _p(be), _p(corner) if corners else None)
        return (hit, score, be[:mu.size]) + ((corner,) if corners else ())


def build_host(directory):
    so = os.path.join(str(directory), 'signal_map_host.so')
    shims = os.path.join(ROOT, 'tests', 'host_shims')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
                    os.path.join(shims, 'events_host.cpp'), os.path.join(shims, 'eventalign_host.cpp'), '-o', so],
                   check=True)
    return MapHost(C.CDLL(so))


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def median_mad(x):
    med = np.median(x)
    return med, np.median(np.abs(x - med))


def base_tables(sequence, seq_off, model, sigma_scale=1.0):
    """-> (mu, ac, mc) per base: the k-mer of kmer.h without contexts (0 outside the read, out-of-range codes as 0)"""
    k, central, alphabet, mean, sigma = model
    sd = np.asarray(sigma, dtype=np.float64) * sigma_scale
    ac_t, mc_t = -np.log(sd * np.sqrt(2.0 * np.pi)), 1.0 / (2.0 * sd * sd)
    ids = np.zeros(sequence.size, dtype=np.int64)
    for r in range(seq_off.size - 1):
        s = np.array(sequence[seq_off[r]:seq_off[r + 1]], dtype=np.int64)
        s[(s < 0) | (s >= alphabet)] = 0
        ext = np.concatenate([np.zeros(central, np.int64), s, np.zeros(k - central - 1, np.int64)])
        v = np.zeros(s.size, dtype=np.int64)
        for t in range(k):
            v = v * alphabet + ext[t:t + s.size]
        ids[seq_off[r]:seq_off[r + 1]] = v
    return np.asarray(mean, np.float64)[ids], ac_t[ids], mc_t[ids]


def transition_costs(E, K):
    E, K = np.asarray(E, dtype=np.float64), np.asarray(K, dtype=np.float64)
    p_stay = np.maximum(1.0 - 1.0 / np.maximum(E / np.maximum(K, 1.0), 1.0001), 0.05)
    return np.log(p_stay), np.log(np.maximum(1.0 - p_stay - 1e-10, 1e-3))


def cpu_signal_map(host, raw, sig_off, sequence, seq_off, model, window=2, threshold=5.0, var_floor=0.02, band=128,
                   sigma_scale=0.5, trim_cost=float(np.log(0.01)), skip_cost=float(np.log(1e-10))):
    """The stages of signal_map_batch on the CPU -> dict of its per-read and flat results."""
    sig_off, seq_off = _a(sig_off, np.int64), _a(seq_off, np.int64)
    n = sig_off.size - 1
    norm = np.zeros(raw.size, dtype=np.float64)
    for r in range(n):
        x = np.asarray(raw[sig_off[r]:sig_off[r + 1]], dtype=np.float64)
        if x.size:
            med, mad = median_mad(x)
            norm[sig_off[r]:sig_off[r + 1]] = np.clip((x - med) / mad, -5.0, 5.0)
    flags = host.flags(norm, sig_off, window, threshold, var_floor)
    ev_pos = np.nonzero(flags)[0].astype(np.int64)
    ev_off = np.searchsorted(ev_pos, sig_off).astype(np.int64)
    start, length, level = host.levels(norm, sig_off, ev_pos)
    mu, ac, mc = base_tables(np.asarray(sequence), seq_off, model, sigma_scale)
    status_in = np.zeros(n, dtype=np.int32)
    shift, scale = np.zeros(n), np.ones(n)
    scaled = np.array(level)
    for r in range(n):
        e, m = level[ev_off[r]:ev_off[r + 1]], mu[seq_off[r]:seq_off[r + 1]]
        if e.size == 0 or m.size == 0:
            status_in[r] = MAP_NO_EVENTS
            continue
        med_e, mad_e = median_mad(e)
        med_l, mad_l = median_mad(m)
        if not mad_e > 0.0:
            status_in[r] = MAP_NO_EVENTS
            continue
        scale[r] = mad_l / mad_e
        shift[r] = med_l - med_e * scale[r]
        scaled[ev_off[r]:ev_off[r + 1]] = (e - med_e) * scale[r] + med_l
    l_stay, l_step = transition_costs(np.diff(ev_off), np.diff(seq_off))
    hit, score, be = host.align(scaled, ev_off, mu, ac, mc, seq_off, l_stay, l_step, band, trim_cost, skip_cost,
                                status_in)
    owner = np.repeat(np.arange(n), np.diff(seq_off))
    inner = np.arange(be.size) - seq_off[:-1][owner]
    keep = be >= 0
    map_base = inner[keep].astype(np.int32)
    map_sig = start[ev_off[:-1][owner[keep]] + be[keep]]
    map_off = offsets(np.bincount(owner[keep], minlength=n))
    return dict(status=hit[:, 0], n_events=hit[:, 1], first_event=hit[:, 2], last_event=hit[:, 3], path_score=score,
                shift=shift, scale=scale, map_base=map_base, map_sig=map_sig, map_off=map_off, base_event=be,
                ev_off=ev_off, ev_start=start, ev_len=length, ev_level=level, scaled=scaled, mu=mu, ac=ac, mc=mc,
                l_stay=l_stay, l_step=l_step, status_in=status_in, norm=norm, flags=flags, ev_pos=ev_pos)


def quality(res, seq_off, true_starts, lead=None):
    """-> (share of bases mapped, share of mapped within 20 samples of the true start, share further off than 40);
    ``true_starts``: per read the samples its bases start at; ``lead``: samples prepended per read"""
    mapped = total = near = far = 0
    for r in range(seq_off.size - 1):
        lo, hi = res['map_off'][r], res['map_off'][r + 1]
        b, s = res['map_base'][lo:hi].astype(np.int64), res['map_sig'][lo:hi].astype(np.int64)
        t = np.asarray(true_starts[r])[b] + (0 if lead is None else lead[r])
        total += seq_off[r + 1] - seq_off[r]
        mapped += b.size
        near += int((np.abs(s - t) <= 20).sum())
        far += int((np.abs(s - t) > 40).sum())
    return mapped / max(total, 1), near / max(mapped, 1), far / max(mapped, 1)


def brute_force_align(level, mu, ac, mc, l_stay, l_step, trim_cost, skip_cost):
    """The rules of nvk_event_align_dev over the FULL matrix of one read, plain Python: the same moves, tie order and
    free ends and lost rule, no band.  -> (status, first_event, last_event, out_score, base_event list)"""
    E, K = len(level), len(mu)
    if E == 0 or K == 0:
        return MAP_NO_EVENTS, -1, -1, -np.inf, [-1] * K
    NINF = -np.inf
    S = [[NINF] * K for _ in range(E)]
    M = [[0] * K for _ in range(E)]
    for i in range(E):
        for j in range(K):
            d = level[i] - mu[j]
            em = ac[j] - d * d * mc[j]
            src = float(i) * trim_cost if j == 0 else (S[i - 1][j - 1] if i > 0 else NINF)
            step = (src + l_step) + em
            stay = ((S[i - 1][j] if i > 0 else NINF) + l_stay) + em
            skip = S[i][j - 1] + skip_cost if j > 0 else NINF
            v, w = step, 0
            if stay > v:
                v, w = stay, 1
            if skip > v:
                v, w = skip, 2
            S[i][j], M[i][j] = v, w
    best, best_i = NINF, -1
    for i in range(E):
        end = S[i][K - 1] + float(E - 1 - i) * trim_cost
        if end > best:
            best, best_i = end, i
    if best_i < 0:
        return MAP_LOST, -1, -1, NINF, [-1] * K
    be = [-1] * K
    i, j, skipped = best_i, K - 1, 0
    while True:
        w = M[i][j]
        if w == 2:
            j -= 1
            skipped += 1
            continue
        be[j] = i
        if w == 1:
            i -= 1
            continue
        if j == 0:
            break
        i, j = i - 1, j - 1
    if 8 * skipped > K:
        return MAP_LOST, -1, -1, NINF, [-1] * K
    return MAP_OK, i, best_i, best, be


def python_flags(x, w, threshold, var_floor):
    """The border rules of nvk_event_flags_dev for one read, plain Python, sample by sample."""
    n = len(x)
    x = [float(v) for v in x]

    def s(i):
        if i < w or i > n - w:
            return 0.0
        sl = sr = 0.0
        for t in range(w):
            sl += x[i - w + t]
        for t in range(w):
            sr += x[i + t]
        ml, mr = sl / float(w), sr / float(w)
        vl = vr = 0.0
        for t in range(w):
            vl += (x[i - w + t] - ml) * (x[i - w + t] - ml)
        for t in range(w):
            vr += (x[i + t] - mr) * (x[i + t] - mr)
        vl, vr = vl / float(w), vr / float(w)
        d = mr - ml
        return (float(w) * (d * d)) / ((vl + vr) + var_floor)

    out = []
    for i in range(n):
        v = s(i)
        border = v >= threshold and all(v > s(u) for u in range(i - w + 1, i)) \
            and all(v >= s(u) for u in range(i + 1, i + w))
        out.append(1 if i == 0 or border else 0)
    return out


def steps(levels, lengths):
    return np.repeat(np.asarray(levels, dtype=np.float64), lengths)


def detector_cases():
    """-> list of (name, signal f64, sig_off, window, threshold, var_floor): the constructed signals of the issue"""
    rng = np.random.default_rng(11)
    cases = []
    add = lambda name, reads, w, th=5.0, vf=0.02: cases.append(
        (name, np.concatenate(reads) if reads else np.zeros(0), offsets([len(r) for r in reads]), w, th, vf))
    add('shorter than 2w', [np.array([0.0, 3.0, -2.0])], 2)
    add('shorter than 2w, window 8', [rng.normal(0, 1, 15)], 8)
    add('constant', [np.full(40, 1.25)], 2)
    add('constant, then an empty read and a one-sample read', [np.full(9, -0.5), np.zeros(0), np.array([2.0])], 3)
    # integer plateaus: s(3) == s(4) for 0 0 0 1 2 2 2 with w = 2, and again mirrored; the first wins
    add('equal adjacent statistics', [steps([0, 1, 2, 1, 0, 3, 3.5, 4], [3, 1, 5, 1, 4, 6, 1, 5])], 2)
    add('equal adjacent statistics, window 3', [steps([0, 1, 2, 5, 8, 9], [6, 1, 1, 1, 1, 6])], 3)
    # a border at a tile edge of the flags kernel and one sample either side, alone and behind another read
    for at in (TILE - 1, TILE, TILE + 1, 2 * TILE):
        add('border at %d' % at, [steps([0.0, 2.0, -1.0], [at, 40, 2 * TILE - at + 7])], 2)
        add('border at %d, window 8' % at, [steps([0.0, 2.0, -1.0], [at, 40, 2 * TILE - at + 7])
                                            + rng.normal(0, 0.05, 2 * TILE + 47)], 8, 4.0)
        add('border at %d behind a read' % at, [rng.normal(0, 1, 100), steps([1.0, -1.0], [at - 100, 60])], 2)
    # a read boundary at the tile edge and next to it
    for at in (TILE - 1, TILE, TILE + 1):
        add('reads meet at %d' % at, [steps([0.0, 1.5], [at - 3, 3]) + rng.normal(0, 0.1, at),
                                      steps([1.5, 0.0, 2.0], [3, 5, 30]) + rng.normal(0, 0.1, 38)], 2)
    for w in (1, 2, 3, 5, 8):
        add('noise, window %d' % w, [np.rint(rng.normal(0, 2, int(m))) / 2 for m in rng.integers(0, 700, 6)], w, 1.5)
    return cases


def align_case(level, mu, sd=None):
    """One read for MapHost.align: levels, the bases' means and the constants of Gaussians of width ``sd`` (0.25)"""
    level, mu = np.asarray(level, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    sd = np.full(mu.size, 0.25) if sd is None else np.asarray(sd, dtype=np.float64)
    l_stay, l_step = transition_costs(level.size, mu.size)
    return dict(level=level, mu=mu, ac=-np.log(sd * np.sqrt(2 * np.pi)), mc=1.0 / (2 * sd * sd), l_stay=float(l_stay),
                l_step=float(l_step))


def small_align_cases():
    """-> list of (name, case): reads small enough (E + K < 60) that a band of 64 covers the whole matrix"""
    rng = np.random.default_rng(5)
    cases = []

    def emit(mu, dwell, noise=0.05):
        return np.concatenate([m + rng.normal(0, noise, int(d)) for m, d in zip(mu, dwell)]) if len(mu) else np.zeros(0)

    mu = rng.normal(0, 1, 16)
    cases.append(('E < K: one skip forced', align_case(emit(np.delete(mu, 7), np.ones(15)), mu)))
    mu = rng.normal(0, 1, 24)
    cases.append(('E < K: two skips forced', align_case(emit(np.delete(mu, [5, 17]), np.ones(22)), mu)))
    cases.append(('E < K: too many skips, lost', align_case(rng.normal(0, 1, 5), rng.normal(0, 1, 8))))
    cases.append(('K = 1', align_case(np.array([3.0, 0.52, 0.47, 0.5, -2.0]), np.array([0.5]))))
    cases.append(('K = 1, E = 1', align_case(np.array([0.1]), np.array([0.5]))))
    cases.append(('K < k', align_case(emit([0.3, -0.8, 1.1], [2, 3, 1]), np.array([0.3, -0.8, 1.1]))))
    cases.append(('E = 1, K = 3: lost', align_case(np.array([0.3]), np.array([0.3, -0.8, 1.1]))))
    mu = rng.normal(0, 1, 12)
    cases.append(('leader and trailer', align_case(np.concatenate([rng.normal(6, 0.5, 9), emit(mu, rng.integers(1, 4, 12)),
                                                                   rng.normal(-6, 0.5, 8)]), mu)))
    mu = np.array([0.5, 0.5, 0.5, -1.0, -1.0, 0.25, 0.25, 0.25, 0.25, 1.5])
    cases.append(('equal neighbouring levels', align_case(emit(mu, rng.integers(1, 4, 10), 0.0), mu)))
    # levels and costs on a coarse grid, so that step, stay and skip tie exactly, often
    for t in range(40):
        E, K = int(rng.integers(1, 30)), int(rng.integers(1, 28))
        c = dict(level=rng.integers(-2, 3, E).astype(np.float64), mu=rng.integers(-2, 3, K).astype(np.float64),
                 ac=np.zeros(K), mc=np.full(K, 0.5), l_stay=-1.0, l_step=-1.0)
        cases.append(('grid %d' % t, c))
    return cases


GRID_COSTS = (-1.0, -2.0)   # trim_cost, skip_cost of the 'grid' cases: ties with the unit costs above


def pack_align_cases(cases):
    """Cases laid end to end -> the arguments of MapHost.align / device.event_align_dev as a dict of numpy arrays"""
    cat = lambda key: np.concatenate([np.atleast_1d(c[key]) for c in cases]).astype(np.float64)
    return dict(level=cat('level'), ev_off=offsets([c['level'].size for c in cases]), mu=cat('mu'), ac=cat('ac'),
                mc=cat('mc'), base_off=offsets([c['mu'].size for c in cases]), l_stay=cat('l_stay'),
                l_step=cat('l_step'))


def cut_read(model, cut_from=100, cut=100, length=300, seed=0):
    """A simulated read with the signal of ``cut`` bases taken out -> (raw int16, sequence codes)"""
    from nadavca_amd import synthetic
    genome = np.random.default_rng(3).integers(0, 4, 3000).astype(np.int32)
    s = synthetic.make_read_spec(np.random.default_rng([5, seed]), genome, model, 0, length=length, spread=0)
    st, raw = s['true_starts'], np.rint(s['raw_signal']).astype(np.int16)
    seq = np.array([{'A': 0, 'C': 1, 'G': 2, 'T': 3}[b] for b in s['sequence']], dtype=np.int32)
    return np.concatenate([raw[:st[cut_from]], raw[st[cut_from + cut]:]]), seq, raw


QUALITY_SEED, QUALITY_READS = 7, 300


def quality_batch(model, n=QUALITY_READS):
    """The batch of the quality tests: ``n`` reads of about 200 bases over a 3 000-base genome.
    -> (ReadBatch, aligner, true_starts per read, (raw, sig_off, lead) of the same reads with 150-300 random-level
    samples before and after each)"""
    from nadavca_amd import synthetic
    kw = dict(length=200, spread=20)
    rb, aligner, genome = synthetic.make_read_batch(n, model, seed=QUALITY_SEED, genome_length=3000, **kw)
    true_starts = [synthetic.make_read_spec(np.random.default_rng([QUALITY_SEED, i]), genome, model, i, **kw)
                   ['true_starts'] for i in range(n)]
    rng = np.random.default_rng(99)
    raws, lead = [], []
    for r in range(n):
        x = rb.raw_signal[rb.sig_off[r]:rb.sig_off[r + 1]]
        a, b = rng.integers(150, 301, 2)
        mk = lambda m: np.rint(12.0 * np.clip(rng.normal(0.0, 1.0, m), -5, 5) + 90.0).astype(x.dtype)
        raws.append(np.concatenate([mk(a), x, mk(b)]))
        lead.append(int(a))
    return rb, aligner, true_starts, (np.concatenate(raws), offsets([x.size for x in raws]), np.array(lead))


def quality_places(model, n=QUALITY_READS):
    """Where the reads of ``quality_batch`` lie -> (g0, length, reverse) arrays: read base b of a forward read is
    genome position g0 + b, of a reverse one g0 + length - 1 - b"""
    from nadavca_amd import synthetic
    genome = np.random.default_rng(QUALITY_SEED).integers(0, 4, 3000).astype(np.int32)
    specs = [synthetic.make_read_spec(np.random.default_rng([QUALITY_SEED, i]), genome, model, i, length=200, spread=20)
             for i in range(n)]
    return (np.array([s['g0'] for s in specs]), np.array([s['length'] for s in specs]),
            np.array([s['reverse'] for s in specs]))
