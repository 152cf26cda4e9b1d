"""The CPU side of the signal_locate tests: the restatement of tests/host_shims/locate_host.cpp on numpy arrays, the
rules of nvk_signal_locate_dev once more as a plain-Python DP, the stages of ``signal_locate_batch`` in numpy
(``cpu_signal_locate``: what nadavca_amd/locate.py does with the kernels and torch, stage for stage, with per-read
loops), and the constructed cases the test files share."""
import ctypes as C
import os
import subprocess

import numpy as np

import signal_map_ref as R

ROOT = R.ROOT
LOC_OK, LOC_NO_EVENTS, LOC_AMBIGUOUS = 0, 1, 2
BLOCK = 256
GAP_SLACK = 16
NINF = -np.inf

_p = lambda x: x.ctypes.data
_a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
offsets = R.offsets


def n_blocks_of(col_off):
    return int(((np.diff(col_off) + BLOCK - 1) // BLOCK).sum())


def valid_width(max_events):
    """V of the kernel instantiation that serves ``max_events`` (csrc/kernels_locate.hip)"""
    return 512 if max_events > 128 else 768


class LocateHost:
    def __init__(self, lib):
        self._f = lib.signal_locate_host
        self._f.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_double] * 4 \
            + [C.c_int64, C.c_void_p, C.c_void_p]
        self._f.restype = None

    def locate(self, level, q_off, mu, ac, mc, col_off, l_stay, l_step, l_skip, trim_cost):
        """-> (score f64 (queries, blocks), hit i32 (queries, blocks, 4))"""
        level, mu, ac, mc = (_a(x, np.float64) for x in (level, mu, ac, mc))
        q_off, col_off = _a(q_off, np.int64), _a(col_off, np.int64)
        nq, nb = q_off.size - 1, n_blocks_of(col_off)
        score, hit = np.zeros((nq, nb), dtype=np.float64), np.zeros((nq, nb, 4), dtype=np.int32)
        if nq and nb:
            self._f(nq, _p(level), _p(q_off), col_off.size - 1, _p(mu), _p(ac), _p(mc), _p(col_off), l_stay, l_step,
                    l_skip, trim_cost, nb, _p(score), _p(hit))
        return score, hit


def build_host(directory):
    so = os.path.join(str(directory), 'locate_host.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
                    os.path.join(ROOT, 'tests', 'host_shims', 'locate_host.cpp'), '-o', so], check=True)
    return LocateHost(C.CDLL(so))


def python_locate(level, mu, ac, mc, l_stay, l_step, l_skip, trim_cost):
    """The rules of nvk_signal_locate_dev for ONE query and ONE target, plain Python floats, cell by cell over the full
    matrix -> (score list, hit list of 4-tuples) per block"""
    Q, L = len(level), len(mu)
    S = [[NINF] * L for _ in range(Q)]
    src = [[None] * L for _ in range(Q)]
    best = [(NINF, (-1, -1, -1, -1))] * L
    for i in range(Q):
        for j in range(L):
            d = float(level[i]) - float(mu[j])
            em = float(ac[j]) - (d * d) * float(mc[j])
            cands = [(float(i) * trim_cost, (j, i))]
            for dj, cost in ((1, l_step), (0, l_stay), (2, l_skip)):
                ok = i > 0 and j - dj >= 0
                cands.append(((S[i - 1][j - dj] if ok else NINF) + cost, src[i - 1][j - dj] if ok else None))
            v, s = cands[0]
            for cv, cs in cands[1:]:
                if cv > v:
                    v, s = cv, cs
            S[i][j], src[i][j] = v + em, s
            end = S[i][j] + float(Q - 1 - i) * trim_cost
            if end > best[j][0]:
                best[j] = (end, (j, i, s[0], s[1]))
    scores, hits = [], []
    for b in range(0, L, BLOCK):
        top = (NINF, (-1, -1, -1, -1))
        for j in range(b, min(L, b + BLOCK)):
            if best[j][0] > top[0]:
                top = best[j]
        scores.append(top[0])
        hits.append(top[1])
    return scores, hits


def block_tables(col_off):
    """-> (target, first column, end column) per block"""
    tgt, lo, hi = [], [], []
    for t, L in enumerate(np.diff(col_off)):
        for b in range(0, int(L), BLOCK):
            tgt.append(t)
            lo.append(b)
            hi.append(min(int(L), b + BLOCK))
    return np.array(tgt, np.int64), np.array(lo, np.int64), np.array(hi, np.int64)


def reduce_blocks(score, hit, n_events, blk_target, blk_lo, blk_hi):
    """Stage 7, query by query -> (best block, best, second, margin, hit (q, 4))"""
    nq = score.shape[0]
    blk, best, second = np.zeros(nq, np.int64), np.zeros(nq), np.zeros(nq)
    margin, top = np.zeros(nq), np.zeros((nq, 4), np.int64)
    for q in range(nq):
        b = 0
        for x in range(1, score.shape[1]):
            if score[q, x] > score[q, b]:
                b = x
        end, reach = int(hit[q, b, 0]), 2 * int(n_events[q])
        sec = NINF
        for x in range(score.shape[1]):
            near = blk_target[x] == blk_target[b] and blk_lo[x] <= end + reach and blk_hi[x] - 1 >= end - reach
            if not near and score[q, x] > sec:
                sec = score[q, x]
        with np.errstate(invalid='ignore'):
            m = (score[q, b] - sec) / np.float64(n_events[q])
        blk[q], best[q], second[q], margin[q], top[q] = b, score[q, b], sec, NINF if np.isnan(m) else m, hit[q, b]
    return blk, best, second, margin, top


def chain_chunks(chunk_off, target, start, end, first_event, last_event, margin, min_margin):
    """Stage 8, read by read -> (status, anchor (flat chunk index or -1), joined per chunk)"""
    n = len(chunk_off) - 1
    status, anchor = np.full(n, LOC_NO_EVENTS, np.int32), np.full(n, -1, np.int64)
    joined = np.zeros(len(target), dtype=bool)
    for r in range(n):
        lo, hi = int(chunk_off[r]), int(chunk_off[r + 1])
        if hi == lo:
            continue
        a = lo
        for c in range(lo + 1, hi):
            if margin[c] > margin[a]:
                a = c
        anchor[r] = a
        if not margin[a] >= min_margin:
            status[r] = LOC_AMBIGUOUS
            continue
        status[r] = LOC_OK
        joined[a] = True
        last = a
        for c in range(a + 1, hi):
            gap = start[c] - end[last] - 1
            between = first_event[c] - last_event[last] - 1
            if target[c] == target[a] and margin[c] >= min_margin and -GAP_SLACK <= gap <= between + GAP_SLACK:
                joined[c] = True
                last = c
        last = a
        for c in range(a - 1, lo - 1, -1):
            gap = start[last] - end[c] - 1
            between = first_event[last] - last_event[c] - 1
            if target[c] == target[a] and margin[c] >= min_margin and -GAP_SLACK <= gap <= between + GAP_SLACK:
                joined[c] = True
                last = c
    return status, anchor, joined


def target_codes(contigs):
    """-> (codes, col_off): per contig its forward strand, then its reverse complement"""
    parts = []
    for c in contigs:
        c = np.asarray(c, dtype=np.int32)
        parts += [c, (3 - c[::-1]).astype(np.int32)]
    return np.concatenate(parts), offsets([p.size for p in parts])


def cpu_signal_locate(map_host, loc_host, raw, sig_off, contigs, model, max_events=128, min_events=32, min_margin=0.2,
                      p_stay=0.5, p_skip=0.02, sigma_scale=0.5, trim_cost=float(np.log(0.01)), window=2,
                      threshold=5.0, var_floor=0.02):
    """The stages of signal_locate_batch on the CPU -> dict of its per-read and per-chunk results.  ``contigs``: list of
    base-code arrays; ``map_host`` / ``loc_host``: signal_map_ref.build_host's and build_host's."""
    import math
    sig_off = _a(sig_off, np.int64)
    n = sig_off.size - 1
    norm = np.zeros(raw.size, dtype=np.float64)
    for r in range(n):
        x = np.asarray(raw[sig_off[r]:sig_off[r + 1]], dtype=np.float64)
        if x.size:
            med, mad = R.median_mad(x)
            norm[sig_off[r]:sig_off[r + 1]] = np.clip((x - med) / mad, -5.0, 5.0)
    flags = map_host.flags(norm, sig_off, window, threshold, var_floor)
    ev_pos = np.nonzero(flags)[0].astype(np.int64)
    ev_off = np.searchsorted(ev_pos, sig_off).astype(np.int64)
    _, _, level = map_host.levels(norm, sig_off, ev_pos)
    codes, col_off = target_codes(contigs)
    mu, ac, mc = R.base_tables(codes, col_off, model, sigma_scale)
    med_l, mad_l = R.median_mad(mu)
    q_level, q_len, chunk_read, chunk_first, n_chunks = [], [], [], [], np.zeros(n, np.int64)
    for r in range(n):
        e = level[ev_off[r]:ev_off[r + 1]]
        if e.size < min_events or e.size == 0:
            continue
        med_e, mad_e = R.median_mad(e)
        if not mad_e > 0.0:
            continue
        scale = mad_l / mad_e
        scaled = (e - med_e) * scale + med_l
        nc = (e.size + max_events - 1) // max_events
        n_chunks[r] = nc
        for c in range(nc):
            a, b = (e.size * c) // nc, (e.size * (c + 1)) // nc
            q_level.append(scaled[a:b])
            q_len.append(b - a)
            chunk_read.append(r)
            chunk_first.append(a)
    q_off = offsets(q_len)
    q_level = np.concatenate(q_level) if q_level else np.zeros(0)
    chunk_first = np.array(chunk_first, np.int64)
    costs = (math.log(p_stay), math.log(1.0 - p_stay - p_skip), math.log(p_skip))
    score, hit = loc_host.locate(q_level, q_off, mu, ac, mc, col_off, *costs, trim_cost)
    blk_target, blk_lo, blk_hi = block_tables(col_off)
    blk, best, second, margin, top = reduce_blocks(score, hit, np.diff(q_off), blk_target, blk_lo, blk_hi)
    q_target = blk_target[blk] if blk.size else np.zeros(0, np.int64)
    end, start = top[:, 0], top[:, 2]
    first_g, last_g = chunk_first + top[:, 3], chunk_first + top[:, 1]
    chunk_off = offsets(n_chunks)
    status, anchor, joined = chain_chunks(chunk_off, q_target, start, end, first_g, last_g, margin, min_margin)
    out = dict(status=status, contig=np.full(n, -1, np.int32), reverse=np.zeros(n, bool),
               ref_start=np.full(n, -1, np.int64), ref_end=np.full(n, -1, np.int64), margin=np.full(n, np.nan),
               score=np.full(n, np.nan), n_events=np.diff(ev_off).astype(np.int32), n_chunks=n_chunks.astype(np.int32),
               n_joined=np.zeros(n, np.int32), first_event=np.full(n, -1, np.int32), last_event=np.full(n, -1, np.int32),
               win_start=np.zeros(n, np.int64), win_len=np.zeros(n, np.int64))
    for r in range(n):
        if anchor[r] < 0:
            continue
        a = anchor[r]
        out['margin'][r], out['score'][r] = margin[a], best[a] / np.float64(q_off[a + 1] - q_off[a])
        if status[r] != LOC_OK:
            continue
        js = [c for c in range(chunk_off[r], chunk_off[r + 1]) if joined[c]]
        s, e = min(start[c] for c in js), max(end[c] for c in js) + 1
        t = int(q_target[a])
        Lc = len(contigs[t // 2])
        out['contig'][r], out['reverse'][r] = t // 2, t % 2 == 1
        out['win_start'][r], out['win_len'][r] = s, e - s
        out['ref_start'][r], out['ref_end'][r] = (Lc - e, Lc - s) if t % 2 else (s, e)
        out['n_joined'][r] = len(js)
        out['first_event'][r], out['last_event'][r] = min(first_g[c] for c in js), max(last_g[c] for c in js)
    out.update(chunk_off=chunk_off, chunk_target=q_target.astype(np.int32), chunk_start=start, chunk_end=end,
               chunk_first_event=first_g, chunk_last_event=last_g, chunk_events=np.diff(q_off).astype(np.int32),
               chunk_score=best, chunk_margin=margin, chunk_joined=joined, q_level=q_level, q_off=q_off, mu=mu, ac=ac,
               mc=mc, col_off=col_off, costs=costs, ev_off=ev_off, ev_level=level)
    return out


# ---- constructed cases ------------------------------------------------------------------------------------------
UNIT_COSTS = (-1.0, -1.0, -2.0, -1.0)   # l_stay, l_step, l_skip, trim_cost of the grid cases: ties with unit emissions
LOG_COSTS = (float(np.log(0.5)), float(np.log(0.48)), float(np.log(0.02)), float(np.log(0.01)))


def gauss(mu, sd=0.25):
    """Columns with means ``mu`` and Gaussians of width ``sd`` -> (mu, ac, mc)"""
    mu = np.asarray(mu, dtype=np.float64)
    sd = np.full(mu.size, sd, dtype=np.float64)
    return mu, -np.log(sd * np.sqrt(2 * np.pi)), 1.0 / (2 * sd * sd)


def pack(queries, targets, costs):
    """``queries``: list of level arrays; ``targets``: list of (mu, ac, mc) -> the operator's arguments as a dict"""
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64) for x in xs]) if len(xs) else np.zeros(0)
    return dict(level=cat(queries), q_off=offsets([len(x) for x in queries]), mu=cat([t[0] for t in targets]),
                ac=cat([t[1] for t in targets]), mc=cat([t[2] for t in targets]),
                col_off=offsets([len(t[0]) for t in targets]), costs=tuple(costs))


def emit(rng, mu, dwell=(1, 3), noise=0.05):
    """Events of a walk over the columns ``mu``: 1..dwell[1]-1 events per column"""
    d = rng.integers(dwell[0], dwell[1], len(mu))
    return np.repeat(np.asarray(mu, np.float64), d) + rng.normal(0, noise, int(d.sum()))


def grid_cases(rng, n, max_q, max_l, n_targets=2):
    """Levels, means and costs on a coarse grid, so that open, step, stay and skip tie exactly, often"""
    cases = []
    for t in range(n):
        queries = [rng.integers(-2, 3, int(rng.integers(1, max_q + 1))).astype(np.float64) for _ in range(3)]
        targets = []
        for _ in range(n_targets):
            L = int(rng.integers(1, max_l + 1))
            targets.append((rng.integers(-2, 3, L).astype(np.float64), np.zeros(L), np.full(L, 0.5)))
        cases.append(('grid %d' % t, pack(queries, targets, UNIT_COSTS)))
    return cases


def small_cases():
    """Cases small enough for the plain-Python DP (a few thousand cells each)"""
    rng = np.random.default_rng(21)
    cases = grid_cases(rng, 30, 24, 40)
    mu = rng.normal(0, 1, 60)
    noisy = np.concatenate([rng.normal(4, 0.3, 5), emit(rng, mu[20:32]), rng.normal(-4, 0.3, 4)])
    cases.append(('noise at both ends', pack([noisy, emit(rng, mu[:9])], [gauss(mu), gauss(mu[::-1])], LOG_COSTS)))
    cases.append(('one column, two columns', pack([rng.normal(0, 1, 6), rng.normal(0, 1, 1)],
                                                  [gauss(rng.normal(0, 1, 1)), gauss(rng.normal(0, 1, 2))], LOG_COSTS)))
    cases.append(('an empty query and an empty target', pack([np.zeros(0), rng.normal(0, 1, 4)],
                                                             [gauss(rng.normal(0, 1, 7)), gauss(np.zeros(0)),
                                                              gauss(rng.normal(0, 1, 3))], LOG_COSTS)))
    wide = rng.integers(-2, 3, 300).astype(np.float64)
    cases.append(('grid, two blocks', pack([rng.integers(-2, 3, 12).astype(np.float64)],
                                           [(wide, np.zeros(300), np.full(300, 0.5))], UNIT_COSTS)))
    return cases


def cone_case(max_events):
    """The cone's extreme: Q = max_events events, every second column of a stretch matches them and l_skip = 0, so the
    best path is all skips and spans 2 Q - 1 columns.  Target 0 holds it ending on the first valid column of the
    kernel's second tile, target 1 on that tile's last.  -> (case, [(block, end, start)] per target)"""
    rng = np.random.default_rng(31)
    Q, V = max_events, valid_width(max_events)
    level = rng.permutation(Q).astype(np.float64) * 0.125 - 8.0
    targets, want = [], []
    for t, end in enumerate((V, 2 * V - 1)):
        mu = np.full(3 * V, 60.0)
        start = end - 2 * (Q - 1)
        mu[start:end + 1:2] = level
        targets.append(gauss(mu))
        want.append((3 * V // BLOCK * t + end // BLOCK, end, start))
    return pack([level], targets, (-1.0, -1.0, 0.0, -1.0)), want


def kernel_cases(max_events):
    """-> list of (name, case) for one instantiation: the constructed cases of the operator's GPU test"""
    rng = np.random.default_rng([41, max_events])
    Q, V = max_events, valid_width(max_events)
    cases = []
    lengths = [1, 2, 3, 255, 256, 257, V - 1, V, V + 1, 2 * V + 3]
    mus = [rng.normal(0, 1, L) for L in lengths]
    queries = [np.zeros(0), rng.normal(0, 1, 1), emit(rng, mus[5][100:101], (2, 3)), emit(rng, mus[9][V - 60:], (1, 3))[:Q],
               emit(rng, mus[7][:Q], (1, 2)), np.zeros(0), emit(rng, mus[3][200:], (1, 3))[:Q]]
    cases.append(('target lengths; Q = 0, 1, 2, max_events', pack(queries, [gauss(m) for m in mus], LOG_COSTS)))
    # three targets: the joins inside one tile, and exactly on a tile's edge; queries that would cross a join
    for name, lengths in (('joins inside a tile', [100, 90, 57]), ('joins on tile edges', [V, 2 * V, 100])):
        mus = [rng.normal(0, 1, L) for L in lengths]
        flat = np.concatenate(mus)
        a, b = lengths[0], lengths[0] + lengths[1]
        queries = [emit(rng, flat[a - 20:a + 20], (1, 3))[:Q], emit(rng, flat[b - 25:b + 15], (1, 3))[:Q],
                   emit(rng, flat[max(a - Q // 2, 0):a + Q // 2], (1, 2))[:Q]]
        cases.append((name, pack(queries, [gauss(m) for m in mus], LOG_COSTS)))
    mu = rng.normal(0, 1, 2 * V + 40)
    seg = emit(rng, mu[V - 30:V + 10], (1, 3))
    noisy = np.concatenate([rng.normal(5, 0.3, 7), seg, rng.normal(-5, 0.3, 9)])[:Q]
    cases.append(('noise at both ends', pack([noisy], [gauss(mu)], LOG_COSTS)))
    cases += grid_cases(rng, 6, Q, 3 * V)
    two = [rng.normal(0, 1, 3000) for _ in range(2)]
    queries = []
    for _ in range(40):
        q = int(rng.integers(1, Q + 1))
        at = int(rng.integers(0, 3000 - q))
        queries.append(emit(rng, two[int(rng.integers(0, 2))][at:at + q], (1, 3), 0.2)[:q])
    cases.append(('40 random queries, two targets of 3000', pack(queries, [gauss(m) for m in two], LOG_COSTS)))
    return cases


def window_quality(res, loc, places, true_starts, lead):
    """``res``: map_base / map_sig / map_off over the located windows as sequences; ``loc``: ref_start / ref_end /
    reverse per read; ``places``: signal_map_ref.quality_places.  A window base is a genome position and so a base of
    the simulated read; one outside the read has no true start and counts as further off than any bound.
    -> (share of the windows' bases mapped, share of the mapped within 20 samples of the true start, share further off
    than 40)"""
    g0, length, _ = places
    mapped = total = near = far = 0
    for r in range(len(g0)):
        lo, hi = res['map_off'][r], res['map_off'][r + 1]
        b, s = res['map_base'][lo:hi].astype(np.int64), res['map_sig'][lo:hi].astype(np.int64)
        pos = loc['ref_end'][r] - 1 - b if loc['reverse'][r] else loc['ref_start'][r] + b
        base = g0[r] + length[r] - 1 - pos if loc['reverse'][r] else pos - g0[r]
        inside = (base >= 0) & (base < length[r])
        off = np.full(b.size, 1 << 30, dtype=np.int64)
        off[inside] = np.abs(s[inside] - (np.asarray(true_starts[r])[base[inside]] + lead[r]))
        total += int(loc['ref_end'][r] - loc['ref_start'][r])
        mapped += b.size
        near += int((off <= 20).sum())
        far += int((off > 40).sum())
    return mapped / max(total, 1), near / max(mapped, 1), far / max(mapped, 1)
