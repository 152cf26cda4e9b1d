"""Reads for the row-switch tests (tests/test_switch_order_cpu.py, tests/test_gpu_row_switch.py) and a host
restatement of the planner's row geometry (csrc/kernels_plan.hip, plan_rows): bands, spans, skew, gap bound and the
least per-row offsets.

The sweeps of csrc/kernels_align3.hip (one wave per read) serve a row switch as a scalar event: the lane that leaves
its row next is the one holding the oldest open row.  That needs the rows to be LEFT in row order,

    forward:  off[r] + be[r]  non-decreasing in r        reverse:  off[r] + bs[r]  non-decreasing in r,

which follows from the planner's gap bound (the derivation stands next to it in kernels_plan.hip).  The cases here are
the smallest shapes at which serving by the oldest row could go wrong."""
import numpy as np

SEED = 20261022
C_CAP, TEAM_W, PLAN_VT = 3, 4, 2048   # ALIGN1_C_CAP, ALIGN3_TEAM_W (csrc/nvk_internal.h), PLAN_VT (kernels_plan.hip)


def rows_of(tr, R):
    return 2 * R if tr else R + 1


def bands(anchors, N, R, bw):
    """dtw.cpp:7-35 as plan_bands restates it: later anchor overwrites, prefix maximum / suffix minimum."""
    bs = np.zeros(R + 1, dtype=np.int64)
    be = np.full(R + 1, N, dtype=np.int64)
    for s, at in np.asarray(anchors).reshape(-1, 2):
        bs[at] = max(0, int(s) - bw)
        be[at] = min(N, int(s) + bw)
    return np.maximum.accumulate(bs), np.minimum.accumulate(be[::-1])[::-1]


def plan_geometry(case, bw, mel, tr):
    """-> dict(T, BS, BE, LO, HI, g, c, cw, fixp, off) for one read: plan_rows' integers, row by row."""
    N, R = len(case['signal']), len(case['reference'])
    bs, be = bands(case['approximate_alignment'], N, R, bw)
    T = rows_of(tr, R)
    rows = np.arange(T)
    j = (rows + 1) >> 1 if tr else rows
    BS, BE = bs[j], be[j]
    rmel = np.where((rows + 1 < T) & ~((rows & 1).astype(bool) & tr), mel, 0)
    LO, HI = BS.copy(), BE.copy()
    pm = rmel[:-1]
    LO[1:] = np.minimum(BS[1:], BS[:-1] + pm) - np.maximum(pm - 1, 0)
    HI[:-1] = np.maximum(BE[:-1], BE[1:] - pm) + np.maximum(pm - 1, 0)
    idle = 2 if tr else 1

    def skew(TL):
        need = max(mel - 1, 1)
        if T > TL:
            d = HI[:-TL] - LO[TL:] + idle
            d = d[d >= 0]
            if d.size:
                need = max(need, int(d.max()) // TL + 1)
        return need
    c = skew(64)
    team = c > C_CAP
    cw = skew(64 * TEAM_W) if team else 0
    gmin = max(mel - 1, 1)
    neg_gaps = tr and mel <= 2
    fixp = (not team) and 64 < T <= PLAN_VT and (neg_gaps or c > gmin)
    g = np.full(T, gmin, dtype=np.int64)
    g[0] = 0
    if neg_gaps:
        g[1:] = np.maximum(1 - rmel[:-1], np.maximum(LO[:-1] - LO[1:], HI[:-1] - HI[1:]))
    g[1:] = np.minimum(g[1:], c)
    if fixp:
        # the least offsets with g[r] <= off[r] - off[r-1] <= c and off[r] - off[r-64] >= HI[r-64] - LO[r] + 1 + idle
        off = np.cumsum(g)
        k = HI[:-64] - LO[64:] + 1 + idle
        for _ in range(64):
            before = off.copy()
            for r in range(1, T):
                off[r] = max(off[r], off[r - 1] + g[r], off[r - 64] + k[r - 64] if r >= 64 else off[r])
            for r in range(T - 1, 0, -1):
                off[r - 1] = max(off[r - 1], off[r] - c)
            if np.array_equal(off, before):
                break
        else:
            off = c * rows           # (not converged: uniform offsets, as the planner falls back)
        off = off - off[0]
    else:
        off = (cw if team else c) * rows
    return dict(T=T, N=N, BS=BS, BE=BE, LO=LO, HI=HI, g=g, c=c, cw=cw, fixp=fixp, off=off)


def leaving_order_holds(p):
    """The rows are left in row order in both sweeps."""
    return bool((np.diff(p['off'] + p['BE']) >= 0).all() and (np.diff(p['off'] + p['BS']) >= 0).all())


def make_read(model, tr, mel, R, bw, dlo, dhi, seed, anchor_density=0.6, jitter=2):
    from nadavca_amd import synthetic
    rng = np.random.default_rng([SEED, mel, int(tr), R, bw, dlo, dhi, seed])
    return synthetic.make_dp_case(rng, model, R=R, bandwidth=bw, dwell=(dlo, dhi), jitter=jitter,
                                  anchor_density=anchor_density, with_context=bool(seed % 2), trim=min(3, R // 3))


def clip_ends(case, n_last, n_first):
    """The read with its signal cut so that the band ends of the last rows clip to N and, where n_first, its anchors
    moved so that the band starts of the first rows clip to 0: several rows leave on the same step at either end."""
    c = dict(case)
    anc = np.array(case['approximate_alignment'], dtype=np.int32)
    if n_first:
        anc[:n_first, 0] = anc[0, 0]
    if n_last:   # (make_dp_case ends the signal one sample behind the last anchor's band: two samples fewer clip it)
        anc[-n_last:, 0] = anc[-1, 0]
        c['signal'] = np.ascontiguousarray(case['signal'][:-2])
    c['approximate_alignment'] = anc
    return c


# name -> (transition rows, min event length, R, bandwidth, dwell lo, dwell hi, seed).  Rows: R + 1, with transition
# rows 2 R.
ROW_CASES = {}
for _tr in (False, True):
    for _mel in (0, 2, 4):
        _t = 'trans' if _tr else 'plain'
        # 63, 64, 65 and 129 rows: no second row, exactly one lane with a second row (65 = 64 + 1; with transition
        # rows the even counts 64, 66), a lane with a third (129; 130)
        for _rows in ((62, 64, 66, 130) if _tr else (63, 64, 65, 129)):
            _R = _rows // 2 if _tr else _rows - 1
            ROW_CASES['%s_mel%d_rows%d' % (_t, _mel, _rows)] = (_tr, _mel, _R, 8, max(_mel, 1), max(_mel, 1) + 3, _rows % 3)


def build_cases(model):
    """-> [dict(name, tr, mel, bw, rows, cases)]: one-read batches, then the two-read batches."""
    out = []
    for name, (tr, mel, R, bw, dlo, dhi, seed) in ROW_CASES.items():
        out.append(dict(name=name, tr=tr, mel=mel, bw=bw, rows=[rows_of(tr, R)],
                        cases=[make_read(model, tr, mel, R, bw, dlo, dhi, seed)]))
    # band ends clipped to N on the last rows, band starts clipped to 0 on the first: a band wider than the read
    # at both ends, every anchor of the ends on one sample
    for tr in (False, True):
        for mel in (0, 2):
            t = 'trans' if tr else 'plain'
            R = 70
            rd = make_read(model, tr, mel, R, 12, max(mel, 1), max(mel, 1) + 2, 3, anchor_density=1.0, jitter=0)
            out.append(dict(name='%s_mel%d_clipped_ends' % (t, mel), tr=tr, mel=mel, bw=12, rows=[rows_of(tr, R)],
                            cases=[clip_ends(rd, 5, 5)]))
    # the last switch hands a lane "no row": 64 < rows < 128, so that every lane's second switch finds none —
    # and two reads per batch: a wave starts its second read with the first one's switch state
    for tr in (False, True):
        t = 'trans' if tr else 'plain'
        Ra, Rb = (45, 33) if tr else (90, 66)
        a = make_read(model, tr, 2, Ra, 8, 2, 5, 5)
        b = make_read(model, tr, 2, Rb, 8, 2, 5, 6)
        out.append(dict(name='%s_mel2_two_reads' % t, tr=tr, mel=2, bw=8, rows=[rows_of(tr, Ra), rows_of(tr, Rb)],
                        cases=[a, b]))
        out.append(dict(name='%s_mel2_two_reads_swapped' % t, tr=tr, mel=2, bw=8,
                        rows=[rows_of(tr, Rb), rows_of(tr, Ra)], cases=[b, a]))
    return out
