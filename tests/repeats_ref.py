"""The CPU side of the repeat-count tests: the restatement of tests/host_shims/repeats_host.cpp on numpy arrays, the
rules of nvk_repeat_count_dev once more as a plain-Python DP with an explicit traceback (one item), the stages of
``count_repeats_batch`` in numpy (``cpu_count_repeats``: what nadavca_amd/repeats.py does with the kernels and torch,
stage for stage, with per-pair loops), and the constructed cases and the simulated batch the test files share."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import decode_ref as D
import signal_map_ref as R

ROOT = R.ROOT
REP_OK, REP_NO_EVENTS, REP_NO_PATH = 0, 1, 2
NINF = -np.inf

_p = lambda x: x.ctypes.data
_a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
offsets = R.offsets


class RepeatsHost:
    def __init__(self, lib):
        self._f = lib.repeat_count_host
        self._f.argtypes = [C.c_int64] + [C.c_void_p] * 7 + [C.c_double] * 4 + [C.c_void_p] * 3
        self._f.restype = None

    def count(self, level, items, mu, ac, mc, st_off, chain_par, l_stay, l_step, l_skip, trim_cost, status_in=None):
        """-> (hit i32 (n, 8): status, events, first, last, loops, i1, i2, 0; score f64 (n, 4): end value,
        S(last, N-1), v1, v2)"""
        level, mu, ac, mc = (_a(x, np.float64) for x in (level, mu, ac, mc))
        items, st_off, chain_par = _a(items, np.int64).reshape(-1, 3), _a(st_off, np.int64), _a(chain_par, np.int32)
        n = items.shape[0]
        hit, score = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 4), dtype=np.float64)
        st = None if status_in is None else _a(status_in, np.int32)
        self._f(n, _p(items), _p(level), _p(mu), _p(ac), _p(mc), _p(st_off), _p(chain_par), l_stay, l_step, l_skip,
                trim_cost, None if st is None else _p(st), _p(hit), _p(score))
        return hit, score


def build_host(directory):
    so = os.path.join(str(directory), 'repeats_host.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
                    os.path.join(ROOT, 'tests', 'host_shims', 'repeats_host.cpp'), '-o', so], check=True)
    return RepeatsHost(C.CDLL(so))


def run_host(host, case):
    return host.count(case['level'], case['items'], case['mu'], case['ac'], case['mc'], case['st_off'],
                      case['chain_par'], *case['costs'], case['trim'], case['status_in'])


TIE_PAIRS = ('open_loop', 'open_stay', 'step_loop', 'loop_stay', 'step_stay', 'stay_skip')


def python_traceback(level, mu, ac, mc, par, l_stay, l_step, l_skip, trim_cost):
    """The rules of nvk_repeat_count_dev for ONE item, plain Python floats: the full matrix with, per cell, the winning
    candidate's value and source, then a walk back from the best end that counts the back-edge traversals and finds
    where the path opens and where it crosses the marks.  Nothing is carried.
    -> (hit list of 8, score list of 4, ties): ``ties`` counts, per pair of TIE_PAIRS, the cells where the two
    candidates are adjacent among those the cell has and both equal its largest."""
    E, N = len(level), len(mu)
    lp_from, lp_to, m1, m2 = (int(x) for x in par)
    level, mu, ac, mc = ([float(x) for x in v] for v in (level, mu, ac, mc))
    ties = dict.fromkeys(TIE_PAIRS, 0)
    if E == 0:
        return [REP_NO_EVENTS, 0, -1, -1, -1, -1, -1, 0], [NINF] * 4, ties
    S, V, back = [], [], []       # back: the source state (-1: open, None: no finite candidate) and whether by the loop
    for i in range(E):
        prev = S[i - 1] if i else None
        rs, rv, rb = [], [], []
        for j in range(N):
            d = level[i] - mu[j]
            em = ac[j] - (d * d) * mc[j]
            cands = []
            if j == 0:
                cands.append(('open', float(i) * trim_cost, -1))
            cands.append(('step', prev[j - 1] + l_step if i and j >= 1 else NINF, j - 1))
            if j == lp_to:
                cands.append(('loop', prev[lp_from] + l_step if i else NINF, lp_from))
            cands.append(('stay', prev[j] + l_stay if i else NINF, j))
            cands.append(('skip', prev[j - 2] + l_skip if i and j >= 2 else NINF, j - 2))
            v, src, how = NINF, None, None
            for name, val, s in cands:
                if val > v:
                    v, src, how = val, s, name
            if v > NINF:
                # (the candidates the cell has: no step at state 0, no skip at states 0 and 1)
                live = [c for c in cands if not (c[0] == 'step' and j == 0) and not (c[0] == 'skip' and j < 2)]
                for (na, va, _), (nb, vb, _) in zip(live[:-1], live[1:]):
                    if va == v and vb == v and na + '_' + nb in ties:
                        ties[na + '_' + nb] += 1
            rs.append(v + em)
            rv.append(v)
            rb.append((src, how == 'loop'))
        S.append(rs)
        V.append(rv)
        back.append(rb)
    best, last = NINF, -1
    for i in range(E):
        end = S[i][N - 1] + float(E - 1 - i) * trim_cost
        if end > best:
            best, last = end, i
    if last < 0:
        return [REP_NO_PATH, E, -1, -1, -1, -1, -1, 0], [NINF] * 4, ties
    i, j, loops = last, N - 1, 0
    marks = {1: (NINF, -1), 2: (NINF, -1)}
    while True:
        src, by_loop = back[i][j]
        loops += by_loop
        for q, m in ((1, m1), (2, m2)):
            if j >= m and src < m and marks[q][1] < 0:     # (walking back: the first met is the path's last crossing)
                marks[q] = (V[i][j], i)
        if src == -1:
            break
        i, j = i - 1, src
    return ([REP_OK, E, i, last, loops, marks[1][1], marks[2][1], 0],
            [best, S[last][N - 1], marks[1][0], marks[2][0]], ties)


def python_case(case, only=None):
    """``python_traceback`` over the items of a case (``only``: those item indices) -> (hit, score, summed ties)"""
    n = case['items'].shape[0]
    hit, score = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 4))
    ties = dict.fromkeys(TIE_PAIRS, 0)
    for t in (range(n) if only is None else only):
        ch, lo, hi = (int(x) for x in case['items'][t])
        s0, s1 = int(case['st_off'][ch]), int(case['st_off'][ch + 1])
        st = 0 if case['status_in'] is None else int(case['status_in'][t])
        if st != 0:
            hit[t], score[t] = [st, hi - lo, -1, -1, -1, -1, -1, 0], NINF
            continue
        h, s, tt = python_traceback(case['level'][lo:hi], case['mu'][s0:s1], case['ac'][s0:s1], case['mc'][s0:s1],
                                    case['chain_par'][ch], *case['costs'], case['trim'])
        hit[t], score[t] = h, s
        for key in ties:
            ties[key] += tt[key]
    return hit, score, ties


# ---- constructed cases ------------------------------------------------------------------------------------------
GRID_COSTS, GRID_TRIM = (-1.0, -1.0, -2.0), -1.0     # ties with unit emissions
LOG_COSTS, LOG_TRIM = D.transition_costs(0.8, 0.01), math.log(0.01)
KERNEL_STATES = [3, 5, 63, 64, 65, 128, 129, 255, 256]
KERNEL_UNITS = [2, 3, 6]


def chain_shape(N, u, rng):
    """(lp_from, lp_to, m1, m2) of a chain of N states with a loop over u states, or None if it has no room"""
    if u > N - 1:
        return None
    a = int(rng.integers(0, N - u))
    lp_to, lp_from = a, a + u - 1
    m2 = int(rng.integers(lp_from + 1, N))
    return lp_from, lp_to, max(a, 1), m2


def walk(rng, par, N, loops, dwell=(1, 4)):
    """The states of a path from 0 to N - 1 that goes round the loop ``loops`` times, every state 1..dwell[1]-1 times"""
    lp_from, lp_to = par[0], par[1]
    order = list(range(0, lp_from + 1)) + list(range(lp_to, lp_from + 1)) * loops + list(range(lp_from + 1, N))
    return np.repeat(order, rng.integers(dwell[0], dwell[1], len(order)))


def pack(chains, items, level, costs, trim, status_in=None):
    """``chains``: list of (mu, ac, mc, par); ``items``: rows (chain, ev_lo, ev_hi) -> the operator's arguments"""
    cat = lambda k: np.concatenate([np.asarray(c[k], np.float64) for c in chains])
    return dict(level=np.asarray(level, np.float64), items=np.asarray(items, np.int64).reshape(-1, 3), mu=cat(0),
                ac=cat(1), mc=cat(2), st_off=offsets([len(c[0]) for c in chains]),
                chain_par=np.array([c[3] for c in chains], dtype=np.int32).reshape(-1, 4), costs=tuple(costs),
                trim=float(trim), status_in=status_in)


def random_chain(rng, N, par, sd=0.3):
    mu = rng.normal(0.0, 1.26, N)
    sd = np.full(N, sd)
    return mu, -np.log(sd * math.sqrt(2.0 * math.pi)), 1.0 / (2.0 * sd * sd), par


def kernel_cases():
    """-> list of (name, case).  'chains': one call over chains of N = 3 .. 256 states (so every instantiation and both
    sides of each of their limits; u = 2, 3, 6 where they fit for N <= 65, one u above), each with items of E = 0, 1,
    (N - 1) // 2 (no path), 64, 65 and one that walks the chain with loops (300 events for two chains); one item carries
    a ``status_in`` entry, and two items take different windows of one read's events.  'grid': integer levels and
    tables with unit costs, chains whose loop starts at state 0 among them."""
    rng = np.random.default_rng(1207)
    chains, items, levels, at = [], [], [], 0
    for N in KERNEL_STATES:
        for u in (KERNEL_UNITS if N <= 65 else [KERNEL_UNITS[len(chains) % 3]]):
            par = chain_shape(N, u, rng)
            if par is None:
                continue
            ch = len(chains)
            chains.append(random_chain(rng, N, par))
            mu = chains[-1][0]
            long_walk = mu[walk(rng, par, N, int(rng.integers(0, 6)))]
            if N in (64, 129) and u == KERNEL_UNITS[0] or N == 129:
                long_walk = np.resize(mu[walk(rng, par, N, 20, (1, 3))], 300)
            for x in (np.zeros(0), rng.normal(0, 1, 1), rng.normal(0, 1, (N - 1) // 2),
                      np.resize(mu[walk(rng, par, N, 1)], 64),
                      np.resize(mu[walk(rng, par, N, 2)], 65), long_walk):
                x = x + rng.normal(0, 0.2, x.size)
                levels.append(x)
                items.append((ch, at, at + x.size))
                at += x.size
    # windows of one read's events: the last item's events without their first 3, and without their last 5
    ch, lo, hi = items[-1]
    items += [(ch, lo + 3, hi), (ch, lo, hi - 5)]
    status_in = np.zeros(len(items), dtype=np.int32)
    status_in[5] = 7
    cases = [('chains', pack(chains, items, np.concatenate(levels), LOG_COSTS, LOG_TRIM, status_in))]
    chains, items, levels, at = [], [], [], 0
    for N, par in ((3, (1, 0, 1, 2)), (5, (3, 1, 1, 4)), (8, (2, 0, 2, 5)), (12, (6, 1, 1, 9)), (9, (3, 0, 1, 4)),
                   (66, (40, 35, 35, 50)), (130, (64, 63, 63, 128))):
        for rep in range(6 if N < 20 else 2):
            ch = len(chains)
            chains.append((rng.integers(-2, 3, N).astype(np.float64), np.zeros(N), np.full(N, 0.5), par))
            for E in (2, 7, 19, 40) if N < 20 else (N, N + 30):
                levels.append(rng.integers(-2, 3, E).astype(np.float64))
                items.append((ch, at, at + E))
                at += E
    cases.append(('grid', pack(chains, items, np.concatenate(levels), GRID_COSTS, GRID_TRIM)))
    return cases


HAND_LEAD, HAND_TAIL, HAND_LOOPS = 3, 2, 4
HAND_PAR = (6, 4, 4, 9)     # 12 states: 0..3 left flank, the loop over 4..6, 7..8 the spelled-out rest, 9..11 right


def hand_case():
    """A noiseless signal over 12 states of distinct levels and narrow Gaussians: 3 events of an alien level, then the
    chain with dwells 1-3, four times round the loop 6 -> 4, then 2 alien events.
    -> (case, expected (first, last, loops, i1, i2))"""
    rng = np.random.default_rng(77)
    N = 12
    mu = rng.permutation(N) * 0.25 - 1.5
    sd = np.full(N, 0.01)
    lp_from, lp_to, m1, m2 = HAND_PAR
    order = list(range(0, lp_from + 1)) + list(range(lp_to, lp_from + 1)) * HAND_LOOPS + list(range(lp_from + 1, N))
    dwell = rng.integers(1, 4, len(order))
    states = np.repeat(order, dwell)
    level = np.concatenate([np.full(HAND_LEAD, 40.0), mu[states], np.full(HAND_TAIL, -40.0)])
    first = HAND_LEAD
    i1 = HAND_LEAD + int(np.nonzero(states == m1)[0][0])
    i2 = HAND_LEAD + int(np.nonzero(states == m2)[0][0])
    case = pack([(mu, -np.log(sd * math.sqrt(2 * math.pi)), 1.0 / (2 * sd * sd), HAND_PAR)], [(0, 0, level.size)],
                level, LOG_COSTS, LOG_TRIM)
    return case, (first, HAND_LEAD + states.size - 1, HAND_LOOPS, i1, i2)


# ---- the simulated batch and the workflow in numpy ----------------------------------------------------------------
class TableModel:
    """What ``repeat_chain`` asks of a KmerModel, on the arrays of ``synthetic.load_model_arrays``"""

    def __init__(self, model):
        self.k, self.central, self.alphabet, self.mean, self.sigma = model

    def get_k(self):
        return self.k

    def get_alphabet_size(self):
        return self.alphabet


SIM_SEED, SIM_ALLELES, SIM_READS, SIM_FLANK, SIM_SIDE = 5, (10, 25), 40, 30, 150
SIM_UNIT = np.array([1, 0, 2])      # CAG


def simulated_batch(model, seed=SIM_SEED, alleles=SIM_ALLELES, reads=SIM_READS):
    """One CAG locus with flanks of 30; per allele ``reads`` simulated reads over 150 + 3 n + 150 bases, odd reads on
    the reverse strand, every fifth read cut off in the middle of the repeat.
    -> (ReadBatch of signals alone, [locus], truth dict: allele copies, reverse, cut per read; the specs, the reference
    (the first allele's genome))"""
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.repeats import RepeatLocus
    rng = np.random.default_rng(seed)
    left, right = rng.integers(0, 4, SIM_SIDE), rng.integers(0, 4, SIM_SIDE)
    genomes = [np.concatenate([left, np.tile(SIM_UNIT, n), right]).astype(np.int32) for n in alleles]
    locus = RepeatLocus.from_reference(genomes[0], SIM_SIDE, SIM_SIDE + 3 * alleles[0], SIM_UNIT, flank=SIM_FLANK,
                                       name='CAG')
    raws, specs, copies, reverse, cut = [], [], [], [], []
    for a, (n, genome) in enumerate(zip(alleles, genomes)):
        for i in range(reads):
            s = synthetic.make_read_spec(np.random.default_rng([seed, a, i]), genome, model, i, length=genome.size,
                                         spread=0)
            raw = np.rint(s['raw_signal']).astype(np.int16)
            is_cut = i % 5 == 4
            if is_cut:
                raw = raw[:int(s['true_starts'][SIM_SIDE + (3 * n) // 2])]
            raws.append(raw)
            specs.append(s)
            copies.append(n)
            reverse.append(s['reverse'])
            cut.append(is_cut)
    rb = ReadBatch.from_signals(np.concatenate(raws), offsets([x.size for x in raws]), np.zeros(0, np.int32),
                                np.zeros(len(raws) + 1, np.int64))
    truth = dict(copies=np.array(copies), reverse=np.array(reverse), cut=np.array(cut))
    return rb, [locus], truth, specs, genomes[0]


def aligned_batch(rb, truth, specs, reference, alleles=SIM_ALLELES):
    """The simulated batch with what a basecaller and an aligner would add: the reads' sequences, the anchors' base ->
    sample rows, and base alignments against ``reference`` (the first allele): the flanks' bases matched one to one,
    the repeat's left out.  -> (ReadBatch, SyntheticBatchAligner)"""
    from nadavca_amd.readbatch import BaseAlignmentBatch, ReadBatch, SyntheticBatchAligner
    inv = {'A': 0, 'C': 1, 'G': 2, 'T': 3}
    seqs, mb, ms, ri, fi = [], [], [], [], []
    G = reference.size
    for r, s in enumerate(specs):
        n, L = int(truth['copies'][r]), s['length']
        n_sig = int(rb.sig_off[r + 1] - rb.sig_off[r])
        seqs.append(np.array([inv[b] for b in s['sequence']], dtype=np.int32))
        rows = [(b, p) for b, p in sorted(s['sequence_to_signal_mapping'].items()) if p < n_sig]
        mb.append(np.array([b for b, _ in rows], dtype=np.int64))
        ms.append(np.array([p for _, p in rows], dtype=np.int64))
        b = np.arange(L)
        own = L - 1 - b if s['reverse'] else b                      # forward position in the read's own genome
        flank = (own < SIM_SIDE) | (own >= SIM_SIDE + 3 * n)
        fwd = np.where(own < SIM_SIDE, own, own - 3 * (n - alleles[0]))
        ri.append(b[flank])
        fi.append(np.where(s['reverse'], G - 1 - fwd, fwd)[flank])
    off = lambda xs: offsets([len(x) for x in xs])
    full = ReadBatch(rb.raw_signal, rb.sig_off, np.concatenate(seqs), off(seqs), np.concatenate(mb),
                     np.concatenate(ms), off(mb))
    ba = BaseAlignmentBatch(np.concatenate(ri), np.concatenate(fi), off(ri), truth['reverse'])
    return full, SyntheticBatchAligner(reference, ba)


DEFAULTS = dict(p_stay=0.8, p_skip=0.01, sigma_scale=0.5, trim_cost=math.log(0.01), min_events=32, window=2,
                threshold=5.0, var_floor=0.02, min_flank_score=None)


def cpu_count_repeats(map_host, rep_host, rb, loci, model, items=None, **kw):
    """The stages of count_repeats_batch on the CPU -> dict of its per-pair results (and the operator's inputs)."""
    from nadavca_amd.repeats import chain_tables
    o = dict(DEFAULTS, **kw)
    scaled, ev_off, ev_start, ok_in = D.cpu_events(map_host, rb.raw_signal, rb.sig_off, model, o['min_events'],
                                                   o['window'], o['threshold'], o['var_floor'])
    ids, st_off, chain_par, c0 = chain_tables(loci, TableModel(model))
    mean, ac, mc = D.state_tables(model, o['sigma_scale'])
    costs, trim, m = D.transition_costs(o['p_stay'], o['p_skip']), o['trim_cost'], len(loci)
    triples, owner, pairs = [], [], []
    if items is None:
        for r in range(rb.n):
            for l in range(m):
                pairs.append((r, l, None))
                for strand in (0, 1):
                    triples.append((2 * l + strand, ev_off[r], ev_off[r + 1]))
                    owner.append(r)
    else:
        for t in range(items.n):
            r, l = int(items.read[t]), int(items.locus[t])
            starts = ev_start[ev_off[r]:ev_off[r + 1]]
            lo, hi = (int(ev_off[r] + np.searchsorted(starts, v)) for v in (items.sig_lo[t], items.sig_hi[t]))
            pairs.append((r, l, int(items.reverse[t])))
            triples.append((2 * l + int(items.reverse[t]), lo, hi))
            owner.append(r)
    triples = np.array(triples, dtype=np.int64).reshape(-1, 3)
    status_in = ok_in[np.array(owner, dtype=np.int64)].astype(np.int32) if owner else np.zeros(0, np.int32)
    case = dict(level=scaled, items=triples, mu=mean[ids], ac=ac[ids], mc=mc[ids], st_off=st_off, chain_par=chain_par,
                costs=costs, trim=trim, status_in=status_in)
    hit, score = run_host(rep_host, case)
    names = ('read', 'locus', 'strand', 'status', 'count', 'loops', 'n_events', 'first', 'last', 'score', 'margin',
             'left_score', 'repeat_score', 'right_score', 'repeat_start', 'repeat_end', 'spanning')
    rows = []
    for p, (r, l, strand) in enumerate(pairs):
        margin = float('nan')
        if strand is None:
            e_f, e_r = float(score[2 * p, 0]), float(score[2 * p + 1, 0])
            strand = 1 if e_r > e_f else 0
            t = 2 * p + strand
            if hit[2 * p, 0] == REP_OK or hit[2 * p + 1, 0] == REP_OK:
                margin = (e_r - e_f) if strand else (e_f - e_r)
        else:
            t = p
        st, E, first, last, loops, i1, i2 = (int(x) for x in hit[t, :7])
        row = [r, l, strand, st, -1, loops, E, first, last] + [float('nan')] * 5 + [-1, -1, False]
        row[10] = margin
        if st == REP_OK:
            _, s_last, v1, v2 = (float(x) for x in score[t])
            div = lambda x, d: x / float(d) if d else (math.copysign(math.inf, x) if x else float('nan'))
            row[4] = int(c0[l]) + loops
            row[9] = (s_last - float(first) * trim) / float(last - first + 1)
            row[11] = div(v1 - float(first) * trim, i1 - first)
            row[12] = div(v2 - v1, i2 - i1)
            row[13] = div(s_last - v2, last - i2 + 1)
            row[14], row[15] = int(ev_start[triples[t, 1] + i1]), int(ev_start[triples[t, 1] + i2])
            row[16] = i1 >= 0 and i2 >= 0 and (o['min_flank_score'] is None or
                                               (row[11] >= o['min_flank_score'] and row[13] >= o['min_flank_score']))
        rows.append(row)
    res = {name: np.array([row[c] for row in rows]) for c, name in enumerate(names)}
    res.update(case=case, hit=hit, path_score=score, c0=c0)
    return res


def quality(res, truth, alleles=SIM_ALLELES):
    """The four conditions of the simulated batch on a result (dict or RepeatCountBatch; one locus, pairs = reads)
    -> dict: wrong_strand and wrong_allele (numbers of spanning, uncut reads), medians and ranges of the spanning
    reads' counts per allele, the cut reads' worse flank scores and the median of the spanning reads'"""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    whole = ~truth['cut'] & get('spanning').astype(bool)
    count, strand = get('count'), get('strand')
    with np.errstate(invalid='ignore'):
        worse = np.fmin(get('left_score'), get('right_score'))
    nearest = np.array(alleles)[np.argmin(np.abs(count[:, None] - np.array(alleles)[None, :]), axis=1)]
    out = dict(spanning_uncut=int(whole.sum()), wrong_strand=int((strand[whole] != truth['reverse'][whole]).sum()),
               wrong_allele=int((nearest[whole] != truth['copies'][whole]).sum()),
               cut_worse=worse[truth['cut']], median_worse=float(np.median(worse[whole])))
    for n in alleles:
        c = count[whole & (truth['copies'] == n)]
        out[n] = (float(np.median(c)), int(c.min()), int(c.max()))
    return out
