"""The CPU side of the repeat-likelihood tests: the restatement of tests/host_shims/repeatlik_host.cpp on numpy arrays,
the rules of nvk_repeat_likelihoods_dev once more as a plain Python forward in the log domain over explicit (layer,
state) cells (``math.log`` / ``math.exp``, no scaling; one item), the stages ``count_repeats_batch(layers=n)`` adds to
``repeats_ref.cpu_count_repeats`` in numpy with per-pair loops, what the simulated batch is measured by, and the
constructed cases the test files share."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import repeats_ref as RR

ROOT = RR.ROOT
REP_OK, REP_NO_EVENTS, REP_NO_PATH = RR.REP_OK, RR.REP_NO_EVENTS, RR.REP_NO_PATH
NINF = -math.inf
MAX_LAYERS = 128
LN2 = math.log(2.0)

_p = lambda x: x.ctypes.data
_a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)


def spl(N):
    """The states a lane of the kernel owns for a chain of N states"""
    return 1 if N <= 64 else 2 if N <= 128 else 4


def wave_layers(N):
    """LB: the layers a wave of the kernel holds for a chain of N states (csrc/kernels_repeatlik.hip, lik_lb)"""
    return 32 if spl(N) == 1 else 16


class RepeatLikHost:
    def __init__(self, lib):
        self._f = lib.repeat_likelihoods_host
        self._f.argtypes = [C.c_int64] + [C.c_void_p] * 7 + [C.c_double] * 4 + [C.c_int] + [C.c_void_p] * 4
        self._f.restype = None

    def run(self, level, items, mu, ac, mc, st_off, chain_par, w_stay, w_step, w_skip, w_trim, layers, status_in=None):
        """-> (z f64 (n, layers), x f64 (n,), status i32 (n,))"""
        level, mu, ac, mc = (_a(v, np.float64) for v in (level, mu, ac, mc))
        items, st_off, chain_par = _a(items, np.int64).reshape(-1, 3), _a(st_off, np.int64), _a(chain_par, np.int32)
        n = items.shape[0]
        z, x, status = np.zeros((n, layers)), np.zeros(n), np.zeros(n, dtype=np.int32)
        st = None if status_in is None else _a(status_in, np.int32)
        self._f(n, _p(items), _p(level), _p(mu), _p(ac), _p(mc), _p(st_off), _p(chain_par), w_stay, w_step, w_skip,
                w_trim, layers, None if st is None else _p(st), _p(z), _p(x), _p(status))
        return z, x, status


def build_host(directory):
    so = os.path.join(str(directory), 'repeatlik_host.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
                    os.path.join(ROOT, 'tests', 'host_shims', 'repeatlik_host.cpp'), '-o', so], check=True)
    return RepeatLikHost(C.CDLL(so))


def weights_of(case):
    """The linear weights of a ``repeats_ref`` case: the numbers whose logs it carries"""
    return tuple(math.exp(c) for c in case['costs']) + (math.exp(case['trim']),)


def run_host(host, case, layers, only=None):
    items = case['items'] if only is None else case['items'][only]
    status = case['status_in'] if only is None or case['status_in'] is None else case['status_in'][only]
    return host.run(case['level'], items, case['mu'], case['ac'], case['mc'], case['st_off'], case['chain_par'],
                    *case['weights'], layers, status)


def loglik(z, x):
    """log L per layer from the operator's outputs, as the library forms it (np.log; -inf where z is 0)"""
    with np.errstate(divide='ignore'):
        return np.log(z) + np.asarray(x)[..., None] * LN2


def exact_parts(z, x):
    """L(c) = z 2^x itself as (mantissa in [0.5, 1), exponent): equal pairs are equal likelihoods, whatever the scale
    the sweep ended on"""
    m, e = np.frexp(z)
    return m, np.where(z > 0.0, e + np.asarray(x)[..., None].astype(np.int64), 0)


# ---- the rules in plain Python, log domain ------------------------------------------------------------------------
def _lse(terms):
    top = max(terms) if terms else NINF
    if top == NINF:
        return NINF
    return top + math.log(sum(math.exp(t - top) for t in terms))


def python_loglik(level, mu, ac, mc, par, w_stay, w_step, w_skip, w_trim, layers):
    """The rules of nvk_repeat_likelihoods_dev for ONE item in the log domain, no scaling: cells (c, j) per event, every
    cell the log-sum-exp of its sources, the emission floored at -300.  ``layers`` None: the same chain without
    layers, the back edge inside the one layer -> log L per layer (a list), or the one log-likelihood."""
    E, N = len(level), len(mu)
    lp_from, lp_to = int(par[0]), int(par[1])
    level, mu, ac, mc = ([float(v) for v in a] for a in (level, mu, ac, mc))
    l_stay, l_step, l_skip, l_trim = (math.log(w) for w in (w_stay, w_step, w_skip, w_trim))
    L = 1 if layers is None else layers
    prev, z = None, [NINF] * L
    for i in range(E):
        em = []
        for j in range(N):
            d = level[i] - mu[j]
            em.append(max(ac[j] - (d * d) * mc[j], -300.0))
        cur = [[NINF] * N for _ in range(L)]
        for c in range(L):
            for j in range(N):
                terms = []
                if c == 0 and j == 0:
                    terms.append(i * l_trim)
                if i:
                    if j >= 1:
                        terms.append(prev[c][j - 1] + l_step)
                    if j == lp_to and (layers is None or c >= 1):
                        terms.append(prev[c if layers is None else c - 1][lp_from] + l_step)
                    terms.append(prev[c][j] + l_stay)
                    if j >= 2:
                        terms.append(prev[c][j - 2] + l_skip)
                cur[c][j] = _lse(terms) + em[j]
        z = [_lse([z[c] + l_trim, cur[c][N - 1]]) for c in range(L)]
        prev = cur
    return z if layers is not None else z[0]


# ---- constructed cases --------------------------------------------------------------------------------------------
def with_weights(case):
    case['weights'] = weights_of(case)
    return case


def small_cases():
    """Items small enough for the Python forward: chains of 5 .. 12 states with loops over 2, 3 and 6 states, each
    with the 5 .. 42 events of a walk with 0, 2 and 5 trips, one item of unrelated levels, one of levels on the floor.
    -> the case (``repeats_ref.pack`` with the weights)"""
    rng = np.random.default_rng(4107)
    chains, items, levels, at = [], [], [], 0
    for N, u in ((5, 2), (7, 3), (9, 2), (12, 6), (12, 3), (8, 3)):
        par = RR.chain_shape(N, u, rng)
        ch = len(chains)
        chains.append(RR.random_chain(rng, N, par))
        mu = chains[-1][0]
        for trips in (0, 2, 5):
            x = mu[RR.walk(rng, par, N, trips, (1, 2))]
            x = x + rng.normal(0, 0.2, x.size)
            levels.append(x)
            items.append((ch, at, at + x.size))
            at += x.size
    for x in (rng.normal(0, 1.26, 25), np.full(12, 1000.0)):
        levels.append(x)
        items.append((0, at, at + x.size))
        at += x.size
    return with_weights(RR.pack(chains, items, np.concatenate(levels), RR.LOG_COSTS, RR.LOG_TRIM))


# (N, lp_from, lp_to): the loop's ends in one lane and in two for two states per lane; in two slots of one lane, in
# neighbouring lanes and two lanes apart (a loop over 6 states) for four
PLACED_LOOPS = ((100, 41, 40), (100, 42, 41), (100, 45, 43), (200, 83, 80), (200, 85, 83), (200, 89, 84))
KERNEL_LAYERS = sorted({1, 2, MAX_LAYERS} | {lb + d for lb in (16, 32) for d in (-1, 0, 1)} | {2 * 16 + 1, 2 * 32 + 1})
SHARP_EVENTS = 300


def kernel_case():
    """One call's worth of items for the kernel against the shim.  Chains of N = 3 .. 256 states (every instantiation
    and both sides of each of their limits; loops over 2, 3 and 6 states where they fit for N <= 65, one above), each
    with items of E = 0, 1, 2, (N - 1) // 2 (no path), 64, 65 and a walk with trips round the loop (300 events with 20
    trips for three chains, one per instantiation: more trips than a small window holds); chains with the loop placed
    inside a lane, across lanes and across slots (PLACED_LOOPS); an item whose every emission sits on the floor; an
    item of 300 events on a chain of narrow Gaussians (X far below -1 000); a ``status_in`` entry; two windows of one
    item's events.  -> the case"""
    rng = np.random.default_rng(2207)
    chains, items, levels = [], [], []
    at = [0]

    def add(ch, x):
        levels.append(np.asarray(x, np.float64))
        items.append((ch, at[0], at[0] + len(x)))
        at[0] += len(x)

    for N in RR.KERNEL_STATES:
        for u in (RR.KERNEL_UNITS if N <= 65 else [RR.KERNEL_UNITS[len(chains) % 3]]):
            par = RR.chain_shape(N, u, rng)
            if par is None:
                continue
            ch = len(chains)
            chains.append(RR.random_chain(rng, N, par))
            mu = chains[-1][0]
            long_walk = mu[RR.walk(rng, par, N, int(rng.integers(0, 6)))]
            if (N, u) in ((64, 2), (128, RR.KERNEL_UNITS[ch % 3]), (256, RR.KERNEL_UNITS[ch % 3])):
                long_walk = np.resize(mu[RR.walk(rng, par, N, 20, (1, 3))], 300)
            for x in (np.zeros(0), rng.normal(0, 1, 1), rng.normal(0, 1, 2), rng.normal(0, 1, (N - 1) // 2),
                      np.resize(mu[RR.walk(rng, par, N, 1)], 64), np.resize(mu[RR.walk(rng, par, N, 2)], 65),
                      long_walk):
                add(ch, x + rng.normal(0, 0.2, x.size))
    for N, lp_from, lp_to in PLACED_LOOPS:
        par = (lp_from, lp_to, max(lp_to, 1), N - 1)
        ch = len(chains)
        chains.append(RR.random_chain(rng, N, par))
        x = chains[-1][0][RR.walk(rng, par, N, 3, (1, 3))]
        add(ch, x + rng.normal(0, 0.2, x.size))
    add(1, np.full(40, 1000.0))                                   # every emission on the floor
    par = (6, 4, 4, 9)
    chains.append(RR.random_chain(rng, 12, par, sd=0.05))
    x = np.resize(chains[-1][0][RR.walk(rng, par, 12, 60, (1, 3))], SHARP_EVENTS)
    add(len(chains) - 1, x + rng.normal(0, 0.2, x.size))
    sharp = len(items) - 1
    ch, lo, hi = items[-1]
    items += [(ch, lo + 3, hi), (ch, lo, hi - 5)]                   # windows of one item's events
    status_in = np.zeros(len(items), dtype=np.int32)
    status_in[5] = 7
    case = with_weights(RR.pack(chains, items, np.concatenate(levels), RR.LOG_COSTS, RR.LOG_TRIM, status_in))
    case['sharp'], case['floor'] = sharp, sharp - 1
    return case


HAND_LAYERS = 8


def hand_case():
    """``repeats_ref.hand_case``: narrow Gaussians, the events those of exactly four trips -> the case"""
    return with_weights(RR.hand_case()[0])


def wide_case():
    """One chain of broad Gaussians (sd 0.4: some nats between any two states per event) and 25 events of 5 trips, so
    that no layer's likelihood falls 2^-1022 below the best one's: what the sweep holds for a layer then does not
    depend on the layers above it, but for the power of two it is scaled by.  -> the case"""
    rng = np.random.default_rng(311)
    par = (5, 3, 3, 8)
    chain = RR.random_chain(rng, 10, par, sd=0.4)
    x = chain[0][RR.walk(rng, par, 10, 5, (1, 2))]
    return with_weights(RR.pack([chain], [(0, 0, x.size)], x + rng.normal(0, 0.2, x.size), RR.LOG_COSTS, RR.LOG_TRIM))


# ---- the workflow in numpy ----------------------------------------------------------------------------------------
SIM_LAYERS = 48
SIM_MIN_FLANK = -3.08    # between the worst uncut flank of the simulated batch (-3.02) and the best cut one (-3.14):
#                          tuned on this very batch


def cpu_count_likelihoods(map_host, rep_host, lik_host, rb, loci, model, layers=SIM_LAYERS, items=None, **kw):
    """``repeats_ref.cpu_count_repeats`` and what ``layers`` adds to it, per pair in plain loops: the likelihood shim
    on the pair's chosen item with the pair's status as its ``status_in``; log L by np.log; the posterior (the row
    less its largest value, np.exp, divided by the ascending sum), its first largest entry, its mean (ascending sum)
    and ``clipped``.  -> the dict of ``cpu_count_repeats`` with the new fields"""
    res = RR.cpu_count_repeats(map_host, rep_host, rb, loci, model, items=items, **kw)
    case = dict(res['case'])
    # the very numbers whose logs the Viterbi call took (exp(log(p)) may be an ulp off p), and exp(trim_cost)
    o = dict(RR.DEFAULTS, **kw)
    case['weights'] = (o['p_stay'], 1.0 - o['p_stay'] - o['p_skip'], o['p_skip'], math.exp(o['trim_cost']))
    n = res['status'].size
    pick = (2 * np.arange(n) + res['strand']) if items is None else np.arange(n)
    case['items'], case['status_in'] = case['items'][pick], res['status'].astype(np.int32)
    z, x, status = run_host(lik_host, case, layers)
    ok = (res['status'] == REP_OK) & (status == REP_OK)
    # np.log and np.exp over the whole (pairs, layers) matrices, as the library calls them
    ll =np.where(ok[:, None], loglik(z, x), np.nan)
    shifted = np.where(ok[:, None], ll, 0.0)
    weight = np.exp(shifted - shifted.max(axis=1, keepdims=True)) if n else np.zeros((0, layers))
    post = np.full((n, layers), np.nan)
    cmap, mean, conf = np.full(n, -1, dtype=np.int64), np.full(n, np.nan), np.full(n, np.nan)
    clipped = np.zeros(n, dtype=bool)
    for p in range(n):
        if not ok[p]:
            continue
        w = weight[p]
        total = 0.0
        for v in w:
            total += float(v)
        post[p] = w / total
        top, c0 = int(np.argmax(post[p])), int(res['c0'][res['locus'][p]])
        acc = 0.0
        for c in range(layers):
            acc += float(post[p, c] * float(c0 + c))
        cmap[p], mean[p], conf[p] = c0 + top, acc, post[p, top]
        clipped[p] = top == layers - 1 or post[p, layers - 1] > 1e-3
    res.update(layers=layers, count_loglik=ll, count_post=post, count_map=cmap, count_mean=mean, count_conf=conf,
               clipped=clipped, lik_z=z, lik_x=x, lik_status=status)
    return res


def auc(score, positive):
    """The share of (positive, negative) pairs the score orders rightly, ties counting half"""
    pos, neg = score[positive], score[~positive]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum())
                 / (pos.size * neg.size))


def lik_quality(res, truth, alleles=RR.SIM_ALLELES):
    """What the simulated batch is measured by, on a result made with ``layers`` and ``min_flank_score`` (a dict or a
    RepeatCountBatch; one locus, pairs = reads) -> dict: the reads used (spanning), how many of them are cut, per
    allele (min, max, mean |error|) of the uncut reads' ``count_map``, how many reads are clipped, how many uncut
    reads have ``count_map`` == ``count`` and how many the true count, the medians of ``count_conf`` where
    ``count_map`` is the true count and where not, the AUC of ``count_conf`` for that, the uncut reads whose true count
    has a posterior below 0.01, and the largest posterior of the last layer"""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    uncut, used = ~truth['cut'], get('spanning').astype(bool)
    cmap, conf, post = get('count_map'), get('count_conf'), get('count_post')
    right = cmap == truth['copies']
    c0 = int(get('c0')[0])
    at_truth = post[np.arange(cmap.size), truth['copies'] - c0]
    out = dict(used=int(used.sum()), used_cut=int((used & truth['cut']).sum()), clipped=int(get('clipped').sum()),
               same_as_viterbi=int((cmap == get('count'))[uncut].sum()), right=int(right[uncut].sum()),
               conf_right=float(np.median(conf[uncut & right])), conf_wrong=float(np.median(conf[uncut & ~right])),
               auc=auc(conf[uncut], right[uncut]), truth_below_1pct=int((at_truth[uncut] < 0.01).sum()),
               last_layer=float(np.nanmax(post[:, -1])))
    for a in alleles:
        c = cmap[uncut & (truth['copies'] == a)]
        out[a] = (int(c.min()), int(c.max()), float(np.abs(c - a).mean()))
    return out


def batch_of(res, loci):
    """The RepeatCountBatch of a restatement's dict"""
    from nadavca_amd.repeats import RepeatCountBatch
    fields = {f: res[f] for f in RepeatCountBatch.FIELDS + RepeatCountBatch.LIK_FIELDS}
    return RepeatCountBatch(loci, res['c0'], None, res['layers'], None, **fields)


# What the restatement gives on the simulated batch (repeats_ref.simulated_batch: one CAG locus, alleles of 10 and 25
# copies, 40 reads each, every fifth cut inside the repeat; c0 = 3, 64 states, 48 layers, the default costs), over the
# 64 uncut reads: count_map is the Viterbi count on 58 and the true count on 29; mean |error| 0.44 / 1.06 for 10 / 25
# copies (Viterbi 0.47 / 1.00); median count_conf 0.88 where count_map is the true count, 0.57 where not; the true
# count's posterior is below 0.01 on 9 reads (ordered, not calibrated); the last layer's posterior is 1.7e-53 at most;
# genotypes(): (10, 26) at -138.16, 4.22 nats over (10, 25), the best homozygote 169.76 nats behind.
MEASURED_AUC = 0.7488            # 29 against 35 reads: one swapped pair moves it by 0.001
MEASURED_HET_MARGIN = 169.76


def check_quality(res, truth, loci):
    """The conditions of the simulated batch on a result with layers (the restatement's here, the device's in
    tests/test_gpu_repeat_likelihoods.py) -> (the measures, the genotype)"""
    q = lik_quality(res, truth)
    batch = res if not isinstance(res, dict) else batch_of(res, loci)
    g = batch.genotypes()[0]
    print(q, {k: v for k, v in g.items() if k != 'table'})
    # min_flank_score = -3.08 (tuned on this batch) keeps the 64 uncut reads and no cut one
    assert q['used'] == 64 and q['used_cut'] == 0
    # the Viterbi ranges of the README
    assert 9 <= q[10][0] and q[10][1] <= 12 and 23 <= q[25][0] and q[25][1] <= 28
    assert q['clipped'] == 0
    assert q['auc'] >= MEASURED_AUC - 0.05
    assert g['reads'] == 64 and abs(g['alleles'][0] - 10) <= 1 and abs(g['alleles'][1] - 25) <= 1
    assert g['het_margin'] >= 0.5 * MEASURED_HET_MARGIN
    return q, g
