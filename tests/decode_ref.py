"""The CPU side of the decode tests: the restatement of tests/host_shims/decode_host.cpp on numpy arrays, the rules of
nvk_viterbi_decode_dev once more as a plain-Python Viterbi (small k), the stages of ``decode_batch`` in numpy
(``cpu_decode``: what nadavca_amd/decode.py does with the kernels and torch, stage for stage, with per-read loops), the
quality measures of the decoded sequences, and the constructed cases the test files share."""
import ctypes as C
import math
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import signal_map_ref as R

ROOT = R.ROOT
DEC_OK, DEC_NO_EVENTS = 0, 1
NINF = -np.inf

_p = lambda x: x.ctypes.data
_a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
offsets = R.offsets


def capacities(ev_off, k):
    """-> cap_off: k + 2 (E - 1) entries for a read with events, none otherwise"""
    E = np.diff(ev_off)
    return offsets(np.where(E >= 1, k + 2 * (E - 1), 0))


class DecodeHost:
    def __init__(self, lib):
        self._f = lib.viterbi_decode_host
        self._f.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 \
            + [C.c_double] * 3 + [C.c_void_p] * 6
        self._f.restype = None

    def decode(self, level, ev_off, k, central, mean, ac, mc, l_stay, l_step, l_skip, status_in=None, cap_off=None,
               threads=1):
        """-> (hit i32 (n, 4): status, events, bases, end state; score f64 (n,); seq i32, base_event i32, laid out by
        ``cap_off`` (default: ``capacities``)).  ``threads``: the reads are independent; more than one spreads them
        over that many calls at once."""
        level, mean, ac, mc = (_a(x, np.float64) for x in (level, mean, ac, mc))
        ev_off = _a(ev_off, np.int64)
        cap_off = capacities(ev_off, k) if cap_off is None else _a(cap_off, np.int64)
        n = ev_off.size - 1
        hit, score = np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.float64)
        seq = np.zeros(max(int(cap_off[-1]), 1), dtype=np.int32)
        be = np.zeros(max(int(cap_off[-1]), 1), dtype=np.int32)
        st = None if status_in is None else _a(status_in, np.int32)

        def run(lo, hi):
            # (the offsets stay the batch's: the call starts at read lo of every per-read array)
            self._f(hi - lo, _p(level), _p(ev_off[lo:]), k, central, _p(mean), _p(ac), _p(mc), l_stay, l_step, l_skip,
                    None if st is None else _p(st[lo:]), _p(cap_off[lo:]), _p(hit[lo:]), _p(score[lo:]), _p(seq),
                    _p(be))

        if threads <= 1 or n < 2:
            run(0, n)
        else:
            cuts = [n * t // (4 * threads) for t in range(4 * threads + 1)]
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(lambda c: run(*c), [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]))
        return hit, score, seq[:int(cap_off[-1])], be[:int(cap_off[-1])]


def build_host(directory):
    so = os.path.join(str(directory), 'decode_host.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC',
                    os.path.join(ROOT, 'tests', 'host_shims', 'decode_host.cpp'), '-o', so], check=True)
    return DecodeHost(C.CDLL(so))


def python_viterbi(level, k, central, mean, ac, mc, l_stay, l_step, l_skip):
    """The rules of nvk_viterbi_decode_dev for ONE read with events, plain Python floats, every candidate of every cell
    looked up flat -> (score, end state, sequence list, base_event list, ties): ``ties`` counts the cells where step and
    stay tie for the largest candidate ('step_stay'), where skip ties with one of them for it ('skip'), and where the
    largest predecessor inside step ('in_step') or inside skip ('in_skip') occurs twice."""
    E, S = len(level), 4 ** k
    mean, ac, mc = [float(x) for x in mean], [float(x) for x in ac], [float(x) for x in mc]
    em = lambda i, s: ac[s] - ((float(level[i]) - mean[s]) * (float(level[i]) - mean[s])) * mc[s]
    ties = dict(step_stay=0, skip=0, in_step=0, in_skip=0)
    V = [em(0, s) for s in range(S)]
    back = []
    for i in range(1, E):
        row, new = [], []
        for s in range(S):
            steps = [V[a * 4 ** (k - 1) + s // 4] for a in range(4)]
            skips = [V[c * 4 ** (k - 2) + s // 16] for c in range(16)]
            a, c = steps.index(max(steps)), skips.index(max(skips))   # (index: the first of equal ones)
            cands = [(steps[a] + l_step, a * 4 ** (k - 1) + s // 4, 1), (V[s] + l_stay, s, 0),
                     (skips[c] + l_skip, c * 4 ** (k - 2) + s // 16, 2)]
            v, pred, adds = cands[0]
            for cv, cp, ca in cands[1:]:
                if cv > v:
                    v, pred, adds = cv, cp, ca
            ties['step_stay'] += cands[0][0] == v and cands[1][0] == v
            ties['skip'] += cands[2][0] == v and (cands[0][0] == v or cands[1][0] == v)
            ties['in_step'] += steps.count(max(steps)) > 1
            ties['in_skip'] += skips.count(max(skips)) > 1
            new.append(v + em(i, s))
            row.append((pred, adds))
        V = new
        back.append(row)
    end = V.index(max(V))
    path, moves = [end], []
    for row in reversed(back):
        pred, adds = row[path[0]]
        moves.insert(0, adds)
        path.insert(0, pred)
    seq = [(path[0] >> (2 * t)) & 3 for t in range(k - 1, -1, -1)]
    owner, owners = central, {central: 0}
    for i, (s, m) in enumerate(zip(path[1:], moves), start=1):
        if m == 2:
            seq.append((s // 4) % 4)
        if m:
            seq.append(s % 4)
            owner += m
            owners[owner] = i
    return V[end], end, seq, [owners.get(b, -1) for b in range(len(seq))], ties


def transition_costs(p_stay, p_skip):
    return math.log(p_stay), math.log(1.0 - p_stay - p_skip), math.log(p_skip)


def state_tables(model, sigma_scale=1.0):
    """-> (mean, ac, mc) of the table's states, as nadavca_amd/decode.py forms them"""
    sd = np.asarray(model[4], dtype=np.float64) * float(sigma_scale)
    return np.asarray(model[3], np.float64), -np.log(sd * math.sqrt(2.0 * math.pi)), 1.0 / (2.0 * sd * sd)


def cpu_events(map_host, raw, sig_off, model, min_events=32, window=2, threshold=5.0, var_floor=0.02):
    """Stages 1 and 2 of decode_batch on the CPU -> (scaled levels, ev_off, ev_start, status_in): the normalisation and
    detector of signal_map_batch, then the events' median and MAD mapped onto those of the table's means"""
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
    start, _, level = map_host.levels(norm, sig_off, ev_pos)
    med_l, mad_l = R.median_mad(np.asarray(model[3], np.float64))
    scaled, status_in = np.array(level), np.zeros(n, dtype=np.int32)
    for r in range(n):
        e = level[ev_off[r]:ev_off[r + 1]]
        mad_e = R.median_mad(e)[1] if e.size else 0.0
        if e.size < min_events or e.size == 0 or not mad_e > 0.0:
            status_in[r] = DEC_NO_EVENTS   # (its levels are not read)
            continue
        med_e = R.median_mad(e)[0]
        scaled[ev_off[r]:ev_off[r + 1]] = (e - med_e) * (mad_l / mad_e) + med_l
    return scaled, ev_off, start, status_in


def cpu_decode(map_host, dec_host, raw, sig_off, model, p_stay=0.7, p_skip=0.01, sigma_scale=1.0, min_events=32,
               window=2, threshold=5.0, var_floor=0.02, threads=None):
    """The stages of decode_batch on the CPU -> dict of its per-read and flat results (and the operator's inputs)."""
    k, central, alphabet = model[0], model[1], model[2]
    scaled, ev_off, ev_start, status_in = cpu_events(map_host, raw, sig_off, model, min_events, window, threshold,
                                                     var_floor)
    mean, ac, mc = state_tables(model, sigma_scale)
    costs = transition_costs(p_stay, p_skip)
    cap_off = capacities(ev_off, k)
    threads = min(16, os.cpu_count() or 1) if threads is None else threads
    hit, score, seq, be = dec_host.decode(scaled, ev_off, k, central, mean, ac, mc, *costs, status_in, cap_off, threads)
    n = ev_off.size - 1
    status, n_bases = hit[:, 0], hit[:, 2]
    seq_off = offsets(n_bases)
    sequence, map_base, map_sig, rows = [], [], [], np.zeros(n, np.int64)
    for r in range(n):
        lo = int(cap_off[r])
        sequence.append(seq[lo:lo + n_bases[r]])
        ev = be[lo:lo + n_bases[r]]
        b = np.nonzero(ev >= 0)[0]
        map_base.append(b.astype(np.int32))
        map_sig.append(ev_start[ev_off[r] + ev[b]])
        rows[r] = b.size
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    with np.errstate(invalid='ignore', divide='ignore'):
        per_event = np.where(status == 0, score / hit[:, 1].astype(np.float64), np.nan)
    return dict(status=status, n_events=hit[:, 1], n_bases=n_bases, score=per_event, seq_off=seq_off,
                sequence=cat(sequence, np.int32), map_base=cat(map_base, np.int32), map_sig=cat(map_sig, np.int32),
                map_off=offsets(rows), end_state=hit[:, 3], path_score=score, scaled=scaled, ev_off=ev_off,
                ev_start=ev_start, status_in=status_in, cap_off=cap_off, mean=mean, ac=ac, mc=mc, costs=costs)


# ---- quality of a decoded sequence ------------------------------------------------------------------------------
def identity(truth, decoded):
    """1 - (edit distance of ``truth`` to the best substring of ``decoded``) / len(truth)"""
    truth, decoded = np.asarray(truth), np.asarray(decoded)
    prev = np.zeros(decoded.size + 1, dtype=np.int64)      # a substring may start anywhere
    ramp = np.arange(decoded.size + 1, dtype=np.int64)
    for i, t in enumerate(truth, start=1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (decoded != t), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - ramp) + ramp    # the moves along the row
    return 1.0 - float(prev.min()) / max(truth.size, 1)


def seed_votes(truth, decoded, k=10, w=64):
    """SeedAligner's vote with ``truth`` as the reference: exact k-mer seeds (i in ``decoded``, p in ``truth``),
    diagonal d = p - i, window c = floor(d / w); -> the largest n(c) + n(c + 1)"""
    def kmers(x):
        x = np.asarray(x, dtype=np.int64)
        v = np.zeros(max(x.size - k + 1, 0), dtype=np.int64)
        for t in range(k):
            v = v * 4 + x[t:t + v.size]
        return v
    kt, kd = kmers(truth), kmers(decoded)
    if kt.size == 0 or kd.size == 0:
        return 0
    order = np.argsort(kt, kind='stable')
    lo, hi = np.searchsorted(kt[order], kd, 'left'), np.searchsorted(kt[order], kd, 'right')
    i = np.repeat(np.arange(kd.size), hi - lo)
    if i.size == 0:
        return 0
    p = order[np.concatenate([np.arange(a, b) for a, b in zip(lo, hi) if b > a])]
    c = np.floor_divide(p - i, w)
    c -= c.min()
    n = np.bincount(c, minlength=int(c.max()) + 2)
    return int((n[:-1] + n[1:]).max())


# ---- constructed cases ------------------------------------------------------------------------------------------
GRID_COSTS = (-1.0, -1.0, -2.0)   # l_stay, l_step, l_skip of the grid cases: ties with unit emissions
LOG_COSTS = transition_costs(0.7, 0.02)


def emit(rng, model, n_events, noise=0.3, dwell=(1, 4), p_skip=0.03):
    """``n_events`` events of a random walk over the table's k-mers: 1..dwell[1]-1 events per k-mer, a k-mer left out
    now and then"""
    k, _, _, mean, _ = model
    S = 4 ** k
    s, out = int(rng.integers(0, S)), []
    while len(out) < n_events:
        out += [mean[s]] * int(rng.integers(dwell[0], dwell[1]))
        for _ in range(2 if rng.random() < p_skip else 1):
            s = (s * 4 + int(rng.integers(0, 4))) % S
    return np.array(out[:n_events]) + rng.normal(0, noise, n_events)


def grid_model(rng, k):
    """A table on the grid: means on the integers -2..2, ac 0, mc 0.5 -> (mean, ac, mc)"""
    S = 4 ** k
    return rng.integers(-2, 3, S).astype(np.float64), np.zeros(S), np.full(S, 0.5)


def pack(levels, k, central, tables, costs, status_in=None):
    """``levels``: list of per-read level arrays -> the operator's arguments as a dict"""
    cat = np.concatenate([np.asarray(x, np.float64) for x in levels]) if levels else np.zeros(0)
    return dict(level=cat, ev_off=offsets([len(x) for x in levels]), k=k, central=central, mean=tables[0],
                ac=tables[1], mc=tables[2], costs=tuple(costs), status_in=status_in)


def small_cases():
    """Cases small enough for the plain-Python Viterbi: k = 2 and 3, central 0, 1 and k - 1, E = 1, 2 and up to 40,
    random tables and grid tables"""
    from nadavca_amd import synthetic
    rng = np.random.default_rng(61)
    cases = []
    for k in (2, 3):
        for central in sorted({0, 1, k - 1}):
            model = synthetic.synth_model_arrays(seed=k, k=k, central=central)
            lengths = [1, 2, 3, 7, 19, 40] if k == 2 else [1, 2, 11, 40]
            cases.append(('k %d central %d random table' % (k, central),
                          pack([emit(rng, model, E) for E in lengths], k, central, state_tables(model), LOG_COSTS)))
            lengths = [1, 2, 5, 12, 30] if k == 2 else [2, 9, 24]
            cases.append(('k %d central %d grid' % (k, central),
                          pack([rng.integers(-2, 3, E).astype(np.float64) for E in lengths], k, central,
                               grid_model(rng, k), GRID_COSTS)))
    return cases


HAND_BASES = [0, 1, 2, 3, 3, 2, 1, 0, 3, 1]          # A C G T T G C A T C
HAND_KMERS = [0, 1, 1, 2, 2, 2, 3, 5, 5, 6, 7, 7]    # the 3-mer (by its first base) of every event: 4 is left out
# per central position: the first event of every base.  The state at event 0 owns base `central`; base central + 4 is
# the one the skip passes; the first `central` and the last 2 - central bases belong to no state
HAND_BASE_EVENT = {0: [0, 1, 3, 6, -1, 7, 9, 10, -1, -1],
                   1: [-1, 0, 1, 3, 6, -1, 7, 9, 10, -1],
                   2: [-1, -1, 0, 1, 3, 6, -1, 7, 9, 10]}


def hand_case(central):
    """Noise-free events of HAND_BASES at k = 3: dwell 1-3 and one planted skip; a table of 64 distinct levels with a
    narrow Gaussian, so that only the true path pays no emission cost"""
    rng = np.random.default_rng(71)
    mean = rng.permutation(64) * 0.0625 - 2.0
    sd = np.full(64, 0.01)
    ids = [HAND_BASES[j] * 16 + HAND_BASES[j + 1] * 4 + HAND_BASES[j + 2] for j in range(8)]
    level = mean[[ids[j] for j in HAND_KMERS]]
    return pack([level], 3, central, (mean, -np.log(sd * math.sqrt(2 * math.pi)), 1.0 / (2 * sd * sd)), LOG_COSTS)


KERNEL_LENGTHS = [0, 1, 2, 3, 64, 65, 300]


def kernel_cases(k):
    """-> list of (name, case) for one instantiation (k = 2..6): reads of E = 0, 1, 2, 3, 64, 65 and 300 events with
    central 0 and k - 1, one of them with a ``status_in`` entry, and grid cases"""
    from nadavca_amd import synthetic
    rng = np.random.default_rng([81, k])
    cases = []
    for central in (0, k - 1):
        model = synthetic.synth_model_arrays(seed=10 + k, k=k, central=central)
        levels = [emit(rng, model, E) for E in KERNEL_LENGTHS + [33]]
        status_in = np.zeros(len(levels), dtype=np.int32)
        status_in[-1] = 7
        cases.append(('k %d central %d' % (k, central),
                      pack(levels, k, central, state_tables(model), LOG_COSTS, status_in)))
        levels = [rng.integers(-2, 3, E).astype(np.float64) for E in (1, 2, 17, 64, 130)]
        cases.append(('k %d central %d grid' % (k, central), pack(levels, k, central, grid_model(rng, k), GRID_COSTS)))
    return cases


def simulated_case(map_host, n=64, length=150, seed=17):
    """The k = 6 case: ``n`` simulated reads of about ``length`` bases through the CPU stages up to the operator, the
    packaged table -> (case, model)"""
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    rb, _, _ = synthetic.make_read_batch(n, model, seed=seed, genome_length=3000, length=length, spread=15)
    scaled, ev_off, _, status_in = cpu_events(map_host, rb.raw_signal, rb.sig_off, model)
    case = dict(level=scaled, ev_off=ev_off, k=model[0], central=model[1], costs=LOG_COSTS, status_in=status_in)
    case['mean'], case['ac'], case['mc'] = state_tables(model)
    return case, model


def read_sequences(rb):
    return [rb.sequence[rb.seq_off[r]:rb.seq_off[r + 1]] for r in range(rb.n)]
