"""Seeded random DP problems shared by tests/dev/fuzz_parity.py, tests/dev/fuzz_repro.py and the regression
tests that pin iterations the fuzzer once failed on, and the gate of the parity contract that all of them share:
classify_difference, which accepts a read that differs from the reference only if its path scores as well."""
import os

import numpy as np


def make_fuzz_batch(seed0, it):
    """-> dict(model, k, central, alphabet, mel, bw, cases, tr, w) for iteration `it` of seed `seed0`:
    random k-mer model (30 % of them with 0.3x or 3x the usual sigma), min event length, bandwidth, 1-9
    reads of 1-259 bases with random dwell, noise, anchor density and jitter."""
    from nadavca_amd import synthetic
    rng = np.random.default_rng([seed0, it])
    k = int(rng.integers(2, 7))
    central = int(rng.integers(0, k))
    alphabet = int(rng.choice([4, 4, 4, 3, 5]))
    model = synthetic.synth_model_arrays(int(rng.integers(1 << 30)), k=k, central=central, alphabet=alphabet)
    if rng.random() < 0.3:  # sharper or blunter levels
        model = model[:4] + (model[4] * float(rng.choice([0.3, 3.0])),)
    mel = int(rng.integers(0, 5))
    bw = int(rng.integers(4, 90))
    cases = []
    for _ in range(int(rng.integers(1, 10))):
        R = int(rng.integers(1, 260))
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(4, 90)),
                                            dwell=(max(mel, 1), int(rng.integers(max(mel, 1) + 1, 14))),
                                            noise=float(rng.choice([0.1, 0.35, 1.0])), jitter=int(rng.integers(0, 25)),
                                            anchor_density=float(rng.uniform(0.05, 1.0)),
                                            with_context=bool(rng.integers(2)), trim=min(3, R // 3)))
    tr, w = bool(rng.integers(2)), bool(rng.integers(2))
    return dict(model=model, k=k, central=central, alphabet=alphabet, mel=mel, bw=bw, cases=cases, tr=tr, w=w)


def make_team_batch(seed0, it):
    """-> dict(model, k, mel, bw, cases, tr) aimed at the wide-band path of refine_alignment (teams of waves,
    kernels_align3.hip): bandwidths 100-700 on reads of 20-700 bases (a few tiny ones and a few narrow bands
    mixed in), min event length 0-4, packaged or random k-mer model."""
    from nadavca_amd import synthetic
    rng = np.random.default_rng([seed0, it])
    if rng.random() < 0.5:
        model = synthetic.load_model_arrays()
        k = model[0]
    else:
        k = int(rng.integers(3, 7))
        model = synthetic.synth_model_arrays(int(rng.integers(1 << 30)), k=k, central=int(rng.integers(0, k)), alphabet=4)
    mel = int(rng.integers(0, 5))
    bw = int(rng.integers(100, 700))
    tr = bool(rng.integers(2))
    cases = []
    for _ in range(int(rng.integers(1, 6))):
        R = int(rng.integers(20, 700)) if rng.random() < 0.8 else int(rng.integers(1, 20))
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(bw if rng.random() < 0.8 else rng.integers(4, 60)),
                                            dwell=(max(mel, 1), int(rng.integers(max(mel, 1) + 1, 14))),
                                            noise=float(rng.choice([0.2, 0.35, 0.8])), jitter=int(rng.integers(0, 25)),
                                            anchor_density=float(rng.uniform(0.02, 1.0)),
                                            with_context=bool(rng.integers(2)), trim=min(3, R // 3)))
    return dict(model=model, k=k, mel=mel, bw=bw, cases=cases, tr=tr)


def make_run_batch(seed0, it, n_reads=16, all_runs=False):
    """-> dict(model, k, mel, bw, cases, tr) aimed at the one-wave-per-read kernels of refine_alignment, every
    variant of which iterations 0-9 reach: min event length it % 5, transition rows on odd it // 5; the packaged
    6-mer model, reads of 3-140 bases, bandwidth 8-60.  Reads 0, 2, .. have homopolymer_rich bases (all of them
    with ``all_runs``) — adjacent equal k-mer levels, so flat posterior plateaus — and two reads of every four
    have their signal rounded to 1/12 (ADC steps: equal samples, so exact ties of path scores)."""
    from nadavca_amd import synthetic
    rng = np.random.default_rng([seed0, it])
    model = synthetic.load_model_arrays()
    mel, tr = it % 5, bool((it // 5) % 2)
    bw = int(rng.integers(8, 61))
    cases = []
    for i in range(n_reads):
        R = int(rng.integers(3, 141))
        c = synthetic.make_dp_case(rng, model, R=R, bandwidth=bw, dwell=(max(mel, 1), 9), jitter=6,
                                   anchor_density=float(rng.uniform(0.1, 0.9)), with_context=bool(i % 3),
                                   trim=min(3, R // 3),
                                   bases=synthetic.homopolymer_rich if all_runs or i % 2 == 0 else None)
        if i % 4 in (1, 2):
            c['signal'] = np.round(c['signal'] * 12.0) / 12.0
        cases.append(c)
    return dict(model=model, k=model[0], mel=mel, bw=bw, cases=cases, tr=tr)


def make_team_shape_batch(seed0, it):
    """-> dict(model, k, mel, bw, cases, tr): the reads tests/plan_cases.py documents as swept by a team of four
    waves (300 and 90 bases under bandwidth 200, two or three samples per base) and a short read with a narrow
    band in the same batch, which the one-wave launch serves.  Min event length (0, 2, 4)[it % 3], transition
    rows on odd it // 3: iterations 0-5 reach every pairing.  At min event length 4 a 300-base read of four or
    five samples per base comes with them."""
    import plan_cases
    from nadavca_amd import synthetic
    model = plan_cases.model_arrays(plan_cases.BASE)
    mel, tr = (0, 2, 4)[it % 3], bool((it // 3) % 2)
    lo = max(mel, 2)
    cases = [plan_cases._read((4, 0), 300, 200, dwell=(2, 3), jitter=10),
             plan_cases._read((9, 0), 90, 200, dwell=(2, 3), jitter=10),
             synthetic.make_dp_case(np.random.default_rng([seed0, it]), model, R=12, bandwidth=8, dwell=(lo, lo + 1),
                                    jitter=2, trim=3)]
    if mel == 4:   # the first read holds fewer than 4 samples per base (no path, for the reference as well): add one
        cases.append(plan_cases._read((4, 1), 300, 200, dwell=(4, 5), jitter=10))   # of the same length that has
    return dict(model=model, k=model[0], mel=mel, bw=200, cases=cases, tr=tr)


def make_plateau_batch(seed0, it):
    """-> dict(model, k, mel, bw, cases, tr): the read of tests/plan_cases.py whose bases 20 and 21 have the same
    level in the PLATEAU table, and its company read; min event length it % 4, transition rows on odd it // 4."""
    import plan_cases
    model = plan_cases.model_arrays(plan_cases.PLATEAU)
    cases = [plan_cases._plateau_read(), plan_cases._read((9, 1), 140, 30, model=plan_cases.BASE, dwell=(3, 4))]
    return dict(model=model, k=model[0], mel=it % 4, bw=30, cases=cases, tr=bool((it // 4) % 2))


def reads_of(cases):
    return [(c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'])
            for c in cases]


_NEAR_LIB = {}


def _near_tie_lib():
    """An instrumented long-double copy of the CPU restatement (oracle/nadavca_oracle.c), built once per process
    in a temporary directory: every `a > b` of the path search (node.cpp:52,72,82 restated) whose two scores
    are equal or differ — in 80-bit arithmetic — by less than the engine's tolerance zone (NVK_TIE_ULPS = 64 ulps
    of the reference's log value: 64 * 2^-52 relative) notes its row.  Test infrastructure."""
    if 'lib' in _NEAR_LIB:
        return _NEAR_LIB['lib']
    import ctypes as C
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = open(os.path.join(root, 'oracle', 'nadavca_oracle.c')).read()
    helper = '''#include <string.h>
int g_near_n; int g_near_row[4096];
static void near_note(double a, double b, int r) {   /* (`double` is long double in this build) */
  if (!(a > -1e300) || !(b > -1e300)) return;
  double d = a - b; if (d < 0) d = -d;   /* d == 0: a tie even in 80-bit arithmetic */
  double m = b < 0 ? -b : b;
  if (d <= m * 64.0 * 2.220446049250313e-16 && g_near_n < 4096) g_near_row[g_near_n++] = r;
}
int orc_near_count(void) { return g_near_n; }
int *orc_near_rows(void) { return g_near_row; }
void orc_near_reset(void) { g_near_n = 0; }
'''
    a = '''        double pv = dp[r - 1][i - bs[r - 1]];
        if (pv > best) {'''
    b = '''          double pv = dp[r - 1][from - bs[r - 1]];
          if (pv > best) {'''
    c = '''      for (int i = bs[r]; i <= be[r]; i++)
        if (dp[r][i - bs[r]] > best) {
          best = dp[r][i - bs[r]];
          best_idx = i;
        }'''
    assert a in s and b in s and c in s and '#include <string.h>' in s, 'oracle/nadavca_oracle.c changed: adapt the patch'
    s = s.replace(a, a.replace('        if (pv > best) {', '        near_note(pv, best, r);\n        if (pv > best) {'))
    s = s.replace(b, b.replace('          if (pv > best) {', '          near_note(pv, best, r);\n          if (pv > best) {'))
    s = s.replace(c, '''      for (int i = bs[r]; i <= be[r]; i++) {
        near_note(dp[r][i - bs[r]], best, r + 1);
        if (dp[r][i - bs[r]] > best) {
          best = dp[r][i - bs[r]];
          best_idx = i;
        }
      }''')
    s = s.replace('#include <string.h>', helper, 1)
    pre = ('#include <math.h>\n#include <stdint.h>\n#include <stdlib.h>\n#include <string.h>\n#include <stdio.h>\n'
           '#define double long double\n#define exp expl\n#define log logl\n#define sqrt sqrtl\n')
    tmp = tempfile.mkdtemp(prefix='orc_near_')
    src, lib = os.path.join(tmp, 'orc_near.c'), os.path.join(tmp, 'liborc_near.so')
    open(src, 'w').write(pre + s)
    subprocess.run(['gcc', '-O2', '-fPIC', '-std=gnu11', '-ffp-contract=off', '-Wno-unused', '-shared', '-o', lib, src,
                    '-lm'], check=True)
    _NEAR_LIB['lib'] = C.CDLL(lib)
    return _NEAR_LIB['lib']


def near_tie_bases(case, fb_model, bw, mel, tr):
    """Bases (event rows) at which the long-double reference compares two path scores inside the engine's
    tolerance zone on this read."""
    import ctypes as C
    from oracle.oracle import LongDoubleReferee
    lib = _near_tie_lib()
    ld = LongDoubleReferee.__new__(LongDoubleReferee)
    ld.lib = lib
    ld._pld = C.POINTER(C.c_longdouble)
    lib.orc_model_create.restype = C.c_void_p
    lib.orc_model_create.argtypes = [C.c_int, C.c_int, C.c_int, ld._pld, ld._pld, C.c_int64]
    lib.orc_refine_alignment.restype = C.c_int
    p_i32 = C.POINTER(C.c_int32)
    lib.orc_refine_alignment.argtypes = [C.c_void_p, ld._pld, C.c_int64, p_i32, C.c_int64, p_i32, C.c_int64, p_i32,
                                         C.c_int64, p_i32, C.c_int64, C.c_int, C.c_int, C.c_int, p_i32]
    k, central, alphabet, mean, sigma = fb_model
    mean_l = np.ascontiguousarray(mean, dtype=np.longdouble)
    sigma_l = np.ascontiguousarray(sigma, dtype=np.longdouble)
    ld.handle = lib.orc_model_create(int(k), int(central), int(alphabet), mean_l.ctypes.data_as(ld._pld),
                                     sigma_l.ctypes.data_as(ld._pld), mean_l.size)
    lib.orc_near_reset()
    c = case
    ld.refine_alignment(c['signal'], c['reference'], c['context_before'], c['context_after'],
                        c['approximate_alignment'], bw, mel, tr)
    lib.orc_near_rows.restype = C.POINTER(C.c_int)
    n = lib.orc_near_count()
    rows = np.array([lib.orc_near_rows()[i] for i in range(n)], dtype=np.int64)
    return np.unique(rows // 2 if tr else rows)


NVK_TIE_ULPS = 64   # nadavca_amd/csrc/xmath.h: the zone in which the reference's own choice hangs on rounding

# One record per classify_difference call of this process: dict(why, valid, d, deficit, margin, ratio, first_row).
# The tests print max(ratio) over the records they added (largest_ratio) so that a later change can tighten it.
SCORED = []


def largest_ratio(since=0):
    """Largest deficit / margin among the differences classified since record ``since`` that were valid paths with
    a positive margin (0.0 where there were none)."""
    r = [x['ratio'] for x in SCORED[since:] if x['valid'] and x['ratio'] is not None]
    return max(r) if r else 0.0


def same_level_bases(case, fb_model, k, central, alphabet):
    """-> bool per base j: its k-mer level equals that of base j - 1 (False for base 0)."""
    from nadavca_amd import synthetic
    c = case
    ext = np.concatenate([c['context_before'], c['reference'], c['context_after']]).astype(np.int64)
    ids = synthetic.kmer_ids(ext, len(c['context_before']), len(c['reference']), k, central, alphabet)
    mean = fb_model[3]
    return np.concatenate([[False], mean[ids[1:]] == mean[ids[:-1]]])


def flat_row(ev2, exp, same_level, j):
    """Every boundary of event row j that differs lies between two bases of equal level: the condition of the
    'flat-plateau' label.  NOT sufficient to accept a difference (moving such a boundary off the reference's
    plateau passes it); classify_difference scores the path as well."""
    return bool((ev2[j, 0] == exp[j, 0] or same_level[j]) and
                (ev2[j, 1] == exp[j, 1] or (j + 1 < len(same_level) and same_level[j + 1])))


def score_difference(ev, exp, case, bw, mel, tr, referee):
    """The path objective of the reference's search (oracle.LongDoubleReferee.path_score: the sum over DP rows of
    the log posterior boundary marginal, in 80-bit arithmetic) on the engine's rows ``ev``, on the double-precision
    reference's ``exp`` and on the long-double reference's own rows.
    -> dict(valid, ok, d, deficit, margin, ratio, first_row, hp):
    valid     the engine's rows are a path the search could have produced (shape, contiguity, bands, minimum
              event lengths, finite posteriors) and at least one of the two reference paths scores;
    d         path rows at which the engine differs from the better of the two reference paths;
    deficit   best - s_eng with best = max(s_ref, s_ld);
    margin    d * NVK_TIE_ULPS * 2^-52 * max_abs, max_abs the largest partial sum of the better reference path:
              each tolerant comparison of a max-product search can cost at most one zone of NVK_TIE_ULPS ulps of
              the reference's log score, and each deviating decision leaves at least one differing row;
    ok        valid and deficit <= margin;
    ratio     deficit / margin (None where margin is 0); first_row: first differing path row; hp: the long-double
              reference's rows."""
    from oracle.oracle import LongDoubleReferee
    c = case
    a = (c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'], bw, mel, tr)
    out = dict(valid=False, ok=False, d=0, deficit=None, margin=None, ratio=None, first_row=-1, hp=None)
    hp = referee.refine_alignment(*a)
    out['hp'] = hp
    R = len(c['reference'])
    p_eng = LongDoubleReferee.events_to_path(ev, R, tr)
    if p_eng is None:
        return out
    s_eng, s_ref, s_ld = referee.path_scores(*a, [ev, exp, hp])
    if s_eng is None:
        return out
    best = None
    for sc, rows in ((s_ref, exp), (s_ld, hp)):   # the double reference first: it wins an exact tie of the scores
        if sc is not None and (best is None or sc[0] > best[0][0]):
            best = (sc, LongDoubleReferee.events_to_path(rows, R, tr))
    if best is None:
        return out
    (s_best, max_abs), p_best = best
    differ = np.nonzero(p_eng != p_best)[0]
    d = int(differ.size)
    deficit = s_best - s_eng[0]
    margin = d * NVK_TIE_ULPS * np.longdouble(2.0) ** -52 * max_abs
    out.update(valid=True, ok=bool(deficit <= margin), d=d, deficit=float(deficit), margin=float(margin),
               ratio=float(deficit / margin) if margin > 0 else None, first_row=int(differ[0]) if d else -1)
    return out


def classify_difference(ev, exp, case, fb_model, k, central, alphabet, bw, mel, tr, referee=None):
    """Why do the engine's rows ``ev`` differ from the double-precision reference's ``exp`` on this read?

    First the proof, the same for every class (score_difference): the engine's rows must be a path the reference's
    search could have produced, and the objective that search maximises, evaluated on them in 80-bit arithmetic,
    must reach the better of the double-precision and the long-double reference's paths to within
    d * NVK_TIE_ULPS ulps of the reference's log score, d the number of differing path rows.  A difference that
    fails it is 'UNEXPLAINED' whatever else holds.

    Then the label, a diagnostic: 'flat-plateau' (every differing boundary lies between two bases with the SAME
    k-mer level), 'reference-rounding' (the same algorithm in 80-bit long double — oracle/liboracle_ld.so — sides
    with the engine on every differing row), 'precision-decided' (the reference changes its OWN answer on every
    differing row when computed in long double: an ill-conditioned arg-max), 'referee-tie' (reference and long
    double agree, and at the differing base the long-double reference itself compares two path scores that are
    equal or closer than the engine's tolerance zone — the read carries NVK_TIE_ULP or NVK_TIE_NEAR), or
    'UNEXPLAINED' where none applies.  The classification tests/dev/fuzz_parity.py prints, shared with the -m gpu
    tests so that a regression cannot hide behind the near-tie flag.  Every call adds a record to SCORED."""
    rec = dict(why='UNEXPLAINED', valid=False, ok=False, d=0, deficit=None, margin=None, ratio=None, first_row=-1)
    rec['why'] = _classify(ev, exp, case, fb_model, k, central, alphabet, bw, mel, tr, referee, rec)
    SCORED.append(rec)
    return rec['why']


def _classify(ev, exp, case, fb_model, k, central, alphabet, bw, mel, tr, referee, rec):
    from oracle.oracle import LongDoubleReferee
    ev2, exp = np.asarray(ev), np.asarray(exp).reshape(-1, 2)
    if ev2.size != exp.size:
        return 'UNEXPLAINED'
    ev2 = ev2.reshape(-1, 2)
    c = case
    ld = referee if referee is not None else LongDoubleReferee(*fb_model)
    sc = score_difference(ev2, exp, c, bw, mel, tr, ld)
    hp = sc.pop('hp')
    rec.update(sc)
    if not sc['ok'] or hp.shape != exp.shape:
        return 'UNEXPLAINED'
    same_level = same_level_bases(c, fb_model, k, central, alphabet)
    rows = np.nonzero((ev2 != exp).any(axis=1))[0]

    def flat(j):
        return flat_row(ev2, exp, same_level, j)

    if all(flat(j) for j in rows):
        return 'flat-plateau'
    if all(np.array_equal(ev2[j], hp[j]) or flat(j) for j in rows):
        return 'reference-rounding'
    if all(not np.array_equal(exp[j], hp[j]) or flat(j) for j in rows):
        return 'precision-decided'
    # The reference's doubles and the long doubles agree with each other and not with the engine: labelled only
    # where the long-double reference ITSELF finds the two path scores it compares at that base (or a neighbouring
    # one) equal, or closer than the engine's tolerance zone.  The reference adds UNNORMALISED log posteriors
    # (node.cpp:39-50): after r rows its scores are ~ r * |ln L(read)|, 5e6 on a sharp model, where even 80-bit
    # arithmetic resolves 1e-12 at best — it then keeps the first maximum — while the engine's scores are products
    # of normalised posteriors, 1e3-1e4 times smaller in the exponent, and tell such cells apart.
    near = near_tie_bases(c, fb_model, bw, mel, tr)
    if all(flat(j) or np.array_equal(ev2[j], hp[j]) or not np.array_equal(exp[j], hp[j]) or
           bool(np.any(np.abs(near - j) <= 1)) for j in rows):
        return 'referee-tie'
    return 'UNEXPLAINED'
