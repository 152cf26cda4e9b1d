"""Seeded smallest cases, one or more per built kernel variant of refine_alignment and of the log-likelihood
operators, shared by tests/test_gpu_variant_census.py and tests/test_variant_cases_cpu.py.  Each case is named after
the variant it is for; the census asserts through the library's launch report (include/nadavca_hip.h) that the case
reached it.

Align cases: ``dict(name, model, bandwidth, mel, transitions, reads, sweeps, rely, team, ...)`` — one
refine_alignment batch.  ``sweeps``: the (mel, transitions, waves, period) variants the batch must report; ``rely``:
the reads that have to equal the oracle without a loose tie bit, so that the variant the case is named for counts as
compared (indices into ``reads``); ``team``: {read index: (lo, hi)} the interval of team skew + min event length the
name claims for a team read, for a lower bound of the skew (an edge or cut case: the sum itself or one below, the
planner's own skew is in ``cw``).

The variants (csrc/kernels_align3.hip, select_sweeps / launch_align3): one wave per read keeps the base rescale period
(8 steps, 16 with transition rows); a team of four waves starts there and doubles the period while it is
<= team skew + min event length.  The team skew of a read is (band width - samples the band moves on in 256 rows) / 256
+ 1, so the team reads here are as short as has more than 256 rows (140 bases with transition rows, 270 without), 8-12
samples per base, and as wide a band as the skew needs.

Log-likelihood cases: ``dict(name, kind, lanes, mel, model, bandwidth, reads, ...)`` — the 40 kernels of ell_dispatch's
tables (csrc/kernels_ell.hip): min event length 0-4 x 8 lanes per hypothesis (k = 5) or 16 (k = 7) x full matrix / listed /
joint / edit hypotheses.  The four kinds of one (mel, lanes) share their reads."""
import numpy as np

import plan_cases
from nadavca_amd import synthetic

ALIGN1_C_CAP = 3    # csrc/nvk_internal.h: skew above it hands a read to a team of waves
TEAM_ROWS = 256     # rows between two rows of one team lane (64 * ALIGN3_TEAM_W)
SEED = 20261019     # of the one-wave batches: tests/test_gpu_parity_scored.py's

# Largest team skew whose rings fit a CU's 160 KB of LDS, per min event length: launch_align3's lds_need with 4 waves,
# 1 KB of exponent table + 4 signal rings of SR samples (SR the power of two >= 64 c + 64) + (c + mel + 1) history
# slots of 256 lanes x 20 B.  Up to c = 15 the rings hold 1024 samples and every min event length fits; c = 16 doubles
# them, and 65 KB of rings leave room for 18 slots: c + mel <= 17.  The census asserts these through the report (the
# lds_cut cases).
TEAM_C_FIT = {0: 17, 1: 16, 2: 15, 3: 15, 4: 15}


def base_period(tr):
    return 16 if tr else 8


def period_of(c, mel, tr):
    """launch_align3's rescale period for a launch that serves skews up to c."""
    p = base_period(tr)
    while p <= c + mel:
        p *= 2
    return p


def _t(tr):
    return 'trans' if tr else 'plain'


# ---------------------------------------------------------------------------------------------------------------------
# refine_alignment
# ---------------------------------------------------------------------------------------------------------------------
def team_read(seed, tr, bandwidth, dwell_lo):
    """A team read: just above 256 rows, anchored at every base without jitter, so that its bands are as even as the
    dwell times allow and the team skew follows the bandwidth (one unit per 128 samples of it).  ``dwell_lo``: 2 for
    two or three samples per base, 4 for four or five, 8 for 8-12."""
    R = 140 if tr else 270
    dwell = (dwell_lo, dwell_lo + (1 if dwell_lo < 8 else 4))
    return plan_cases._read((30,) + tuple(seed), R, bandwidth, dwell=dwell, jitter=0, anchor_density=1.0)


def narrow_read(seed, mel):
    """The company of a team read: 12 bases under a band of 8 samples; whatever the batch's bandwidth, its band is its
    whole slice and one wave serves it."""
    lo = max(mel, 2)
    return synthetic.make_dp_case(np.random.default_rng([SEED, 31] + list(seed)), plan_cases.model_arrays(plan_cases.BASE),
                                  R=12, bandwidth=8, dwell=(lo, lo + 1), jitter=2, trim=3)


def _align(name, model, bandwidth, mel, tr, reads, sweeps, rely, team=None, **kw):
    return dict(name=name, model=model, bandwidth=bandwidth, mel=mel, transitions=tr, reads=list(reads),
                sweeps=sorted(sweeps), rely=tuple(rely), team=dict(team or {}), **kw)


# The team cases.  Under a band hundreds of bases wide the sweeps hand many reads on to the exact kernel (cells far off
# the path leave the number range of the scaled doubles; which reads, depends on their samples), and a read the exact
# kernel redid says nothing about the team kernel — beyond team skew ~13 the exact kernel's one-wave rings do not
# hold it either and it ends as NVK_READ_TOO_WIDE.  So every read below was chosen, by seed, among reads the sweeps
# keep: the census asserts that nothing was handed on (reads_redone_exact) and that the read carries no loose tie bit.
# Bandwidths: in the middle of the stretch that gives the team skew wanted, by the planner's skew restated on the
# oracle's bands; the census asserts the skew through nvk_last_read_skews.
# A read: (dwell_lo, seed salt, bandwidth it is made with, team skew under the batch's bandwidth — None: above the LDS
# fit, handed to the exact kernel, which refuses it[, 'handed': a read the sweeps are known to hand on, there to size
# the launch, not relied on]).  A read made with a narrower band than the batch runs under has its bands clipped by
# its slice.
# TEAM_SPECS: (mel, transitions, period) -> (batch bandwidth, [reads]); the narrow read comes with every batch.
TEAM_SPECS = {
    (0, False, 8): (520, [(8, 0, 520, 1)]),
    (0, False, 32): (2678, [(2, 0, 621, 8), (2, 0, 2678, None)]),
    (0, True, 16): (520, [(8, 0, 520, 1)]),
    (0, True, 32): (2524, [(2, 0, 784, 8), (2, 0, 2524, None)]),
    (1, False, 8): (280, [(2, 0, 280, 1)]),
    (1, False, 16): (2486, [(8, 5, 2486, 10)]),
    (1, False, 32): (2298, [(2, 0, 2298, 16)]),
    (1, True, 16): (520, [(8, 0, 520, 1)]),
    (1, True, 32): (2608, [(8, 0, 2608, 16)]),
    (2, False, 8): (280, [(2, 0, 280, 1)]),
    (2, False, 16): (1401, [(2, 0, 1401, 9)]),
    (2, False, 32): (2426, [(2, 0, 624, 8), (2, 0, 2426, None)]),
    (2, True, 16): (520, [(8, 0, 520, 1)]),
    (2, True, 32): (2271, [(2, 0, 789, 8), (2, 0, 2271, None)]),
    (3, False, 8): (520, [(8, 0, 520, 2)]),
    (3, False, 16): (2218, [(8, 1, 2218, 8)]),
    (3, True, 16): (520, [(8, 0, 520, 2)]),
    (3, True, 32): (2742, [(8, 0, 259, 8), (8, 0, 2742, None)]),
    (4, False, 8): (520, [(8, 0, 520, 3)]),
    (4, False, 16): (2096, [(8, 0, 2096, 7)]),
    (4, False, 32): (2873, [(8, 1, 2873, 13)]),
    (4, True, 16): (520, [(8, 0, 520, 3)]),
    (4, True, 32): (2747, [(8, 0, 269, 8), (8, 0, 2747, None)]),
    # (0, plain, 16): every read of team skew 8-11 tried alone was handed on (56 of 56); a read of skew 4 is kept, beside
    # the read of skew 12 that sizes the launch and is itself handed on.  (3, plain, 32): 4-5 samples per base — reads
    # of two or three samples per base hold events shorter than the min event length and were handed on 54 of 54 times
    (0, False, 16): (1786, [(2, 0, 114, 4), (2, 0, 1786, 12, 'handed')]),
    (3, False, 32): (2683, [(4, 2, 355, 8), (4, 0, 2683, None)]),
}
# The edges of launch_align3's arithmetic, on ONE read each, the batch's bandwidth a sample apart: team skew + min
# event length 7 | 8 (the period of 8 doubles; without transition rows only, with them the period starts at 16) and
# 15 | 16.  name -> (transitions, mel, reads, bandwidth below the edge, above it); the widest read's skew is the one
# below the edge
EDGE_SPECS = {
    'edge_plain_7_8': (False, 2, [(8, 4, 3152, 5)], 1906, 1907),
    'edge_plain_15_16': (False, 2, [(2, 0, 619, 8), (2, 0, 2876, 13, 'handed')], 1982, 1983),
    'edge_trans_15_16': (True, 2, [(2, 0, 785, 8), (2, 0, 2876, 13, 'handed')], 1820, 1821),
}
# A team batch whose widest read is cut by the LDS fit: a read at TEAM_C_FIT, made with a narrower band than the batch
# runs under (its slice clips its bands), which is swept; a read two units of skew above the fit; the narrow read.
# (mel, transitions) -> (batch bandwidth, [read at the fit, read above it])
CUT_SPECS = {
    (1, False): (3490, [(8, 0, 638, 16), (8, 0, 3490, None)]),
    (1, True): (2870, [(8, 0, 1288, 16), (8, 0, 2870, None)]),
}
TEAM_INTERVALS = {(8, False): (1, 7), (16, False): (8, 15), (16, True): (1, 15), (32, False): (16, 99),
                  (32, True): (16, 99)}


def _spec_read(tag, tr, spec):
    dwell_lo, salt, bw_made = spec[:3]
    return team_read(tuple(tag) + (salt,), tr, bw_made, dwell_lo)


def _team_batch(name, tag, mel, tr, period, bw, specs, **kw):
    """A batch of team reads by their specs and the narrow read: the launch class of the teams is sized by the widest
    skew among them that fits, and reports ``period``."""
    reads = [_spec_read(tag + (i,), tr, sp) for i, sp in enumerate(specs)] + [narrow_read(tag, mel)]
    cws = {i: sp[3] for i, sp in enumerate(specs) if sp[3] is not None}
    above = tuple(i for i, sp in enumerate(specs) if sp[3] is None)
    handed = tuple(i for i, sp in enumerate(specs) if len(sp) > 4)
    team = {i: TEAM_INTERVALS[(period_of(c, mel, tr), tr)] for i, c in cws.items()}
    team.update({i: (TEAM_C_FIT[mel] + mel + 1, 99) for i in above})
    c_launch = min(max([TEAM_C_FIT[mel] + 1] * len(above) + list(cws.values())), TEAM_C_FIT[mel])
    assert period_of(c_launch, mel, tr) == period, (name, c_launch, period)
    return _align(name, plan_cases.model_arrays(plan_cases.BASE), bw, mel, tr, reads,
                  [(mel, tr, 4, period), (mel, tr, 1, base_period(tr))], rely=sorted(set(cws) - set(handed)), team=team,
                  cw=cws, above=above, handed=handed, c_launch=c_launch, **kw)


def wave_cases():
    """One wave per read, min event length 0-4 x transition rows on/off: the batches of fuzz_cases.make_run_batch."""
    from fuzz_cases import make_run_batch
    out = []
    for it in range(10):
        fb = make_run_batch(SEED, it)
        mel, tr = fb['mel'], fb['tr']
        out.append(_align('wave_mel%d_%s' % (mel, _t(tr)), fb['model'], fb['bw'], mel, tr, fb['cases'],
                          [(mel, tr, 1, base_period(tr))], rely=range(len(fb['cases'])), rely_any=True))
    return out


def team_cases():
    out = []
    for (mel, tr, period), (bw, specs) in sorted(TEAM_SPECS.items()):
        out.append(_team_batch('team_mel%d_%s_p%d' % (mel, _t(tr), period), (1, mel, int(tr), period), mel, tr, period,
                               bw, specs))
    return out


def edge_cases():
    out = []
    for name, (tr, mel, specs, bw_lo, bw_hi) in sorted(EDGE_SPECS.items()):
        widest = max(range(len(specs)), key=lambda i: specs[i][3])
        for bw, up in ((bw_lo, 0), (bw_hi, 1)):
            sp = [x if i != widest else x[:3] + (x[3] + up,) + x[4:] for i, x in enumerate(specs)]
            c = sp[widest][3]
            case = _team_batch('%s_sum%d' % (name, c + mel), (2,) + tuple(name.encode()), mel, tr,
                               period_of(c, mel, tr), bw, sp, edge=True)
            case['team'][widest] = (c + mel - 1, c + mel)   # (the lower bound may be one short at the edge itself)
            out.append(case)
    return out


def cut_cases():
    out = []
    for (mel, tr), (bw, specs) in sorted(CUT_SPECS.items()):
        fit = TEAM_C_FIT[mel]
        assert specs[0][3] == fit and len(specs[0]) == 4 and specs[1][3] is None
        case = _team_batch('lds_cut_mel%d_%s' % (mel, _t(tr)), (3, mel, int(tr)), mel, tr, period_of(fit, mel, tr), bw,
                           specs, cut=fit)
        case['team'][0] = (fit + mel - 1, fit + mel)
        out.append(case)
    return out


def retry_case():
    """A read the sweeps really hand on to the exact kernel: tests/dev/fuzz_parity.py seed 11, iteration 4230, a model
    three times sharper than the signal's noise (tests/test_gpu_edge_cases.py pins its result)."""
    from fuzz_cases import make_fuzz_batch
    fb = make_fuzz_batch(11, 4230)
    return _align('retry_sharp_model', fb['model'], fb['bw'], fb['mel'], fb['tr'], fb['cases'],
                  [(fb['mel'], fb['tr'], 1, base_period(fb['tr']))], rely=(), retry=True)


def exact_cases():
    """align_kernel<MEL>, min event length 0-4, under NADAVCA_ALIGN_KERNEL=1: a one-wave batch (fewer reads of it) and
    the small team read with its company, so that both classes of the exact launch run; transition rows on at even
    min event lengths."""
    from fuzz_cases import make_run_batch
    out = []
    for mel in range(5):
        tr = mel % 2 == 0
        fb = make_run_batch(SEED, mel + (5 if tr else 0), n_reads=6)
        assert fb['mel'] == mel and fb['tr'] == tr
        out.append(_align('exact_mel%d_%s' % (mel, _t(tr)), fb['model'], fb['bw'], mel, tr, fb['cases'], [],
                          rely=range(6), rely_any=True, exact=True))
        period = base_period(tr)
        if (mel, tr, period) in TEAM_SPECS:
            bw, specs = TEAM_SPECS[(mel, tr, period)]
            case = _team_batch('exact_team_mel%d_%s' % (mel, _t(tr)), (1, mel, int(tr), period), mel, tr, period, bw,
                               specs, exact=True)
            case['sweeps'] = []
            out.append(case)
    return out


def align_cases():
    """Every refine_alignment case run in the test's own process, from the variants the rest of the suite runs to
    those only these cases reach."""
    cases = wave_cases() + [retry_case()]
    teams = team_cases()
    cases += sorted(teams, key=lambda c: max(v[3] for v in c['sweeps']))
    cases += edge_cases() + cut_cases()
    assert len({c['name'] for c in cases}) == len(cases)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# estimate_log_likelihoods and the listed / joint / edit hypotheses
# ---------------------------------------------------------------------------------------------------------------------
ELL_KINDS = ('full', 'listed', 'joint', 'edit')
ELL_LANES = {8: (41, 5, 2), 16: (42, 7, 3)}   # lanes per hypothesis -> (seed, k, central) of synth_model_arrays
ELL_BW = 200
JOINT_ROWS = 14      # csrc/ell_items.h: rows one hypothesis re-runs at most
ELL_C_MAX = 62       # launch_ell's largest skew: at 63 the signal ring doubles to 8192 samples and leaves 160 KB
_ell_models = {}
_ell_batches = {}


def ell_model(lanes):
    if lanes not in _ell_models:
        seed, k, central = ELL_LANES[lanes]
        _ell_models[lanes] = synthetic.synth_model_arrays(seed, k=k, central=central)
    return _ell_models[lanes]


def ell_reads(mel, lanes):
    """The reads the four kinds of (mel, lanes) share: 3-90 bases with random dwell, anchors and contexts as
    tests/test_gpu_ell.py::test_ell_vs_oracle_random has them (skew 1: at most 64 bases, or a band that moves on
    faster than it is wide), one of 3 and one of 12 bases, and an 85-base read of lo .. lo + 1 samples per base whose
    band of 401 samples is wider than the samples 64 bases take (skew >= 2)."""
    key = (mel, lanes)
    if key not in _ell_batches:
        model = ell_model(lanes)
        lo = max(mel, 1)
        reads = []
        for i in range(6):
            rng = np.random.default_rng([SEED, 40, mel, lanes, i])
            R = int(rng.integers(13, 91)) if i > 1 else (3, 12)[i]
            reads.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(8, 50)), dwell=(lo, 9),
                                                jitter=6, anchor_density=float(rng.uniform(0.1, 0.7)),
                                                with_context=bool(i % 3), trim=min(3, R // 3)))
        reads.append(synthetic.make_dp_case(np.random.default_rng([SEED, 41, mel, lanes]), model, R=85,
                                            bandwidth=ELL_BW, dwell=(lo, lo + 1), jitter=4, anchor_density=0.5))
        _ell_batches[key] = reads
    return _ell_batches[key]


def ell_cases():
    out = []
    for lanes in (8, 16):
        for mel in range(5):
            for kind in ELL_KINDS:
                out.append(dict(name='ell_mel%d_l%d_%s' % (mel, lanes, kind), kind=kind, lanes=lanes, mel=mel,
                                model=ell_model(lanes), bandwidth=ELL_BW, reads=ell_reads(mel, lanes), wide_read=6,
                                hyp_reads=(2, 5, 6)))
    # what the suite ran before these cases first: 8 lanes, and 16 lanes at min event length 2
    out.sort(key=lambda c: (c['lanes'] == 16 and c['mel'] != 2, c['lanes'], c['mel']))
    assert len({c['name'] for c in out}) == len(out)
    return out


def ell_too_wide_case():
    """Beside the reads of (2, 8): an 80-base read of two or three samples per base under bandwidth 2400, skew ~ 70,
    above launch_ell's ELL_C_MAX.  Every read of 64 bases or fewer has skew 1 under any bandwidth."""
    model = ell_model(8)
    reads = [c for c in ell_reads(2, 8) if len(c['reference']) <= 64]
    wide = synthetic.make_dp_case(np.random.default_rng([SEED, 42]), model, R=80, bandwidth=2400, dwell=(2, 3),
                                  jitter=4, anchor_density=0.5)
    return dict(name='ell_too_wide', kind='full', lanes=8, mel=2, model=model, bandwidth=2400, reads=reads + [wide],
                too_wide=len(reads))


def _sub(ref, alphabet, p, shift=1):
    return [p, (int(ref[p]) + shift) % alphabet]


def joint_rows(h, ref, k, central):
    """Rows the joint hypothesis h re-runs (include/nadavca_hip.h): first .. last of its effective substitutions."""
    R = len(ref)
    eff = [int(p) for p, b in h if b != ref[p]]
    return min(R - 1, eff[-1] + central) - max(0, eff[0] - (k - central - 1)) + 1 if eff else 0


def joint_list(ref, k, central, alphabet, lanes):
    """Joint hypotheses of a read, by the rows they re-run: two adjacent substitutions (k + 1 rows: with k = 5 the
    6 rows that still fit a group of 8 lanes beside its two other roles, rows + 2 <= 8) and two with a base between
    them (k + 2: 7 rows, filed from the back of the list at 8 lanes); the full JOINT_ROWS with two and with three
    substitutions; windows clipped at row 0 and at the last row; a hypothesis without an effective substitution (the
    read's total); a duplicate.  Reads too short for a span leave it out."""
    ref = np.asarray(ref)
    R = len(ref)
    out = []
    mid = max(k - central - 1, (R - JOINT_ROWS) // 2)
    for span in (1, 2, JOINT_ROWS - k):
        if mid + span + central < R:
            out.append(np.array([_sub(ref, alphabet, mid), _sub(ref, alphabet, mid + span, 2)]))
    span = JOINT_ROWS - k
    if span >= 2 and mid + span + central < R:
        out.append(np.array([_sub(ref, alphabet, mid), _sub(ref, alphabet, mid + 1, 3), _sub(ref, alphabet, mid + span)]))
    if R >= 3:
        out.append(np.array([_sub(ref, alphabet, 0), _sub(ref, alphabet, min(2, R - 1))]))
        out.append(np.array([_sub(ref, alphabet, R - 2), _sub(ref, alphabet, R - 1, 2)]))
        out.append(np.array([[1, int(ref[1])]]))
    if out:
        out.append(out[0])
    assert all(joint_rows(h, ref, k, central) <= JOINT_ROWS for h in out)
    return out


def joint_one_row_more(ref, k, central, alphabet):
    """Two substitutions that re-run JOINT_ROWS + 1 rows in the read's interior: NVK_READ_BAD_INPUT."""
    ref = np.asarray(ref)
    mid = k - central - 1
    h = np.array([_sub(ref, alphabet, mid), _sub(ref, alphabet, mid + JOINT_ROWS - k + 1)])
    assert joint_rows(h, ref, k, central) == JOINT_ROWS + 1
    return h


def edit_rows(R, k, central, p, d, i):
    """Rows of the edited reference the edit (p, d, i letters) re-runs (include/nadavca_hip.h)."""
    back, fwd = k - central - 1, central
    return min(R - d + i - 1, p + i - 1 + fwd) - max(0, min(p - 1, p - back)) + 1


def edit_list(ref, anchors, k, central, alphabet, lanes):
    """Edits of a read, by the rows they re-run: a deletion of one base without an anchor, insertions of 1 .. n
    letters with n the largest whose window has JOINT_ROWS rows (with k = 5: 2 letters re-run 6 rows, 3 letters 7 —
    either side of rows + 2 <= 8), an insertion at p = 1 and at p = R - 1 (windows clipped at the ends), a mixed edit,
    a duplicate.  Deletions only of bases without an anchor: the mapped band is then the one the reference computes."""
    ref = np.asarray(ref)
    R = len(ref)
    anchored = set(np.asarray(anchors).reshape(-1, 2)[:, 1].tolist())
    letters = lambda n, s: [(s + 3 * q) % alphabet for q in range(n)]
    out = []
    mid = max(2, R // 2)
    if mid > R - 2:
        return out
    n = 0
    while n < 13 and edit_rows(R, k, central, mid, 0, n + 1) <= JOINT_ROWS:
        n += 1
    for i in sorted({1, 2, 3, n} & set(range(1, n + 1))):
        out.append((mid, 0, letters(i, i)))
    free = [p for p in range(1, R - 1) if p not in anchored]
    if free:
        out.append((free[len(free) // 2], 1, []))
        out.append((free[0], 1, letters(2, 1)))
    out.append((1, 0, letters(1, 2)))
    out.append((R - 1, 0, letters(1, 3)))
    out = [(p, d, s) for p, d, s in out if 1 <= p and p + d <= R - 1 and edit_rows(R, k, central, p, d, len(s)) <= JOINT_ROWS]
    if out:
        out.append(out[0])
    return out


def edit_one_row_more(ref, k, central, alphabet):
    """An insertion whose window has JOINT_ROWS + 1 rows: NVK_READ_BAD_INPUT."""
    R = len(ref)
    mid = max(2, R // 2)
    n = 1
    while edit_rows(R, k, central, mid, 0, n) <= JOINT_ROWS:
        n += 1
    assert edit_rows(R, k, central, mid, 0, n) == JOINT_ROWS + 1 and n <= 13
    return (mid, 0, [q % alphabet for q in range(n)])


def reads_of(cases):
    return [(c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'])
            for c in cases]


def skew_lower_bound(oracle, read, bandwidth, transitions, rows):
    """tests/test_gpu_plan_shapes.py::_skew_lower_bound for lanes ``rows`` rows apart: a lower bound of the skew the
    planner finds, from the oracle's bands alone."""
    R, N = len(read['reference']), len(read['signal'])
    bs, be = oracle.bands(read['approximate_alignment'], R, N, bandwidth)
    T = 2 * R if transitions else R + 1
    band = (lambda r: (r + 1) // 2) if transitions else (lambda r: r)
    need = 1
    for r in range(rows, T):
        d = int(be[band(r - rows)]) - int(bs[band(r)]) + 1
        if d >= 0:
            need = max(need, d // rows + 1)
    return need
