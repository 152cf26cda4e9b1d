"""GPU parity of the joint-hypotheses operator (nvk_estimate_joint_hypotheses_batch_dev,
dtw.estimate_joint_hypotheses_batch).  A hypothesis (p_1, b_1) .. (p_m, b_m) with b_m != ref[p_m] has an exact
counterpart in the reference: the entry [p_m, b_m] of EstimateLogLikelihoods on ref', the read's reference with the
substitutions 1 .. m-1 applied (include/nadavca_hip.h) — that entry of the CPU oracle is the expectation, with the
tolerance and -inf rule of tests/test_gpu_hypotheses.py (1e-9 relative + 1e-9 absolute, equal -inf pattern, no NaN).
Then bit-for-bit consistency with the listed operator, and the refusals."""
import numpy as np
import pytest

from conftest import dp_args

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-9


@pytest.fixture(scope='module')
def dtw():
    from nadavca_amd import dtw as d
    return d


def _reads(cases):
    return [(c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'])
            for c in cases]


def _close(got, exp):
    got, exp = np.asarray(got, dtype=float), np.asarray(exp, dtype=float)
    assert got.shape == exp.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(exp))
    assert not np.any(np.isnan(got))
    fin = np.isfinite(exp)
    err = float(np.max(np.abs(got[fin] - exp[fin]))) if fin.any() else 0.0
    assert np.allclose(got[fin], exp[fin], rtol=RTOL, atol=ATOL), err
    return err


def _hyp(rng, ref, alphabet, p1, pm, m):
    """m substitutions on p1 .. pm (both ends taken), the first and the last one effective, the inner ones random
    letters (some equal the reference: no-ops)."""
    inner = np.sort(rng.choice(np.arange(p1 + 1, pm), m - 2, replace=False)) if m > 2 else np.zeros(0, dtype=np.int64)
    pos = np.concatenate([[p1], inner, [pm]]).astype(np.int64)
    base = rng.integers(0, alphabet, pos.size)
    for i in (0, -1):
        base[i] = (ref[pos[i]] + 1 + rng.integers(0, alphabet - 1)) % alphabet
    return np.stack([pos, base], 1)


def _random_joint_list(rng, ref, k, central, alphabet, j):
    """Joint hypotheses for a read: read j % 5 == 4 gets none.  Otherwise 2 .. 4 substitutions at the largest span
    the read's interior allows (p_m - p_1 = 14 - k) and at smaller ones, hypotheses whose re-run clips at row 0 and
    at row R - 1 (there the span may be larger: 14 rows from the read's end), and duplicates."""
    R = len(ref)
    if j % 5 == 4:
        return []
    span, back, fwd = 14 - k, k - central - 1, central
    out = []
    for m in (2, 3, 4, 2, 3):
        s = span if len(out) < 3 else int(rng.integers(1, span + 1))
        m = min(m, s + 1)
        if m < 2 or R <= s:
            continue
        p1 = int(rng.integers(0, R - s))
        out.append(_hyp(rng, ref, alphabet, p1, p1 + s, m))
    # clipped at the start: first = 0, so p_m may go up to 13 - fwd; clipped at the end likewise
    pm = min(13 - fwd, R - 1)
    if pm >= 1:
        out.append(_hyp(rng, ref, alphabet, 0, pm, min(3, pm + 1)))
        if pm >= 2:
            out.append(_hyp(rng, ref, alphabet, 1, pm - 1 if pm - 1 > 1 else pm, 2))
    p1 = max(R - 14 + back, 0)
    if p1 < R - 1:
        out.append(_hyp(rng, ref, alphabet, p1, R - 1, min(3, R - p1)))
    out = [h for h in out if _rows(h, ref, R, back, fwd) <= 14]
    if out:
        out += [out[0], out[-1]]
    return [out[i] for i in rng.permutation(len(out))]


def _rows(h, ref, R, back, fwd):
    eff = [int(p) for p, b in h if b != ref[p]]
    return min(R - 1, eff[-1] + fwd) - max(0, eff[0] - back) + 1 if eff else 0


def _expected(oracle_port, mo, c, h, bw, mel, w, cache):
    """The oracle's entry [p_m, b_m] on the reference with the other substitutions applied."""
    ref2 = np.array(c['reference'], copy=True)
    ref2[h[:-1, 0]] = h[:-1, 1]
    key = ref2.tobytes()
    if key not in cache:
        cache[key] = np.asarray(oracle_port.estimate_log_likelihoods(
            c['signal'], ref2, c['context_before'], c['context_after'], c['approximate_alignment'], bw, mel, mo, w))
    return cache[key][h[-1, 0], h[-1, 1]]


def _check_against_oracle(dtw, oracle_port, mg, mo, model, cases, bw, mel, w, seed):
    k, central, alphabet = model[:3]
    lists = [_random_joint_list(np.random.default_rng([seed, j]), np.asarray(c['reference']), k, central, alphabet, j)
             for j, c in enumerate(cases)]
    total, got = dtw.estimate_joint_hypotheses_batch(_reads(cases), lists, bw, mel, mg, w)
    n, worst = 0, 0.0
    for j, (c, hs, vals) in enumerate(zip(cases, lists, got)):
        cache = {}
        assert vals.shape == (len(hs),)
        exp = np.array([_expected(oracle_port, mo, c, h, bw, mel, w, cache) for h in hs], dtype=float)
        worst = max(worst, _close(vals, exp))
        plain = np.asarray(oracle_port.estimate_log_likelihoods(
            c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'], bw, mel,
            mo, w))
        _close(total[j:j + 1], plain[0:1, c['reference'][0]])
        n += len(hs)
    print('k %d alphabet %d mel %d wobbling %d: %d joint hypotheses, largest |difference| %.3e'
          % (k, alphabet, mel, w, n, worst))
    return n


@pytest.mark.parametrize('mel', [0, 1, 2, 3, 4])
def test_joint_vs_oracle_random(dtw, oracle_port, mel):
    """k = 5 and 4 letters, with and without contexts, every compiled min_event_length, wobbling on / off."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(21, k=5, central=2)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases = []
    for i in range(10):
        rng = np.random.default_rng([288, mel, i])
        R = int(rng.integers(3, 90)) if i else 12
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(8, 50)),
                                            dwell=(max(mel, 1), 9), jitter=6,
                                            anchor_density=float(rng.uniform(0.1, 0.9)),
                                            with_context=bool(i % 3), trim=min(3, R // 3)))
    n = 0
    for bw in (12, 40):
        for w in (False, True):
            n += _check_against_oracle(dtw, oracle_port, mg, mo, model, cases, bw, mel, w, 900 + mel)
    assert n > 150


@pytest.mark.parametrize('k,central,alphabet', [(4, 1, 3), (4, 1, 5), (4, 0, 4), (5, 2, 5), (6, 2, 4), (6, 2, 5),
                                                (6, 3, 3), (8, 3, 5), (10, 4, 4)])
def test_joint_kmer_sizes_and_alphabets(dtw, oracle_port, k, central, alphabet):
    """k = 4, 5, 6 (items of up to 6 rows in groups of 8 lanes, the others in groups of 16) with 3 to 5 letters, and
    k = 8 and 10 (every item in a group of 16) at their spans."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(331 + k + alphabet, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases = []
    for i in range(6):
        rng = np.random.default_rng([289, k, alphabet, i])
        R = int(rng.integers(4, 70)) if i else 15
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(10, 40)), dwell=(2, 9),
                                            jitter=5, anchor_density=float(rng.uniform(0.2, 0.9)),
                                            with_context=bool(i % 2), trim=min(3, R // 3)))
    n = 0
    for w in (False, True):
        n += _check_against_oracle(dtw, oracle_port, mg, mo, model, cases, 30, 2, w, 1000 + k)
    assert n > 40


def test_joint_golden_nopath(dtw, golden_nopath):
    """Reads whose band holds no path: status NO_PATH and -inf, as the listed operator gives."""
    from nadavca_amd import _lib
    g = golden_nopath
    mg = dtw.KmerModel(*g.model)
    k, central, alphabet = g.model[:3]
    seen = 0
    for case in g.cases:
        sig, ref, cb, ca, anc, bw, mel = dp_args(case)
        R = len(ref)
        hs = [np.array([[p, (ref[p] + 1) % alphabet], [p + 1, (ref[p + 1] + 2) % alphabet]])
              for p in range(0, R - 1, 3)] + [np.zeros((0, 2), dtype=int)]
        for w in (0, 1):
            total, got, status = dtw.estimate_joint_hypotheses_batch([(sig, ref, cb, ca, anc)], [hs], bw, mel, mg,
                                                                     bool(w), return_status=True)
            exp = np.asarray(case['ell_w%d' % w])
            _close(total, exp[0:1, ref[0]])
            if np.isneginf(exp).all():
                assert status[0] == _lib.READ_NO_PATH
                assert np.isneginf(got[0]).all() and got[0].shape == (len(hs),)
                seen += 1
    assert seen > 0


@pytest.mark.parametrize('k,central,alphabet,mel', [(6, 2, 5, 2), (4, 1, 3, 1), (8, 3, 4, 2), (5, 2, 4, 0),
                                                    (5, 2, 4, 4), (6, 2, 4, 3)])
def test_consistency_with_the_listed_operator(dtw, k, central, alphabet, mel):
    """Single substitutions as joint hypotheses: ``hyp`` and ``total`` bit-equal to estimate_hypotheses_batch; a
    hypothesis padded with b == ref[p] rows bit-equal to the one without them; one made of such rows only (or of no
    row) bit-equal to ``total``."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(431 + k, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    batch = synthetic.make_batch(16, model, seed=27 + k, R=70, R_spread=40, bandwidth=40, dwell=(max(mel, 1), 9),
                                 jitter=6)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for w in (False, True):
        singles, padded, noops = [], [], []
        for j, c in enumerate(batch.cases):
            rng = np.random.default_rng([5, k, j])
            ref = np.asarray(c['reference'])
            R = ref.size
            p = rng.integers(0, R, 2 * R)
            rows = np.stack([p, rng.integers(0, alphabet, p.size)], 1)      # some with b == ref[p]
            singles.append(rows)
            pad, noop = [], []
            for pp, b in rows:
                extra = np.unique(np.concatenate([rng.integers(0, R, 3), [0, R - 1]]))   # no-ops anywhere in the read
                extra = extra[extra != pp]
                h = np.concatenate([[[pp, b]], np.stack([extra, ref[extra]], 1)])
                pad.append(h[np.argsort(h[:, 0])])
                noop.append(np.stack([extra, ref[extra]], 1) if pp % 2 else np.zeros((0, 2), dtype=np.int64))
            padded.append(pad)
            noops.append(noop)
        total, listed = dtw.estimate_hypotheses_batch(_reads(batch.cases), singles, 40, mel, mg, w)
        total1, got1 = dtw.estimate_joint_hypotheses_batch(_reads(batch.cases), [[r[None, :] for r in rows]
                                                                                 for rows in singles], 40, mel, mg, w)
        total2, got2 = dtw.estimate_joint_hypotheses_batch(_reads(batch.cases), padded, 40, mel, mg, w)
        total3, got3 = dtw.estimate_joint_hypotheses_batch(_reads(batch.cases), noops, 40, mel, mg, w)
        assert not np.isnan(total).any()
        for t in (total1, total2, total3):
            assert np.array_equal(bits(t), bits(total))
        for j in range(len(batch.cases)):
            assert not np.isnan(listed[j]).any()
            assert np.array_equal(bits(got1[j]), bits(listed[j])), (j, w)
            assert np.array_equal(bits(got2[j]), bits(listed[j])), (j, w)
            assert np.array_equal(bits(got3[j]), bits(np.full(len(noops[j]), total[j]))), (j, w)


def test_refusals(dtw):
    """Positions that do not ascend, a re-run of more than 14 rows, a position or base out of range: each fails ITS
    read with READ_BAD_INPUT, its outputs stay untouched and the neighbours equal a run without it.  Broken offsets
    are refused as a whole (NVK_ERR_INVALID -> ValueError).  Empty batches and lists pass."""
    import torch
    from nadavca_amd import synthetic, _lib
    from nadavca_amd.device import DeviceBatch, estimate_joint_hypotheses_dev
    k, alphabet = 6, 5
    model = synthetic.synth_model_arrays(77, k=k, central=2, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    batch = synthetic.make_batch(5, model, seed=4, R=60, R_spread=20, bandwidth=30, dwell=(2, 9), jitter=5)
    cases = batch.cases
    refs = [np.asarray(c['reference']) for c in cases]

    def sub(j, *ps):
        return np.array([[p, (refs[j][p] + 1) % alphabet] for p in ps])
    good = [[sub(j, p, p + 3, p + 8) for p in range(0, len(refs[j]) - 8, 5)] + [sub(j, 7)] for j in range(5)]
    total0, got0, st0 = dtw.estimate_joint_hypotheses_batch(_reads(cases), good, 30, 2, mg, True, return_status=True)
    assert (st0 == _lib.READ_OK).all() and all(np.isfinite(v).all() for v in got0)
    R1 = len(refs[1])
    r1 = refs[1]
    other = lambda p: (r1[p] + 1) % alphabet
    bad_hyps = {
        'descending': np.array([[20, other(20)], [18, other(18)]]),
        'repeated': np.array([[20, other(20)], [20, other(20)]]),
        'descending no-ops': np.array([[20, r1[20]], [18, r1[18]]]),
        'span 9 > 14 - k': np.array([[20, other(20)], [29, other(29)]]),
        'far apart': np.array([[5, other(5)], [40, other(40)]]),
        'position R': np.array([[R1 - 2, other(R1 - 2)], [R1, 0]]),
        'position -1': np.array([[-1, 0], [3, other(3)]]),
        'base 5': np.array([[3, other(3)], [4, 5]]),
        'base -1': np.array([[3, -1], [4, other(4)]]),
    }
    for name, h in bad_hyps.items():
        lists = list(good)
        lists[1] = good[1][:3] + [h] + good[1][3:]
        total, got, st = dtw.estimate_joint_hypotheses_batch(_reads(cases), lists, 30, 2, mg, True, on_error='status',
                                                             return_status=True)
        assert st.tolist() == [0, _lib.READ_BAD_INPUT, 0, 0, 0], name
        assert np.isnan(total[1]) and np.isnan(got[1]).all(), name          # left untouched
        for j in (0, 2, 3, 4):
            assert np.array_equal(got[j], got0[j]) and total[j] == total0[j], name
        with pytest.raises(ValueError, match='invalid input for read'):
            dtw.estimate_joint_hypotheses_batch(_reads(cases), lists, 30, 2, mg, True)
    # allowed: the span 14 - k exactly; a larger one where the read's end clips the re-run to 14 rows; no-ops far
    # away from the effective substitutions
    fine = [sub(1, 20, 28), sub(1, 0, 11), sub(1, R1 - 11, R1 - 1),
            np.array([[2, r1[2]], [20, other(20)], [24, other(24)], [R1 - 1, r1[R1 - 1]]])]
    _, _, st = dtw.estimate_joint_hypotheses_batch(_reads(cases), [good[0], fine, [], [], []], 30, 2, mg, True,
                                                   return_status=True)
    assert (st == 0).all()
    # a run without the bad read gives the neighbours the same values
    keep = [0, 2, 3, 4]
    total2, got2 = dtw.estimate_joint_hypotheses_batch(_reads([cases[j] for j in keep]), [good[j] for j in keep], 30,
                                                       2, mg, True)
    for a, j in enumerate(keep):
        assert np.array_equal(got2[a], got0[j]) and total2[a] == total0[j]
    # broken offsets, either level
    dev = torch.device('cuda', mg.context.device)
    db = DeviceBatch(batch, dev)
    T = lambda x: torch.tensor(x, dtype=torch.int64)
    pos = torch.arange(10, dtype=torch.int32)
    base = torch.zeros(10, dtype=torch.int32)
    ok_hyp, ok_sub = [0, 1, 2, 3, 4, 5], [0, 2, 4, 6, 8, 10]
    estimate_joint_hypotheses_dev(db, 30, 2, mg, True, T(ok_hyp), T(ok_sub), pos, base)
    for off in ([1, 2, 3, 4, 5, 5], [0, 3, 2, 4, 5, 5], [0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6]):
        with pytest.raises(ValueError, match='hypothesis offsets'):
            estimate_joint_hypotheses_dev(db, 30, 2, mg, True, T(off), T(ok_sub), pos, base)
    for off in ([1, 2, 4, 6, 8, 10], [0, 4, 2, 6, 8, 10], [0, 2, 4, 6, 8, 9], [0, 2, 4, 6, 8, 12]):
        with pytest.raises(ValueError, match='substitution offsets'):
            estimate_joint_hypotheses_dev(db, 30, 2, mg, True, T(ok_hyp), T(off), pos, base)
    # an empty batch, a batch without any hypothesis, hypotheses without any substitution
    assert dtw.estimate_joint_hypotheses_batch([], [], 30, 2, mg, True)[1] == []
    total3, got3 = dtw.estimate_joint_hypotheses_batch(_reads(cases), [[]] * 5, 30, 2, mg, True)
    assert np.array_equal(total3, total0) and all(v.size == 0 for v in got3)
    total4, got4 = dtw.estimate_joint_hypotheses_batch(_reads(cases), [[np.zeros((0, 2), int)] * 3] * 5, 30, 2, mg,
                                                       True)
    assert np.array_equal(total4, total0) and all(np.array_equal(v, np.full(3, t)) for v, t in zip(got4, total0))
