"""GPU parity of the edit-hypotheses operator (nvk_estimate_edit_hypotheses_batch_dev,
dtw.estimate_edit_hypotheses_batch).  An edit (p, d, s) that deletes no anchored base has an exact counterpart in the
reference: the no-substitution total of EstimateLogLikelihoods on (ref', anchors') of ``call_indels.apply_edit`` —
the entry [0, ref'[0]] of the CPU oracle is the expectation, with the tolerance and -inf rule of
tests/test_gpu_hypotheses.py (1e-9 relative + 1e-9 absolute, equal -inf pattern, no NaN).  Then the engine's own
invariants, the no-path golden and the refusals."""
import numpy as np
import pytest

from conftest import dp_args

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-9
MAX_ROWS, MAX_INS = 14, 13


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


def _rows(R, k, central, p, d, i):
    """Rows of the edited reference the edit re-runs: first' .. last' of include/nadavca_hip.h."""
    back, fwd = k - central - 1, central
    return min(R - d + i - 1, p + i - 1 + fwd) - max(0, min(p - 1, p - back)) + 1


def _valid(R, k, central, p, d, i):
    return 1 <= p and d >= 0 and p + d <= R - 1 and i <= MAX_INS and _rows(R, k, central, p, d, i) <= MAX_ROWS


def _largest_insertion(R, k, central, p, d=0):
    i = 0
    while _valid(R, k, central, p, d, i + 1):
        i += 1
    return i


def _random_edit_list(rng, ref, anchors, k, central, alphabet, j):
    """Edits for a read: read j % 5 == 4 gets none.  Deletions only of bases without an anchor (then the mapped band
    is the band the reference computes, so every edit is comparable): pure ones of 1 .. 3 bases, mixed (d, i);
    insertions of 1 letter up to the row limit; edits at p = 1 and at p + d = R - 1; windows clipped at row 0 and at
    row R' - 1 with the largest insertion that fits; duplicates."""
    R = len(ref)
    if j % 5 == 4:
        return []
    anchored = set(np.asarray(anchors).reshape(-1, 2)[:, 1].tolist())
    free = lambda p, d: all(q not in anchored for q in range(p, p + d))
    letters = lambda i: rng.integers(0, alphabet, i).tolist()
    out = []
    for d in (1, 2, 3, 1, 2):                                             # pure deletions
        at = [p for p in range(1, R - d) if free(p, d)]
        if at:
            out.append((int(rng.choice(at)), d, []))
    for d, i in ((1, 1), (2, 1), (1, 3), (3, 2)):                         # mixed
        at = [p for p in range(1, R - d) if free(p, d)]
        if at:
            out.append((int(rng.choice(at)), d, letters(i)))
    for i in (1, 1, 2, None, None):                                       # insertions, up to the row limit
        p = int(rng.integers(1, R))
        out.append((p, 0, letters(_largest_insertion(R, k, central, p) if i is None else i)))
    # the ends: p = 1 and p + d = R - 1, clipped at row 0 / at row R' - 1, with the largest insertion that fits
    out += [(1, 0, letters(1)), (R - 1, 0, letters(1)), (1, 0, letters(_largest_insertion(R, k, central, 1))),
            (R - 1, 0, letters(_largest_insertion(R, k, central, R - 1)))]
    if R > 3:
        out += [(2, 0, letters(_largest_insertion(R, k, central, 2))),
                (R - 2, 0, letters(_largest_insertion(R, k, central, R - 2)))]
    for d in (1, 2):
        if R - 1 - d >= 1 and free(1, d):
            out.append((1, d, letters(int(rng.integers(0, 2)))))
        if R - 1 - d >= 1 and free(R - 1 - d, d):
            out.append((R - 1 - d, d, letters(int(rng.integers(0, 3)))))
    out = [(p, d, s) for p, d, s in out if (d or s) and _valid(R, k, central, p, d, len(s))]
    if out:
        out += [out[0], out[-1]]
    return [out[i] for i in rng.permutation(len(out))]


def _expected(oracle_port, mo, c, edit, bw, mel, w, cache):
    """The oracle's no-substitution total on the edited reference and anchors."""
    from nadavca_amd.call_indels import apply_edit
    ref2, anchors2, clean = apply_edit(c['reference'], c['approximate_alignment'], *edit)
    assert clean
    key = (ref2.tobytes(), anchors2.tobytes())
    if key not in cache:
        ll = np.asarray(oracle_port.estimate_log_likelihoods(
            c['signal'], ref2.astype(np.int32), c['context_before'], c['context_after'], anchors2.astype(np.int32), bw,
            mel, mo, w))
        cache[key] = ll[0, ref2[0]]
    return cache[key]


def _check_against_oracle(dtw, oracle_port, mg, mo, model, cases, bw, mel, w, seed):
    k, central, alphabet = model[:3]
    lists = [_random_edit_list(np.random.default_rng([seed, j]), np.asarray(c['reference']),
                               c['approximate_alignment'], k, central, alphabet, j) for j, c in enumerate(cases)]
    total, got = dtw.estimate_edit_hypotheses_batch(_reads(cases), lists, bw, mel, mg, w)
    n = n_del = 0
    worst = 0.0
    for j, (c, es, vals) in enumerate(zip(cases, lists, got)):
        cache = {}
        assert vals.shape == (len(es),)
        exp = np.array([_expected(oracle_port, mo, c, e, bw, mel, w, cache) for e in es], dtype=float)
        worst = max(worst, _close(vals, exp))
        plain = np.asarray(oracle_port.estimate_log_likelihoods(
            c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'], bw, mel,
            mo, w))
        _close(total[j:j + 1], plain[0:1, c['reference'][0]])
        n += len(es)
        n_del += sum(1 for _, d, _ in es if d > 0)
    print('k %d central %d alphabet %d mel %d wobbling %d bandwidth %d: %d edit hypotheses (%d delete), largest '
          '|difference| %.3e' % (k, central, alphabet, mel, w, bw, n, n_del, worst))
    return n, n_del


@pytest.mark.parametrize('mel', [0, 1, 2, 3, 4])
def test_edits_vs_oracle_random(dtw, oracle_port, mel):
    """k = 5 and 4 letters, R 3 .. 90, with and without contexts, every compiled min_event_length, wobbling on / off,
    bandwidth 12 and 40."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(21, k=5, central=2)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases = []
    for i in range(10):
        rng = np.random.default_rng([388, mel, i])
        R = int(rng.integers(3, 91)) if i > 1 else (3, 12)[i]
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(8, 50)),
                                            dwell=(max(mel, 1), 9), jitter=6,
                                            anchor_density=float(rng.uniform(0.1, 0.7)),
                                            with_context=bool(i % 3), trim=min(3, R // 3)))
    n = n_del = 0
    for bw in (12, 40):
        for w in (False, True):
            a, b = _check_against_oracle(dtw, oracle_port, mg, mo, model, cases, bw, mel, w, 1900 + mel)
            n, n_del = n + a, n_del + b
    assert n > 100 and n_del >= 20


@pytest.mark.parametrize('k,central,alphabet', [(4, 0, 4), (4, 3, 4), (4, 1, 3), (6, 2, 4), (6, 2, 5), (8, 3, 5),
                                                (10, 4, 4)])
def test_edit_kmer_sizes_and_alphabets(dtw, oracle_port, k, central, alphabet):
    """k = 4 and 6 (windows of up to 6 rows in groups of 8 lanes, the others in groups of 16; central = k - 1 has
    back = 0: the extra row p - 1) with 3 to 5 letters, and k = 8 and 10 (every window in a group of 16)."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(531 + k + alphabet, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases = []
    for i in range(6):
        rng = np.random.default_rng([389, k, central, alphabet, i])
        R = int(rng.integers(4, 70)) if i else 15
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(10, 40)), dwell=(2, 9),
                                            jitter=5, anchor_density=float(rng.uniform(0.2, 0.7)),
                                            with_context=bool(i % 2), trim=min(3, R // 3)))
    n = n_del = 0
    for w in (False, True):
        a, b = _check_against_oracle(dtw, oracle_port, mg, mo, model, cases, 30, 2, w, 2000 + k)
        n, n_del = n + a, n_del + b
    assert n > 100 and n_del >= 20


def test_edit_golden_nopath(dtw, golden_nopath):
    """Reads whose band holds no path: status NO_PATH and -inf, as the listed operator gives."""
    from nadavca_amd import _lib
    g = golden_nopath
    mg = dtw.KmerModel(*g.model)
    k, central, alphabet = g.model[:3]
    seen = 0
    for case in g.cases:
        sig, ref, cb, ca, anc, bw, mel = dp_args(case)
        R = len(ref)
        es = [(p, p % 2, [(ref[p] + 1) % alphabet] * (1 - p % 2)) for p in range(1, R - 1, 3)] + [(1, 0, [])]
        for w in (0, 1):
            total, got, status = dtw.estimate_edit_hypotheses_batch([(sig, ref, cb, ca, anc)], [es], bw, mel, mg,
                                                                    bool(w), return_status=True)
            exp = np.asarray(case['ell_w%d' % w])
            _close(total, exp[0:1, ref[0]])
            if np.isneginf(exp).all():
                assert status[0] == _lib.READ_NO_PATH
                assert np.isneginf(got[0]).all() and got[0].shape == (len(es),)
                seen += 1
    assert seen > 0


@pytest.mark.parametrize('k,central,alphabet,mel', [(6, 2, 5, 2), (4, 3, 3, 1), (8, 3, 4, 2), (5, 2, 4, 0),
                                                    (5, 2, 4, 4), (6, 2, 4, 3)])
def test_engine_invariants(dtw, k, central, alphabet, mel):
    """(d, i) = (0, 0) is bit-equal to ``total``; ``total`` is bit-equal to the listed operator's; edits that delete
    anchored bases run with status OK and without NaN; a batch run twice gives the same bits."""
    from nadavca_amd import synthetic, _lib
    model = synthetic.synth_model_arrays(631 + k, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    batch = synthetic.make_batch(16, model, seed=37 + k, R=70, R_spread=40, bandwidth=40, dwell=(max(mel, 1), 9),
                                 jitter=6)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for w in (False, True):
        noops, anchored = [], []
        for j, c in enumerate(batch.cases):
            rng = np.random.default_rng([6, k, j])
            R = len(c['reference'])
            noops.append([(int(p), 0, []) for p in rng.integers(1, R, 9)] + [(1, 0, []), (R - 1, 0, [])])
            on = [int(a) for a in np.asarray(c['approximate_alignment'])[:, 1] if 1 <= a <= R - 2]
            es = []
            for a in on[:12]:
                for p, d in ((a, 1), (a - 1, 2), (a, 2)):
                    i = int(rng.integers(0, 3))
                    if _valid(R, k, central, p, d, i):
                        es.append((p, d, rng.integers(0, alphabet, i).tolist()))
            anchored.append(es)
        assert sum(len(es) for es in anchored) > 100
        total, _ = dtw.estimate_hypotheses_batch(_reads(batch.cases), [np.zeros((0, 2), int)] * batch.n, 40, mel, mg, w)
        total1, got1 = dtw.estimate_edit_hypotheses_batch(_reads(batch.cases), noops, 40, mel, mg, w)
        total2, got2, st2 = dtw.estimate_edit_hypotheses_batch(_reads(batch.cases), anchored, 40, mel, mg, w,
                                                               return_status=True)
        total3, got3 = dtw.estimate_edit_hypotheses_batch(_reads(batch.cases), anchored, 40, mel, mg, w)
        assert not np.isnan(total).any() and (st2 == _lib.READ_OK).all()
        for t in (total1, total2, total3):
            assert np.array_equal(bits(t), bits(total))
        for j in range(batch.n):
            assert np.array_equal(bits(got1[j]), bits(np.full(len(noops[j]), total[j]))), (j, w)
            assert not np.isnan(got2[j]).any() and got2[j].shape == (len(anchored[j]),)
            assert np.array_equal(bits(got2[j]), bits(got3[j])), (j, w)


def test_refusals(dtw):
    """No base in front of the edit or behind it, a letter out of range, a window of 15 rows, d negative or beyond the
    item code, more letters than a window holds: each fails ITS read with READ_BAD_INPUT, its outputs stay untouched
    and the neighbours equal a run without it.  Broken offsets are refused as a whole (NVK_ERR_INVALID -> ValueError).
    Empty batches and lists pass."""
    import torch
    from nadavca_amd import synthetic, _lib
    from nadavca_amd.device import DeviceBatch, estimate_edit_hypotheses_dev
    k, central, alphabet = 6, 2, 5
    model = synthetic.synth_model_arrays(77, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    batch = synthetic.make_batch(5, model, seed=4, R=60, R_spread=20, bandwidth=30, dwell=(2, 9), jitter=5)
    cases = batch.cases
    Rs = [len(c['reference']) for c in cases]
    good = [[(p, p % 3, [p % alphabet] * (p % 2 + (p % 3 == 0))) for p in range(1, Rs[j] - 3, 4)] + [(7, 0, [])]
            for j in range(5)]
    total0, got0, st0 = dtw.estimate_edit_hypotheses_batch(_reads(cases), good, 30, 2, mg, True, return_status=True)
    assert (st0 == _lib.READ_OK).all() and all(np.isfinite(v).all() for v in got0)
    R1 = Rs[1]
    bad_edits = {
        'p = 0': (0, 0, [1]),
        'p = 0, nothing': (0, 0, []),
        'p = -1': (-1, 1, []),
        'p + d = R': (R1 - 2, 2, []),
        'p = R': (R1, 0, [1]),
        'letter 5': (9, 0, [1, 5]),
        'letter -1': (9, 1, [-1]),
        '15 rows': (20, 0, [1] * 10),
        '15 rows with a deletion': (20, 3, [2] * 10),
        '15 rows at row 0': (1, 0, [1] * 12),
        'negative d': (20, -1, [1]),
        'd beyond the item code': (2, 256, []),
        '14 letters': (20, 0, [1] * 14),
    }
    assert _rows(R1, k, central, 20, 0, 10) == 15 and _rows(R1, k, central, 1, 0, 12) == 15
    for name, e in bad_edits.items():
        lists = list(good)
        lists[1] = good[1][:3] + [e] + good[1][3:]
        total, got, st = dtw.estimate_edit_hypotheses_batch(_reads(cases), lists, 30, 2, mg, True, on_error='status',
                                                            return_status=True)
        assert st.tolist() == [0, _lib.READ_BAD_INPUT, 0, 0, 0], name
        assert np.isnan(total[1]) and np.isnan(got[1]).all(), name          # left untouched
        for j in (0, 2, 3, 4):
            assert np.array_equal(got[j], got0[j]) and total[j] == total0[j], name
        with pytest.raises(ValueError, match='invalid input for read'):
            dtw.estimate_edit_hypotheses_batch(_reads(cases), lists, 30, 2, mg, True)
    # allowed: 14 rows exactly, in the interior and against either end; deletions of 8 and more
    fine = [(20, 0, [1] * 9), (20, 2, [3] * 9), (1, 0, [1] * 11), (R1 - 1, 0, [0] * 10), (5, 8, []), (5, 8, [1, 2]),
            (1, R1 - 2, []), (1, 0, []), (R1 - 1, 0, [])]
    assert all(_valid(R1, k, central, p, d, len(s)) for p, d, s in fine)
    assert _rows(R1, k, central, 20, 0, 9) == 14 and _rows(R1, k, central, 1, 0, 11) == 14
    _, got, st = dtw.estimate_edit_hypotheses_batch(_reads(cases), [good[0], fine, [], [], []], 30, 2, mg, True,
                                                    return_status=True)
    assert (st == 0).all() and not np.isnan(got[1]).any()
    # a run without the bad read gives the neighbours the same values
    keep = [0, 2, 3, 4]
    total2, got2 = dtw.estimate_edit_hypotheses_batch(_reads([cases[j] for j in keep]), [good[j] for j in keep], 30,
                                                      2, mg, True)
    for a, j in enumerate(keep):
        assert np.array_equal(got2[a], got0[j]) and total2[a] == total0[j]
    # broken offsets, either level
    dev = torch.device('cuda', mg.context.device)
    db = DeviceBatch(batch, dev)
    T = lambda x: torch.tensor(x, dtype=torch.int64)
    pos = torch.full((5,), 3, dtype=torch.int32)
    dele = torch.zeros(5, dtype=torch.int32)
    base = torch.zeros(10, dtype=torch.int32)
    ok_hyp, ok_ins = [0, 1, 2, 3, 4, 5], [0, 2, 4, 6, 8, 10]
    estimate_edit_hypotheses_dev(db, 30, 2, mg, True, T(ok_hyp), pos, dele, T(ok_ins), base)
    for off in ([1, 2, 3, 4, 5, 5], [0, 3, 2, 4, 5, 5], [0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6]):
        with pytest.raises(ValueError, match='hypothesis offsets'):
            estimate_edit_hypotheses_dev(db, 30, 2, mg, True, T(off), pos, dele, T(ok_ins), base)
    for off in ([1, 2, 4, 6, 8, 10], [0, 4, 2, 6, 8, 10], [0, 2, 4, 6, 8, 9], [0, 2, 4, 6, 8, 12]):
        with pytest.raises(ValueError, match='insertion offsets'):
            estimate_edit_hypotheses_dev(db, 30, 2, mg, True, T(ok_hyp), pos, dele, T(off), base)
    # an empty batch, a batch without any edit, edits that change nothing
    assert dtw.estimate_edit_hypotheses_batch([], [], 30, 2, mg, True)[1] == []
    total3, got3 = dtw.estimate_edit_hypotheses_batch(_reads(cases), [[]] * 5, 30, 2, mg, True)
    assert np.array_equal(total3, total0) and all(v.size == 0 for v in got3)
    total4, got4 = dtw.estimate_edit_hypotheses_batch(_reads(cases), [[(2, 0, [])] * 3] * 5, 30, 2, mg, True)
    assert np.array_equal(total4, total0) and all(np.array_equal(v, np.full(3, t)) for v, t in zip(got4, total0))
