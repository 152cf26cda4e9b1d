"""GPU parity of the listed-hypotheses operator (nvk_estimate_hypotheses_batch_dev, dtw.estimate_hypotheses_batch):
every listed (position, base) against the entry of the CPU oracle's full matrix for the same read — tolerance and -inf
rule of tests/test_gpu_ell.py (log-likelihoods to 1e-9 relative + 1e-9 absolute, equal -inf pattern, no NaN) — and the
list of ALL substitutions bit for bit against the full entry's matrix."""
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
    assert np.allclose(got[fin], exp[fin], rtol=RTOL, atol=ATOL), float(np.max(np.abs(got[fin] - exp[fin])))


def _random_list(rng, R, alphabet, ref, j):
    """A hypothesis list for a read of R bases: read j % 4 == 3 gets none; the others random (p, b) rows with
    duplicates, rows with b == ref[p], and the positions 0 and R - 1."""
    if j % 4 == 3:
        return np.zeros((0, 2), dtype=np.int64)
    m = int(rng.integers(1, 3 * R))
    p = rng.integers(0, R, m)
    b = rng.integers(0, alphabet, m)
    rows = np.stack([p, b], 1)
    same = rng.integers(0, R, 3)
    rows = np.concatenate([rows, rows[:max(1, m // 4)], np.stack([same, np.asarray(ref)[same]], 1),
                           [[0, int(rng.integers(0, alphabet))], [R - 1, int(rng.integers(0, alphabet))]]])
    return rows[rng.permutation(len(rows))].astype(np.int64)


def _check_against_oracle(dtw, oracle_port, mg, mo, cases, bw, mel, w, seed):
    alphabet = mg.get_alphabet_size()
    lists = [_random_list(np.random.default_rng([seed, j]), len(c['reference']), alphabet, c['reference'], j)
             for j, c in enumerate(cases)]
    total, got = dtw.estimate_hypotheses_batch(_reads(cases), lists, bw, mel, mg, w)
    for j, (c_, rows, vals) in enumerate(zip(cases, lists, got)):
        exp = np.asarray(oracle_port.estimate_log_likelihoods(c_['signal'], c_['reference'], c_['context_before'],
                                                              c_['context_after'], c_['approximate_alignment'], bw,
                                                              mel, mo, w))
        assert vals.shape == (len(rows),)
        _close(vals, exp[rows[:, 0], rows[:, 1]])
        _close(total[j:j + 1], exp[0:1, c_['reference'][0]])


@pytest.mark.parametrize('mel', [0, 1, 2, 3, 4])
def test_hypotheses_vs_oracle_random(dtw, oracle_port, mel):
    """k = 5 and 4-letter tables, with and without contexts, every compiled min_event_length, wobbling on / off."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(21, k=5, central=2)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases = []
    for i in range(12):
        rng = np.random.default_rng([188, mel, i])
        R = int(rng.integers(3, 90))
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(8, 50)),
                                            dwell=(max(mel, 1), 9), jitter=6,
                                            anchor_density=float(rng.uniform(0.1, 0.9)),
                                            with_context=bool(i % 3), trim=min(3, R // 3)))
    for bw in (12, 40):
        for w in (False, True):
            _check_against_oracle(dtw, oracle_port, mg, mo, cases, bw, mel, w, 700 + mel)


@pytest.mark.parametrize('k,central,alphabet', [(4, 1, 3), (4, 1, 5), (4, 0, 4), (6, 2, 4), (6, 2, 5), (7, 3, 4),
                                                (10, 4, 4), (8, 3, 5)])
def test_hypotheses_kmer_sizes_and_alphabets(dtw, oracle_port, k, central, alphabet):
    """Alphabets 3, 4, 5; k = 4 and 6 (groups of 8 lanes) and k > 6 (groups of 16)."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(131 + k + alphabet, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases = []
    for i in range(6):
        rng = np.random.default_rng([189, k, alphabet, i])
        R = int(rng.integers(4, 70))
        cases.append(synthetic.make_dp_case(rng, model, R=R, bandwidth=int(rng.integers(10, 40)), dwell=(2, 9),
                                            jitter=5, anchor_density=float(rng.uniform(0.2, 0.9)),
                                            with_context=bool(i % 2), trim=min(3, R // 3)))
    for w in (False, True):
        _check_against_oracle(dtw, oracle_port, mg, mo, cases, 30, 2, w, 800 + k)


def test_hypotheses_packaged_table_extended(dtw, oracle_port):
    """The packaged 6-mer table extended to 5 letters, the M level of the premise check (C's level + N(0, 0.6^2)):
    the modified-base hypotheses at the CG sites, config-shaped reads."""
    from nadavca_amd import synthetic, kmer_train
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    ids = np.arange(5 ** k)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (ids // 5 ** m) % 5 == 4
    mean5 = mean5 + np.where(has_m, np.random.default_rng(5).normal(0.0, 0.6, 5 ** k), 0.0)
    model = (k, central, 5, mean5, sigma5)
    mg = dtw.KmerModel(*model)
    mo = oracle_port.KmerModel(*model)
    cases, lists = [], []
    for i in range(6):
        rng = np.random.default_rng([190, i])
        case = synthetic.make_dp_case(rng, model, R=120, bandwidth=60, with_context=bool(i % 2),
                                      bases=lambda r, n, a: r.integers(0, 4, n))
        ref = case['reference']
        at = np.nonzero((ref[:-1] == 1) & (ref[1:] == 2))[0]
        cases.append(case)
        lists.append(np.stack([at, np.full(at.size, 4)], 1))
    assert sum(len(rows) for rows in lists) > 20
    total, got = dtw.estimate_hypotheses_batch(_reads(cases), lists, 60, 2, mg, True)
    for j, (c_, rows, vals) in enumerate(zip(cases, lists, got)):
        exp = np.asarray(oracle_port.estimate_log_likelihoods(c_['signal'], c_['reference'], c_['context_before'],
                                                              c_['context_after'], c_['approximate_alignment'], 60, 2,
                                                              mo, True))
        _close(vals, exp[rows[:, 0], 4])
        _close(total[j:j + 1], exp[0:1, c_['reference'][0]])


def test_hypotheses_golden_nopath(dtw, golden_nopath):
    """Reads whose band holds no path: status NO_PATH, and the values are the reference's (-inf everywhere)."""
    from nadavca_amd import _lib
    g = golden_nopath
    mg = dtw.KmerModel(*g.model)
    alphabet = g.model[2]
    seen = 0
    for case in g.cases:
        sig, ref, cb, ca, anc, bw, mel = dp_args(case)
        R = len(ref)
        rows = np.stack([np.repeat(np.arange(R), alphabet), np.tile(np.arange(alphabet), R)], 1)
        for w in (0, 1):
            total, got, status = dtw.estimate_hypotheses_batch([(sig, ref, cb, ca, anc)], [rows], bw, mel, mg, bool(w),
                                                               return_status=True)
            exp = np.asarray(case['ell_w%d' % w])
            _close(got[0], exp[rows[:, 0], rows[:, 1]])
            _close(total, exp[0:1, ref[0]])
            if np.isneginf(exp).all():
                assert status[0] == _lib.READ_NO_PATH
                seen += 1
    assert seen > 0


def test_hypotheses_appendix_c(dtw):
    """The known answer of tests/test_gpu_ell.py::test_ell_appendix_c, entries picked by list."""
    ids = np.arange(64)
    m = dtw.KmerModel(3, 1, 4, ((ids * 37) % 64) / 16 - 2, 0.4 + (ids % 3) * 0.1)
    ref, cb, ca = [0, 1, 2, 3, 3, 1, 0, 2], [2], [1]
    es = m.get_expected_signal(ref, cb, ca)
    sig = np.round(np.repeat(es, 3) + 0.1 * ((np.arange(24) * 7) % 5 - 2), 4)
    anc = [[0, 0], [9, 3], [21, 7]]
    rows = [[4, 2], [0, 1], [4, 3], [0, 3], [4, 0], [0, 0], [0, 2], [4, 1]]
    total, got = dtw.estimate_hypotheses_batch([(sig, ref, cb, ca, anc)], [rows], 4, 2, m, True)
    assert got[0].tolist() == pytest.approx(
        [-105.98247035339004, -4.629338921878056, 1.0189036593406566, -5.317795793541511, -7.647671624614224,
         1.0189036593406566, -13.895064347992593, -25.626219563738044], rel=1e-10)
    assert total.tolist() == pytest.approx([1.0189036593406566], rel=1e-10)
    total, got = dtw.estimate_hypotheses_batch([(sig, ref, cb, ca, anc)], [[[7, 3], [7, 0], [7, 2], [7, 1]]], 4, 2, m,
                                               False)
    assert got[0].tolist() == pytest.approx(
        [-27.310869151977293, -5.049523388951718, -0.2599469729028855, -27.40554597190469], rel=1e-10)


@pytest.mark.parametrize('k,central,alphabet,mel', [(6, 2, 4, 2), (6, 2, 5, 2), (8, 3, 4, 2), (5, 2, 4, 0),
                                                    (5, 2, 4, 4), (4, 1, 3, 1), (6, 2, 4, 3)])
def test_all_substitutions_bit_equal_to_full_matrix(dtw, k, central, alphabet, mel):
    """The list of all (p, b != ref[p]) of a batch, in the full entry's order and shuffled: ``hyp`` bit-equal to the
    existing full entry's matrix, ``total`` bit-equal to its reference-base column.  (A hypothesis's arithmetic does
    not depend on which others share its wave step: trip rounding only appends cells beyond every band.)"""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(231 + k, k=k, central=central, alphabet=alphabet)
    mg = dtw.KmerModel(*model)
    batch = synthetic.make_batch(24, model, seed=17 + k, R=90, R_spread=60, bandwidth=40, dwell=(max(mel, 1), 9),
                                 jitter=6)
    for w in (False, True):
        full = dtw.estimate_log_likelihoods_batch(_reads(batch.cases), 40, mel, mg, w)
        for shuffle in (False, True):
            lists = []
            for j, c in enumerate(batch.cases):
                ref = np.asarray(c['reference'])
                p = np.repeat(np.arange(ref.size), alphabet)
                b = np.tile(np.arange(alphabet), ref.size)
                rows = np.stack([p, b], 1)[b != ref[p]]
                if shuffle:
                    rows = rows[np.random.default_rng([3, j]).permutation(len(rows))]
                lists.append(rows)
            total, got = dtw.estimate_hypotheses_batch(_reads(batch.cases), lists, 40, mel, mg, w)
            for j, (c, rows, vals) in enumerate(zip(batch.cases, lists, got)):
                exp = full[j][rows[:, 0], rows[:, 1]]
                assert not np.isnan(exp).any()
                assert np.array_equal(vals.view(np.int64), np.ascontiguousarray(exp).view(np.int64)), (j, w, shuffle)
                want = np.float64(full[j][0, c['reference'][0]])
                assert np.float64(total[j]).view(np.int64) == want.view(np.int64)


def test_bad_lists(dtw):
    """A position or base out of range fails ITS read with READ_BAD_INPUT; the neighbours equal a run without the bad
    read.  Broken offsets are refused as a whole (NVK_ERR_INVALID -> ValueError)."""
    import torch
    from nadavca_amd import synthetic, _lib
    from nadavca_amd.device import DeviceBatch, estimate_hypotheses_dev
    model = synthetic.synth_model_arrays(77, k=6, central=2, alphabet=5)
    mg = dtw.KmerModel(*model)
    batch = synthetic.make_batch(5, model, seed=4, R=60, R_spread=20, bandwidth=30, dwell=(2, 9), jitter=5)
    cases = batch.cases
    good = [np.stack([np.arange(len(c['reference'])), (np.asarray(c['reference']) + 1) % 5], 1) for c in cases]
    total0, got0, st0 = dtw.estimate_hypotheses_batch(_reads(cases), good, 30, 2, mg, True, return_status=True)
    assert (st0 == _lib.READ_OK).all()
    R1 = len(cases[1]['reference'])
    for bad_row in ([R1, 0], [-1, 0], [0, 5], [0, -1]):
        lists = list(good)
        lists[1] = np.concatenate([good[1][:7], [bad_row], good[1][7:]])
        total, got, st = dtw.estimate_hypotheses_batch(_reads(cases), lists, 30, 2, mg, True, on_error='status',
                                                       return_status=True)
        assert st.tolist() == [0, _lib.READ_BAD_INPUT, 0, 0, 0], bad_row
        assert np.isnan(total[1]) and np.isnan(got[1]).all()       # outputs of the failed read: left untouched
        for j in (0, 2, 3, 4):
            assert np.array_equal(got[j], got0[j]) and total[j] == total0[j]
        with pytest.raises(ValueError, match='invalid input for read'):
            dtw.estimate_hypotheses_batch(_reads(cases), lists, 30, 2, mg, True)
    # a run without the bad read gives the neighbours the same values
    keep = [0, 2, 3, 4]
    total2, got2 = dtw.estimate_hypotheses_batch(_reads([cases[j] for j in keep]), [good[j] for j in keep], 30, 2, mg,
                                                 True)
    for a, j in enumerate(keep):
        assert np.array_equal(got2[a], got0[j]) and total2[a] == total0[j]
    # broken offsets
    dev = torch.device('cuda', mg.context.device)
    db = DeviceBatch(batch, dev)
    pos = torch.zeros(10, dtype=torch.int32)
    base = torch.zeros(10, dtype=torch.int32)
    for off in ([1, 2, 4, 6, 8, 10], [0, 4, 2, 6, 8, 10], [0, 2, 4, 6, 8, 9], [0, 2, 4, 6, 8, 12]):
        with pytest.raises(ValueError, match='hypothesis offsets'):
            estimate_hypotheses_dev(db, 30, 2, mg, True, torch.tensor(off, dtype=torch.int64), pos, base)
    # an empty batch and a batch without any hypothesis
    assert dtw.estimate_hypotheses_batch([], [], 30, 2, mg, True)[1] == []
    total3, got3 = dtw.estimate_hypotheses_batch(_reads(cases), [np.zeros((0, 2), int)] * 5, 30, 2, mg, True)
    assert np.array_equal(total3, total0) and all(v.size == 0 for v in got3)
