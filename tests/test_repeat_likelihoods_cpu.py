"""The per-count likelihoods of the repeat counter without a GPU: the CPU restatement of nvk_repeat_likelihoods_dev
(tests/host_shims/repeatlik_host.cpp, the scaled linear sweep over the full (E, L, N) trellis) against a plain Python
forward in the log domain; the layering against the same chain without layers; a window too small; a hand-made path;
the workflow ``count_repeats_batch(layers=48)`` in numpy on the simulated batch and what it is worth there;
``genotypes`` on constructed posteriors."""
import math

import numpy as np
import pytest

import repeatlik_ref as K
import repeats_ref as P
import signal_map_ref as R

TOL = 1e-9          # of max(1, |log L|): both sides sum a few thousand terms of relative error 2^-53 each
NEAR = 500.0        # nats below the item's best within which the linear sweep has lost nothing to underflow


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return K.build_host(tmp_path_factory.mktemp('repeatlik_host'))


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def item_args(case, t):
    ch, lo, hi = (int(v) for v in case['items'][t])
    s0, s1 = int(case['st_off'][ch]), int(case['st_off'][ch + 1])
    return (case['level'][lo:hi], case['mu'][s0:s1], case['ac'][s0:s1], case['mc'][s0:s1], case['chain_par'][ch]) \
        + tuple(case['weights'])


def close(got, want):
    return abs(got - want) <= TOL * max(1.0, abs(want))


# ---- the restatement against the log-domain Python ------------------------------------------------------------------
def test_restatement_equals_log_domain_forward(host):
    """log L(c) of every layer within 500 nats of the item's best agrees within 1e-9 * max(1, |value|); further down
    the linear sweep may have lost terms to underflow and must only not exceed the Python value.  Largest difference
    seen, relative to max(1, |value|): 7.4e-16, over the 99 near layers of the 160."""
    case = K.small_cases()
    L = 8
    z, x, status = K.run_host(host, case, L)
    got = K.loglik(z, x)
    worst, near = 0.0, 0
    for t in range(case['items'].shape[0]):
        want = K.python_loglik(*item_args(case, t), L)
        best = max(want)
        assert status[t] == (K.REP_OK if best > K.NINF else K.REP_NO_PATH), t
        for c in range(L):
            if want[c] == K.NINF:
                assert got[t, c] == K.NINF, (t, c)
            elif want[c] >= best - NEAR:
                assert close(got[t, c], want[c]), (t, c, got[t, c], want[c])
                worst, near = max(worst, abs(got[t, c] - want[c]) / max(1.0, abs(want[c]))), near + 1
            else:
                assert got[t, c] <= want[c] + TOL * max(1.0, abs(want[c])), (t, c, got[t, c], want[c])
    print('largest relative difference over %d near layers: %.3g' % (near, worst))
    assert near >= 80          # of the 160 layers
    # the walks went round the loop: the best layer of most items with 5 trips is near 5
    assert (np.argmax(got[2::3][:6], axis=1) >= 3).sum() >= 4


def test_layers_sum_to_the_unlayered_forward(host):
    """With more layers than events no path is dropped: the sum of L(c) over the layers is the likelihood of the same
    chain with the back edge inside one layer"""
    case = K.small_cases()
    E = case['items'][:, 2] - case['items'][:, 1]
    L = int(E.max()) + 1
    z, x, status = K.run_host(host, case, L)
    got = K.loglik(z, x)
    for t in range(0, case['items'].shape[0], 2):
        want = K.python_loglik(*item_args(case, t), None)
        total = K._lse([float(v) for v in got[t]])
        assert close(total, want), (t, total, want)
        assert (z[t, E[t]:] == 0.0).all()        # a trip takes at least one event


def test_smaller_window_keeps_the_lower_layers(host):
    """Layers only feed upward: with a window too small for the trips the events make, L(c) of the layers it has is the
    large window's, bit for bit as (mantissa, exponent) of z 2^x (``wide_case``: broad Gaussians, so that nothing
    underflows in either run and the two differ by the power of two of the scale alone)"""
    case = K.wide_case()
    z_big, x_big, _ = K.run_host(host, case, 40)
    assert int(np.argmax(K.loglik(z_big, x_big)[0])) >= 3
    for L in (1, 2, 3, 17):
        z, x, status = K.run_host(host, case, L)
        assert status[0] == K.REP_OK
        m, e = K.exact_parts(z, x)
        m_big, e_big = K.exact_parts(z_big[:, :L], x_big)
        assert np.array_equal(bits(m), bits(m_big)) and np.array_equal(e, e_big), L


def test_hand_made_chain(host):
    """Narrow Gaussians and the events of exactly four trips: the posterior of four is above 0.99"""
    case = K.hand_case()
    z, x, status = K.run_host(host, case, K.HAND_LAYERS)
    ll = K.loglik(z, x)[0]
    post = np.exp(ll - ll.max())
    post /= post.sum()
    assert status[0] == K.REP_OK and int(np.argmax(post)) == P.HAND_LOOPS and post[P.HAND_LOOPS] > 0.99
    want = K.python_loglik(*item_args(case, 0), K.HAND_LAYERS)
    assert close(ll[P.HAND_LOOPS], want[P.HAND_LOOPS])


def test_status_and_items_that_are_not_run(host):
    case = K.kernel_case()
    only = np.array([0, 1, 3, 5])              # E = 0, 1, (N - 1) // 2 = 1 and the status_in entry, chain of 3 states
    z, x, status = K.run_host(host, case, 4, only)
    assert status.tolist() == [K.REP_NO_EVENTS, K.REP_NO_PATH, K.REP_NO_PATH, 7]
    assert (z == 0.0).all() and (x[[0, 3]] == 0.0).all()


def test_kernel_case_covers_what_it_claims(host):
    case = K.kernel_case()
    N = np.diff(case['st_off'])
    chain, E = case['items'][:, 0], case['items'][:, 2] - case['items'][:, 1]
    assert set(P.KERNEL_STATES) <= set(N.tolist())
    for n in P.KERNEL_STATES:
        assert {0, 1, 2, (n - 1) // 2, 64, 65} <= set(E[N[chain] == n].tolist()), n
    assert {K.spl(int(n)) for n in N[chain[E == 300]]} == {1, 2, 4}
    par = case['chain_par']
    assert set(P.KERNEL_UNITS) <= set((par[:, 0] - par[:, 1] + 1).tolist())
    for s in (2, 4):            # the loop's ends in one lane, and in two
        here = np.array([K.spl(int(n)) == s for n in N])
        same = par[here, 0] // s == par[here, 1] // s
        assert same.any() and (~same).any(), s
    assert {K.wave_layers(n) for n in P.KERNEL_STATES} == {16, 32}
    for lb in (16, 32):
        assert {1, 2, lb - 1, lb, lb + 1, 2 * lb + 1, K.MAX_LAYERS} <= set(K.KERNEL_LAYERS)
    # the floor item and the sharp one, in the shim: every emission on the floor still leaves a path; X far below -1000
    z, x, status = K.run_host(host, case, 33, np.array([case['floor'], case['sharp']]))
    assert status.tolist() == [K.REP_OK, K.REP_OK] and x[1] < -1000.0 and z[0, 0] > 0.0
    assert (case['status_in'] != 0).sum() == 1
    a, b, c = case['items'][-3:]
    assert a[0] == b[0] == c[0] and (b[1], b[2]) == (a[1] + 3, a[2]) and (c[1], c[2]) == (a[1], a[2] - 5)


# ---- the workflow in numpy on the simulated batch -------------------------------------------------------------------
@pytest.fixture(scope='module')
def simulated(host, model, tmp_path_factory):
    """-> (ReadBatch, loci, truth, specs, reference, the numpy workflow's result with layers, the hosts)"""
    sim = P.simulated_batch(model)
    map_host = R.build_host(tmp_path_factory.mktemp('map_host'))
    rep_host = P.build_host(tmp_path_factory.mktemp('repeats_host'))
    res = K.cpu_count_likelihoods(map_host, rep_host, host, sim[0], sim[1], model, min_flank_score=K.SIM_MIN_FLANK)
    return sim + (res, (map_host, rep_host, host))


def test_workflow_quality(simulated):
    """The most likely count is no better a count than Viterbi's; what the likelihoods add is the order of
    ``count_conf`` and a genotype likelihood (the figures are in the README)."""
    rb, loci, truth, _, _, res, _ = simulated
    assert (res['status'] == K.REP_OK).all() and (res['lik_status'] == K.REP_OK).all()
    K.check_quality(res, truth, loci)


def test_library_fields_equal_the_restatement(simulated, tmp_path):
    """``pair_results`` with layers (numpy, what count_repeats_batch ends with) on the shims' outputs: the per-pair
    loops of the restatement, log L bit for bit; ``write_tsv`` appends the four columns"""
    from nadavca_amd.repeats import pair_results
    import decode_ref as D
    rb, loci, truth, _, _, res, (map_host, _, _) = simulated
    n = rb.n
    from nadavca_amd import synthetic
    ev_start = D.cpu_events(map_host, rb.raw_signal, rb.sig_off, synthetic.load_model_arrays())[2]
    seen = {}

    def likelihoods(pick, status):
        seen['pick'], seen['status'] = pick, status
        return res['lik_z'], res['lik_x'], res['lik_status'], None

    got = pair_results(loci, res['c0'], np.arange(n), np.zeros(n, np.int64), None, res['hit'], res['path_score'],
                       res['case']['items'][:, 1], ev_start, res['case']['trim'], K.SIM_MIN_FLANK, None, K.SIM_LAYERS,
                       likelihoods)
    assert np.array_equal(seen['pick'], 2 * np.arange(n) + res['strand']) and np.array_equal(seen['status'], res['status'])
    assert got.layers == K.SIM_LAYERS
    for name in got.FIELDS + got.LIK_FIELDS:
        a, b = getattr(got, name), res[name]
        if name in ('count_post', 'count_mean', 'count_conf'):      # within 4 units of the last place
            assert np.array_equal(np.isnan(a), np.isnan(b)), name
            fin = ~np.isnan(a)
            assert np.abs(bits(a[fin]) - bits(b[fin])).max() <= 4, name
            continue
        same = np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
        assert same, name
    path = tmp_path / 'counts.tsv'
    assert got.write_tsv(str(path)) == n
    lines = path.read_text().splitlines()
    assert lines[0].split('\t')[-4:] == ['count_map', 'count_mean', 'count_conf', 'clipped']
    first = lines[1].split('\t')
    assert int(first[-4]) == got.count_map[0] and first[-1] == '0' and len(first) == len(lines[0].split('\t'))


def test_pairs_that_are_not_counted(simulated):
    """A pair that is not REP_OK has NaN rows, -1 and False; a window of one layer clips every read"""
    from nadavca_amd.repeats import likelihood_fields
    res = simulated[5]
    status = res['status'].copy()
    status[3] = K.REP_NO_EVENTS
    f = likelihood_fields(np.full(status.size, 3), status, res['lik_z'], res['lik_x'], res['lik_status'])
    assert np.isnan(f['count_loglik'][3]).all() and np.isnan(f['count_post'][3]).all() and f['count_map'][3] == -1
    assert np.isnan(f['count_mean'][3]) and np.isnan(f['count_conf'][3]) and not f['clipped'][3]
    assert np.array_equal(bits(f['count_loglik'][4]), bits(res['count_loglik'][4]))
    one = likelihood_fields(np.full(status.size, 3), res['status'], res['lik_z'][:, :1], res['lik_x'], res['lik_status'])
    assert one['clipped'].all() and (one['count_map'] == 3).all() and (one['count_conf'] == 1.0).all()
    # a layer whose sum is 0 has -inf and the posterior 0
    z = res['lik_z'].copy()
    z[:, 40:] = 0.0
    f = likelihood_fields(np.full(status.size, 3), res['status'], z, res['lik_x'], res['lik_status'])
    assert np.isneginf(f['count_loglik'][:, 40:]).all() and (f['count_post'][:, 40:] == 0.0).all()


def test_without_layers_nothing_is_added(simulated, model):
    """``layers=0``: the new fields are None and ``genotypes`` refuses; a bad ``layers`` is refused before any device
    call, and an empty batch with layers has empty fields"""
    from nadavca_amd import count_repeats_batch
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.repeats import pair_results
    rb, loci, _, _, _, res, _ = simulated
    n = rb.n
    got = pair_results(loci, res['c0'], np.arange(n), np.zeros(n, np.int64), None, res['hit'], res['path_score'],
                       res['case']['items'][:, 1], np.zeros(int(res['case']['level'].size), np.int64),
                       res['case']['trim'], None)
    assert got.layers == 0 and all(getattr(got, f) is None for f in got.LIK_FIELDS)
    with pytest.raises(ValueError, match='layers'):
        got.genotypes()
    km = P.TableModel(model)
    for bad in (-1, K.MAX_LAYERS + 1):
        with pytest.raises(ValueError, match='layers'):
            count_repeats_batch(rb, loci, kmer_model=km, layers=bad)
    none = np.zeros(0, np.int32)
    silent = ReadBatch.from_signals(np.zeros(0, np.int16), np.zeros(4, np.int64), none, np.zeros(4, np.int64))
    res0 = count_repeats_batch(silent, loci, kmer_model=km, layers=5)
    assert res0.layers == 5 and res0.count_post.shape == (3, 5) and np.isnan(res0.count_post).all()
    assert (res0.count_map == -1).all() and not res0.clipped.any() and res0.genotypes() == [None]


# ---- genotypes on constructed posteriors --------------------------------------------------------------------------
def constructed(counts, c0=3, layers=48):
    """A RepeatCountBatch of one locus whose reads' posteriors are points at ``counts``"""
    from nadavca_amd.repeats import RepeatCountBatch, RepeatLocus
    n = len(counts)
    post = np.zeros((n, layers))
    post[np.arange(n), np.array(counts) - c0] = 1.0
    i64, f64 = np.zeros(n, np.int64), np.zeros(n)
    fields = dict(read=np.arange(n), locus=i64, strand=i64, status=i64, count=np.array(counts), loops=i64, n_events=i64,
                  first=i64, last=i64, score=f64, margin=f64, left_score=f64, repeat_score=f64, right_score=f64,
                  repeat_start=i64, repeat_end=i64, spanning=np.ones(n, bool), count_loglik=np.log(np.maximum(post, 1e-300)),
                  count_post=post, count_map=np.array(counts), count_mean=np.array(counts, float), count_conf=np.ones(n),
                  clipped=np.zeros(n, bool))
    locus = RepeatLocus('x', 'ACGTACGTAC', 'CAG', 'ACGTACGTAC')
    return RepeatCountBatch([locus], [c0], None, layers, None, **fields)


def test_genotypes_on_constructed_posteriors():
    g = constructed([10] * 15 + [25] * 15).genotypes()[0]
    assert g['alleles'] == (10, 25) and g['reads'] == 30 and g['het_margin'] > 0 and g['margin'] > 0
    assert g['table'].shape == (48, 48) and g['loglik'] == g['table'][7, 22] and np.isneginf(g['table'][22, 7])
    g = constructed([10] * 30).genotypes()[0]
    assert g['alleles'] == (10, 10) and g['het_margin'] < 0
    # one read at 40 among 30 at 10 is an outlier, not an allele
    g = constructed([10] * 30 + [40]).genotypes()[0]
    assert g['alleles'] == (10, 10)
    # ... and six of them are one
    assert constructed([10] * 30 + [40] * 6).genotypes()[0]['alleles'] == (10, 40)
    # reads that do not span, or are clipped, are left out; none left: None
    b = constructed([10] * 10 + [25] * 10)
    b.spanning[10:] = False
    assert b.genotypes()[0]['alleles'] == (10, 10) and b.genotypes()[0]['reads'] == 10
    b.clipped[:10] = True
    assert b.genotypes() == [None]


def test_genotype_table_is_the_formula():
    """G against the issue's formulas written out in plain loops, on random posteriors over a window of six"""
    from nadavca_amd.repeats import genotype_table
    rng = np.random.default_rng(8)
    post = rng.dirichlet(np.ones(6), 9)
    stutter, decay, outlier = 0.4, 0.3, 0.02
    G = genotype_table(post, stutter, decay, outlier)
    n = 6
    Kmat = [[(1 - stutter) if c == a else stutter / 2 * (1 - decay) * decay ** (abs(c - a) - 1) for a in range(n)]
            for c in range(n)]
    col = [sum(Kmat[c][a] for c in range(n)) for a in range(n)]
    like = [[(1 - outlier) * sum(Kmat[c][a] / col[a] * post[r, c] for c in range(n)) + outlier / n for a in range(n)]
            for r in range(9)]
    for a1 in range(n):
        for a2 in range(n):
            if a2 < a1:
                assert np.isneginf(G[a1, a2])
            else:
                want = sum(math.log(0.5 * like[r][a1] + 0.5 * like[r][a2]) for r in range(9))
                assert abs(G[a1, a2] - want) < 1e-12
    with pytest.raises(ValueError):
        genotype_table(post, stutter=1.0)
