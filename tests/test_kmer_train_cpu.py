"""Host side of k-mer table training (nadavca_amd/kmer_train.py): the numpy restatement of the statistics contract
(tests/kmer_stats_ref.py) against a plain per-k-mer loop, ``expand_kmer_model``, ``save_kmer_model_npz``, the
argument checks, and the calibration of the recovery thresholds of tests/test_gpu_kmer_train.py.  No GPU."""
import numpy as np
import pytest

from kmer_stats_ref import kmer_stats

from nadavca_amd import defaults
from nadavca_amd.kmer_train import estimate_kmer_model, expand_kmer_model, save_kmer_model_npz


def _random_case(rng, k, alphabet=4, n_reads=6):
    """A flat batch with short or missing contexts, empty, clamped and long events and reads with status != 0."""
    sig, ref, cb, ca, ev, st = [], [], [], [], [], []
    for j in range(n_reads):
        R = int(rng.integers(0, 30))
        N = int(rng.integers(0, 200))
        sig.append(rng.normal(0.0, 1.0, N))
        ref.append(rng.integers(0, alphabet, R))
        cb.append(rng.integers(0, alphabet, int(rng.integers(0, k + 2))))
        ca.append(rng.integers(0, alphabet, int(rng.integers(0, k + 2))))
        s = rng.integers(-5, N + 5, R)
        e = s + rng.integers(-2, 20, R)          # empty (e <= s) and beyond the slice on both sides
        ev.append(np.stack([s, e], 1))
        st.append(int(rng.choice([0, 0, 0, 1, -1])))
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return dict(signal=cat(sig, np.float64), sig_off=off(sig), reference=cat(ref, np.int32), ref_off=off(ref),
                ctx_before=cat(cb, np.int32), cb_off=off(cb), ctx_after=cat(ca, np.int32), ca_off=off(ca),
                events=cat(ev, np.int32).reshape(-1, 2), status=np.array(st, dtype=np.int32))


def _plain_loop(c, k, central, alphabet, trim):
    """Per k-mer, the events that carry it, found by walking every base of every read: -> per-k-mer lists of sample
    arrays (batch order)."""
    per = {}
    for j in range(len(c['ref_off']) - 1):
        if c['status'][j] != 0:
            continue
        r0, R = int(c['ref_off'][j]), int(c['ref_off'][j + 1] - c['ref_off'][j])
        x = c['signal'][c['sig_off'][j]:c['sig_off'][j + 1]]
        cb = list(c['ctx_before'][c['cb_off'][j]:c['cb_off'][j + 1]])
        ca = list(c['ctx_after'][c['ca_off'][j]:c['ca_off'][j + 1]])
        ext = cb + list(c['reference'][r0:r0 + R]) + ca
        for g in range(R):
            if not trim <= g < R - trim:
                continue
            a = min(max(int(c['events'][r0 + g, 0]), 0), len(x))
            b = min(max(int(c['events'][r0 + g, 1]), 0), len(x))
            if b <= a:
                continue
            first = g - central + len(cb)
            if first < 0 or first + k > len(ext):
                continue
            kid = 0
            for base in ext[first:first + k]:
                kid = kid * alphabet + int(base)
            per.setdefault(kid, []).append(x[a:b])
    return per


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 6])
def test_restatement_equals_a_plain_per_kmer_loop(k):
    rng = np.random.default_rng(100 + k)
    for central in range(k):
        for trim in (0, 1, 3, 40):                # 40: more than half of every read
            c = _random_case(rng, k)
            got = kmer_stats(c['signal'], c['sig_off'], c['events'], c['ref_off'], c['reference'], c['ctx_before'],
                             c['cb_off'], c['ctx_after'], c['ca_off'], c['status'], k, central, 4, trim)
            per = _plain_loop(c, k, central, 4, trim)
            n_kmers = 4 ** k
            assert set(np.nonzero(got['e'])[0].tolist()) == set(per)
            for kid in range(n_kmers):
                evs = per.get(kid, [])
                assert got['e'][kid] == len(evs)
                assert got['N'][kid] == sum(len(v) for v in evs)
                if not evs:
                    assert got['S'][kid] == 0.0 and got['Q'][kid] == 0.0
                    continue
                S = np.sum(np.array([np.sum(v) for v in evs]))
                m = S / sum(len(v) for v in evs)
                Q = np.sum(np.array([np.sum((v - m) * (v - m)) for v in evs]))
                assert got['S'][kid].tobytes() == S.tobytes()
                assert got['m'][kid].tobytes() == m.tobytes()
                assert got['Q'][kid].tobytes() == Q.tobytes()
            if trim == 40:
                assert got['e'].sum() == 0


def test_restatement_skips_reads_with_status_and_windows_off_the_contexts():
    # one read, k = 3, central 1: base 0 needs one context base before, base R-1 one after
    c = dict(signal=np.arange(12, dtype=np.float64), sig_off=np.array([0, 12]), reference=np.array([0, 1, 2, 3]),
             ref_off=np.array([0, 4]), ctx_before=np.zeros(0, np.int32), cb_off=np.array([0, 0]),
             ctx_after=np.array([2]), ca_off=np.array([0, 1]),
             events=np.array([[0, 3], [3, 6], [6, 6], [9, 15]]), status=np.array([0]))
    args = [c[n] for n in ('signal', 'sig_off', 'events', 'ref_off', 'reference', 'ctx_before', 'cb_off', 'ctx_after',
                           'ca_off', 'status')]
    got = kmer_stats(*args, 3, 1, 4, 0)
    # base 0: window starts before the (empty) context; base 2: empty event; base 3: (2, 3, 2), samples 9..11
    assert got['key'].tolist() == [-1, 0 * 16 + 1 * 4 + 2, -1, 2 * 16 + 3 * 4 + 2]
    assert got['N'][2 * 16 + 3 * 4 + 2] == 3 and got['S'][6] == 3 + 4 + 5
    args[-1] = np.array([1])
    assert kmer_stats(*args, 3, 1, 4, 0)['e'].sum() == 0


def test_expand_kmer_model_embeds_the_small_table():
    rng = np.random.default_rng(3)
    for (k0, c0, k, c) in ((3, 1, 5, 2), (3, 1, 5, 3), (2, 0, 4, 0), (6, 2, 10, 4), (1, 0, 3, 2)):
        m0, s0 = rng.normal(0, 1, 4 ** k0), rng.uniform(0.1, 0.5, 4 ** k0)
        m, s = expand_kmer_model(k0, c0, 4, m0, s0, k, c)
        assert m.shape == s.shape == (4 ** k,)
        off = c - c0
        for kid in rng.integers(0, 4 ** k, 300):
            digits = [(int(kid) // 4 ** (k - 1 - i)) % 4 for i in range(k)]
            sub = 0
            for d in digits[off:off + k0]:
                sub = sub * 4 + d
            assert m[kid] == m0[sub] and s[kid] == s0[sub]


def test_expand_kmer_model_identity_and_impossible_central():
    z = np.load(defaults.KMER_MODEL_FILE)
    m, s = expand_kmer_model(6, 2, 4, z['mean'], z['sigma'], 6, 2)
    assert np.array_equal(m, z['mean']) and np.array_equal(s, z['sigma'])
    for k, c in ((10, 1), (10, 9), (5, 2), (10, 10), (13, 4)):
        with pytest.raises(ValueError):
            expand_kmer_model(6, 2, 4, z['mean'], z['sigma'], k, c)
    with pytest.raises(ValueError):
        expand_kmer_model(6, 2, 4, z['mean'][:10], z['sigma'], 10, 4)


def test_save_kmer_model_npz_writes_the_packaged_layout(tmp_path):
    z = np.load(defaults.KMER_MODEL_FILE)
    m, s = expand_kmer_model(6, 2, 4, z['mean'], z['sigma'], 7, 3)
    p = tmp_path / 'model7.npz'
    save_kmer_model_npz(p, 7, 3, 4, m, s)
    got = np.load(p)
    assert sorted(got.files) == sorted(z.files) == sorted(['k', 'central_pos', 'alphabet_size', 'mean', 'sigma'])
    for name in ('k', 'central_pos', 'alphabet_size'):
        assert got[name].dtype == z[name].dtype and got[name].shape == z[name].shape == ()
    assert got['mean'].dtype == z['mean'].dtype and got['sigma'].dtype == z['sigma'].dtype
    assert got['mean'].shape == got['sigma'].shape == (4 ** 7,)
    assert int(got['k']) == 7 and int(got['central_pos']) == 3 and int(got['alphabet_size']) == 4
    assert np.array_equal(got['mean'], m) and np.array_equal(got['sigma'], s)
    save_kmer_model_npz(str(tmp_path / 'same.npz'), 6, 2, 4, z['mean'], z['sigma'])
    again = np.load(tmp_path / 'same.npz')
    assert all(np.array_equal(again[n], z[n]) for n in z.files)


def test_save_kmer_model_npz_rejects_other_suffixes_and_sizes(tmp_path):
    m = np.zeros(4 ** 3)
    for name in ('model.h5', 'model', 'model.npz.tmp'):
        with pytest.raises(ValueError):
            save_kmer_model_npz(tmp_path / name, 3, 1, 4, m, m)
    with pytest.raises(ValueError):
        save_kmer_model_npz(tmp_path / 'x.npz', 3, 1, 4, m[:5], m)
    with pytest.raises(ValueError):
        save_kmer_model_npz(tmp_path / 'x.npz', 3, 3, 4, m, m)


@pytest.mark.parametrize('kw', [dict(rounds=0), dict(rounds=1.5), dict(renorm_rounds=-1), dict(min_events=0),
                                dict(min_sigma=0.0), dict(min_sigma=float('nan')), dict(trim=-1)])
def test_estimate_kmer_model_rejects_bad_arguments_before_any_work(kw):
    with pytest.raises(ValueError):
        estimate_kmer_model(None, None, **kw)


# ---- calibration of the recovery test (tests/test_gpu_kmer_train.py) -----------------------------------------------
# Reads of synthetic.make_read_batch from the packaged table; start: means + N(0, 0.25), sigmas x 1.5.  What the
# GPU loop does, with the TRUE events in place of the alignment: per-read median/MAD normalisation, the linear re-fit
# of the event means on the starting table's levels (no contexts) and the rescale, then the statistics.  The
# re-fit's slope is diluted by the start's noise (var / (var + 0.25^2), 1.26 sd of levels), and every round keeps the
# scale it is given, so the recovered means keep a few per cent of scale error: that, not the sampling noise, is
# what the bound has to allow for.
RECOVERY_READS, RECOVERY_SEED, RECOVERY_MIN_EVENTS = 1200, 11, 100


def recovery_start(model):
    k, central, alphabet, mean, sigma = model
    rng = np.random.default_rng(RECOVERY_SEED + 1)
    return mean + rng.normal(0.0, 0.25, mean.size), sigma * 1.5


def _true_event_stats(n_reads):
    import torch
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import signal_alignments
    model = synthetic.load_model_arrays()
    k, central, alphabet, mean, sigma = model
    rb, aligner, genome = synthetic.make_read_batch(n_reads, model, seed=RECOVERY_SEED)
    start_mean, _ = recovery_start(model)
    sa = signal_alignments(rb, aligner.get_base_alignments(rb), 60, aligner.reference_num, k, central).host()
    sig, events, ref_parts = [], [], []
    map_base = np.split(rb.map_base, rb.map_off[1:-1])
    for j, rd in enumerate(sa.live):
        raw = rb.raw_signal[rb.sig_off[rd]:rb.sig_off[rd + 1]].astype(np.float64)
        c = np.median(raw)
        x = np.clip((raw - c) / np.median(np.abs(raw - c)), -5, 5)
        # true dwell boundaries: the spec's starts, regenerated from the same draws as make_read_batch
        spec = synthetic.make_read_spec(np.random.default_rng([RECOVERY_SEED, int(rd)]),
                                        aligner.reference_num, model, int(rd))
        starts = spec['true_starts']
        first_base = int(sa.read_seq_start[j])
        mapped = np.asarray(map_base[rd])
        first_base = int(mapped[mapped >= first_base].min())
        R = int(sa.ref_off[j + 1] - sa.ref_off[j])
        st = starts[first_base:first_base + R + 1] - int(sa.slice_start[j])
        events.append(np.stack([st[:-1], st[1:]], 1))
        lo = int(sa.slice_start[j])
        sig.append(x[lo:lo + int(sa.win_len[j])])
        ref_parts.append(sa.reference[sa.ref_off[j]:sa.ref_off[j + 1]])
    # the linear re-fit against the starting table's levels without contexts (base 0 outside), per read
    from nadavca_amd.synthetic import kmer_ids
    for j in range(len(sig)):
        ids = kmer_ids(ref_parts[j], 0, ref_parts[j].size, k, central)
        ex = start_mean[ids]
        ev = events[j]
        mu = np.array([np.mean(sig[j][a:b]) for a, b in ev])
        slope = np.cov(ex, mu, bias=True)[0, 1] / np.var(ex)
        icpt = mu.mean() - slope * ex.mean()
        sig[j] = (sig[j] - icpt) / slope
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    st = kmer_stats(np.concatenate(sig), off(sig), np.concatenate(events), sa.ref_off, sa.reference,
                    sa.context_before, sa.cb_off, sa.context_after, sa.ca_off, None, k, central, alphabet, 5)
    return model, st


def test_recovery_thresholds_hold_on_the_true_events():
    """The bounds written into test_gpu_kmer_train.py::test_recovery_from_a_perturbed_table, met here by the
    restatement on the true events (measured: RMS ratio 0.21 over 2 323 k-mers, median sigma 0.365)."""
    pytest.importorskip('torch')
    model, st = _true_event_stats(RECOVERY_READS)
    start_mean, _ = recovery_start(model)
    well = st['e'] >= RECOVERY_MIN_EVENTS
    assert well.sum() > 1000
    true_mean = model[3]
    rms_start = np.sqrt(np.mean((start_mean[well] - true_mean[well]) ** 2))
    rms_got = np.sqrt(np.mean((st['m'][well] - true_mean[well]) ** 2))
    assert rms_got <= 0.25 * rms_start
    assert abs(np.median(st['sigma'][well]) - 0.35) <= 0.05
