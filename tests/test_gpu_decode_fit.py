"""``decode_batch(fit=n)`` end to end on the leader-padded reads of the signal_map quality batch: against the workflow in
numpy on the shims (tests/expect_ref.py ``cpu_fit``) on the first 48 reads, ``fit=0`` against the plain call, two rounds
against one round and a call that starts from it, and on all 300 reads what the fit is for: the objective does not fall,
every read still decodes, and the decoded sequences are at least as close to the truth."""
import numpy as np
import pytest

import decode_ref as D
import expect_ref as X
import posterior_ref as P
import signal_map_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ('status', 'n_events', 'n_bases', 'score', 'seq_off', 'sequence', 'map_base', 'map_sig', 'map_off', 'loglik',
          'base_post', 'quality')
FIT_FIELDS = ('scale', 'shift', 'q', 'objective', 'counts', 'floored')
FIRST = 48


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def batch():
    """-> (bare ReadBatch of the padded signals, the true sequences)"""
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import ReadBatch
    rb, _, _, (raw, sig_off, _) = R.quality_batch(synthetic.load_model_arrays())
    return ReadBatch.from_signals(raw, sig_off, np.zeros(0, np.int32), np.zeros(rb.n + 1, np.int64)), \
        D.read_sequences(rb)


@pytest.fixture(scope='module')
def first(batch):
    """The first 48 reads as a batch of their own"""
    from nadavca_amd.readbatch import ReadBatch
    bare = batch[0]
    end = int(bare.sig_off[FIRST])
    return ReadBatch.from_signals(bare.raw_signal[:end], bare.sig_off[:FIRST + 1], np.zeros(0, np.int32),
                                  np.zeros(FIRST + 1, np.int64))


@pytest.fixture(scope='module')
def two_rounds(first, km):
    from nadavca_amd import decode_batch
    return decode_batch(first, kmer_model=km, qualities=True, fit=2)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return a.shape == b.shape and np.array_equal(a, b)


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_two_rounds_equal_the_workflow_in_numpy(first, two_rounds, km, tmp_path):
    """Every integer, ``scale``, ``shift``, ``sigma_scale``, the weights, the counts and ``base_post`` bit for bit;
    ``objective`` and ``loglik`` pass through a library log, on the device torch's or numpy's and in the restatement
    Python's: within 4 ulp."""
    model = (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)
    fit, ref, want = X.cpu_fit(R.build_host(tmp_path), D.build_host(tmp_path), X.build_host(tmp_path), first.raw_signal,
                               first.sig_off, model, 2, post_host=P.build_host(tmp_path))
    got = two_rounds
    assert got.n_decoded == first.n and got.fit.rounds == 2 and got.fit.parts == 1
    for name in ('status', 'n_events', 'n_bases', 'seq_off', 'sequence', 'map_base', 'map_sig', 'map_off'):
        assert same_bits(getattr(got, name), ref[name]), name
    assert same_bits(got.score, ref['score'])
    for name in ('scale', 'shift', 'q', 'counts', 'floored'):
        assert same_bits(getattr(got.fit, name), fit[name]), name
    for name in ('sigma_scale', 'p_stay', 'p_skip'):
        assert getattr(got.fit, name) == fit[name], name
    assert fit['sigma_scale'] != 1.0 and fit['p_stay'] != 0.7 and (fit['scale'] != 1.0).all()
    bad = np.nonzero(got.base_post.view(np.int64) != want['base_post'].view(np.int64))[0]
    assert bad.size == 0, (bad.size, bad[:5].tolist())
    assert np.array_equal(got.quality, want['quality'])
    worst = ulps(got.loglik, want['loglik']).max(), ulps(got.fit.objective, fit['objective']).max()
    print('largest difference: loglik %.2f ulp, objective %.2f ulp' % worst)
    assert got.fit.objective.shape == (3,) and max(worst) <= 4.0


def test_no_rounds_change_nothing(first, km):
    from nadavca_amd import decode_batch
    plain = decode_batch(first, kmer_model=km, qualities=True)
    none = decode_batch(first, kmer_model=km, qualities=True, fit=0, fit_params=('scale',))
    for name in FIELDS:
        assert same_bits(getattr(none, name), getattr(plain, name)), name
    assert none.parts == plain.parts and none.post_parts == plain.post_parts
    assert none.fit is None and plain.fit is None


def test_two_rounds_equal_one_round_and_a_call_that_starts_from_it(first, two_rounds, km):
    from nadavca_amd import decode_batch
    one = decode_batch(first, kmer_model=km, fit=1)
    then = decode_batch(first, kmer_model=km, qualities=True, fit=1, fit_start=one.fit, sigma_scale=one.fit.sigma_scale,
                        p_stay=one.fit.p_stay, p_skip=one.fit.p_skip)
    for name in FIELDS:
        assert same_bits(getattr(then, name), getattr(two_rounds, name)), name
    for name in FIT_FIELDS:
        got, want = getattr(then.fit, name), getattr(two_rounds.fit, name)
        assert same_bits(got, want[1:] if name == 'objective' else want), name
    for name in ('sigma_scale', 'p_stay', 'p_skip'):
        assert getattr(then.fit, name) == getattr(two_rounds.fit, name), name
    assert same_bits(one.fit.objective, two_rounds.fit.objective[:2])
    # the fitted values only applied: the same decode again
    again = decode_batch(first, kmer_model=km, qualities=True, fit_start=then.fit, sigma_scale=then.fit.sigma_scale,
                         p_stay=then.fit.p_stay, p_skip=then.fit.p_skip)
    for name in FIELDS:
        assert same_bits(getattr(again, name), getattr(two_rounds, name)), name
    assert again.fit.rounds == 0 and same_bits(again.fit.objective, two_rounds.fit.objective[2:])
    with pytest.raises(ValueError, match='fit_params'):
        decode_batch(first, kmer_model=km, fit=1, fit_params=('scale', 'drift'))
    with pytest.raises(ValueError, match='rounds'):
        decode_batch(first, kmer_model=km, fit=-1)


def test_three_rounds_on_the_whole_batch_do_not_hurt(batch, km):
    """All 300 reads, ``fit=3`` with the default ``fit_params``: the objective of every round is at least the one
    before (less 1e-9 of its size), every read still decodes, and the mean identity of the decoded sequences to the
    true ones is at least the plain call's.  Measured (on the CPU through the shims first, then here, the same figures):
    objective -224 763.49, -221 841.94, -220 409.06, -219 622.60; mean identity 0.7414 plain, 0.7686 fitted (0.7844 with
    'scale' alone, 0.7824 with scale and sigma, 0.7809 with scale and moves: every group holds, so the default is the
    full set); sigma_scale 1.0759, p_stay 0.7667, p_skip 0.00615."""
    from nadavca_amd import decode_batch
    bare, truths = batch
    plain = decode_batch(bare, kmer_model=km)
    fitted = decode_batch(bare, kmer_model=km, fit=3)
    obj = fitted.fit.objective
    print('objective per round:', ' '.join('%.2f' % v for v in obj))
    assert obj.shape == (4,) and (np.diff(obj) >= -1e-9 * np.abs(obj[:-1])).all()
    assert fitted.n_decoded == plain.n_decoded == bare.n
    mean_identity = lambda dec: float(np.mean([D.identity(t, dec.sequence[dec.seq_off[r]:dec.seq_off[r + 1]])
                                               for r, t in enumerate(truths)]))
    before, after = mean_identity(plain), mean_identity(fitted)
    print('mean identity: plain %.4f, fit=3 %.4f; sigma_scale %.4f, p_stay %.4f, p_skip %.5f'
          % (before, after, fitted.fit.sigma_scale, fitted.fit.p_stay, fitted.fit.p_skip))
    assert after >= before
