"""``estimate_decode_model`` end to end on the first 48 leader-padded reads of the signal_map quality batch, against the
workflow in numpy on the shims (tests/moments_ref.py ``cpu_train``); ``decode_train.train_loop`` on the device's two
E-steps over the levels of the HMM case, against the CPU run and so with its falling errors; the chain of one-round
calls through ``start=``; and ``decode_batch`` before and after, which nothing here may move."""
import numpy as np
import pytest

import decode_ref as D
import expect_ref as X
import moments_ref as M
import signal_map_ref as R

pytestmark = pytest.mark.gpu

FIRST = 48
DECODE_FIELDS = ('status', 'n_events', 'n_bases', 'score', 'seq_off', 'sequence', 'map_base', 'map_sig', 'map_off',
                 'loglik', 'base_post', 'quality')


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def first():
    """The first 48 padded reads as a bare batch"""
    from nadavca_amd import synthetic
    from nadavca_amd.readbatch import ReadBatch
    _, _, _, (raw, sig_off, _) = R.quality_batch(synthetic.load_model_arrays())
    end = int(sig_off[FIRST])
    return ReadBatch.from_signals(raw[:end], sig_off[:FIRST + 1], np.zeros(0, np.int32), np.zeros(FIRST + 1, np.int64))


@pytest.fixture(scope='module')
def decoded_before(first, km):
    from nadavca_amd import decode_batch
    return decode_batch(first, kmer_model=km, qualities=True, fit=1)


@pytest.fixture(scope='module')
def two_rounds(first, km, decoded_before):
    from nadavca_amd import estimate_decode_model
    return estimate_decode_model(first, kmer_model=km, rounds=2, fit=1)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return a.shape == b.shape and np.array_equal(a, b)


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_two_rounds_equal_the_workflow_in_numpy(first, two_rounds, km, tmp_path):
    """``updated`` and the history's counts equal; ``mean``, ``sigma``, ``weight``, ``scale`` and ``shift`` bit for
    bit; ``objective`` passes through a library log (numpy's here, Python's in the restatement): within 4 ulp."""
    model = (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)
    want, _ = M.cpu_train(R.build_host(tmp_path), X.build_host(tmp_path), M.build_host(tmp_path), first.raw_signal,
                          first.sig_off, model, 2)
    got = two_rounds
    for name in ('mean', 'sigma', 'weight'):
        assert same_bits(getattr(got, name), want[name]), name
    assert np.array_equal(got.updated, want['updated'])
    assert same_bits(got.fit.scale, want['fit']['scale']) and same_bits(got.fit.shift, want['fit']['shift'])
    assert [h['kmers_updated'] for h in got.history] == [h['kmers_updated'] for h in want['history']]
    assert [h['rms_mean_change'] for h in got.history] == [h['rms_mean_change'] for h in want['history']]
    worst = ulps(got.objective, want['objective']).max()
    print('objective per round: %s (largest difference %.2f ulp); states updated %s'
          % (' '.join('%.2f' % v for v in got.objective), worst, [h['kmers_updated'] for h in got.history]))
    assert got.objective.shape == (3,) and worst <= 4.0
    assert (np.diff(got.objective) >= -1e-9 * np.abs(got.objective[:-1])).all()
    assert 0 < got.updated.sum() and same_bits(got.sigma, km.sigma)
    assert same_bits(got.model.mean, got.mean) and got.model.get_k() == 6 and got.k == 6
    assert all(h['parts'] == 1 for h in got.history)


def test_two_rounds_equal_two_chained_calls_of_one(first, two_rounds, km, tmp_path):
    from nadavca_amd import estimate_decode_model
    from nadavca_amd.kmer_model import KmerModel
    one = estimate_decode_model(first, kmer_model=km, rounds=1, fit=1)
    then = estimate_decode_model(first, kmer_model=one.model, rounds=1, fit=1, start=one.fit)
    for name in ('mean', 'sigma', 'weight', 'updated'):
        assert same_bits(getattr(then, name), getattr(two_rounds, name)), name
    assert same_bits(then.fit.scale, two_rounds.fit.scale) and same_bits(then.fit.shift, two_rounds.fit.shift)
    assert same_bits(one.objective[:1], two_rounds.objective[:1]) and same_bits(then.objective, two_rounds.objective[1:])
    assert same_bits(then.fit.anchor, km.mean)
    path = str(tmp_path / 'table.npz')
    then.save(path)
    back = KmerModel.load_from_hdf5(path)
    assert same_bits(back.mean, then.mean) and same_bits(back.sigma, then.sigma) and back.get_k() == 6
    with pytest.raises(ValueError, match='update'):
        estimate_decode_model(first, kmer_model=km, update=('level',))
    with pytest.raises(ValueError, match='rounds'):
        estimate_decode_model(first, kmer_model=km, rounds=0)


def test_train_loop_on_the_device_equals_the_cpu_run(tmp_path):
    """The HMM case of tests/test_state_moments_cpu.py (30 reads of 200 events at k = 3, displaced means), three rounds
    with means and sigmas updated: ``train_loop`` on the device wrappers gives the bits of the run on the shims, and
    so its errors, which fall with every round."""
    import torch
    from nadavca_amd import _lib, decode_train
    ctx = _lib.default_context()
    dev = torch.device('cuda', ctx.device)
    case = X.hmm_case()
    n = case['ev_off'].size - 1
    start, sigma = M.displaced_means(case), np.asarray(case['model'][4], dtype=np.float64)
    args = (np.diff(case['ev_off']), np.ones(n, bool), start, sigma, 3, 1, ('scale',), ('mean', 'sd'), 8.0, 0.05, 1.0,
            0.7, 0.01)
    steps = M.shim_steps(X.build_host(tmp_path), M.build_host(tmp_path), case['level'], case['ev_off'], 3, threads=8)
    want = M.train_rounds(*steps, *args)
    dev_steps = decode_train.device_steps(ctx, torch.from_numpy(case['level']).to(dev),
                                          torch.from_numpy(case['ev_off']).to(dev), None, 3)
    mean, sig, weight, updated, fit, objective, history = decode_train.train_loop(*dev_steps, *args)
    for name, got in (('mean', mean), ('sigma', sig), ('weight', weight)):
        assert same_bits(got, want[name]), name
    assert np.array_equal(updated, want['updated'])
    assert same_bits(fit.scale, want['fit']['scale']) and same_bits(fit.shift, want['fit']['shift'])
    assert ulps(objective, want['objective']).max() <= 4.0
    true = np.asarray(case['model'][3])
    before, after = M.mean_errors(true, start), M.mean_errors(true, mean)
    print('RMS error of the means: %.4f -> %.4f raw, %.4f -> %.4f after the affine map' % (before[0], after[0],
                                                                                          before[1], after[1]))
    assert after[0] < before[0] and after[1] < before[1]


def test_decode_batch_did_not_move(first, km, decoded_before, two_rounds):
    """``decode_batch`` on the same batch, context and table before and after the estimate: identical bits"""
    from nadavca_amd import decode_batch
    after = decode_batch(first, kmer_model=km, qualities=True, fit=1)
    for name in DECODE_FIELDS:
        assert same_bits(getattr(after, name), getattr(decoded_before, name)), name
    for name in ('scale', 'shift', 'objective', 'counts', 'floored'):
        assert same_bits(getattr(after.fit, name), getattr(decoded_before.fit, name)), name
    assert after.parts == decoded_before.parts and after.post_parts == decoded_before.post_parts
    # the estimate's fit starts a decode on the new table
    dec = decode_batch(first, kmer_model=two_rounds.model, fit_start=two_rounds.fit)
    assert dec.n_decoded == first.n and dec.fit.rounds == 0
