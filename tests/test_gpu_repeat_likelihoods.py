"""``count_repeats_batch(layers=48)`` end to end on the simulated batch of tests/repeats_ref.py: against the workflow
in numpy (tests/repeatlik_ref.py), the quality conditions of tests/test_repeat_likelihoods_cpu.py on the device's
result, the windows ``repeat_items`` makes, and ``layers=0`` against the call without the keyword."""
import numpy as np
import pytest

import repeatlik_ref as K
import repeats_ref as P
import signal_map_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def model(km):
    return (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)


@pytest.fixture(scope='module')
def simulated(model):
    return P.simulated_batch(model)


@pytest.fixture(scope='module')
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp('hosts')
    return R.build_host(d), P.build_host(d), K.build_host(d)


@pytest.fixture(scope='module')
def counted(simulated, km):
    from nadavca_amd import count_repeats_batch
    return count_repeats_batch(simulated[0], simulated[1], kmer_model=km, layers=K.SIM_LAYERS,
                               min_flank_score=K.SIM_MIN_FLANK)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def ulps(a, b):
    """The distance of two arrays of non-negative doubles in units of the last place (NaN beside NaN: 0)"""
    both = np.isnan(a) & np.isnan(b)
    return np.where(both, 0, np.abs(bits(np.where(both, 0.0, a)) - bits(np.where(both, 0.0, b))))


def assert_equals_restatement(got, ref):
    """Every integer and boolean equal, every earlier f64 and ``count_loglik`` bit for bit (where it is finite: the
    rest must be the same -inf or NaN), ``count_post``, ``count_mean`` and ``count_conf`` within 4 ulp"""
    assert got.layers == ref['layers']
    for name in got.FIELDS + got.LIK_FIELDS:
        a, b = getattr(got, name), ref[name]
        assert a.shape == b.shape, name
        if name in ('count_post', 'count_mean', 'count_conf'):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and ulps(a, b).max() <= 4, (name, int(ulps(a, b).max()))
        elif a.dtype == np.float64:
            assert np.array_equal(bits(a), bits(b)), name
        else:
            assert np.array_equal(a, b), name


def test_count_repeats_batch_with_layers_equals_its_stages_in_numpy(simulated, counted, hosts, model):
    rb, loci = simulated[0], simulated[1]
    ref = K.cpu_count_likelihoods(*hosts, rb, loci, model, min_flank_score=K.SIM_MIN_FLANK)
    assert_equals_restatement(counted, ref)
    assert np.isfinite(counted.count_loglik).any() and counted.lik_ms is None and counted.c0.tolist() == [3]


def test_quality(simulated, counted):
    """The conditions of the CPU test (``repeatlik_ref.check_quality``: its figures and margins) on the device's result"""
    K.check_quality(counted, simulated[2], simulated[1])


def test_windows_from_base_alignments(simulated, hosts, model, km):
    """``items=repeat_items(...)``: each pair's own item gets the likelihoods; equal to the numpy workflow on the same
    items"""
    from nadavca_amd import count_repeats_batch, repeat_items
    rb, loci, truth, specs, reference = simulated
    full, aligner = P.aligned_batch(rb, truth, specs, reference)
    items = repeat_items(full, aligner, loci)
    got = count_repeats_batch(full, loci, kmer_model=km, items=items, layers=20)
    assert_equals_restatement(got, K.cpu_count_likelihoods(*hosts, rb, loci, model, layers=20, items=items))
    # 20 layers end at 22 copies: the reads of 25 are clipped, those of 10 are not
    copies = truth['copies'][items.read]
    assert got.clipped[copies == 25].all() and not got.clipped[copies == 10].any()
    g = got.genotypes()[0]
    assert g['reads'] == int((copies == 10).sum()) and g['alleles'][0] in (9, 10, 11)


def test_layers_zero_is_the_call_without_the_keyword(simulated, km):
    from nadavca_amd import count_repeats_batch
    rb, loci = simulated[0], simulated[1]
    plain, zero = count_repeats_batch(rb, loci, kmer_model=km), count_repeats_batch(rb, loci, kmer_model=km, layers=0)
    for name in plain.FIELDS:
        a, b = getattr(plain, name), getattr(zero, name)
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), name
    for res in (plain, zero):
        assert res.layers == 0 and all(getattr(res, f) is None for f in res.LIK_FIELDS)
        with pytest.raises(ValueError):
            res.genotypes()


def test_timer_reports_the_stage_and_the_launch(simulated, km):
    from nadavca_amd import count_repeats_batch
    seen = []
    res = count_repeats_batch(simulated[0], simulated[1], kmer_model=km, layers=4, timer=seen.append)
    assert 'likelihoods' in seen and seen.index('count') < seen.index('likelihoods') < seen.index('results')
    assert res.lik_ms > 0.0 and res.kernel_ms > 0.0
