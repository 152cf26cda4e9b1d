"""``estimate_mod_model`` on the GPU: about 300 reads of about 200 bases over a 3 000-base genome, drawn from
the packaged table extended with M levels = C levels + N(0, 0.6^2) (``test_gpu_call_mods._model5``), trained from the
table whose M levels are the C levels.

Asserted: ``rounds=3`` equals three chained ``rounds=1`` calls bit for bit, for a wholly modified sample with
``labels='all'`` and a half modified one with ``labels='em'``; the last round recomputed from its own alignment (gamma
from the ratios of a separate ``call_mods_batch``, the updated entries from the statistics and the update rule, every
other entry untouched); the RMS error of the M means over the updated k-mers below the start's; consistent history
counts; the saved table loads back and is accepted by ``call_mods_batch``; the refusals.  No quality figure is asserted
beyond those inequalities: the measured ones are in the README."""
import math

import numpy as np
import pytest

from mod_model_ref import update_rule
from test_gpu_call_mods import _model5

pytestmark = pytest.mark.gpu
N_READS, GENOME, LENGTH, SPREAD, BANDWIDTH = 300, 3000, 200, 20, 40
# every other read is a reverse one, so a strand of the genome is covered 300 * 200 / 3000 / 2 = 10 times and a site
# modified in half of the reads carries a weight of about 5: the default min_weight of 10 would leave most k-mers out
MIN_WEIGHT = 4.0
MODES = {'all': dict(labels='all', modified_fraction=1.0, seed=71),
         'em': dict(labels='em', modified_fraction=0.5, seed=72)}


@pytest.fixture(scope='module')
def config():
    from nadavca_amd import defaults
    from nadavca_amd.batchflow import load_config
    cfg = dict(load_config(defaults.CONFIG_FILE))
    cfg['bandwidth'] = BANDWIDTH
    return cfg


@pytest.fixture(scope='module')
def truth():
    return _model5()


@pytest.fixture(scope='module')
def start(truth):
    from nadavca_amd import dtw, kmer_train, synthetic
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    return dtw.KmerModel(k, central, 5, mean5, sigma5)


@pytest.fixture(scope='module')
def runs(truth, start, config):
    """Per mode: the batch, ``rounds=3`` in one call and as three chained calls.  Computed once."""
    from nadavca_amd import estimate_mod_model, synthetic
    out = {}
    for mode, m in MODES.items():
        rb, aligner, _, _ = synthetic.make_modified_read_batch(N_READS, truth, seed=m['seed'], genome_length=GENOME,
                                                               modified_fraction=m['modified_fraction'], length=LENGTH,
                                                               spread=SPREAD)
        est = estimate_mod_model(rb, aligner, start, labels=m['labels'], rounds=3, min_weight=MIN_WEIGHT,
                                 config=config)
        chain, model, fraction = [], start, 0.5
        for _ in range(3):
            chain.append(estimate_mod_model(rb, aligner, model, labels=m['labels'], rounds=1, fraction=fraction,
                                            min_weight=MIN_WEIGHT, config=config))
            model, fraction = chain[-1].model, chain[-1].fraction
        out[mode] = dict(rb=rb, aligner=aligner, est=est, chain=chain)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize('mode', ['all', 'em'])
def test_rounds_equal_chained_single_rounds(runs, mode):
    est, chain = runs[mode]['est'], runs[mode]['chain']
    last = chain[-1]
    for name in ('mean', 'sigma', 'weight', 'samples', 'gamma'):
        assert np.array_equal(_bits(getattr(est, name)), _bits(getattr(last, name))), name
    assert np.array_equal(est.updated, last.updated) and est.fraction == last.fraction
    assert len(est.history) == 3 and est.history == [c.history[0] for c in chain]
    assert (est.k, est.central, est.alphabet) == (6, 2, 5) and est.model.alphabet_size == 5
    for h in est.history:
        assert h['reads'] == N_READS and 0 < h['status_ok'] <= h['aligned'] <= h['reads']
        assert h['rows'] > 0 and h['sites'] > 0 and h['kmers_updated'] > 0 and h['windows_skipped'] == 0
        assert 1e-3 <= h['fraction'] <= 1.0 - 1e-3 and h['rms_mean_change'] >= 0.0
    if mode == 'all':
        assert est.fraction == 0.5 and (est.gamma == 1.0).all()
    print(mode, 'fraction per round', [h['fraction'] for h in est.history], 'updated',
          [h['kmers_updated'] for h in est.history])


@pytest.mark.parametrize('mode', ['all', 'em'])
def test_last_round_from_its_own_alignment(runs, start, config, mode):
    import torch
    from nadavca_amd import call_mods_batch, defaults
    from nadavca_amd.batchflow import align_batch
    from nadavca_amd.call_mods import score_sites
    from nadavca_amd.device import mod_kmer_stats_dev
    from nadavca_amd.mod_train import holds_code
    r = runs[mode]
    rb, aligner, est, before = r['rb'], r['aligner'], r['est'], r['chain'][1]
    res = align_batch(rb, config, before.model, defaults.RENORM_ROUNDS, aligner)
    sc = score_sites(res, config, before.model, [1, 2], 0, 4, True, 4, before.fraction)
    site_off, pos = sc.site_off, sc.pos
    if mode == 'em':
        mb = call_mods_batch(rb, aligner, before.model, joint=True, max_joint=4, site_prior=before.fraction,
                             config=config)
        llr = torch.from_numpy(mb.llr).to(sc.llr.device)
        assert np.array_equal(_bits(sc.llr.cpu().numpy()), _bits(mb.llr))            # the shared path, row for row
        gamma = torch.sigmoid(llr + math.log(before.fraction / (1.0 - before.fraction)))
        assert np.array_equal(_bits(gamma.cpu().numpy()), _bits(est.gamma))
        # and against numpy's exponential: both are within a few ulp of the sigmoid, whose values lie in [0, 1]
        z = mb.llr + math.log(before.fraction / (1.0 - before.fraction))
        with np.errstate(over='ignore'):
            assert np.abs(est.gamma - 1.0 / (1.0 + np.exp(-z))).max() <= 1e-14
        assert est.fraction == min(max(float(gamma.mean()), 1e-3), 1.0 - 1e-3)
        # the scored sites per read: those of the reads that the scoring left with status 0
        pos = sc.pos[sc.ok].contiguous()
        site_off = torch.zeros_like(sc.site_off)
        torch.cumsum(torch.bincount(sc.owner[sc.ok], minlength=res.stage.n_live), 0, out=site_off[1:])
    else:
        gamma = torch.ones(int(pos.numel()), dtype=torch.float64, device=pos.device)
        assert est.gamma.size == int(pos.numel())
    stats = mod_kmer_stats_dev(before.model.context, res.stage.dbatch, res.events, res.status, 6, 2, 5, 5, site_off,
                               pos, gamma, 4, torch.from_numpy(before.mean).to(pos.device))
    key, sums = stats['key'].cpu().numpy(), stats['sums'].cpu().numpy()
    mean, sigma, updated = update_rule(before.mean, before.sigma, key, sums, 6, 5, 4, MIN_WEIGHT, 0.05)
    assert np.array_equal(est.updated, updated) and updated.sum() == est.history[-1]['kmers_updated']
    assert np.array_equal(_bits(est.mean), _bits(mean)) and np.array_equal(_bits(est.sigma), _bits(sigma))
    assert np.array_equal(_bits(est.mean[~updated]), _bits(before.mean[~updated]))
    assert np.array_equal(_bits(est.weight[key]), _bits(sums[:, 0]))
    assert np.array_equal(_bits(est.samples[key]), _bits(sums[:, 1]))
    assert stats['rows'] == est.history[-1]['rows']
    # whatever no round wrote holds the start's bits: every k-mer without M among them
    ever = r['chain'][0].updated | r['chain'][1].updated | updated
    has_m = holds_code(6, 5, 4)
    assert not (ever & ~has_m).any()
    assert np.array_equal(_bits(est.mean[~ever]), _bits(start.mean[~ever]))
    assert np.array_equal(_bits(est.sigma[~ever]), _bits(start.sigma[~ever]))
    assert (est.sigma[updated] >= 0.05).all()


def _rms(mean, truth, sel):
    return float(np.sqrt(np.mean((mean[sel] - truth[sel]) ** 2)))


@pytest.mark.parametrize('mode', ['all', 'em'])
def test_m_levels_move_towards_the_truth(runs, start, truth, mode):
    est, chain = runs[mode]['est'], runs[mode]['chain']
    true_mean = truth[3]
    sel = est.updated
    assert sel.sum() > 100
    rms_start = _rms(start.mean, true_mean, sel)
    per_round = [_rms(c.mean, true_mean, sel) for c in chain]
    print(mode, 'rms error of the M means over %d updated k-mers: start %.4f, rounds %s, ratios %s'
          % (sel.sum(), rms_start, ['%.4f' % v for v in per_round], ['%.3f' % (v / rms_start) for v in per_round]))
    assert per_round[-1] < rms_start
    if mode == 'all':
        assert per_round[0] < rms_start


def test_saved_table_loads_and_calls(runs, config, tmp_path):
    from nadavca_amd import call_mods_batch
    from nadavca_amd.kmer_model import KmerModel
    r = runs['em']
    p = tmp_path / 'trained5.npz'
    r['est'].save(p)
    loaded = KmerModel.load_from_hdf5(str(p))
    assert np.array_equal(loaded.mean, r['est'].mean) and np.array_equal(loaded.sigma, r['est'].sigma)
    assert (loaded.k, loaded.central_position, loaded.alphabet_size) == (6, 2, 5)
    mb = call_mods_batch(r['rb'], r['aligner'], loaded, joint=True, config=config)
    assert len(mb) > 0 and not np.isnan(mb.llr).any()


def test_refusals(runs, start, config):
    from nadavca_amd import dtw, estimate_mod_model, synthetic
    rb, aligner = runs['all']['rb'], runs['all']['aligner']
    km4 = dtw.KmerModel(*synthetic.load_model_arrays())
    with pytest.raises(ValueError, match='no modified base'):
        estimate_mod_model(rb, aligner, km4, config=config)
    with pytest.raises(ValueError, match='no modified base'):
        estimate_mod_model(rb, aligner, start, mod_code=5, config=config)
    for kw in (dict(labels='x'), dict(rounds=0), dict(min_weight=0.0), dict(min_weight=-2.0), dict(fraction=0.0),
               dict(fraction=1.0), dict(fraction=1.5), dict(mod_offset=2), dict(max_joint=9), dict(min_sigma=0.0)):
        with pytest.raises(ValueError):
            estimate_mod_model(rb, aligner, start, config=config, **kw)


def test_nothing_to_train_on_leaves_the_table_alone(runs, start, config):
    """A pattern without an occurrence, and a batch in which no read has an approximate alignment."""
    from nadavca_amd import estimate_mod_model
    from nadavca_amd.readbatch import BaseAlignmentBatch, SyntheticBatchAligner
    rb, aligner = runs['em']['rb'], runs['em']['aligner']
    none = SyntheticBatchAligner(aligner.reference_num, BaseAlignmentBatch(
        np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(rb.n + 1, np.int64), np.zeros(rb.n, bool)))
    for labels in ('all', 'em'):
        for kw, aligned in ((dict(pattern='A' * 14), True), (dict(aligner=none), False)):
            est = estimate_mod_model(rb, kw.pop('aligner', aligner), start, labels=labels, rounds=2, config=config,
                                     **kw)
            assert np.array_equal(_bits(est.mean), _bits(start.mean))
            assert np.array_equal(_bits(est.sigma), _bits(start.sigma))
            assert not est.updated.any() and not est.weight.any() and est.gamma.size == 0 and est.fraction == 0.5
            for h in est.history:
                assert h['sites'] == h['rows'] == h['kmers_updated'] == 0 and (h['aligned'] > 0) == aligned
