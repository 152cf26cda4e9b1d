"""GPU tests of ``estimate_allele_fractions_batch``: a 1 500-base genome and a second haplotype with 7 substitutions
(two of them 3 bases apart), 300 reads of about 200 bases drawn from either with probability 0.5 on both strands
(``synthetic.make_mixed_read_batch``), ``SeedAligner`` on the first haplotype, bandwidth 40, the packaged table.

Measured on the MI355X for this batch (event_length 1): coverage 37 .. 50 at the planted sites, largest
|fraction - realised| 0.023, smallest planted lrt 873.5, largest lrt more than k - 1 = 5 positions from every planted site
47.7 (4 278 such rows); 6 of the 7 planted bases have a NEGATIVE consensus sum at the consensus scale.  The CPU oracle
(tests/allele_ref.py: oracle_front, no spline tweak, the true pairs as the alignment) gave 0.024 / 880.6 / 46.4 for the
same batch before the test was run on the device; seeds 1, 2 and 4 gave 0.039 / 691 / 71, 0.021 / 1 122 / 86 and
0.049 / 591 / 69 there."""
import copy

import numpy as np
import pytest

import allele_ref

pytestmark = pytest.mark.gpu

PLANTED = [200, 400, 403, 650, 900, 1150, 1350]
SEED = 3


@pytest.fixture(scope='module')
def km():
    from nadavca_amd.kmer_model import KmerModel
    from nadavca_amd import defaults
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def config():
    from nadavca_amd import defaults
    from nadavca_amd.batchflow import load_config
    return dict(load_config(defaults.CONFIG_FILE), bandwidth=40)


class Mixture:
    """The batch, its front end run ONCE (stage, rows and status kept on the device and fetched to the host), and the
    numpy restatement's answer for those rows at event_length 1."""

    def __init__(self, km, config):
        from nadavca_amd import synthetic
        from nadavca_amd.batchflow import device_stage, likelihood_rows
        from nadavca_amd.seedalign import SeedAligner
        self.ref, self.hap, self.alts = allele_ref.planted_haplotypes(1500, PLANTED, SEED)
        self.rb, self.truth, self.info = synthetic.make_mixed_read_batch(300, [self.ref, self.hap], [0.5, 0.5],
                                                                         seed=SEED, length=200, spread=20)
        self.aligner = SeedAligner(self.ref)
        self.stage = device_stage(copy.deepcopy(self.rb), self.ref, config, km, self.aligner, 'pooled')
        self.ll, self.status, _ = likelihood_rows(self.stage, config, km)
        self.sa = self.stage.sa.host()
        self.ll_host, self.status_host = self.ll.cpu().numpy(), self.status.cpu().numpy()

    def restated(self, event_length):
        sa = self.sa
        key, val = allele_ref.rows(self.ll_host, sa.reference, sa.ref_off, sa.ref_start, sa.reverse, self.status_host,
                                   event_length, self.ref.size)
        P, b, D, valid, coverage = allele_ref.sites(key, val, self.ref)
        return P, b, D, valid, coverage, allele_ref.solve(D, valid)

    def rows(self, km, **kw):
        from nadavca_amd.allele_fractions import allele_fractions_of_rows
        return allele_fractions_of_rows(self.stage, self.ll, self.status, self.ref, None, km, **kw)


@pytest.fixture(scope='module')
def mix(km, config):
    return Mixture(km, config)


def test_every_row_against_the_restatement(mix, km):
    assert mix.sa.live.size >= 290 and (mix.status_host == 0).sum() >= 280
    assert mix.sa.reverse.any() and not mix.sa.reverse.all()
    P, b, D, valid, coverage, ref = mix.restated(1.0)
    got = mix.rows(km, keep='all')
    assert np.array_equal(got.position, P) and np.array_equal(got.alt_base, b) and len(got) > 4000
    assert np.array_equal(got.position_coverage, coverage) and np.array_equal(got.coverage, coverage[P])
    assert np.array_equal(got.ref_base, mix.ref[P]) and (got.contig == 0).all() and got.contig_names is None
    counts = allele_ref.check_against(ref, got.fraction, got.lrt, got.ll_half, got.ll_full, D, valid)
    print('%d rows; fraction surely 0 / 1 / inside: %d / %d / %d; sharp optima: %d' % ((len(got),) + counts))
    # the derived columns, from the rows themselves
    best = np.stack([np.zeros(len(got)), got.ll_half, got.ll_full])
    assert np.array_equal(got.genotype, np.argmax(best, axis=0))
    top = np.zeros(mix.ref.size)                  # (the reference base's column holds lrt 0 at every position)
    np.maximum.at(top, got.position, got.lrt)
    k = km.get_k()
    near = np.array([max([top[q] for q in range(max(0, p - k + 1), min(top.size, p + k)) if q != p]) for p in P])
    assert np.array_equal(got.shadowed, near > got.lrt)
    assert not got.called.any() and got.threshold is None
    # keep='positive' is the subset with fraction > 0; a threshold calls rows
    pos = mix.rows(km, keep='positive', threshold=100.0, min_fraction=0.2, min_coverage=8)
    sel = got.fraction > 0
    assert 0 < len(pos) == int(sel.sum()) < len(got)
    for f in ('position', 'alt_base', 'coverage', 'fraction', 'lrt', 'll_half', 'll_full', 'genotype', 'shadowed'):
        assert np.array_equal(getattr(pos, f), getattr(got, f)[sel]), f
    assert np.array_equal(pos.called, (pos.lrt >= 100.0) & (pos.fraction >= 0.2) & (pos.coverage >= 8))
    assert 7 <= pos.called.sum() < 100
    # a second call returns the same bits
    again = mix.rows(km, keep='all')
    for f in got.FIELDS:
        assert np.array_equal(getattr(again, f), getattr(got, f)), f


def test_full_sum_is_the_consensus_sum(mix, km, config):
    """At the configuration's normalization_event_length ll_full is what consensus_accumulate_dev adds up (a division
    here, a multiplication by the reciprocal and atomic adds in any order there: 1e-9 relative)."""
    import torch
    from nadavca_amd.device import consensus_accumulate_dev
    nel = config['normalization_event_length']
    got = mix.rows(km, event_length=nel, keep='all')
    sa = mix.stage.sa
    acc, cov = consensus_accumulate_dev(km.context, mix.stage.dbatch, mix.ll, sa.ref_start.contiguous(),
                                        sa.reverse.to(torch.int32), mix.status, nel, mix.ref.size)
    acc, cov = acc.cpu().numpy(), cov.cpu().numpy()
    assert np.array_equal(got.position_coverage, cov)
    want = acc[got.position, got.alt_base]
    with np.errstate(invalid='ignore'):
        same = (got.ll_full == want) | (np.abs(got.ll_full - want) <= 1e-9 * np.abs(want))
    assert same.all(), (got.ll_full[~same][:4], want[~same][:4])
    negative = sum(got.ll_full[(got.position == x) & (got.alt_base == a)][0] < 0 for x, a in zip(PLANTED, mix.alts))
    print('planted bases with a negative consensus sum at event_length %g: %d of %d' % (nel, negative, len(PLANTED)))


def test_planted_sites(mix, km):
    got = mix.rows(km, keep='all')
    hap = mix.info['haplotype'][mix.sa.live]
    shares = [allele_ref.realised_share(x, mix.sa, mix.status_host, hap) for x in PLANTED]
    print('coverage at the planted sites: %s' % [n for _, n in shares])
    assert min(n for _, n in shares) >= 8
    assert [int(got.position_coverage[x]) for x in PLANTED] == [n for _, n in shares]
    allele_ref.planted_check(got.position, got.alt_base.astype(np.int64), got.fraction, got.lrt, PLANTED, mix.alts,
                             [s for s, _ in shares], km.get_k())


def test_the_workflow_itself(mix, km, config):
    """The public entry runs the same front end and the same back half: its rows are those of ``mix``."""
    from nadavca_amd import estimate_allele_fractions_batch
    want = mix.rows(km, keep='all', threshold=50.0)
    got = estimate_allele_fractions_batch(mix.ref, copy.deepcopy(mix.rb), config=config, kmer_model=km,
                                          aligner=mix.aligner, threshold=50.0, keep='all')
    assert len(got) == len(want) > 0 and np.array_equal(got.position_coverage, want.position_coverage)
    for f in ('position', 'alt_base', 'ref_base', 'coverage', 'genotype', 'shadowed', 'called'):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    for f in ('fraction', 'lrt', 'll_half', 'll_full'):
        assert np.allclose(getattr(got, f), getattr(want, f), rtol=1e-9, atol=1e-9), f
    assert got.called.sum() >= 7


def test_no_read_aligns(km, config):
    from nadavca_amd import estimate_allele_fractions_batch, synthetic
    from nadavca_amd.seedalign import SeedAligner
    other = np.random.default_rng(8).integers(0, 4, 1500).astype(np.int32)
    rb = synthetic.make_mixed_read_batch(4, [other], [1.0], seed=1, length=150, spread=0)[0]
    genome = np.random.default_rng(9).integers(0, 4, 800).astype(np.int32)
    got = estimate_allele_fractions_batch(genome, rb, config=config, kmer_model=km, aligner=SeedAligner(genome))
    assert len(got) == 0 and got.position_coverage.tolist() == [0] * 800


def test_over_a_reference_set(km):
    """Rows over a ReferenceSet are those of the concatenation as one sequence, contig-local and named; a position does
    not shadow one in another contig."""
    from contig_fixture import ContigFixture, NAMES
    from nadavca_amd import estimate_allele_fractions_batch, synthetic
    from nadavca_amd.readbatch import SyntheticBatchAligner
    from nadavca_amd.seedalign import SeedAligner
    fx = ContigFixture(synthetic.load_model_arrays())
    multi = estimate_allele_fractions_batch(fx.refset, copy.deepcopy(fx.rb), kmer_model=km, keep='all',
                                            aligner=SeedAligner(fx.refset))
    single = estimate_allele_fractions_batch(fx.refset.codes, copy.deepcopy(fx.rb), kmer_model=km, keep='all',
                                             aligner=SyntheticBatchAligner(fx.refset.codes, fx.global_alignments()))
    assert len(multi) == len(single) > 100 and multi.contig_names == NAMES and single.contig_names is None
    c, local = fx.refset.locate(single.position)
    assert np.array_equal(multi.contig, c) and np.array_equal(multi.position, local)
    assert set(multi.contig.tolist()) == {0, 1, 2}
    assert np.array_equal(multi.position_coverage, single.position_coverage)
    for f in ('alt_base', 'ref_base', 'coverage', 'genotype'):
        assert np.array_equal(getattr(multi, f), getattr(single, f)), f
    for f in ('fraction', 'lrt', 'll_half', 'll_full'):
        assert np.allclose(getattr(multi, f), getattr(single, f), rtol=1e-9, atol=1e-9), f
    inside = np.abs(single.position[:, None] - fx.refset.offsets[None, 1:4]).min(axis=1) > km.get_k()
    assert np.array_equal(multi.shadowed[inside], single.shadowed[inside])
    with pytest.raises(ValueError, match='concatenation'):
        from nadavca_amd.refset import ReferenceSet
        estimate_allele_fractions_batch(ReferenceSet.from_arrays(NAMES[:2], [fx.contigs[1], fx.contigs[0]]),
                                        copy.deepcopy(fx.rb), kmer_model=km, aligner=SeedAligner(fx.refset))
