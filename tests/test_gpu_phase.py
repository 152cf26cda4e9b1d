"""GPU tests of ``phase_reads_batch``: a 1 500-base genome, haplotype A with 6 substitutions and haplotype B with 5, the
sites alternating between them 100 .. 110 bases apart with one gap of 280 bases that no read spans, 300 reads of about
200 bases drawn from A and B with probability 0.5 each on both strands (``synthetic.make_mixed_read_batch``),
``SeedAligner`` on the reference, bandwidth 40, the packaged table, sites from ``select_sites`` at threshold 200.

SEED was chosen with the numpy restatement (tests/phase_ref.py) on the CPU oracle (tests/allele_ref.py: oracle_front, no
spline tweak, the true pairs as the alignment) before the test was run on the device.  There seed 3 gave: the 11 planted
(position, alt) pairs selected and no other (smallest lrt 366.2), blocks of 6 and 5, every phase right, 279 of 300 reads
tagged and all of them right, smallest joined |link| 161.8, smallest |vote| 326.2, smallest |read llr| 0.61, no flip.
Seed 4: the same sites and blocks, 278 of 279 tagged reads right, smallest joined |link| 399.1.  Seed 5 misses site 640
in the selection.
Measured on the MI355X for this batch: the same 11 sites and two blocks, every phase right, 279 of 300 reads tagged
and all of them right, smallest joined |link| 161.7, smallest |vote| 350.4, smallest |read llr| 0.90, smallest |h| 0.15,
no flip."""
import copy

import numpy as np
import pytest

import allele_ref
import phase_ref

pytestmark = pytest.mark.gpu

SITES_A = [100, 310, 530, 920, 1140, 1360]
SITES_B = [200, 420, 640, 1030, 1250]
SEED = 3
THRESHOLD = 200.0


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


class Diploid:
    """The batch and its front end run ONCE: stage, rows and status kept on the device and fetched to the host."""

    def __init__(self, km, config):
        from nadavca_amd import synthetic
        from nadavca_amd.batchflow import device_stage, likelihood_rows
        from nadavca_amd.seedalign import SeedAligner
        self.ref, self.hap_a, alts_a = allele_ref.planted_haplotypes(1500, SITES_A, SEED)
        _, self.hap_b, alts_b = allele_ref.planted_haplotypes(1500, SITES_B, SEED)
        self.planted = sorted(zip(SITES_A + SITES_B, [int(x) for x in alts_a] + [int(x) for x in alts_b],
                                  [1] * len(SITES_A) + [2] * len(SITES_B)))
        self.owner = np.array([h for _, _, h in self.planted])
        self.rb, self.truth, self.info = synthetic.make_mixed_read_batch(
            300, [self.ref, self.hap_a, self.hap_b], [0, .5, .5], SEED, length=200, spread=20)
        self.aligner = SeedAligner(self.ref)
        self.stage = device_stage(copy.deepcopy(self.rb), self.ref, config, km, self.aligner, 'pooled')
        self.ll, self.status, _ = likelihood_rows(self.stage, config, km)
        self.sa = self.stage.sa.host()
        sa = self.sa
        self.key, self.val = allele_ref.rows(self.ll.cpu().numpy(), sa.reference, sa.ref_off, sa.ref_start, sa.reverse,
                                             self.status.cpu().numpy(), 1.0, self.ref.size)

    def rows(self, km, **kw):
        from nadavca_amd.phase import phase_of_rows
        return phase_of_rows(self.stage, self.ll, self.status, self.ref, None, km, self.rb.n, **kw)

    def restated(self, site_pos, site_alt, clip=30.0, min_shared=3, min_link=2.0, rounds=2):
        sa = self.sa
        has, E = phase_ref.evidence(self.key, self.val, sa.ref_off, sa.ref_start, sa.reverse, site_pos, site_alt, clip)
        chain = np.ones(len(site_pos), dtype=np.int32)
        chain[:1] = 0
        return phase_ref.refine(has, E, chain, min_shared, min_link, rounds)


@pytest.fixture(scope='module')
def dip(km, config):
    return Diploid(km, config)


def as_loop_output(batch, live):
    """A PhaseBatch over one sequence as the dict ``phase_ref.check_against`` takes (reads: the live ones)."""
    phase_set = batch.read_phase_set[live]
    read_block = np.where(phase_set >= 0, np.searchsorted(batch.position, np.maximum(phase_set, 0)), -1)
    return dict(link=batch.link, shared=batch.shared, block=batch.block, sigma=batch.phase, vote=batch.vote,
                n_agree=batch.n_agree, n_against=batch.n_against, read_block=read_block,
                read_llr=batch.read_llr[live], read_sites=batch.read_sites[live], flips=batch.flips_per_round)


def test_every_row_against_the_restatement(dip, km):
    got = dip.rows(km, threshold=THRESHOLD)
    live = dip.sa.live
    assert live.size >= 290 and dip.sa.reverse.any() and not dip.sa.reverse.all()
    assert len(got) >= 2 and (np.diff(got.position) > 0).all() and got.contig_names is None
    ref = dip.restated(got.position, got.alt_base.astype(np.int64))
    print('sites %r; margins %r; flips %r' % (got.position.tolist(), ref['margins'], ref['flips_per_round']))
    phase_ref.check_against(ref, as_loop_output(got, live), 'workflow')
    # the derived columns
    assert np.array_equal(got.phase_set, got.position[got.block]) and (got.contig == 0).all()
    assert np.array_equal(got.block_size, np.bincount(got.block, minlength=len(got))[got.block])
    assert np.array_equal(got.ref_base, dip.ref[got.position]) and (got.alt_base != got.ref_base).all()
    assert got.gt.tolist() == ['1|0' if p > 0 else '0|1' for p in got.phase]
    assert np.array_equal(got.haplotype[live], ref['haplotype']) and got.haplotype.size == dip.rb.n
    dead = np.setdiff1d(np.arange(dip.rb.n), live)
    assert (got.haplotype[dead] == 0).all() and (got.read_phase_set[dead] == -1).all()
    assert np.array_equal(got.read_contig, np.where(got.read_phase_set >= 0, 0, -1))
    # the site columns taken from the fractions are those of its (position, alternative) rows
    f = got.fractions
    for t in range(len(got)):
        row = np.nonzero((f.position == got.position[t]) & (f.alt_base == got.alt_base[t]))[0]
        assert row.size == 1 and got.fraction[t] == f.fraction[row[0]] and got.lrt[t] == f.lrt[row[0]]
        assert got.coverage[t] == f.coverage[row[0]] == f.position_coverage[got.position[t]]
    # a second call returns the same bits
    again = dip.rows(km, threshold=THRESHOLD)
    for name in got.SITE_FIELDS + got.READ_FIELDS:
        assert np.array_equal(getattr(again, name), getattr(got, name)), name
    assert again.flips_per_round == got.flips_per_round
    # other settings: no refinement; a clip that bites at most sites (sums of clipped values are exact, so a read whose
    # sites disagree at the clip ends at H = 0 or h = 0 in exact arithmetic, here and on the device)
    for kw, exact in ((dict(rounds=0), ()), (dict(clip=8.0, rounds=1), ('llr', 'h'))):
        other = dip.rows(km, threshold=THRESHOLD, **kw)
        assert np.array_equal(other.position, got.position)
        phase_ref.check_against(dip.restated(other.position, other.alt_base.astype(np.int64), **kw),
                                as_loop_output(other, live), repr(kw), exact)


def test_planted_sites_are_phased_and_reads_tagged(dip, km):
    got = dip.rows(km, threshold=THRESHOLD)
    assert list(zip(got.position.tolist(), got.alt_base.tolist())) == [(x, a) for x, a, _ in dip.planted]
    first = SITES_A.index(920) + SITES_B.index(1030)          # no read spans 640 .. 920: two blocks
    assert got.block.tolist() == [0] * first + [first] * (len(got) - first) and got.n_blocks == 2
    assert got.phase.tolist() == np.where(dip.owner == dip.owner[got.block], 1, -1).tolist()
    assert got.phase_set.tolist() == [100] * first + [920] * (len(got) - first)
    tagged = got.haplotype > 0
    block_of = np.searchsorted(got.position, np.maximum(got.read_phase_set, 0))
    first_owner = dip.owner[block_of]
    called = np.where(got.haplotype == 1, first_owner, 3 - first_owner)
    right = int((called[tagged] == dip.info['haplotype'][tagged]).sum())
    print('tagged %d of %d reads, %d right; smallest joined |link| %.1f, smallest |vote| %.1f; flips %r'
          % (tagged.sum(), dip.rb.n, right, np.abs(got.link[got.block != np.arange(len(got))]).min(),
             np.abs(got.vote).min(), got.flips_per_round))
    assert tagged.sum() >= 0.75 * dip.rb.n
    assert right >= 0.95 * tagged.sum()


def test_the_workflow_itself_and_known_sites(dip, km, config):
    """The public entry runs the same front end and the same back half; ``sites=`` with the selected pairs gives the
    same phases and tags without a threshold."""
    from nadavca_amd import phase_reads_batch
    want = dip.rows(km, threshold=THRESHOLD)
    got = phase_reads_batch(dip.ref, copy.deepcopy(dip.rb), config=config, kmer_model=km, aligner=dip.aligner,
                            threshold=THRESHOLD)
    known = phase_reads_batch(dip.ref, copy.deepcopy(dip.rb), config=config, kmer_model=km, aligner=dip.aligner,
                              sites=(want.position, want.alt_base))
    assert len(want) > 0
    for other in (got, known):
        for name in want.SITE_FIELDS + want.READ_FIELDS:
            a, b = getattr(other, name), getattr(want, name)
            if a.dtype.kind == 'f':
                assert np.allclose(a, b, rtol=1e-9, atol=1e-9), name
            else:
                assert np.array_equal(a, b), name
        assert other.flips_per_round == want.flips_per_round
    assert known.fractions.threshold is None and not known.fractions.called.any() and got.fractions.called.any()
    # a known site whose alternative no read carries has no row among the fractions: fraction and lrt 0
    quiet = int(np.setdiff1d(np.arange(700, 800), want.fractions.position)[0])
    alt = (int(dip.ref[quiet]) + 1) % 4
    lone = phase_reads_batch(dip.ref, copy.deepcopy(dip.rb), config=config, kmer_model=km, aligner=dip.aligner,
                             sites=([quiet], [alt]))
    assert len(lone) == 1 and lone.fraction[0] == 0.0 and lone.lrt[0] == 0.0 and lone.coverage[0] > 8
    assert lone.block.tolist() == [0] and lone.phase.tolist() == [1] and lone.link[0] == 0.0 and lone.vote[0] == 0.0
    assert (lone.read_sites <= 1).all() and (lone.read_sites == 1).sum() == lone.coverage[0]


def test_no_read_aligns_and_no_site(dip, km, config):
    from nadavca_amd import phase_reads_batch, synthetic
    from nadavca_amd.seedalign import SeedAligner
    other = np.random.default_rng(8).integers(0, 4, 1500).astype(np.int32)
    rb = synthetic.make_mixed_read_batch(4, [other], [1.0], seed=1, length=150, spread=0)[0]
    genome = np.random.default_rng(9).integers(0, 4, 800).astype(np.int32)
    got = phase_reads_batch(genome, rb, config=config, kmer_model=km, aligner=SeedAligner(genome), threshold=100.0)
    assert len(got) == 0 and got.haplotype.tolist() == [0] * 4 and got.read_phase_set.tolist() == [-1] * 4
    assert got.flips_per_round == [0, 0] and got.fractions.position_coverage.tolist() == [0] * 800
    # reads align, no site passes the threshold: the fractions are kept
    none = dip.rows(km, threshold=1e9)
    assert len(none) == 0 and len(none.fractions) > 0 and none.haplotype.size == dip.rb.n and not none.haplotype.any()


def test_over_a_reference_set(km):
    """Known sites on both sides of a join: the block breaks there, positions are contig-local and named."""
    from contig_fixture import ContigFixture, NAMES
    from nadavca_amd import phase_reads_batch, synthetic
    from nadavca_amd.seedalign import SeedAligner
    fx = ContigFixture(synthetic.load_model_arrays())
    contig, local = np.array([1, 1, 2, 2, 2]), np.array([3700, 3800, 30, 130, 330])
    alt = (fx.refset.codes[fx.refset.offsets[contig] + local] + 1) % 4
    got = phase_reads_batch(fx.refset, copy.deepcopy(fx.rb), kmer_model=km, aligner=SeedAligner(fx.refset),
                            sites=((contig, local), alt), min_shared=1, min_link=0.0)
    assert got.contig_names == NAMES and got.contig.tolist() == contig.tolist()
    assert got.position.tolist() == local.tolist() and got.alt_base.tolist() == alt.tolist()
    assert np.array_equal(got.ref_base, fx.refset.codes[fx.refset.offsets[contig] + local])
    # the reads of the 400-base contig cover it end to end: its three sites form one block that starts at ITS first
    # site, although the reads of the contig before it lie flush against the join
    assert got.block.tolist()[2:] == [2, 2, 2] and got.phase_set.tolist()[2:] == [30, 30, 30]
    assert got.link[2] == 0.0 and got.shared[2] == 0 and got.shared[3] >= 40 and got.block[1] in (0, 1)
    assert (got.block[:2] < 2).all() and got.phase_set[0] == 3700
    tagged = got.read_phase_set >= 0
    assert tagged.sum() >= 48 and np.array_equal(got.read_contig[tagged], fx.contig[tagged])
    assert (got.read_phase_set[tagged & (fx.contig == 2)] == 30).all()
    assert set(got.read_phase_set[tagged & (fx.contig == 1)].tolist()) <= {3700, 3800}
    assert (got.read_contig[~tagged] == -1).all()
