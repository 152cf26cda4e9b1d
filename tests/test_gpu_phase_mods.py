"""GPU tests of ``phase_mods_batch``: the diploid genome of tests/test_gpu_phase.py (1 500 bases, haplotype A with 6
substitutions and haplotype B with 5, alternating) with one CG planted 2 bases behind the substitution at 310, 600 reads
of about 200 bases drawn from A and B with probability 0.5 each on both strands
(``synthetic.make_phased_modified_read_batch``), ``SeedAligner``, bandwidth 40, the packaged table for the phasing and
its 5-letter extension (an M k-mer = its C k-mer's level + N(0, 0.6^2)) for the calls.  The CG
occurrences at least 12 bases from every substitution are dealt into four classes in turn (occurrences that share a
k-mer as one group: ``Diploid.deal``): modified on haplotype A only, on B only, on both, on neither.

The phasing takes the 11 substitutions as KNOWN variants (``sites=``).  Left to ``select_sites`` at threshold 200 the
4-letter phase step also picks the CGs that are modified on one haplotype only, which are heterozygous signal to it: on
this batch 46 sites instead of 11, blocks cut at them, and 472 of 599 tagged reads right instead of 562 of 563 (measured
on the MI355X).  A 5-letter phase step is not part of this workflow.

SEED 3 is the phase test's; it was run on the device before it was kept: the 11 sites in two blocks (phase sets 100 and
920), 563 of 600 reads tagged and 562 of them right.  Measured on the MI355X for this batch, 202 sites, 194 of them with
both haplotypes at ``min_tagged``:
  class     sites  asm_lrt median / smallest / largest   p median / largest     |delta| smallest / largest
  A only     38      53.49 / 19.41 / 76.38               2.7e-13 / 1.1e-05      0.938 / 1.000
  B only     42      53.05 / 13.74 / 80.23               3.3e-13 / 2.1e-04      0.574 / 1.000
  both       32       0.00 /  0.00 /  0.00               1 / 1                  0.000 / 0.000
  neither    44       0.00 /  0.00 /  1.25               1 / 1                  0.000 / 0.046
|f^ - realised share of modified rows| per (site, haplotype), 312 pairs: median 0.0000, 90 % 0.0000, largest 0.3547.
Share of tagged reads: 563 / 600 = 0.938.
With the classes dealt per single CG instead of per group (``Diploid.deal``), one site fails (b): position 799, B only,
f^_B = 0.462 with 0.97 of its rows ``crowded`` — the CGs at 794, 796, 799 and 803 span more than one joint hypothesis
and the neighbours at 796 and 803 were modified on the other haplotype."""
import copy

import numpy as np
import pytest

import allele_ref
import mod_sites_ref

pytestmark = pytest.mark.gpu

SITES_A = [100, 310, 530, 920, 1140, 1360]
SITES_B = [200, 420, 640, 1030, 1250]
NEAR_CG = 312            # a CG planted within k - 1 of the substitution at 310
SEED = 3
N_READS = 600
CLASSES = ('A only', 'B only', 'both', 'neither')


def _model5(seed=5, sd=0.6):
    """The packaged 6-mer table extended to 5 letters: an M k-mer = its C k-mer's level + N(0, sd^2) (as
    tests/test_gpu_call_mods.py makes it)."""
    from nadavca_amd import synthetic, kmer_train
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
    mean5 = mean5 + np.where(has_m, np.random.default_rng(seed).normal(0.0, sd, 5 ** k), 0.0)
    return k, central, 5, mean5, sigma5


@pytest.fixture(scope='module')
def km():
    from nadavca_amd.kmer_model import KmerModel
    from nadavca_amd import defaults
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def model5():
    return _model5()


@pytest.fixture(scope='module')
def km5(model5):
    from nadavca_amd import dtw
    return dtw.KmerModel(*model5)


@pytest.fixture(scope='module')
def config():
    from nadavca_amd import defaults
    from nadavca_amd.batchflow import load_config
    return dict(load_config(defaults.CONFIG_FILE), bandwidth=40)


def numpy_solve(site_lo, site_hi, val, group, set_mask, clip):
    return mod_sites_ref.solve(site_lo.cpu().numpy(), site_hi.cpu().numpy(), val.cpu().numpy(), group.cpu().numpy(),
                               set_mask, clip)


class Diploid:
    """The genome, its classes of CG occurrences, the batch, and ONE run of the workflow."""

    def __init__(self, km, km5, model5, config, n_reads=N_READS, seed=SEED, run=True):
        from nadavca_amd import phase_mods_batch, synthetic
        from nadavca_amd.seedalign import SeedAligner
        ref, _, _ = allele_ref.planted_haplotypes(1500, SITES_A, SEED)
        ref[NEAR_CG:NEAR_CG + 2] = [1, 2]
        planted = np.array(sorted(SITES_A + SITES_B))
        rng = np.random.default_rng(SEED)
        self.ref = ref
        self.hap_a, self.hap_b = ref.copy(), ref.copy()
        for hap, sites in ((self.hap_a, SITES_A), (self.hap_b, SITES_B)):
            hap[sites] = (ref[sites] + rng.integers(1, 4, len(sites))) % 4
        cg = np.nonzero((ref[:-1] == 1) & (ref[1:] == 2))[0]
        far = np.array([np.abs(planted - x).min() >= 12 and np.abs(planted - (x + 1)).min() >= 12 for x in cg])
        self.cg, self.far = cg, cg[far]
        self.cls = self.deal(self.far, km.get_k())                          # forward coordinate of the C -> class
        on = lambda *classes: [x for x in self.far.tolist() if self.cls[x] in classes]
        self.modified = [[], on(0, 2), on(1, 2)]
        self.rb, self.truth, self.info = synthetic.make_phased_modified_read_batch(
            n_reads, [ref, self.hap_a, self.hap_b], [0, .5, .5], self.modified, model5, seed, length=200, spread=20)
        self.aligner = SeedAligner(ref)
        self.k = km.get_k()
        # the phased sites are the KNOWN substitutions (``sites=``), not ``select_sites``' own choice: see the docstring
        alts = np.where(np.isin(planted, SITES_A), self.hap_a[planted], self.hap_b[planted])
        self.args = dict(config=config, sites=(planted, alts))
        self.before = copy.deepcopy(self.rb)
        self.got = phase_mods_batch(ref, self.rb, self.aligner, km, km5, **self.args) if run else None

    @staticmethod
    def deal(cg, k):
        """The four classes dealt in turn, one GROUP of occurrences at a time: occurrences within k - 1 bases of each
        other share a k-mer and get one class.  ``call_mods_batch`` scores a site whose cluster had to be cut (four CGs
        over more than 14 - k bases) with the neighbour outside taken as canonical (``crowded``), so a neighbour that is
        modified on ANOTHER haplotype would confound the site's ratios: a documented limit of the calls, not what these
        tests are about."""
        group = np.concatenate([[0], np.cumsum(np.diff(cg) > k - 1)])
        return {int(x): int(g) % 4 for x, g in zip(cg, group)}

    def site_class(self, position, strand):
        """The class of the CG a row of (position, strand) belongs to (its C lies at position - strand), or -1"""
        return self.cls.get(int(position) - int(strand), -1)

    def labels(self):
        """phase set -> the truth haplotype (1: A, 2: B) that its label 1 stands for, by the tagged reads' majority"""
        ph, truth = self.got.phase, self.info['haplotype']
        out = {}
        for ps in np.unique(ph.read_phase_set[ph.read_phase_set >= 0]).tolist():
            one = truth[(ph.read_phase_set == ps) & (ph.haplotype == 1)]
            out[ps] = 1 if (one == 1).sum() >= (one == 2).sum() else 2
        return out


@pytest.fixture(scope='module')
def dip(km, km5, model5, config):
    return Diploid(km, km5, model5, config)


def test_every_column_against_the_restatement(dip):
    from nadavca_amd.phase_mods import PhasedModBatch, phase_mods_of_rows
    from scipy.special import chdtrc
    got = dip.got
    want = phase_mods_of_rows(got.mods, got.phase, numpy_solve, dip.k)
    assert len(got) == len(want) > 100 and got.contig_names is None and (got.contig == 0).all()
    for name in ('contig', 'position', 'strand', 'phase_set', 'reads', 'n_h1', 'n_h2', 'n_untagged', 'near_variant'):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    table = got.mods.site_table()
    for name in ('contig', 'position', 'strand', 'reads'):
        assert np.array_equal(getattr(got, name), table[name]), name
    # the four sets of every site with the tolerances of the allele kernels; the operator's L is visible in lrt (set
    # "all"), the restatement's own value stands in for the other sets and for ll_half / ll_full
    order, lo, hi, site_ps, group = mod_sites_ref.phase_sets(got.mods, got.phase)
    assert np.array_equal(site_ps, got.phase_set)
    _, _, r_ll, ref, D, valid = mod_sites_ref.solve(lo, hi, got.mods.llr[order], group, mod_sites_ref.MASKS, got.clip,
                                                    full=True)
    fraction = np.stack([got.fraction, got.fraction_h1, got.fraction_h2, got.fraction_tagged], 1).reshape(-1)
    lrt = ref['lrt'].reshape(-1, 4).copy()
    lrt[:, 0] = got.lrt
    counts = allele_ref.check_against(ref, fraction, lrt.reshape(-1), ref['ll_half'], ref['ll_full'], D, valid,
                                      'workflow')
    print('%d sites; (site, set) pairs with fraction surely 0 / 1 / inside: %d / %d / %d; sharp optima: %d'
          % ((len(got),) + counts))
    assert np.array_equal(got.delta, got.fraction_h1 - got.fraction_h2)
    # asm_lrt = 2 ((L_1 + L_2) - L_T): each L within 1e-9 (1 + |L|) of the restatement's
    gate = (got.n_h1 >= got.min_tagged) & (got.n_h2 >= got.min_tagged)
    assert np.array_equal(np.isnan(got.asm_lrt), ~gate) and np.array_equal(np.isnan(got.p), ~gate) and gate.sum() > 100
    bound = 2e-9 * (3.0 + np.abs(r_ll[:, 1:]).sum(1))
    assert (np.abs(got.asm_lrt - want.asm_lrt)[gate] <= bound[gate]).all() and (got.asm_lrt[gate] >= 0).all()
    assert np.array_equal(got.p[gate], chdtrc(1.0, got.asm_lrt[gate]))
    assert isinstance(got, PhasedModBatch) and got.min_tagged == 4 and got.clip == 30.0
    # the two workflows ran on the caller's ReadBatch and left it as it was
    for name, value in vars(dip.before).items():
        now = getattr(dip.rb, name)
        assert np.array_equal(now, value) if isinstance(value, np.ndarray) else now == value, name


def test_planted_classes(dip):
    """(b) and (c) of the planted classes; the figures it prints are in the module's docstring.  Two further floors
    from those figures: p <= 0.01 at every one-haplotype site (measured largest 2.1e-4: a factor 48), asm_lrt <= 5 at
    every site modified on both or on neither (measured largest 1.25: a factor 4)."""
    got = dip.got
    label = dip.labels()
    cls = np.array([dip.site_class(p, s) for p, s in zip(got.position, got.strand)])
    gate = (got.n_h1 >= got.min_tagged) & (got.n_h2 >= got.min_tagged)
    # delta with the sign of "A minus B"
    flip = np.array([1.0 if label.get(int(ps), 1) == 1 else -1.0 for ps in got.phase_set])
    delta_ab = got.delta * flip
    f_a = np.where(flip > 0, got.fraction_h1, got.fraction_h2)
    f_b = np.where(flip > 0, got.fraction_h2, got.fraction_h1)
    ph = got.phase
    tagged = ph.haplotype > 0
    truth = dip.info['haplotype']
    called = np.array([label[int(ps)] if h == 1 else 3 - label[int(ps)]
                       for ps, h in zip(ph.read_phase_set[tagged], ph.haplotype[tagged])])
    print('tagged %d of %d reads, %d right; %d phased sites %r; sites %d, gated %d'
          % (tagged.sum(), ph.haplotype.size, (called == truth[tagged]).sum(), len(ph), ph.position.tolist(), len(got),
             gate.sum()))
    # the realised share of modified rows per (site, label): from the rows' true haplotypes
    order, lo, hi, _, group = mod_sites_ref.phase_sets(got.mods, got.phase)
    row_truth = truth[got.mods.read[order]]
    err = []
    for s in np.nonzero(gate & (cls >= 0))[0]:
        x = int(got.position[s]) - int(got.strand[s])
        for g, f in ((1, got.fraction_h1[s]), (2, got.fraction_h2[s])):
            rows = row_truth[lo[s]:hi[s]][group[lo[s]:hi[s]] == g]
            err.append(abs(f - np.mean([x in dip.modified[t] for t in rows])))
    print('|f^ - realised share| per (site, haplotype): median %.4f, 90%% %.4f, largest %.4f over %d'
          % (np.median(err), np.quantile(err, 0.9), max(err), len(err)))
    for c, name in enumerate(CLASSES):
        m = gate & (cls == c)
        print('%-8s %3d sites: asm_lrt median %8.2f, smallest %8.2f, largest %8.2f; p median %.3g, largest %.3g; '
              '|delta| smallest %.3f largest %.3f'
              % (name, m.sum(), np.median(got.asm_lrt[m]), got.asm_lrt[m].min(), got.asm_lrt[m].max(),
                 np.median(got.p[m]), got.p[m].max(), np.abs(got.delta[m]).min(), np.abs(got.delta[m]).max()))
        assert m.sum() >= 10, name
    # (b) modified on one haplotype: that haplotype's fraction above 0.5, the other's below, delta of the planted sign
    only_a, only_b = gate & (cls == 0), gate & (cls == 1)
    crowded = np.array([got.mods.crowded[order[lo[s]:hi[s]]].mean() for s in range(len(got))])
    for s in np.nonzero((only_a & ~((f_a > 0.5) & (f_b < 0.5))) | (only_b & ~((f_b > 0.5) & (f_a < 0.5))))[0]:
        print('one-haplotype site off: position %d strand %d class %s n_h1 %d n_h2 %d f_a %.3f f_b %.3f crowded rows %.2f'
              % (got.position[s], got.strand[s], CLASSES[cls[s]], got.n_h1[s], got.n_h2[s], f_a[s], f_b[s], crowded[s]))
    assert (f_a[only_a] > 0.5).all() and (f_b[only_a] < 0.5).all() and (delta_ab[only_a] > 0).all()
    assert (f_b[only_b] > 0.5).all() and (f_a[only_b] < 0.5).all() and (delta_ab[only_b] < 0).all()
    # (c) modified on both or on neither: no |delta| above the smallest one of the one-haplotype sites
    smallest = np.abs(got.delta[only_a | only_b]).min()
    assert (np.abs(got.delta[gate & (cls >= 2)]) < smallest).all()
    assert (got.p[only_a | only_b] <= 0.01).all() and (got.asm_lrt[gate & (cls >= 2)] <= 5.0).all()
    assert tagged.sum() >= 0.75 * ph.haplotype.size and (called == truth[tagged]).sum() >= 0.95 * tagged.sum()


def test_near_variant(dip):
    got = dip.got
    phased = got.phase.position
    assert 310 in phased.tolist()
    want = np.array([np.abs(phased - p).min() <= dip.k - 1 for p in got.position])
    assert np.array_equal(got.near_variant, want)
    at = lambda p, s: int(np.nonzero((got.position == p) & (got.strand == s))[0][0])
    assert got.near_variant[at(NEAR_CG, 0)] and got.near_variant[at(NEAR_CG + 1, 1)]
    assert want.sum() < 0.2 * want.size
    # no CG of the four classes is near a variant: they lie 12 bases away at least
    cls = np.array([dip.site_class(p, s) for p, s in zip(got.position, got.strand)])
    assert not got.near_variant[cls >= 0].any()


def test_frequencies_without_haplotypes_and_tsv(dip, tmp_path):
    from nadavca_amd import mod_site_frequencies
    got = dip.got
    freq = mod_site_frequencies(got.mods)
    for name in ('contig', 'position', 'strand', 'reads', 'fraction', 'lrt'):
        assert np.array_equal(freq[name], getattr(got, name)), name          # set "all" alone: the same bits
        assert freq[name].dtype == getattr(got, name).dtype, name
    tight = mod_site_frequencies(got.mods, clip=2.0)
    assert np.array_equal(tight['reads'], got.reads) and not np.array_equal(tight['lrt'], got.lrt)
    path = tmp_path / 'sites.tsv'
    got.write_tsv(path)
    lines = path.read_text().splitlines()
    assert len(lines) == len(got) + 1 and lines[0].startswith('contig\tposition\tstrand\tphase_set\treads')
    row = lines[1].split('\t')
    assert row[1] == str(got.position[0]) and float(row[8]) == got.fraction[0] and len(row) == 17


def test_empty_cases(dip, km, km5, model5, config):
    from nadavca_amd import mod_site_frequencies, phase_mods_batch, synthetic
    from nadavca_amd.call_mods import ModCallBatch
    from nadavca_amd.seedalign import SeedAligner
    small = Diploid(km, km5, model5, config, n_reads=40, seed=9, run=False)
    # no read aligns: reads of another genome
    other = np.random.default_rng(8).integers(0, 4, 1500).astype(np.int32)
    rb = synthetic.make_mixed_read_batch(4, [other], [1.0], seed=1, length=150, spread=0)[0]
    genome = np.random.default_rng(9).integers(0, 4, 800).astype(np.int32)
    got = phase_mods_batch(genome, rb, SeedAligner(genome), km, km5, config=config, threshold=100.0)
    assert len(got) == 0 and len(got.mods) == 0 and len(got.phase) == 0 and got.phase.haplotype.tolist() == [0] * 4
    # no site is phased: every row untagged, no contrast
    got = phase_mods_batch(small.ref, copy.deepcopy(small.rb), small.aligner, km, km5, config=config, threshold=1e9)
    assert len(got.phase) == 0 and len(got) > 50 and (got.phase_set == -1).all() and np.isnan(got.p).all()
    assert np.array_equal(got.n_untagged, got.reads) and not got.n_h1.any() and not got.near_variant.any()
    assert (got.fraction_tagged == 0).all() and got.fraction.max() > 0.5
    # a batch without the pattern
    pattern = 'CGCGCGCG'
    text = ''.join('ACGT'[b] for b in small.ref)
    assert pattern not in text
    got = phase_mods_batch(small.ref, copy.deepcopy(small.rb), small.aligner, km, km5, pattern=pattern, config=config,
                           threshold=1e9)
    assert len(got) == 0 and len(got.mods) == 0 and got.reads.dtype == np.int64
    assert mod_site_frequencies(ModCallBatch.empty())['fraction'].size == 0
    with pytest.raises(ValueError):
        phase_mods_batch(small.ref, small.rb, small.aligner, km, km5, config=config, threshold=1e9, clip=0.0)
    with pytest.raises(ValueError):
        phase_mods_batch(small.ref, small.rb, small.aligner, km, km5, config=config, threshold=1e9, min_tagged=-1)
