"""CPU-only tests of ``phase_reads_batch``: the numpy restatement of its contract (tests/phase_ref.py) against brute
force, the constructed case in which the refinement flips a site, the tie rules, ``select_sites``, the argument checks
made before any device call, the TSV writers, the new entries of the C-ABI, and the planted two-haplotype experiment
through the CPU oracle."""
import io
import itertools
import os

import numpy as np
import pytest

import allele_ref
import phase_ref
from phase_ref import dense, refinement_case


def test_sum64_is_the_kernels_order():
    rng = np.random.default_rng(0)
    for n in (0, 1, 63, 64, 65, 129, 200):
        t = rng.normal(0, 1e3, n) * 10.0 ** rng.integers(-8, 8, n)
        lanes = [0.0] * 64
        for j, x in enumerate(t):
            lanes[j % 64] += x
        for d in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ d] for l in range(64)]
        assert phase_ref.sum64(t) == lanes[0]
    assert phase_ref.sum64([1.5, -0.25]) == 1.25
    assert not np.signbit(phase_ref.sum64([-0.0] * 70))        # every partial starts at +0.0


def test_evidence_and_clip():
    assert phase_ref.clip_value([-np.inf, np.inf, np.nan, -600.0, 600.0, 3.0, -30.0], 30.0).tolist() == \
        [-30.0, 30.0, -30.0, -30.0, 30.0, 3.0, -30.0]
    # two reads of 6 bases over positions 10 .. 15, one reverse; a row whose key is -1 inside the covering read
    ref_off = np.array([0, 6, 12, 12, 18])
    start, reverse = np.array([10, 10, 0, 40]), np.array([0, 1, 0, 0])
    key = np.concatenate([10 + np.arange(6), 15 - np.arange(6), 40 + np.arange(6)])
    val = np.arange(18 * 4, dtype=np.float64).reshape(18, 4) / 8.0 - 3.0
    key[3] = -1
    has, E = phase_ref.evidence(key, val, ref_off, start, reverse, [11, 13, 15, 45], [2, 0, 3, 1], 5.0)
    assert has.tolist() == [[True, False, True, False], [True, True, True, False], [False] * 4,
                            [False, False, False, True]]
    assert E[0, 0] == val[1, 2] and E[1, 0] == val[6 + 4, 2] and E[1, 1] == val[6 + 2, 0] and E[0, 2] == val[5, 3]
    assert E[3, 3] == 5.0 and val[17, 1] > 5.0 and E[0, 1] == 0.0


def test_links_against_brute_force_for_two_sites():
    """With two sites the likelihood of every read marginalised over its haplotype decides by exactly the link."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        n = int(rng.integers(1, 150))
        E = rng.normal(0, 6, (n, 2))
        has = rng.random((n, 2)) < 0.8
        E = np.where(has, phase_ref.clip_value(E, 8.0), 0.0)
        link, shared = phase_ref.links(has, E, [1, 1])
        same = phase_ref.phasing_likelihood(has, E, np.array([1, 1]))
        other = phase_ref.phasing_likelihood(has, E, np.array([1, -1]))
        assert shared.tolist() == [0, int((has[:, 0] & has[:, 1]).sum())] and link[0] == 0.0
        assert abs(link[1] - (same - other)) <= 1e-9 * (1 + abs(same) + abs(other))
    assert phase_ref.links(has, E, [1, 0])[0][1] == 0.0 and phase_ref.links(has, E, [1, 0])[1][1] == 0


def test_phasing_against_brute_force_up_to_six_sites():
    """Reads drawn from two haplotypes with clear evidence: the phases of the restatement are the maximum of the
    likelihood over all 2^(S - 1) phasings with the first site at +1."""
    rng = np.random.default_rng(6)
    for S in (2, 3, 4, 5, 6):
        truth = np.where(rng.random(S) < 0.5, 1, -1)
        truth[0] = 1
        n = 60
        hap = np.where(rng.random(n) < 0.5, 1, -1)
        first = rng.integers(0, S - 1, n)
        has = (np.arange(S)[None, :] >= first[:, None]) & (np.arange(S)[None, :] <= first[:, None] + 2)
        E = np.where(has, hap[:, None] * truth[None, :] * 6.0 + rng.normal(0, 2.0, (n, S)), 0.0)
        got = phase_ref.refine(has, E, np.ones(S, dtype=int), 3, 2.0, 2)
        assert (got['block'] == 0).all() and got['flips_per_round'] == [0, 0]
        best = max(itertools.product([1, -1], repeat=S - 1),
                   key=lambda t: phase_ref.phasing_likelihood(has, E, np.array((1,) + t)))
        assert got['sigma'].tolist() == [1] + list(best) == truth.tolist()
        assert (got['haplotype'] == np.where(hap > 0, 1, 2)).mean() >= 0.95


def test_refinement_flips_a_site():
    has, E = refinement_case()
    link, shared = phase_ref.links(has, E, [1, 1, 1])
    assert shared.tolist() == [0, 28, 11] and link[1] > 100 and link[2] < -20
    block, sigma, joined, _ = phase_ref.chain(link, shared, [1, 1, 1], 3, 2.0)
    assert block.tolist() == [0, 0, 0] and sigma.tolist() == [1, 1, -1] and joined.tolist() == [False, True, True]
    rb, llr, ns, _ = phase_ref.tag(has, E, block, sigma)
    vote, agree, against, _ = phase_ref.votes(has, E, block, sigma, rb, llr, ns)
    assert vote[2] == 50.0 and (agree[2], against[2]) == (3, 8)        # the link put c at -1, the vote says +1
    got = phase_ref.refine(has, E, [1, 1, 1], 3, 2.0, 2)
    assert got['flips_per_round'] == [1, 0] and got['sigma'].tolist() == [1, 1, 1]
    assert got['block'].tolist() == [0, 0, 0]                # the refinement neither merges nor splits
    assert got['haplotype'].tolist() == [1] * 10 + [2] * 10 + [0] * 3 + [1] * 4 + [2] * 4
    assert phase_ref.refine(has, E, [1, 1, 1], 3, 2.0, 0)['flips_per_round'] == []
    assert phase_ref.refine(has, E, [1, 1, 1], 3, 2.0, 0)['sigma'].tolist() == [1, 1, -1]
    # a flip of a block's FIRST site turns the whole block, so that the first site stays at +1
    has2, E2 = dense([(5.0, 5.0, 5.0)] * 6 + [(-5.0, -5.0, -5.0)] * 6, 3)
    got = phase_ref.refine(has2, E2, [1, 1, 1], 3, 2.0, 1)
    assert got['sigma'].tolist() == [1, 1, 1] and got['flips_per_round'] == [0]


def test_tie_rules_and_thresholds():
    # |link| == min_link joins; shared < min_shared does not; chain 0 opens a block; link <= 0 at a join is -1
    link = np.array([0.0, 2.0, -2.0, 1.999, 50.0, 50.0, 0.0])
    shared = np.array([0, 3, 3, 9, 2, 9, 9])
    chain_flag = np.array([1, 1, 1, 1, 1, 0, 1])
    block, sigma, joined, m = phase_ref.chain(link, shared, chain_flag, 3, 2.0)
    assert joined.tolist() == [False, True, True, False, False, False, False]
    assert block.tolist() == [0, 0, 0, 3, 4, 5, 6] and sigma.tolist() == [1, 1, -1, 1, 1, 1, 1]
    assert m['join'] == 0.0 and m['sign'] == 2.0
    block, sigma, joined, _ = phase_ref.chain(np.array([0.0, 0.0]), np.array([0, 5]), [1, 1], 3, 0.0)
    assert joined.tolist() == [False, True] and sigma.tolist() == [1, -1]
    # tag: the first of two runs with equal |H|; H == 0 is haplotype 0; a read without a site
    has, E = dense([(4.0, None, -4.0), (3.0, -3.0, None), (None, None, None), (1.0, None, 2.0)], 3)
    blk, sg = np.array([0, 0, 2]), np.array([1, 1, 1])
    rb, llr, ns, m = phase_ref.tag(has, E, blk, sg)
    assert rb.tolist() == [0, 0, -1, 2] and llr.tolist() == [4.0, 0.0, 0.0, 2.0] and ns.tolist() == [1, 2, 0, 1]
    assert m['gap'] == 0.0 and m['llr'] == 0.0
    # vote: a read's only site has h == 0 and does not count; read 1 (H = 0) counts at both of its sites
    vote, agree, against, _ = phase_ref.votes(has, E, blk, sg, rb, llr, ns)
    assert vote.tolist() == [-3.0, -3.0, 0.0] and agree.tolist() == [0, 0, 0] and against.tolist() == [1, 1, 0]


def test_select_sites():
    from nadavca_amd.allele_fractions import AlleleFractionBatch
    from nadavca_amd.phase import select_sites
    n = 10
    position = np.array([5, 5, 5, 9, 12, 12, 20, 21, 30, 5])
    contig = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1], dtype=np.int32)
    lrt = np.array([300.0, 400.0, 400.0, 500.0, 250.0, 250.0, 900.0, 199.9, 200.0, 600.0])
    fraction = np.array([0.5, 0.5, 0.5, 0.9, 0.25, 0.75, 0.5, 0.5, 0.5, 0.5])
    coverage = np.array([20, 20, 20, 20, 8, 8, 7, 20, 20, 20])
    shadowed = np.zeros(n, dtype=bool)
    shadowed[8] = True
    f = AlleleFractionBatch(contig, position, np.zeros(n, np.int8), np.array([1, 2, 3, 1, 1, 2, 1, 1, 1, 1], np.int8),
                            coverage, fraction, lrt, lrt, lrt, np.zeros(n, np.int8), shadowed, np.zeros(n, bool),
                            np.zeros(40, np.int64))
    # position 5: the largest lrt, the first on ties; 9: fraction outside; 12: both bounds are inside, the first of a
    # tie; 20: coverage; 21: lrt; 30: shadowed; (1, 5) is another position than (0, 5)
    assert select_sites(f, 200.0, 0.25, 8).tolist() == [1, 4, 9]
    assert select_sites(f, 200.0, 0.25, 7).tolist() == [1, 4, 6, 9]
    assert select_sites(f, 199.0, 0.05, 8).tolist() == [1, 3, 4, 7, 9]
    assert select_sites(f, 1e9).size == 0 and select_sites(AlleleFractionBatch.empty(3), 1.0).size == 0


def test_argument_errors_before_any_device_call():
    from nadavca_amd import phase_reads_batch
    from nadavca_amd.refset import ReferenceSet

    class Model:   # (never reaches a kernel: the checks come first)
        alphabet_size = 4

    class Model5:
        alphabet_size = 5

    class Aligner:
        reference_num = np.zeros(50, dtype=np.int32)
    ref = np.zeros(50, dtype=np.int32)
    base = dict(kmer_model=Model(), aligner=Aligner(), threshold=100.0)
    call = lambda reference=ref, **kw: phase_reads_batch(reference, None, config={}, **{**base, **kw})
    sites = lambda P, a: dict(sites=(np.array(P), np.array(a)))
    for kw in (dict(kmer_model=Model5()), dict(aligner=None), dict(threshold=None), dict(threshold=float('nan')),
               dict(clip=0.0), dict(clip=-1.0), dict(clip=float('inf')), dict(clip=float('nan')),
               dict(event_length=0.0), dict(event_length=float('inf')), dict(min_fraction=-0.1),
               dict(min_fraction=0.6), dict(min_coverage=-1), dict(min_coverage=2.5), dict(min_shared=-1),
               dict(min_shared=1.5), dict(min_link=-1.0), dict(min_link=float('nan')), dict(rounds=-1),
               dict(rounds=0.5), dict(sites=3), sites([3, 3], [1, 1]), sites([5, 3], [1, 1]), sites([3, 50], [1, 1]),
               sites([-1, 3], [1, 1]), sites([3, 5], [1, 4]), sites([3, 5], [1, 0]), sites([3, 5], [1]),
               sites([3.0, 5.0], [1, 1]), sites([[3, 5]], [[1, 1]])):
        with pytest.raises(ValueError):
            call(**kw)
    # over a ReferenceSet the positions are (contig, local)
    rs = ReferenceSet.from_arrays(['a', 'b'], [np.zeros(20, np.int32), np.zeros(30, np.int32)])
    pair = lambda c, p, a: dict(sites=((np.array(c), np.array(p)), np.array(a)))
    for kw in (sites([3, 5], [1, 1]), pair([0, 2], [3, 5], [1, 1]), pair([0, 0], [3, 20], [1, 1]),
               pair([1, 0], [3, 5], [1, 1]), pair([0, 1], [3, 5], [1, 0]), pair([0], [3, 5], [1, 1])):
        with pytest.raises(ValueError):
            call(reference=rs, **kw)
    from nadavca_amd.phase import _check_sites
    P, a = _check_sites(((np.array([0, 1, 1]), np.array([19, 0, 29])), np.array([1, 2, 3])), rs.codes, rs)
    assert P.tolist() == [19, 20, 49] and a.tolist() == [1, 2, 3] and a.dtype == np.int32
    assert _check_sites(([], []), ref, None)[0].size == 0


def test_result_table_and_tsv(tmp_path):
    from nadavca_amd.phase import PhaseBatch, _read_table, _site_table
    z = PhaseBatch.empty(3, 7, 2, 5.0, ['a'])
    assert len(z) == 0 and z.haplotype.tolist() == [0, 0, 0] and z.read_phase_set.tolist() == [-1] * 3
    assert z.flips_per_round == [0, 0] and len(z.fractions) == 0 and z.fractions.position_coverage.size == 7
    assert z.gt.size == 0 and z.n_blocks == 0 and z.read_contig.tolist() == [-1] * 3
    s, r = _site_table(2), _read_table(3)
    s['contig'][:], s['position'][:], s['ref_base'][:], s['alt_base'][:] = [0, 1], [5, 2], [0, 3], [2, 1]
    s['phase'][:], s['block'][:], s['phase_set'][:], s['block_size'][:] = [1, -1], [0, 1], [5, 2], [1, 1]
    s['link'][:], s['shared'][:], s['vote'][:], s['n_agree'][:], s['n_against'][:] = [0.0, -12.5], [0, 9], \
        [80.0, 0.25], [7, 1], [0, 2]
    s['fraction'][:], s['lrt'][:], s['coverage'][:] = [0.5, 0.25], [300.0, 250.5], [30, 12]
    r['haplotype'][:], r['read_contig'][:], r['read_phase_set'][:] = [1, 0, 2], [0, -1, 1], [5, -1, 2]
    b = PhaseBatch(s, r, z.fractions, [1, 0], ['chrA', 'chrB'])
    assert b.gt.tolist() == ['1|0', '0|1'] and b.n_blocks == 2 and b.flips_per_round == [1, 0]
    buf = io.StringIO(newline='')
    b.write_sites_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0].split('\t') == ['contig', 'position', 'ref', 'alt', 'gt', 'phase_set', 'block_size', 'link',
                                    'shared', 'vote', 'n_agree', 'n_against', 'fraction', 'lrt', 'coverage']
    assert lines[1] == 'chrA\t5\tA\tG\t1|0\t5\t1\t0.0\t0\t80.0\t7\t0\t0.5\t300.0\t30'
    assert lines[2] == 'chrB\t2\tT\tC\t0|1\t2\t1\t-12.5\t9\t0.25\t1\t2\t0.25\t250.5\t12' and lines[3] == ''
    buf = io.StringIO(newline='')
    b.write_reads_tsv(buf)
    assert buf.getvalue() == 'read\thaplotype\tphase_set\tcontig\n0\tH1\t5\tchrA\n1\tnone\t.\t.\n2\tH2\t2\tchrB\n'
    path = os.path.join(str(tmp_path), 'r.tsv')
    b.write_reads_tsv(path)
    assert open(path).read() == buf.getvalue()
    path = os.path.join(str(tmp_path), 's.tsv')
    b.write_sites_tsv(path)
    assert open(path).read().count('\n') == 3


def test_phase_blocks_on_the_host():
    """The integer work between the kernels (``device.phase_blocks``, torch) against the restatement."""
    import torch
    from nadavca_amd.device import phase_blocks
    rng = np.random.default_rng(3)
    for S in (0, 1, 2, 40):
        link = np.round(rng.normal(0, 4, S), 1)
        shared = rng.integers(0, 8, S)
        chain_flag = (rng.random(S) < 0.9).astype(np.int32)
        want = phase_ref.chain(link, shared, chain_flag, 3, 2.0)
        block, sigma = phase_blocks(torch.from_numpy(link), torch.from_numpy(shared), torch.from_numpy(chain_flag),
                                    3, 2.0)
        assert block.tolist() == want[0].tolist() and sigma.tolist() == want[1].tolist()
        assert block.dtype == torch.int64 and sigma.dtype == torch.int32


def test_new_entries_declared_bound_and_exported():
    from conftest import ROOT
    import nadavca_amd
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    lib = _lib.load()
    for name in ('nvk_phase_links_dev', 'nvk_phase_tag_dev', 'nvk_phase_votes_dev'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'NVK_K_COUNT = 13' in header and len(_lib.KERNEL_NAMES) == 13
    for f in ('allele_sorted_rows_dev', 'phase_links_dev', 'phase_tag_dev', 'phase_votes_dev', 'phase_sites_dev'):
        assert callable(getattr(device, f))
    for f in ('phase_reads_batch', 'PhaseBatch'):
        assert f in nadavca_amd.__all__ and hasattr(nadavca_amd, f)


SITES_A = [100, 275, 455, 800, 975, 1150]
SITES_B = [190, 370, 885, 1060]


def test_planted_haplotypes_on_the_oracle(oracle_port):
    """The planted experiment through the CPU oracle: the packaged 6-mer table, a 1 200-base genome, 6 substitutions on
    haplotype A and 4 on haplotype B, 240 reads of 150 +- 20 bases on both strands drawn from A and B with probability
    0.5 each (none from the reference), signals in the table's own units (no normalisation), anchors on 75 % of the true
    bases moved by up to 20 samples, bandwidth 40, wobbling on; sites from ``select_sites`` with threshold 200.
    Observed with seed 4: the 10 planted (position, alt) pairs selected and no other, two blocks of 5 (no read spans
    455 .. 800), every phase right, 194 reads tagged, all of them right; smallest joined |link| 173.6, smallest |vote|
    220.0, smallest |read llr| of a tagged read 3.58, no flip."""
    from nadavca_amd import synthetic
    from nadavca_amd.allele_fractions import AlleleFractionBatch
    from nadavca_amd.phase import select_sites
    model = synthetic.load_model_arrays()
    k = model[0]
    ref, hap_a, alts_a = allele_ref.planted_haplotypes(1200, SITES_A, 4)
    ref_b, hap_b, alts_b = allele_ref.planted_haplotypes(1200, SITES_B, 4)
    assert np.array_equal(ref, ref_b)
    rb, truth, info = synthetic.make_mixed_read_batch(240, [ref, hap_a, hap_b], [0.0, 0.5, 0.5], seed=4, model=model,
                                                      length=150, spread=20, anchor_density=0.75, jitter=20,
                                                      raw_scale=1.0, raw_shift=0.0, raw_dtype=np.float64)
    ll, sa = allele_ref.oracle_front(oracle_port, rb, truth, ref, model, 40, normalise=False)
    key, val = allele_ref.rows(ll, sa.reference, sa.ref_off, sa.ref_start, sa.reverse, None, 1.0, ref.size)
    P, b, D, valid, coverage = allele_ref.sites(key, val, ref)
    got = allele_ref.solve(D, valid)
    top = np.zeros(ref.size)
    np.maximum.at(top, P, got['lrt'])
    near = np.array([max(top[q] for q in range(max(0, p - k + 1), min(top.size, p + k)) if q != p) for p in P])
    n = P.size
    fractions = AlleleFractionBatch(np.zeros(n, np.int32), P, ref[P].astype(np.int8), b.astype(np.int8), coverage[P],
                                    got['fraction'], got['lrt'], got['ll_half'], got['ll_full'], np.zeros(n, np.int8),
                                    near > got['lrt'], np.zeros(n, bool), coverage)
    picked = select_sites(fractions, 200.0, 0.25, 8)
    planted = sorted(zip(SITES_A + SITES_B, list(alts_a) + list(alts_b), [1] * 6 + [2] * 4))
    assert list(zip(P[picked].tolist(), b[picked].tolist())) == [(x, a) for x, a, _ in planted]
    owner = np.array([h for _, _, h in planted])
    site_pos, site_alt = P[picked], b[picked]
    has, E = phase_ref.evidence(key, val, sa.ref_off, sa.ref_start, sa.reverse, site_pos, site_alt, 30.0)
    chain_flag = np.ones(10, dtype=np.int32)
    chain_flag[0] = 0
    res = phase_ref.refine(has, E, chain_flag, 3, 2.0, 2)
    first = int(np.nonzero(site_pos == 800)[0][0])
    assert first == 5 and res['block'].tolist() == [0] * 5 + [5] * 5
    assert res['sigma'].tolist() == np.where(owner == owner[res['block']], 1, -1).tolist()
    hap = info['haplotype'][sa.live]
    tagged = res['haplotype'] > 0
    first_owner = owner[np.maximum(res['read_block'], 0)]
    called = np.where(res['haplotype'] == 1, first_owner, 3 - first_owner)
    right = int((called[tagged] == hap[tagged]).sum())
    joined_links = np.abs(res['link'][res['joined']])
    print('tagged %d of %d reads, %d right; smallest joined |link| %.1f, smallest |vote| %.1f, smallest |llr| %.2f; '
          'flips %r' % (tagged.sum(), rb.n, right, joined_links.min(), np.abs(res['vote']).min(),
                        np.abs(res['read_llr'][tagged]).min(), res['flips_per_round']))
    assert tagged.sum() >= 180
    assert right >= 0.95 * tagged.sum()
