"""CPU tests of ``phase_mods``: the numpy restatement of nvk_mod_site_solve_dev on constructed sites, and the real host
code of the workflow (``phase_mods_of_rows``: torch on the CPU) run with that restatement as its ``solve``."""
import io
import os

import numpy as np
import pytest

import allele_ref
import mod_sites_ref

CLIP = 30.0


def numpy_solve(site_lo, site_hi, val, group, set_mask, clip):
    """The ``solve`` of ``phase_mods_of_rows`` on the restatement."""
    return mod_sites_ref.solve(site_lo.cpu().numpy(), site_hi.cpu().numpy(), val.cpu().numpy(),
                               None if group is None else group.cpu().numpy(), set_mask, clip)


def make_mods(read, contig, position, strand, llr, names=None):
    from nadavca_amd.call_mods import ModCallBatch
    n = len(read)
    z = np.zeros(0)
    return ModCallBatch(np.asarray(read, dtype=np.int64), np.asarray(contig, dtype=np.int32),
                        np.asarray(position, dtype=np.int64), np.asarray(strand, dtype=np.int8),
                        np.asarray(llr, dtype=np.float64), np.zeros(n, dtype=bool), z.astype(np.int32),
                        z.astype(np.int64), z, names)


def make_phase(haplotype, phase_set, contig=None, site_contig=(), site_position=()):
    """A PhaseBatch with the given per-read tags and (for ``near_variant``) phased sites."""
    from nadavca_amd.phase import PhaseBatch
    haplotype = np.asarray(haplotype, dtype=np.int8)
    ph = PhaseBatch.empty(haplotype.size)
    ph.haplotype = haplotype
    ph.read_phase_set = np.asarray(phase_set, dtype=np.int64)
    ph.read_contig = np.where(ph.read_phase_set >= 0, 0, -1).astype(np.int32) if contig is None else \
        np.asarray(contig, dtype=np.int32)
    ph.contig = np.asarray(site_contig, dtype=np.int32)
    ph.position = np.asarray(site_position, dtype=np.int64)
    return ph


def run(mods, phase, k=6, **kw):
    from nadavca_amd.phase_mods import phase_mods_of_rows
    return phase_mods_of_rows(mods, phase, numpy_solve, k, **kw)


# ---- (a) the restatement on constructed sites -----------------------------------------------------------------------
def test_restatement_on_constructed_sites():
    rng = np.random.default_rng(11)
    mixed = np.concatenate([rng.normal(6, 2.5, 9), -rng.normal(6, 2.5, 5)])
    val = np.concatenate([np.full(7, CLIP), np.full(6, -CLIP), mixed, -mixed])
    lo, hi = np.array([0, 7, 13, 27]), np.array([7, 13, 27, 41])
    count, f, ll = mod_sites_ref.solve(lo, hi, val, None, (1,), CLIP)
    assert count[:, 0].tolist() == [7, 6, 14, 14]
    assert f[0, 0] == 1.0 and ll[0, 0] == 7 * CLIP          # all +clip: f^ = 1, L(1) = the sum
    assert f[1, 0] == 0.0 and ll[1, 0] == 0.0               # all -clip: f^ = 0, L(0) = 0
    assert 0.5 < f[2, 0] < 0.8 and abs(f[2, 0] + f[3, 0] - 1.0) <= 1e-9      # the mirror image gives 1 - f^
    # L of the mirror image: L(1 - f; -d) = L(f; d) - sum d
    assert abs(ll[3, 0] - (ll[2, 0] - mixed.sum())) <= 1e-9 * (1 + abs(ll[2, 0]))
    # at the estimate the likelihood is the restated t summed in row order
    assert abs(ll[2, 0] - allele_ref.t_term(f[2, 0], mixed).sum()) <= 1e-9 * (1 + abs(ll[2, 0]))


def test_restatement_masks_nan_groups_and_infinities():
    val = np.array([5.0, -4.0, 7.0, np.nan, 3.0, -6.0, np.inf, -np.inf, 2.0, 1.0])
    group = np.array([0, 1, 2, 1, 1, 2, 1, 2, 32, -1], dtype=np.int32)
    lo, hi = np.array([0]), np.array([10])
    count, f, ll = mod_sites_ref.solve(lo, hi, val, group, mod_sites_ref.MASKS, CLIP)
    # NaN (row 3) and the groups 32 and -1 (rows 8, 9) are in no set
    assert count[0].tolist() == [7, 3, 3, 6]
    vec = mod_sites_ref.site_vectors(lo, hi, val, group, mod_sites_ref.MASKS, CLIP)
    assert vec[0].tolist() == [5.0, -4.0, 7.0, 3.0, -6.0, CLIP, -CLIP]          # row order kept, +-inf clipped
    assert vec[1].tolist() == [-4.0, 3.0, CLIP] and vec[2].tolist() == [7.0, -6.0, -CLIP]
    assert vec[3].tolist() == [-4.0, 7.0, 3.0, -6.0, CLIP, -CLIP]
    for q in range(4):
        one = mod_sites_ref.solve(np.array([0]), np.array([vec[q].size]), vec[q], None, (1,), CLIP)
        assert one[1][0, 0] == f[0, q] and one[2][0, 0] == ll[0, q]
    # bit 31 is a group like any other; an empty mask is an empty set
    g31 = np.full(10, 31, dtype=np.int32)
    c31 = mod_sites_ref.solve(lo, hi, val, g31, (1 << 31, 0, 0xffffffff), CLIP)
    assert c31[0][0].tolist() == [9, 0, 9] and c31[1][0, 1] == 0.0 and c31[2][0, 1] == 0.0
    assert c31[1][0, 0] == c31[1][0, 2]
    # a smaller clip changes the values, not the membership
    tight = mod_sites_ref.solve(lo, hi, val, group, mod_sites_ref.MASKS, 2.5)
    assert tight[0][0].tolist() == [7, 3, 3, 6]
    assert np.abs(mod_sites_ref.site_vectors(lo, hi, val, group, (0b111,), 2.5)[0]).max() == 2.5


# ---- (b) the sites, their order and their rows are site_table's -----------------------------------------------------
def random_batches(seed, n_rows=400, n_reads=30):
    rng = np.random.default_rng(seed)
    read = rng.integers(0, n_reads, n_rows)
    mods = make_mods(read, rng.integers(0, 3, n_rows), rng.integers(0, 25, n_rows) * 3, rng.integers(0, 2, n_rows),
                     np.where(rng.random(n_rows) < 0.5, 1, -1) * rng.normal(6, 2.5, n_rows), names=['a', 'b', 'c'])
    hap = rng.integers(0, 3, n_reads)
    ps = np.where(hap > 0, rng.choice([10, 40, 70], n_reads), -1)
    rc = np.where(hap > 0, rng.integers(0, 3, n_reads), -1)
    return mods, make_phase(hap, ps, rc, [0, 1, 1, 2], [12, 3, 40, 71])


def test_sites_order_and_reads_are_site_tables():
    for seed in (1, 2):
        mods, phase = random_batches(seed)
        got, table = run(mods, phase), mods.site_table()
        assert len(got) == table['position'].size > 50
        for name in ('contig', 'position', 'strand', 'reads'):
            assert np.array_equal(getattr(got, name), table[name]), name
            assert getattr(got, name).dtype == table[name].dtype, name
        assert got.contig_names == ['a', 'b', 'c'] and got.mods is mods and got.phase is phase
        assert np.array_equal(got.n_h1 + got.n_h2 + got.n_untagged, got.reads)


# ---- (c) the phase-set rule -----------------------------------------------------------------------------------------
def test_phase_set_rule_by_hand():
    #        read: 0  1  2  3  4  5  6  7
    hap = [1, 2, 1, 2, 1, 0, 2, 1]
    ps = [100, 100, 300, 300, 300, -1, 100, 300]
    phase = make_phase(hap, ps)
    rows = [(0, 50), (1, 50), (2, 50), (3, 50), (4, 50), (5, 50),       # site 50: 2 rows of set 100, 3 of 300
            (0, 60), (1, 60), (2, 60), (3, 60), (5, 60),                # site 60: 2 and 2 -> the smaller, 100
            (5, 70)]                                                     # site 70: no tagged row
    mods = make_mods([r for r, _ in rows], [0] * len(rows), [p for _, p in rows], [0] * len(rows),
                     np.linspace(-8, 8, len(rows)))
    got = run(mods, phase)
    assert got.position.tolist() == [50, 60, 70] and got.phase_set.tolist() == [300, 100, -1]
    # site 50: reads 2 and 4 are haplotype 1 of set 300, read 3 haplotype 2; reads 0 and 1 are tagged ELSEWHERE
    assert (got.n_h1.tolist(), got.n_h2.tolist(), got.n_untagged.tolist()) == ([2, 1, 0], [1, 1, 0], [3, 3, 1])
    assert got.reads.tolist() == [6, 5, 1]
    assert np.isnan(got.asm_lrt).all() and np.isnan(got.p).all()     # below min_tagged = 4 everywhere


def test_phase_set_rule_against_the_per_site_loop():
    import torch
    from nadavca_amd.phase_mods import site_phase_sets, site_ranges
    for seed in (3, 4, 5):
        mods, phase = random_batches(seed)
        order, lo, hi, site_of = site_ranges(mods, torch.device('cpu'))
        site_ps, group = site_phase_sets(order, site_of, int(lo.numel()), mods, phase, torch.device('cpu'))
        r_order, r_lo, r_hi, r_ps, r_group = mod_sites_ref.phase_sets(mods, phase)
        assert np.array_equal(order.numpy(), r_order) and np.array_equal(lo.numpy(), r_lo)
        assert np.array_equal(hi.numpy(), r_hi)
        assert np.array_equal(site_ps.numpy(), r_ps) and np.array_equal(group.numpy(), r_group)
        assert group.dtype == torch.int32 and (r_ps >= 0).sum() > 20 and len(set(r_group.tolist())) == 3
        # a read tagged on another contig than the row's counts as untagged
        assert ((phase.read_contig[mods.read[r_order]] != mods.contig[r_order]) & (r_group == 0)).any()


# ---- (d) gating and flags -------------------------------------------------------------------------------------------
def two_haplotype_site(position, v1, v2):
    """Rows of one site: reads 0 .. len(v1)-1 of haplotype 1, then those of haplotype 2, interleaved in read order."""
    n1, n2 = len(v1), len(v2)
    return ([(r, position, v) for r, v in enumerate(v1)] + [(100 + r, position, v) for r, v in enumerate(v2)], n1, n2)


def test_gating_and_flags():
    rng = np.random.default_rng(5)
    mixed = np.concatenate([rng.normal(6, 2.5, 6), -rng.normal(6, 2.5, 4)])
    sites = [two_haplotype_site(10, np.full(5, 9.0), np.full(5, 9.0)),          # the same rows, f^ = 1
             two_haplotype_site(30, np.full(5, -7.0), np.full(5, -7.0)),        # the same rows, f^ = 0
             two_haplotype_site(50, mixed, mixed),                              # the same rows, 0 < f^ < 1
             two_haplotype_site(70, np.abs(mixed), -np.abs(mixed)),             # all against none
             two_haplotype_site(90, mixed[:3], mixed),                          # 3 rows of haplotype 1
             two_haplotype_site(110, mixed, mixed[:4])]                          # 4 rows of haplotype 2: enough
    rows = sorted((r, p, v) for s, _, _ in sites for r, p, v in s)
    hap = np.zeros(200, dtype=np.int8)
    hap[:100], hap[100:] = 1, 2
    k = 6
    phase = make_phase(hap, np.zeros(200), None, [0, 0, 0], [10 + k - 1, 70 - k, 107])
    mods = make_mods([r for r, _, _ in rows], [0] * len(rows), [p for _, p, _ in rows], [0] * len(rows),
                     [v for _, _, v in rows])
    got = run(mods, phase, k=k)
    assert got.position.tolist() == [10, 30, 50, 70, 90, 110] and (got.phase_set == 0).all()
    assert got.n_h1.tolist() == [5, 5, 10, 10, 3, 10] and got.n_h2.tolist() == [5, 5, 10, 10, 10, 4]
    ok = ~np.isnan(got.asm_lrt)
    assert ok.tolist() == [True, True, True, True, False, True] and np.array_equal(np.isnan(got.p), ~ok)
    assert (got.asm_lrt[ok] >= 0).all() and ((got.p[ok] >= 0) & (got.p[ok] <= 1)).all()
    # f^ = 1 and f^ = 0 in all sets: every L is an exact sum (of the values, or of nothing), so the contrast is 0
    # exactly.  With 0 < f^ < 1 the pooled sums run in another order than the two halves and agree only to rounding.
    assert got.asm_lrt[0] == 0.0 and got.asm_lrt[1] == 0.0 and got.p[0] == 1.0 and got.p[1] == 1.0
    assert got.asm_lrt[2] <= 1e-9 and got.delta[2] == 0.0 and got.fraction_h1[2] == got.fraction_h2[2]
    assert got.fraction_h1[3] == 1.0 and got.fraction_h2[3] == 0.0 and got.delta[3] == 1.0
    assert got.asm_lrt[3] > 20 and got.p[3] < 1e-5 and abs(got.fraction_tagged[3] - 0.5) < 1e-6
    from scipy.special import chdtrc
    assert np.array_equal(got.p[ok], chdtrc(1.0, got.asm_lrt[ok]))
    # min_tagged moves the gate; 0 opens it everywhere
    assert (~np.isnan(run(mods, phase, k=k, min_tagged=3).asm_lrt)).all()
    assert (~np.isnan(run(mods, phase, k=k, min_tagged=11).asm_lrt)).sum() == 0
    # near_variant: a phased site at distance k - 1 counts, at k it does not (64 and 70); 107 is within 5 of 110
    assert got.near_variant.tolist() == [True, False, False, False, False, True]
    other = make_phase(hap, np.zeros(200), None, [1], [10])                    # another contig: never near
    assert not run(mods, other, k=k).near_variant.any()
    with pytest.raises(ValueError):
        run(mods, phase, clip=float('inf'))


def test_empty_batches_and_tsv():
    from nadavca_amd.call_mods import ModCallBatch
    from nadavca_amd.phase import PhaseBatch
    got = run(ModCallBatch.empty(), PhaseBatch.empty(5))
    assert len(got) == 0 and got.p.dtype == np.float64 and got.reads.dtype == np.int64
    assert got.near_variant.dtype == bool
    # rows but no tagged read: every site untagged, no contrast
    mods = make_mods([0, 1, 2, 0], [0] * 4, [7, 7, 7, 9], [1, 1, 1, 0], [4.0, -3.0, 5.0, -np.inf])
    got = run(mods, PhaseBatch.empty(3))
    assert got.phase_set.tolist() == [-1, -1] and got.n_untagged.tolist() == [3, 1] and np.isnan(got.p).all()
    assert got.fraction_h1.tolist() == [0.0, 0.0] and got.fraction[1] == 0.0 and got.lrt[1] == 0.0
    text = io.StringIO()
    got.write_tsv(text)
    lines = text.getvalue().splitlines()
    assert lines[0].split('\t')[:5] == ['contig', 'position', 'strand', 'phase_set', 'reads'] and len(lines) == 3
    assert lines[1].split('\t')[:8] == ['0', '7', '-', '-1', '3', '0', '0', '3']
    assert len(lines[1].split('\t')) == len(lines[0].split('\t')) == 17 and lines[2].split('\t')[-2] == 'nan'
    assert float(lines[1].split('\t')[8]) == got.fraction[0]


# ---- (f) mod_site_frequencies on a hand-made batch ---------------------------------------------------------------------
def test_mod_site_frequencies_against_the_restatement():
    from nadavca_amd.call_mods import ModCallBatch
    from nadavca_amd.phase_mods import mod_site_frequencies_of_rows
    mods, _ = random_batches(6)
    mods.llr[[3, 50, 51]] = [np.nan, np.inf, -np.inf]
    got = mod_site_frequencies_of_rows(mods, numpy_solve, clip=12.0)
    table = mods.site_table()
    for name in ('contig', 'position', 'strand'):
        assert np.array_equal(got[name], table[name]) and got[name].dtype == table[name].dtype, name
    # per site by hand: the rows in batch order, NaN dropped, clipped, solved alone
    assert int((table['reads'] - got['reads']).sum()) == 1 and got['reads'].dtype == np.int64
    for s in range(table['position'].size):
        rows = (mods.contig == got['contig'][s]) & (mods.position == got['position'][s]) & (mods.strand == got['strand'][s])
        v = mods.llr[rows]
        v = np.clip(v[~np.isnan(v)], -12.0, 12.0)
        ref = allele_ref.solve(*allele_ref.pad([v]))
        assert got['reads'][s] == v.size and got['fraction'][s] == ref['fraction'][0] and got['lrt'][s] == ref['lrt'][0]
    assert ((got['fraction'] > 0) & (got['fraction'] < 1)).sum() > 20
    wide = mod_site_frequencies_of_rows(mods, numpy_solve)
    assert np.array_equal(wide['reads'], got['reads']) and not np.array_equal(wide['lrt'], got['lrt'])
    empty = mod_site_frequencies_of_rows(ModCallBatch.empty(), numpy_solve)
    assert all(empty[name].size == 0 for name in ('contig', 'position', 'strand', 'reads', 'fraction', 'lrt'))
    with pytest.raises(ValueError):
        mod_site_frequencies_of_rows(mods, numpy_solve, clip=0.0)


# ---- (e) the simulation behind the p-value's description ------------------------------------------------------------
def simulated(rng, n_sites, per_hap, f1, f2):
    """``n_sites`` sites of ``per_hap`` rows per haplotype: a row of haplotype h is modified with probability f_h and
    its ratio is +N(6, 2.5^2) when modified, -N(6, 2.5^2) otherwise (clipped at 30 by the operator)."""
    n = 2 * per_hap
    size = rng.normal(6.0, 2.5, (n_sites, n))
    share = np.where(np.arange(n) < per_hap, f1, f2)
    llr = np.where(rng.random((n_sites, n)) < share, size, -size)
    hap = np.where(np.arange(n) < per_hap, 1, 2)
    mods = make_mods(np.tile(np.arange(n), n_sites), np.zeros(n_sites * n), np.repeat(np.arange(n_sites), n),
                     np.zeros(n_sites * n), llr.reshape(-1))
    return run(mods, make_phase(hap, np.zeros(n)))


@pytest.mark.parametrize('per_hap', [10, 20])
def test_null_sites_keep_the_level(per_hap):
    got = simulated(np.random.default_rng([20261020, per_hap]), 4000, per_hap, 0.5, 0.5)
    share = [float((got.p <= a).mean()) for a in (0.05, 0.01, 0.001)]
    print('null, %d rows per haplotype: p <= 0.05 / 0.01 / 0.001 on %.4f / %.4f / %.4f of 4000 sites'
          % ((per_hap,) + tuple(share)))
    assert not np.isnan(got.p).any() and (got.asm_lrt >= 0).all()
    assert share[1] <= 0.025


def test_planted_contrast_is_found():
    got = simulated(np.random.default_rng([20261020, 3]), 2000, 10, 0.95, 0.05)
    found = float((got.p <= 0.001).mean())
    print('planted 0.95 / 0.05, 10 rows per haplotype: p <= 0.001 on %.4f of 2000 sites' % found)
    assert found >= 0.90
    assert ((got.fraction_h1 > 0.5) & (got.fraction_h2 < 0.5)).all()


# ---- the C-ABI entry and the synthetic batch ------------------------------------------------------------------------
def test_abi_declares_the_operator():
    import ctypes as C
    from nadavca_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'nadavca_hip.h')).read()
    name = 'nvk_mod_site_solve_dev'
    res, args = _lib.SIGNATURES[name]
    assert name + '(' in header and hasattr(_lib.load(), name)
    assert res is C.c_int and len(args) == 13 and args[7] is C.c_int and args[9] is C.c_double
    assert 'NVK_K_COUNT = 13' in header and len(_lib.KERNEL_NAMES) == 13      # timed under NVK_K_ALLELE: no new id


def test_phased_modified_read_batch():
    from nadavca_amd import synthetic
    from nadavca_amd.kmer_train import extend_kmer_model
    model = synthetic.load_model_arrays()
    k, central, _, mean, sigma = model
    mean5, sigma5 = extend_kmer_model(k, central, mean, sigma)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
    model5 = (k, central, 5, mean5 + 1.5 * has_m, sigma5)      # every k-mer with an M: its C k-mer's level + 1.5
    hap0 = np.random.default_rng(2).integers(0, 4, 600)
    cg = list(range(20, 560, 60))
    for x in cg:
        hap0[x:x + 2] = [1, 2]
    hap1, hap2 = hap0.copy(), hap0.copy()
    hap1[305] = (hap1[305] + 1) % 4
    hap2[125] = (hap2[125] + 2) % 4
    mod = [[], [cg[0], cg[2]], [cg[2], cg[4]]]
    args = dict(seed=4, length=150, spread=10, raw_dtype=np.float64, noise=0.0)
    rb, truth, info = synthetic.make_phased_modified_read_batch(60, [hap0, hap1, hap2], [0, .5, .5], mod, model5, **args)
    plain, truth0, info0 = synthetic.make_mixed_read_batch(60, [hap0, hap1, hap2], [0, .5, .5], model=model, **args)
    # the reads, their canonical sequences and their pairs are make_mixed_read_batch's; only the signal moves, and only
    # where a k-mer of the read's own strand holds a base that is modified on the read's haplotype
    for name in ('haplotype', 'reverse', 'start'):
        assert np.array_equal(info[name], info0[name]), name
    assert set(info['haplotype'].tolist()) == {1, 2} and info['reverse'].any() and not info['reverse'].all()
    assert np.array_equal(rb.sequence, plain.sequence) and rb.sequence.max() <= 3
    assert np.array_equal(rb.sig_off, plain.sig_off) and np.array_equal(rb.map_sig, plain.map_sig)
    assert np.array_equal(truth.read_idx, truth0.read_idx) and np.array_equal(truth.ref_idx, truth0.ref_idx)
    G, changed = hap0.size, 0
    for i in range(60):
        h, rev, x0 = int(info['haplotype'][i]), bool(info['reverse'][i]), int(info['start'][i])
        L = int(rb.seq_off[i + 1] - rb.seq_off[i])
        # strand coordinates of the bases modified on this read's strand: the C at forward x, or the C paired with the
        # G at forward x + 1
        at = [G - 1 - (x + 1) if rev else x for x in mod[h]]
        # the k-mer of read base j covers j - central .. j - central + k - 1
        seen = [y for y in at if x0 - (k - 1 - central) <= y < x0 + L + central]
        a, b = (r.raw_signal[r.sig_off[i]:r.sig_off[i + 1]] for r in (rb, plain))
        assert bool((a != b).any()) == bool(seen), (i, h, rev, seen)
        if seen:
            # the first sample that moves belongs to the first base whose k-mer holds the modified base
            dw = np.nonzero(a != b)[0]
            seq = rb.sequence[rb.seq_off[i]:rb.seq_off[i + 1]]
            assert all(seq[y - x0] == 1 for y in seen if x0 <= y < x0 + L)      # it is a C of the canonical read
            assert np.allclose((a - b)[dw] / 12.0, np.round((a - b)[dw] / 12.0 / 1.5) * 1.5, atol=1e-9)
        changed += bool(seen)
    assert changed >= 10
    with pytest.raises(ValueError):
        synthetic.make_phased_modified_read_batch(2, [hap0], [1.0], [[5]], model5, seed=1)   # no CG at 5
    with pytest.raises(ValueError):
        synthetic.make_phased_modified_read_batch(2, [hap0], [1.0], [[]], model5, seed=1, pattern='CA')
    with pytest.raises(ValueError):
        synthetic.make_phased_modified_read_batch(2, [hap0], [1.0], [[]], model, seed=1)     # a 4-letter table
