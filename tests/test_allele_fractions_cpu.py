"""CPU-only tests of ``estimate_allele_fractions_batch``: the numpy restatement of its contract (tests/allele_ref.py)
against brute force, the synthetic mixture, the argument checks made before any device call, the new entries of the
C-ABI, and the planted-site experiment through the CPU oracle."""
import io
import os

import numpy as np
import pytest

import allele_ref


def d_vectors():
    """Random d vectors of every kind the kernel meets: mixed signs, all <= 0, all > 0, +-600 and -inf entries, one
    value, values near 0."""
    rng = np.random.default_rng(11)
    out = []
    for trial in range(40):
        n = int(rng.integers(1, 70))
        d = rng.normal(0, 5, n)
        kind = trial % 8
        if kind == 1:
            d = -np.abs(d)
        elif kind == 2:
            d = np.abs(d) + 1e-3
        elif kind == 3:
            d[rng.integers(0, n, 3)] = [600.0, -600.0, -np.inf]
        elif kind == 4:
            d = rng.normal(-3, 10, n)
        elif kind == 5:
            d = rng.normal(0, 1e-3, n)
        elif kind == 6:
            d = np.where(rng.random(n) < 0.3, 289.0, -40.0) + rng.normal(0, 1, n)
        elif kind == 7:
            d = np.full(n, -np.inf)
        out.append(d)
    return out


def test_restatement_against_brute_force():
    vectors = d_vectors()
    D, valid = allele_ref.pad(vectors)
    got = allele_ref.solve(D, valid)
    grid = np.linspace(0.0, 1.0, 10001)
    L_hat = allele_ref.likelihood(got['fraction'], D, valid)
    interior = 0
    for m, d in enumerate(vectors):
        Dm, vm = np.repeat(D[m:m + 1], grid.size, 0), np.repeat(valid[m:m + 1], grid.size, 0)
        L_grid = allele_ref.likelihood(grid, Dm, vm)
        assert L_hat[m] >= np.max(L_grid) - 1e-9, (m, got['fraction'][m], L_hat[m], np.max(L_grid))
        assert got['lrt'][m] == (2.0 * L_hat[m] if got['fraction'][m] > 0 else 0.0)
        assert got['ll_full'][m] == np.cumsum(d)[-1] or (np.isinf(d).any() and got['ll_full'][m] == -np.inf)
        # g does not increase on [0, 1]
        g = allele_ref.derivative(grid[::100], Dm[::100], vm[::100])
        assert (np.diff(g[np.isfinite(g)]) <= 1e-9 * np.abs(g[np.isfinite(g)][:-1]) + 1e-12).all()
        interior += 0 < got['fraction'][m] < 1
    assert interior >= 10


def test_boundary_rules():
    D, valid = allele_ref.pad([np.array([-1.0, -2.0, -0.5]), np.array([3.0, 1.0, 250.0]), np.array([0.0, 0.0]),
                               np.array([-np.inf, -np.inf]), np.array([600.0]), np.array([5.0, -5.0, 5.0, -5.0])])
    got = allele_ref.solve(D, valid)
    assert got['fraction'][:5].tolist() == [0.0, 1.0, 0.0, 0.0, 1.0]
    assert got['lrt'][[0, 2, 3]].tolist() == [0.0, 0.0, 0.0]
    assert got['lrt'][1] == 2.0 * 254.0 and got['lrt'][4] == 1200.0
    assert got['ll_full'][:3].tolist() == [-3.5, 254.0, 0.0] and got['ll_full'][3] == -np.inf
    assert abs(got['fraction'][5] - 0.5) < 1e-12           # symmetric evidence: half the reads
    # g(0) > 0 and g(1) < 0 bracket the root; the estimate is the midpoint of the last bisection interval
    assert got['g0'][5] > 0 > got['g1'][5]
    assert abs(allele_ref.derivative(got['fraction'][5:6], D[5:6], valid[5:6])[0]) < 1e-9


def test_make_mixed_read_batch():
    from nadavca_amd import synthetic
    ref, hap, alts = allele_ref.planted_haplotypes(900, [100, 300, 302, 700], 5)
    assert (hap != ref).sum() == 4 and (hap[[100, 300, 302, 700]] == alts).all()
    rb, truth, info = synthetic.make_mixed_read_batch(400, [ref, hap], [3.0, 1.0], seed=9, length=150, spread=20)
    assert rb.n == 400 and abs((info['haplotype'] == 1).mean() - 0.25) < 0.07
    assert info['reverse'].tolist() == [bool(i % 2) for i in range(400)] and (truth.reverse == info['reverse']).all()
    strands = (ref.astype(np.int64), 3 - ref[::-1].astype(np.int64))
    hap_strands = (hap.astype(np.int64), 3 - hap[::-1].astype(np.int64))
    missing = 0
    for i in range(rb.n):
        seq = rb.sequence[rb.seq_off[i]:rb.seq_off[i + 1]]
        rev, x0, h = bool(info['reverse'][i]), int(info['start'][i]), int(info['haplotype'][i])
        own = (strands, hap_strands)[h][rev][x0:x0 + seq.size]
        assert np.array_equal(seq, own)
        ri, xi = (a[truth.off[i]:truth.off[i + 1]] for a in (truth.read_idx, truth.ref_idx))
        # a pair wherever the read equals the first haplotype, and only there
        same = np.nonzero(seq == strands[rev][x0:x0 + seq.size])[0]
        assert np.array_equal(ri, same) and np.array_equal(xi, x0 + same)
        assert h == 1 or same.size == seq.size
        missing += seq.size - same.size
        assert rb.sig_off[i + 1] - rb.sig_off[i] >= 3 * seq.size
    assert missing > 0
    again = synthetic.make_mixed_read_batch(400, [ref, hap], [3.0, 1.0], seed=9, length=150, spread=20)[0]
    assert np.array_equal(again.raw_signal, rb.raw_signal)
    fwd = synthetic.make_mixed_read_batch(10, [ref, hap], [1, 1], seed=9, length=150, both_strands=False)[2]
    assert not fwd['reverse'].any()
    with pytest.raises(ValueError):
        synthetic.make_mixed_read_batch(4, [ref, hap[:-1]], [1, 1])
    with pytest.raises(ValueError):
        synthetic.make_mixed_read_batch(4, [ref, hap], [1.0])


def test_argument_errors_before_any_device_call():
    from nadavca_amd import estimate_allele_fractions_batch

    class Model:   # (never reaches a kernel: the checks come first)
        alphabet_size = 4

    class Model5:
        alphabet_size = 5
    ref = np.zeros(50, dtype=np.int32)
    call = lambda **kw: estimate_allele_fractions_batch(ref, None, config={}, **{**dict(kmer_model=Model(),
                                                                                         aligner=object()), **kw})
    for kw in (dict(kmer_model=Model5()), dict(keep='called'), dict(keep=None), dict(event_length=-1.0),
               dict(event_length=0.0), dict(event_length=float('nan')), dict(event_length=float('inf')),
               dict(min_fraction=1.5), dict(min_coverage=-1), dict(min_coverage=1.5), dict(threshold=float('nan')),
               dict(aligner=None)):
        with pytest.raises(ValueError):
            call(**kw)


def test_result_table_and_tsv(tmp_path):
    from nadavca_amd.allele_fractions import AlleleFractionBatch
    z = AlleleFractionBatch.empty(7, 3.0, ['a'])
    assert len(z) == 0 and z.position_coverage.tolist() == [0] * 7 and z.called.size == 0
    b = AlleleFractionBatch(np.array([0, 1], np.int32), np.array([5, 2]), np.array([0, 3], np.int8),
                            np.array([2, 1], np.int8), np.array([30, 4]), np.array([0.25, 1.0]),
                            np.array([12.5, 80.0]), np.array([-3.0, 20.0]), np.array([-50.0, 40.0]),
                            np.array([0, 2], np.int8), np.array([False, True]), np.array([True, False]),
                            np.zeros(9, np.int64), 10.0, ['chrA', 'chrB'])
    buf = io.StringIO(newline='')
    b.write_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0].split('\t') == ['contig', 'position', 'ref', 'alt', 'coverage', 'fraction', 'lrt', 'll_half',
                                    'll_full', 'genotype', 'shadowed', 'called']
    assert lines[1] == 'chrA\t5\tA\tG\t30\t0.25\t12.5\t-3.0\t-50.0\t0\t0\t1'
    assert lines[2] == 'chrB\t2\tT\tC\t4\t1.0\t80.0\t20.0\t40.0\t2\t1\t0' and lines[3] == ''
    path = os.path.join(str(tmp_path), 'f.tsv')
    b.write_tsv(path)
    assert open(path).read() == buf.getvalue()


def test_neighbour_max():
    import torch
    from nadavca_amd.allele_fractions import neighbour_max
    best = torch.tensor([1.0, 5.0, 2.0, 0.0, 0.0, 0.0, 9.0, 0.0], dtype=torch.float64)
    ninf = float('-inf')
    assert neighbour_max(best, None, 2).tolist() == [5.0, 2.0, 5.0, 5.0, 9.0, 9.0, 0.0, 9.0]
    contig = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2])
    assert neighbour_max(best, contig, 2).tolist() == [5.0, 2.0, 5.0, 5.0, 9.0, 9.0, 0.0, ninf]
    assert neighbour_max(best[:1], None, 5).tolist() == [ninf]
    # against a loop
    rng = np.random.default_rng(2)
    x, c = rng.normal(size=40), np.sort(rng.integers(0, 3, 40))
    want = [max([x[j] for j in range(40) if j != i and abs(j - i) <= 5 and c[j] == c[i]], default=ninf)
            for i in range(40)]
    assert neighbour_max(torch.from_numpy(x), torch.from_numpy(c), 5).tolist() == want


def test_new_entries_declared_bound_and_exported():
    from conftest import ROOT
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    lib = _lib.load()
    for name in ('nvk_allele_rows_dev', 'nvk_allele_solve_dev'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'NVK_K_ALLELE = %d' % _lib.K_ALLELE in header and _lib.KERNEL_NAMES[_lib.K_ALLELE] == 'allele'
    assert 'NVK_K_COUNT = %d' % len(_lib.KERNEL_NAMES) in header
    assert callable(device.allele_fractions_dev)


def test_planted_sites_on_the_oracle(oracle_port):
    """The planted-site experiment at divisor 1 through the CPU oracle: the packaged 6-mer table, a 600-base genome,
    7 substitutions on a second haplotype (two of them 2 bases apart), 150 forward reads of 120 bases drawn from either
    haplotype with probability 0.5, signals in the table's own units (no normalisation), anchors on 75 % of the true
    bases moved by up to 20 samples, bandwidth 40, wobbling on.
    Observed with seed 4: coverage 17 .. 52 at the planted sites, largest |fraction - realised| 0.039, smallest planted
    lrt 630.5, largest lrt more than k - 1 = 5 positions from every planted site 44.5 (1 563 such rows), 3 of the 7
    planted bases with a NEGATIVE summed ratio (the haploid consensus does not see them).  Seed 2 gave 0.056 / 403.1 /
    71.6.  Seeds 1, 3 and 5 miss the 0.1 bound at the two sites that lie 2 bases apart (0.12, 0.38, 0.51; every other
    site within 0.04): hypotheses of one substitution each cannot explain a haplotype that carries two inside one
    k-mer, and how much that costs depends on the levels of the k-mers drawn."""
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    planted = [80, 150, 152, 260, 350, 440, 520]
    ref, hap, alts = allele_ref.planted_haplotypes(600, planted, 4)
    rb, truth, info = synthetic.make_mixed_read_batch(150, [ref, hap], [0.5, 0.5], seed=4, model=model, length=120,
                                                      spread=0, anchor_density=0.75, jitter=20, both_strands=False,
                                                      raw_scale=1.0, raw_shift=0.0, raw_dtype=np.float64)
    ll, sa = allele_ref.oracle_front(oracle_port, rb, truth, ref, model, 40, normalise=False)
    assert sa.live.size == 150
    key, val = allele_ref.rows(ll, sa.reference, sa.ref_off, sa.ref_start, sa.reverse, None, 1.0, ref.size)
    dropped = np.array([key[sa.ref_off[j]] < 0 for j in range(sa.live.size)])
    P, b, D, valid, coverage = allele_ref.sites(key, val, ref)
    got = allele_ref.solve(D, valid)
    realised = [allele_ref.realised_share(x, sa, dropped, info['haplotype'][sa.live])[0] for x in planted]
    assert min(coverage[planted]) >= 8
    allele_ref.planted_check(P, b, got['fraction'], got['lrt'], planted, alts, realised, model[0])
    negative = sum(got['ll_full'][(P == x) & (b == a)][0] < 0 for x, a in zip(planted, alts))
    print('planted bases with a negative summed ratio: %d of %d' % (negative, len(planted)))
