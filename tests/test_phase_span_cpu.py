"""CPU-only tests of ``phase_reads_batch(span=...)``: the numpy restatement of the span contract
(tests/phase_span_ref.py) against ``phase_ref.refine`` at span 1, the weak-site case in which today's chain cuts a block
and the span forest does not, ``device.phase_forest`` (torch on CPU tensors) against the sequential ``forest``, the tie
rules, the argument checks made before any device call, the new fields of ``PhaseBatch`` with both forms of the TSV,
and the new entries of the C-ABI."""
import io
import os

import numpy as np
import pytest

import phase_ref
import phase_span_ref
from phase_span_ref import first_of_chain, forest, refine_span, span_links, tag_blocks, weak_site_case


def random_case(seed, S=8, n=40):
    rng = np.random.default_rng(seed)
    truth = np.where(rng.random(S) < 0.5, 1, -1)
    hap = np.where(rng.random(n) < 0.5, 1, -1)
    first = rng.integers(0, S - 1, n)
    cols = np.arange(S)[None, :]
    has = (cols >= first[:, None]) & (cols <= first[:, None] + rng.integers(0, 4, n)[:, None])
    has &= rng.random((n, S)) < 0.9
    E = np.where(has, hap[:, None] * truth[None, :] * 4.0 + rng.normal(0, 3.0, (n, S)), 0.0)
    chain_flag = np.array([0] + [1] * (S - 1), dtype=np.int32)
    chain_flag[5] = 0
    return has, E, chain_flag


def test_span_one_is_the_chain():
    cases = [phase_ref.refinement_case() + (np.array([0, 1, 1], dtype=np.int32),), random_case(21)]
    for has, E, chain_flag in cases:
        want = phase_ref.refine(has, E, chain_flag, 3, 2.0, 2)
        got = refine_span(has, E, first_of_chain(chain_flag), 3, 2.0, 2, 1)
        for k, v in want.items():
            if k == 'margins':
                assert {m: got[k][m] for m in v} == v and got[k]['choice'] == np.inf
            else:
                assert np.array_equal(got[k], v) and np.asarray(got[k]).dtype == np.asarray(v).dtype, k
        assert got['span_link'].shape == (has.shape[1], 1) and np.array_equal(got['span_link'][:, 0], want['link'])
        S = has.shape[1]
        assert np.array_equal(got['parent'], np.where(want['joined'], np.arange(S) - 1, -1))
    assert (cases[1][0].sum(axis=0) > 0).all() and np.unique(got['block']).size > 1 and got['joined'].sum() >= 3


def test_weak_site_and_decoy():
    """Six sites, site 2 with evidence +-0.01 and a decoy at site 4: the chain cuts at 2 and at 3, the forest of span 3
    joins 0, 1, 3 and 5 (and the decoy) and leaves the weak site a singleton inside the block."""
    has, E, truth = weak_site_case()
    chain_flag = np.array([0, 1, 1, 1, 1, 1], dtype=np.int32)
    real = [0, 1, 2, 3, 5]
    old = phase_ref.refine(has, E, chain_flag, 3, 2.0, 2)
    assert old['block'].tolist() == [0, 0, 2, 3, 3, 3] and np.unique(old['block'][real]).size >= 3
    new = refine_span(has, E, first_of_chain(chain_flag), 3, 2.0, 2, 3)
    assert new['block'].tolist() == [0, 0, 2, 0, 0, 0] and new['parent'].tolist() == [-1, 0, -1, 1, 3, 3]
    strong = [0, 1, 3, 5]
    assert new['sigma'][strong].tolist() == truth[strong].tolist() and new['sigma'][2] == 1
    assert abs(new['span_link'][2]).max() < 1.0 and abs(new['span_link'][3, 0]) < 1.0
    assert abs(new['span_link'][3, 1]) > 2.0
    assert min(new['margins'].values()) > 1e-6
    assert phase_ref.phasing_likelihood(has, E, new['sigma']) >= phase_ref.phasing_likelihood(has, E, old['sigma'])
    # every read is tagged in the big block unless the weak site is all it has
    assert (new['read_block'][has[:, strong].any(axis=1)] == 0).all()
    # span 2 reaches across the weak site but site 5 can see the decoy and site 3 only: the same roots
    assert refine_span(has, E, first_of_chain(chain_flag), 3, 2.0, 2, 2)['block'].tolist() == [0, 0, 2, 0, 0, 0]


def forest_triple(rng, S, span, mode):
    """A seeded (link, shared, site_first) for ``phase_forest``: 'ties' draws |link| from a few values, 'path' makes
    every site a qualifying child so that one path runs through the whole array."""
    if mode == 'path':
        link = rng.choice([-1.0, 1.0], (S, span)) * rng.uniform(3.0, 9.0, (S, span))
        shared = np.full((S, span), 5, dtype=np.int64)
        link[:, 1:] *= rng.random((S, max(span - 1, 0))) < 0.3             # mostly the previous site: a long path
        site_first = np.zeros(S, dtype=np.int64)
        return link, shared, site_first
    if mode == 'ties':
        link = rng.choice([-4.0, -2.0, 0.0, 2.0, 4.0, 1.5], (S, span))
    else:
        link = np.round(rng.normal(0, 4, (S, span)), 1)
    shared = rng.integers(0, 8, (S, span))
    chain_flag = (rng.random(S) < 0.85).astype(np.int32)
    return link, shared, first_of_chain(chain_flag)


def test_phase_forest_on_cpu_tensors():
    import torch
    from nadavca_amd.device import phase_blocks, phase_forest
    rng = np.random.default_rng(17)
    seen = dict(tie=0, start_inside=0, negative=0, deep=0, trials=0)
    sizes = [(S, span) for S in (0, 1, 2, 9, 70) for span in (1, 2, 3, 8)]
    for trial in range(200):
        S, span = sizes[trial % len(sizes)]
        mode = ('plain', 'ties', 'path')[(trial // len(sizes)) % 3]
        link, shared, site_first = forest_triple(rng, S, span, mode)
        parent, block, sigma, margins = forest(link, shared, site_first, 3, 2.0)
        got = phase_forest(torch.from_numpy(link), torch.from_numpy(shared), torch.from_numpy(site_first), 3, 2.0)
        assert [t.dtype for t in got] == [torch.int64, torch.int64, torch.int32]
        assert got[0].tolist() == parent.tolist(), (trial, S, span, mode)
        assert got[1].tolist() == block.tolist() and got[2].tolist() == sigma.tolist(), (trial, S, span, mode)
        seen['trials'] += 1
        seen['tie'] += margins['choice'] == 0.0
        seen['start_inside'] += bool(((np.arange(S) - site_first > 0) & (np.arange(S) - site_first < span)).any())
        seen['negative'] += bool((sigma < 0).any())
        depth = np.zeros(S, dtype=np.int64)
        for s in range(S):
            depth[s] = depth[parent[s]] + 1 if parent[s] >= 0 else 0
        seen['deep'] += bool(S and depth.max() > 64)
        if span == 1:
            chain_flag = (np.arange(S) > site_first).astype(np.int32)
            want = phase_blocks(torch.from_numpy(link[:, 0].copy()), torch.from_numpy(shared[:, 0].copy()),
                                torch.from_numpy(chain_flag), 3, 2.0)
            assert got[1].tolist() == want[0].tolist() and got[2].tolist() == want[1].tolist()
            assert got[2].dtype == want[1].dtype and got[1].dtype == want[0].dtype
    assert seen['trials'] == 200 and min(seen['tie'], seen['start_inside'], seen['negative'], seen['deep']) >= 3, seen


def test_tie_rules():
    import torch
    from nadavca_amd.device import phase_forest
    # equal |link| takes the smaller w, whatever the signs; a larger |link| further away wins; |link| == min_link joins
    link = np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [-3.0, 3.0, 0.0], [3.0, -3.0, 3.0], [2.0, -7.0, 1.0],
                     [9.0, 9.0, 9.0]])
    shared = np.array([[9] * 3] * 5 + [[2, 3, 9]])
    first = np.zeros(6, dtype=np.int64)
    parent, block, sigma, m = forest(link, shared, first, 3, 2.0)
    assert parent.tolist() == [-1, 0, 1, 2, 2, 3] and block.tolist() == [0] * 6 and m['choice'] == 0.0
    assert sigma.tolist() == [1, 1, -1, -1, 1, -1] and m['join'] == 0.0
    got = phase_forest(torch.from_numpy(link), torch.from_numpy(shared), torch.from_numpy(first), 3, 2.0)
    assert got[0].tolist() == parent.tolist() and got[2].tolist() == sigma.tolist()
    # a candidate before site_first does not qualify however strong
    first = np.array([0, 0, 2, 2, 2, 5])
    assert forest(link, shared, first, 3, 2.0)[0].tolist() == [-1, 0, -1, 2, 2, -1]
    got = phase_forest(torch.from_numpy(link), torch.from_numpy(shared), torch.from_numpy(first), 3, 2.0)
    assert got[0].tolist() == [-1, 0, -1, 2, 2, -1] and got[1].tolist() == [0, 0, 2, 2, 2, 5]
    # tag: equal |H| takes the smaller block index, although the other block's site comes first in the read; all of a
    # block's sites count, not a run of them
    has, E = phase_ref.dense([(4.0, -4.0, None, None), (1.0, 5.0, 2.0, None), (None, None, None, None),
                              (3.0, None, -3.0, 0.5)], 4)
    block, sigma = np.array([3, 0, 3, 0]), np.array([1, 1, 1, 1])
    rb, llr, ns, m = tag_blocks(has, E, block, sigma)
    assert rb.tolist() == [0, 0, -1, 0] and llr.tolist() == [-4.0, 5.0, 0.0, 0.5] and ns.tolist() == [1, 1, 0, 1]
    assert m['gap'] == 0.0
    rb, llr, ns, _ = tag_blocks(has, E, np.array([0, 1, 0, 1]), sigma)
    assert rb.tolist() == [0, 1, -1, 1] and llr.tolist() == [4.0, 5.0, 0.0, 0.5] and ns.tolist() == [1, 1, 0, 1]
    # on interval blocks it is phase_ref.tag
    hasr, Er, chain_flag = random_case(5)
    res = phase_ref.refine(hasr, Er, chain_flag, 3, 2.0, 0)
    a = phase_ref.tag(hasr, Er, res['block'], res['sigma'])
    b = tag_blocks(hasr, Er, res['block'], res['sigma'])
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_span_links_columns():
    has, E, chain_flag = random_case(9)
    first = first_of_chain(chain_flag)
    assert first.tolist() == [0, 0, 0, 0, 0, 5, 5, 5]
    link1, shared1 = phase_ref.links(has, E, chain_flag)
    for span in (1, 2, 3, 8):
        link, shared = span_links(has, E, first, span)
        assert link.shape == (8, span) and np.array_equal(link[:, 0], link1) and np.array_equal(shared[:, 0], shared1)
        for s in range(8):
            for w in range(1, span + 1):
                if s - w < first[s]:
                    assert link[s, w - 1] == 0.0 and shared[s, w - 1] == 0
                else:
                    assert shared[s, w - 1] == (has[:, s] & has[:, s - w]).sum()


def test_argument_errors_before_any_device_call():
    from nadavca_amd import phase_mods_batch, phase_reads_batch
    from nadavca_amd.device import phase_sites_dev
    from nadavca_amd.phase import phase_of_rows

    class Model:   # (never reaches a kernel: the checks come first)
        alphabet_size = 4

    class Aligner:
        reference_num = np.zeros(50, dtype=np.int32)
    ref = np.zeros(50, dtype=np.int32)
    for bad in (0, 9, True, 2.5, '2', -1, None):
        with pytest.raises(ValueError, match='span'):
            phase_reads_batch(ref, None, config={}, kmer_model=Model(), aligner=Aligner(), threshold=100.0, span=bad)
        with pytest.raises(ValueError, match='span'):
            phase_of_rows(None, None, None, ref, None, Model(), 0, 100.0, span=bad)
        with pytest.raises(ValueError, match='span'):
            phase_sites_dev(*[None] * 16, span=bad)
        with pytest.raises(ValueError, match='span'):
            phase_mods_batch(ref, None, Aligner(), Model(), Model(), config={}, threshold=100.0, span=bad)
    # a valid span passes the check: the next one speaks
    for span in (1, 2, 8, np.int64(3)):
        with pytest.raises(ValueError, match='aligner'):
            phase_reads_batch(ref, None, config={}, kmer_model=Model(), aligner=None, threshold=100.0, span=span)


def test_result_fields_and_both_tsv_forms():
    from nadavca_amd.phase import PhaseBatch, _read_table, _site_table
    for f in ('parent', 'parent_link', 'parent_shared'):
        assert f in PhaseBatch.SITE_FIELDS
    z = PhaseBatch.empty(2, 7, 2, 5.0, span=3)
    assert z.span == 3 and z.parent.size == 0 and z.parent.dtype == np.int64 and z.parent_link.dtype == np.float64
    assert PhaseBatch.empty(2).span == 1 and z.parent_shared.dtype == np.int64
    s, r = _site_table(3), _read_table(1)
    s['contig'][:], s['position'][:], s['ref_base'][:], s['alt_base'][:] = [0, 0, 0], [5, 9, 12], [0, 3, 1], [2, 1, 0]
    s['phase'][:], s['block'][:], s['phase_set'][:], s['block_size'][:] = [1, 1, -1], [0, 1, 0], [5, 9, 5], [2, 1, 2]
    s['link'][:], s['shared'][:] = [0.0, 0.5, -0.25], [0, 9, 8]
    s['parent'][:], s['parent_link'][:], s['parent_shared'][:] = [-1, -1, 0], [0.0, 0.0, -12.5], [0, 0, 7]
    old_header = 'contig\tposition\tref\talt\tgt\tphase_set\tblock_size\tlink\tshared\tvote\tn_agree\tn_against\t' \
                 'fraction\tlrt\tcoverage'
    buf = io.StringIO(newline='')
    PhaseBatch(s, r, z.fractions, [0], ['chrA']).write_sites_tsv(buf)
    lines = buf.getvalue().split('\n')
    assert lines[0] == old_header and lines[3] == 'chrA\t12\tC\tA\t0|1\t5\t2\t-0.25\t8\t0.0\t0\t0\t0.0\t0.0\t0'
    buf = io.StringIO(newline='')
    b = PhaseBatch(s, r, z.fractions, [0], ['chrA'], span=2)
    b.write_sites_tsv(buf)
    wide = buf.getvalue().split('\n')
    assert wide[0] == old_header + '\tparent\tparent_link' and len(wide) == 5 and wide[4] == ''
    assert [w.split('\t')[-2:] for w in wide[1:4]] == [['.', '0.0'], ['.', '0.0'], ['5', '-12.5']]
    assert [w.rsplit('\t', 2)[0] for w in wide[:4]] == lines[:4] and b.n_blocks == 2


def test_new_entries_declared_bound_and_exported():
    from conftest import ROOT
    from nadavca_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    lib = _lib.load()
    for name in ('nvk_phase_span_links_dev', 'nvk_phase_tag_blocks_dev'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'NVK_K_COUNT = 13' in header and len(_lib.KERNEL_NAMES) == 13       # timed under NVK_K_ALLELE: no new slot
    for f in ('phase_span_links_dev', 'phase_tag_blocks_dev', 'phase_forest', 'phase_sites_dev', 'check_span'):
        assert callable(getattr(device, f))
    makefile = open(os.path.join(ROOT, 'nadavca_amd', 'csrc', 'Makefile')).read()
    assert 'kernels_phase.hip' in makefile                      # the span kernels live with the other phase kernels
