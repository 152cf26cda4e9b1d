"""The host side of ``call_mods_batch`` without a GPU: the 5-letter table layout (``kmer_train.extend_kmer_model``),
the site finder on CPU tensors (``call_mods.find_sites``) against plain loops, ``ModCallBatch``'s TSV and site table
against plain loops, the simulated modified reads, and the C-ABI's three descriptions of the new entry."""
import io
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT


# ---- extend_kmer_model ---------------------------------------------------------------------------------------
def _digits(i, base, k):
    return [(i // base ** (k - 1 - m)) % base for m in range(k)]


@pytest.mark.parametrize('k', [3, 6])
def test_extend_kmer_model_against_loop(k):
    from nadavca_amd.kmer_train import extend_kmer_model
    rng = np.random.default_rng(k)
    mean, sigma = rng.normal(0, 1, 4 ** k), rng.uniform(0.2, 0.5, 4 ** k)
    for base in (1, 0, 3):
        mean5, sigma5 = extend_kmer_model(k, k // 2, mean, sigma, base=base)
        assert mean5.shape == sigma5.shape == (5 ** k,) and mean5.dtype == np.float64
        for i in range(5 ** k):
            d = _digits(i, 5, k)
            i4 = 0
            for x in d:
                i4 = i4 * 4 + (base if x == 4 else x)
            assert mean5[i] == mean[i4] and sigma5[i] == sigma[i4], (i, d)
    # the 4-letter sub-table is reproduced exactly, in the indexing of synthetic.kmer_ids
    from nadavca_amd import synthetic
    seq = rng.integers(0, 4, 200)
    mean5, sigma5 = extend_kmer_model(k, k // 2, mean, sigma)
    i4 = synthetic.kmer_ids(seq, 0, seq.size, k, k // 2, 4)
    i5 = synthetic.kmer_ids(seq, 0, seq.size, k, k // 2, 5)
    assert np.array_equal(mean5[i5], mean[i4]) and np.array_equal(sigma5[i5], sigma[i4])
    # levels override, as a dict and as arrays; everything else stays
    at = [int(x) for x in rng.choice(5 ** k, 9, replace=False)]
    levels = {i: (float(j), 0.1 * (j + 1)) for j, i in enumerate(at)}
    for form in (levels, (np.array(at), np.arange(9.0), 0.1 * (np.arange(9) + 1))):
        m2, s2 = extend_kmer_model(k, k // 2, mean, sigma, levels=form)
        for i in range(5 ** k):
            if i in levels:
                assert (m2[i], s2[i]) == levels[i]
            else:
                assert m2[i] == mean5[i] and s2[i] == sigma5[i]
    for bad in (dict(base=4), dict(base=-1), dict(levels={5 ** k: (0.0, 1.0)})):
        with pytest.raises(ValueError):
            extend_kmer_model(k, k // 2, mean, sigma, **bad)
    with pytest.raises(ValueError):
        extend_kmer_model(k, k // 2, mean[:-1], sigma[:-1])


# ---- the site finder -------------------------------------------------------------------------------------------
def _loop_sites(parts, starts, ends, reverse, pattern, mod_offset, k, keep=None):
    """Plain loops: -> rows (read, pos, forward, crowded), in read order and ascending position."""
    rows = []
    for j, part in enumerate(parts):
        if keep is not None and not keep[j]:
            continue
        mine = []
        for q in range(len(part) - len(pattern) + 1):
            if all(0 <= c <= 3 and part[q + t] == c for t, c in enumerate(pattern)):
                p = q + mod_offset
                mine.append((p, ends[j] - 1 - p if reverse[j] else starts[j] + p))
        for p, f in mine:
            crowded = any(p2 != p and abs(p2 - p) <= k - 1 for p2, _ in mine)
            rows.append((j, p, f, crowded))
    return rows


def _run_find(parts, starts, ends, reverse, pattern, mod_offset, k, keep=None):
    import torch
    from nadavca_amd.call_mods import find_sites
    flat = np.concatenate([np.asarray(p, dtype=np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    T = torch.from_numpy
    site_off, owner, pos, forward, crowded = find_sites(
        T(flat if flat.size else np.zeros(1, np.int32)), T(off), T(np.asarray(starts, dtype=np.int64)),
        T(np.asarray(ends, dtype=np.int64)), T(np.asarray(reverse, dtype=bool)), pattern, mod_offset, k,
        keep=None if keep is None else T(np.asarray(keep, dtype=bool)))
    rows = list(zip(owner.tolist(), pos.tolist(), forward.tolist(), crowded.tolist()))
    assert pos.dtype == torch.int32 and site_off.dtype == torch.int64
    assert site_off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(owner.numpy(),
                                                                           minlength=len(parts)))]).tolist()
    return rows


def test_find_sites_against_loop():
    rng = np.random.default_rng(11)
    # hand-made parts: the pattern at both ends, overlapping occurrences, a part shorter than the pattern, an
    # empty part, then random ones
    parts = [[1, 2, 0, 0, 1, 2], [1, 1, 1, 1, 1], [1], [], [2, 1, 2, 1, 2, 1, 2], [0, 1, 2, 1, 2, 3, 3, 3, 3, 3, 1, 2]]
    parts += [rng.integers(0, 3, int(rng.integers(0, 80))).tolist() for _ in range(40)]
    starts = [int(rng.integers(0, 1000)) for _ in parts]
    ends = [s + len(p) for s, p in zip(starts, parts)]
    reverse = [bool(j % 2) for j in range(len(parts))]
    keep = [bool(j % 5) for j in range(len(parts))]
    total = 0
    for pattern, offsets in (([1, 2], (0, 1)), ([1, 1], (0, 1)), ([2, 1, 2], (0, 1, 2)), ([1], (0,)),
                             ([1, 2, 1, 2, 0, 0, 0, 0, 0], (0, 8))):
        for mod_offset in offsets:
            for k in (1, 3, 6):
                for kp in (None, keep):
                    got = _run_find(parts, starts, ends, reverse, pattern, mod_offset, k, kp)
                    exp = _loop_sites(parts, starts, ends, reverse, pattern, mod_offset, k, kp)
                    assert got == exp, (pattern, mod_offset, k)
                    total += len(exp)
    assert total > 1000
    got = _run_find(parts[:1], starts[:1], ends[:1], [False], [1, 2], 0, 6)
    assert [(r[1], r[3]) for r in got] == [(0, True), (4, True)]     # both ends of the part; 4 bases apart
    assert [(r[1], r[3]) for r in _run_find(parts[:1], starts[:1], ends[:1], [False], [1, 2], 0, 4)] == \
        [(0, False), (4, False)]
    # a pattern letter outside ACGT matches nothing; a batch without parts is empty
    from nadavca_amd.detect_meth import pattern_codes
    for pattern in ('CN', 'cg', 'C-'):
        assert _run_find(parts, starts, ends, reverse, pattern_codes(pattern), 0, 6) == []
    assert _run_find([], [], [], [], [1, 2], 0, 6) == []
    for bad in (2, -1):
        with pytest.raises(ValueError):
            _run_find(parts, starts, ends, reverse, [1, 2], bad, 6)


def test_find_sites_on_the_contig_fixture():
    """Through ``readbatch.signal_alignments`` with the multi-contig fixture: every site's (contig, forward position)
    is an occurrence of the substituted base of the pattern on the read's strand of that contig, and every
    occurrence inside a read's range is found."""
    import torch
    from contig_fixture import ContigFixture
    from nadavca_amd import synthetic, readbatch
    from nadavca_amd.call_mods import find_sites
    model = synthetic.load_model_arrays()
    fx = ContigFixture(model)
    sa = readbatch.signal_alignments(fx.rb, fx.local_alignments(), 150, fx.refset, model[0], model[1])
    start, end = readbatch.contig_local_range(sa, fx.refset)
    for pattern, mod_offset in (([1, 2], 0), ([1, 2], 1), ([2, 0, 3, 1], 2)):
        site_off, owner, pos, forward, crowded = find_sites(sa.reference, sa.ref_off, start, end, sa.reverse, pattern,
                                                            mod_offset, model[0])
        assert int(owner.numel()) > 100
        m = len(pattern)
        seen = set()
        for j, p, f in zip(owner.tolist(), pos.tolist(), forward.tolist()):
            contig = fx.contigs[int(sa.contig[j])]
            assert int(start[j]) <= f < int(end[j])
            if bool(sa.reverse[j]):
                # the reverse strand's base at forward coordinate f, and the pattern read along that strand
                window = [3 - int(contig[f + mod_offset - t]) for t in range(m)]
            else:
                window = [int(contig[f - mod_offset + t]) for t in range(m)]
            assert window == list(pattern), (j, p, f)
            seen.add((j, f))
        for j in range(int(sa.live.numel())):
            contig = fx.contigs[int(sa.contig[j])]
            s, e = int(start[j]), int(end[j])
            seg = [int(x) for x in contig[s:e]]
            if bool(sa.reverse[j]):
                seg = [3 - x for x in seg[::-1]]
            for q in range(len(seg) - m + 1):
                if seg[q:q + m] == list(pattern):
                    p = q + mod_offset
                    assert (j, e - 1 - p if bool(sa.reverse[j]) else s + p) in seen
    assert torch.equal(site_off[1:] - site_off[:-1], torch.bincount(owner, minlength=int(sa.live.numel())))


# ---- ModCallBatch ------------------------------------------------------------------------------------------------
def _mod_batch(n, seed, names=None):
    from nadavca_amd.call_mods import ModCallBatch
    rng = np.random.default_rng(seed)
    llr = np.round(rng.normal(0, 4, n), 3)
    llr[::7] = 2.0
    llr[3::7] = -2.0
    llr[5::11] = 1e-17 + rng.normal(0, 1e-3, len(llr[5::11]))
    return ModCallBatch(rng.integers(0, 30, n), rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 12, n),
                        rng.integers(0, 2, n).astype(np.int8), llr, rng.random(n) < 0.3,
                        np.zeros(30, np.int32), np.arange(30), np.zeros(30), names)


def test_write_tsv_against_loop(tmp_path):
    from nadavca_amd.call_mods import ModCallBatch
    for names, read_names in ((None, None), (['a', 'b', 'c'], ['r%03d' % i for i in range(30)])):
        mb = _mod_batch(200, 5, names)
        exp = ['read\tcontig\tposition\tstrand\tllr\tcrowded\n']
        for i in range(len(mb)):
            exp.append('\t'.join([read_names[mb.read[i]] if read_names else 'read%d' % mb.read[i],
                                  names[mb.contig[i]] if names else str(int(mb.contig[i])), str(int(mb.position[i])),
                                  '-' if mb.strand[i] else '+', repr(float(mb.llr[i])),
                                  '1' if mb.crowded[i] else '0']) + '\n')
        buf = io.StringIO()
        mb.write_tsv(buf, read_names)
        assert buf.getvalue() == ''.join(exp)
        path = tmp_path / 'calls.tsv'
        mb.write_tsv(str(path), read_names)
        assert path.read_text() == ''.join(exp)
        assert [float(line.split('\t')[4]) for line in exp[1:]] == mb.llr.tolist()      # repr round-trips
    empty = ModCallBatch.empty()
    buf = io.StringIO()
    empty.write_tsv(buf)
    assert buf.getvalue() == 'read\tcontig\tposition\tstrand\tllr\tcrowded\n' and len(empty) == 0


def test_site_table_against_loop():
    from nadavca_amd.call_mods import ModCallBatch
    mb = _mod_batch(600, 6)
    for threshold in (2.0, 0.0, 5.5):
        sites = {}
        for i in range(len(mb)):
            s = sites.setdefault((int(mb.contig[i]), int(mb.position[i]), int(mb.strand[i])), [0, 0, 0])
            s[0] += 1
            s[1] += mb.llr[i] >= threshold
            s[2] += mb.llr[i] <= -threshold
        tab = mb.site_table(threshold) if threshold != 2.0 else mb.site_table()
        keys = sorted(sites)
        assert list(zip(tab['contig'].tolist(), tab['position'].tolist(), tab['strand'].tolist())) == keys
        assert tab['reads'].tolist() == [sites[q][0] for q in keys]
        assert tab['modified'].tolist() == [sites[q][1] for q in keys]
        assert tab['unmodified'].tolist() == [sites[q][2] for q in keys]
        if threshold > 0:
            assert tab['ambiguous'].tolist() == [sites[q][0] - sites[q][1] - sites[q][2] for q in keys]
        for f, q in zip(tab['frequency'].tolist(), keys):
            _, a, b = sites[q]
            assert (math.isnan(f) if a + b == 0 else f == a / (a + b))
    # the NaN frequency: a site whose only read is ambiguous
    one = ModCallBatch(np.array([0, 1]), np.zeros(2, np.int32), np.array([7, 9]), np.zeros(2, np.int8),
                       np.array([0.5, 3.0]), np.zeros(2, bool), np.zeros(2, np.int32), np.arange(2), np.zeros(2))
    tab = one.site_table()
    assert math.isnan(tab['frequency'][0]) and tab['frequency'][1] == 1.0
    assert tab['ambiguous'].tolist() == [1, 0] and tab['reads'].tolist() == [1, 1]
    tab = ModCallBatch.empty().site_table()
    assert all(len(v) == 0 for v in tab.values()) and set(tab) == {
        'contig', 'position', 'strand', 'reads', 'modified', 'unmodified', 'ambiguous', 'frequency'}


# ---- simulated modified reads -------------------------------------------------------------------------------
def test_make_modified_read_batch_truth():
    """The truth masks mark occurrences of the pattern's substituted base on their strand only, about the asked
    fraction of them; sequence, mapping and aligner are the canonical ``make_read_batch`` ones, the signals differ
    exactly where a modified k-mer lies under them."""
    from nadavca_amd import synthetic
    from nadavca_amd.kmer_train import extend_kmer_model
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = extend_kmer_model(k, central, mean, sigma)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
    mean5 = mean5 + 2.0 * has_m
    model5 = (k, central, 5, mean5, sigma5)
    rb, aligner, genome, truth = synthetic.make_modified_read_batch(40, model5, seed=9, genome_length=3000)
    rb0, aligner0, genome0 = synthetic.make_read_batch(40, (k, central, 4, mean, sigma), seed=9, genome_length=3000)
    assert np.array_equal(genome, genome0) and np.array_equal(rb.sequence, rb0.sequence)
    assert np.array_equal(rb.sig_off, rb0.sig_off) and np.array_equal(rb.map_sig, rb0.map_sig)
    ba, ba0 = aligner.get_base_alignments(rb), aligner0.get_base_alignments(rb0)
    assert np.array_equal(ba.ref_idx, ba0.ref_idx) and np.array_equal(ba.reverse, ba0.reverse)
    assert not np.array_equal(rb.raw_signal, rb0.raw_signal)
    G = genome.size
    fwd_sites = np.nonzero((genome[:-1] == 1) & (genome[1:] == 2))[0]             # C of CG, forward strand
    rev_sites = fwd_sites + 1                                                     # G of CG: the C of the other strand
    assert set(np.nonzero(truth['forward'])[0]) <= set(fwd_sites)
    assert set(np.nonzero(truth['reverse'])[0]) <= set(rev_sites)
    for mask, sites in ((truth['forward'], fwd_sites), (truth['reverse'], rev_sites)):
        assert mask.shape == (G,) and 0.35 < mask.sum() / sites.size < 0.65
    with pytest.raises(ValueError):
        synthetic.make_modified_read_batch(4, (k, central, 4, mean, sigma), seed=9)


# ---- the C-ABI's three descriptions ---------------------------------------------------------------------------
def test_new_entry_declared_bound_and_exported():
    from nadavca_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    m = re.search(r'int nvk_estimate_hypotheses_batch_dev\(([^;]*)\);', header)
    assert m, 'nvk_estimate_hypotheses_batch_dev is not declared'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES['nvk_estimate_hypotheses_batch_dev']
    assert len(params) == len(args) == 25
    import ctypes as C
    for p, a in zip(params, args):
        want = C.c_void_p if '*' in p else C.c_int64 if p.startswith('int64_t') else C.c_int
        assert a is want, p
    # the same leading arguments as the full entry
    full = re.search(r'int nvk_estimate_log_likelihoods_batch_dev\(([^;]*)\);', header).group(1)
    full = [p.strip() for p in full.replace('\n', ' ').split(',')]
    assert params[:18] == full[:18] and params[-1] == full[-1]
    assert hasattr(_lib.load(), 'nvk_estimate_hypotheses_batch_dev')
    import nadavca_amd
    assert callable(nadavca_amd.call_mods_batch) and 'call_mods_batch' in nadavca_amd.__all__
