"""The host side of ``call_indels_batch`` without a GPU: the band map of the edit operator
(``call_indels.mapped_bands``) against a numpy restatement of the reference's ComputeBandStarts / ComputeBandEnds (dtw.cpp:7-35) on the edited
reference and anchors (``call_indels.apply_edit``); the left-aligned candidates (``canonical_candidates``) against a
brute-force enumeration of the distinct edited sequences; the strand mapping (``to_read_frame``); the batched
enumeration on CPU tensors against the per-read helpers; ``synthetic.apply_edits``; the TSV; and the argument
refusals that need no device."""
import io

import numpy as np
import pytest


def _band_starts(anchors, N, R, bw):
    out = np.zeros(R + 1, dtype=np.int64)
    for sig, at in anchors:
        out[at] = max(0, sig - bw)
    return np.maximum.accumulate(out)


def _band_ends(anchors, N, R, bw):
    out = np.full(R + 1, N, dtype=np.int64)
    for sig, at in anchors:
        out[at] = min(N, sig + bw)
    return np.minimum.accumulate(out[::-1])[::-1]


def _check_edit(case, bw, p, d, s):
    """-> clean; asserts the map where the issue says it must equal the recomputed band."""
    from nadavca_amd.call_indels import apply_edit, mapped_bands
    ref, anchors, N = case['reference'], case['approximate_alignment'], len(case['signal'])
    R = len(ref)
    bs, be = _band_starts(anchors, N, R, bw), _band_ends(anchors, N, R, bw)
    ref2, anchors2, clean = apply_edit(ref, anchors, p, d, s)
    i = len(s)
    assert ref2.tolist() == list(ref[:p]) + list(s) + list(ref[p + d:]) and len(ref2) == R - d + i
    deleted = set(range(p, p + d))
    assert clean == (not deleted & set(anchors[:, 1].tolist()))
    assert clean or d > 0
    ms, me = mapped_bands(bs, be, R, p, d, i)
    assert ms.shape == me.shape == (R - d + i + 1,)
    assert (np.diff(ms) >= 0).all() and (np.diff(me) >= 0).all() and (ms <= me).all()      # monotone, never empty
    if clean:
        assert np.array_equal(ms, _band_starts(anchors2, N, R - d + i, bw)), (p, d, i)
        assert np.array_equal(me, _band_ends(anchors2, N, R - d + i, bw)), (p, d, i)
    return clean


@pytest.mark.parametrize('k,central', [(5, 2), (4, 0), (4, 3), (6, 2), (10, 4)])
def test_mapped_bands_against_recomputed_bands(k, central):
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(3, k=k, central=central)
    back, fwd = k - central - 1, central
    n_clean = n_ins = n_all = 0
    for seed in range(12):
        rng = np.random.default_rng([71, k, central, seed])
        R = int(rng.integers(12, 90))
        bw = int(rng.integers(8, 50))
        case = synthetic.make_dp_case(rng, model, R=R, bandwidth=bw, dwell=(2, 9), jitter=6,
                                      anchor_density=float(rng.uniform(0.1, 0.9)), trim=3)
        # the largest insertion 14 rows allow in the interior: rows = k - 1 + i (back = 0: k + i)
        i_max = 14 - (k - 1 if back else k)
        edits = [(1, 0, [0] * min(i_max, 3)), (1, 1, []), (1, 0, []), (R - 1, 0, [1]), (R - 2, 1, []),
                 (R - 2, 1, [2, 3]), (R // 2, 0, [0] * i_max)]
        edits += [(R - 1 - d, d, []) for d in range(1, 9) if R - 1 - d >= 1]
        edits += [(int(rng.integers(1, R - 9)), d, [1] * int(rng.integers(0, 3))) for d in range(1, 9)]
        for _ in range(30):
            d = int(rng.integers(0, 4))
            p = int(rng.integers(1, R - d))
            edits.append((p, d, rng.integers(0, 4, int(rng.integers(0, i_max + 1))).tolist()))
        for p, d, s in edits:
            assert 1 <= p and p + d <= R - 1
            clean = _check_edit(case, bw, p, d, s)
            n_all += 1
            n_clean += clean
            n_ins += d == 0
            assert clean or d > 0            # every pure insertion is clean
    assert n_clean > 100 and n_ins > 50 and n_all > n_clean


def _brute_force(fwd, max_del):
    """Every (x, d, letter) of the whole sequence with the sequence it makes."""
    G = len(fwd)
    out = {}
    for d in range(1, max_del + 1):
        for x in range(0, G - d + 1):
            out.setdefault(tuple(fwd[:x]) + tuple(fwd[x + d:]), []).append((x, d, -1))
    for s in range(4):
        for x in range(0, G + 1):
            out.setdefault(tuple(fwd[:x]) + (s,) + tuple(fwd[x:]), []).append((x, 0, s))
    return out


@pytest.mark.parametrize('max_del', [1, 3])
def test_canonical_candidates_are_the_leftmost_of_their_classes(max_del):
    from nadavca_amd import synthetic
    from nadavca_amd.call_indels import canonical_candidates
    for seed in range(20):
        rng = np.random.default_rng([72, seed])
        G = int(rng.integers(30, 61))
        fwd = synthetic.homopolymer_rich(rng, G, 4).tolist()
        x, d, letter = canonical_candidates(fwd, 0, G, max_del=max_del, trim=0)
        got = list(zip(x.tolist(), d.tolist(), letter.tolist()))
        assert len(set(got)) == len(got)
        classes = _brute_force(fwd, max_del)
        assert len(classes) == len(got), (seed, len(classes), len(got))
        assert sorted(got) == sorted(min(members) for members in classes.values())        # each the leftmost
        assert len(classes) < sum(len(m) for m in classes.values())                        # (homopolymers: it matters)
        # a window of the sequence lists the whole sequence's candidates that keep `trim` bases from its ends
        start, end, trim = 7, G - 4, 5
        wx, wd, wl = canonical_candidates(fwd, start, end, max_del=max_del, trim=trim)
        exp = [c for c in got if start + trim <= c[0] and c[0] + c[1] <= end - trim]
        assert sorted(zip(wx.tolist(), wd.tolist(), wl.tolist())) == sorted(exp)
        assert wx.tolist() == sorted(wx.tolist())


def test_to_read_frame_commutes_with_the_reverse_complement():
    from nadavca_amd import synthetic
    from nadavca_amd.call_indels import apply_edit, canonical_candidates, to_read_frame
    none = np.zeros((0, 2), dtype=np.int64)
    rc = lambda a: (3 - np.asarray(a))[::-1]
    n = 0
    for seed in range(8):
        rng = np.random.default_rng([73, seed])
        G = 80
        fwd = synthetic.homopolymer_rich(rng, G, 4)
        start, end = int(rng.integers(0, 20)), int(rng.integers(50, G + 1))
        part = fwd[start:end]
        x, d, letter = canonical_candidates(fwd, start, end, max_del=3, trim=2)
        for reverse in (False, True):
            p, d2, l2 = to_read_frame(x, d, letter, start, end, reverse)
            assert (p >= 1).all() and (p + d2 <= len(part) - 1).all()
            for xi, di, li, pi, dri, lri in zip(x.tolist(), d.tolist(), letter.tolist(), p.tolist(), d2.tolist(),
                                                l2.tolist()):
                fwd_edit = apply_edit(part, none, xi - start, di, [li] if li >= 0 else [])[0]
                if reverse:
                    got = apply_edit(rc(part), none, pi, dri, [lri] if lri >= 0 else [])[0]
                    assert np.array_equal(got, rc(fwd_edit))
                else:
                    assert (pi, dri, lri) == (xi - start, di, li)
                n += 1
    assert n > 2000


def test_enumerate_candidates_against_the_per_read_helpers():
    """The batched enumeration on CPU tensors: per read, canonical_candidates of its forward range mapped with
    to_read_frame, in the same order; the lists the operator takes."""
    import torch
    from nadavca_amd import synthetic
    from nadavca_amd.call_indels import canonical_candidates, enumerate_candidates, to_read_frame
    rng = np.random.default_rng(74)
    G = 400
    fwd = synthetic.homopolymer_rich(rng, G, 4)
    ranges = [(0, 40), (10, 25), (100, 171), (300, 400), (50, 61), (200, 260)]
    reverse = np.array([False, True, True, False, True, False])
    keep = np.array([True, True, True, True, True, False])
    parts = [(3 - fwd[a:b])[::-1] if r else fwd[a:b] for (a, b), r in zip(ranges, reverse)]
    ref_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    for max_del, trim in ((1, 5), (3, 1), (0, 6)):
        hyp_off, owner, local, edit_pos, edit_del, letter, ins_off, ins_base = enumerate_candidates(
            torch.from_numpy(np.concatenate(parts).astype(np.int32)), torch.from_numpy(ref_off),
            torch.from_numpy(reverse), torch.from_numpy(keep), max_del, trim)
        assert hyp_off[0] == 0 and hyp_off[-1] == owner.numel() == ins_off.numel() - 1
        assert ins_off[-1] == ins_base.numel() == int((letter >= 0).sum())
        for j, ((a, b), r) in enumerate(zip(ranges, reverse)):
            lo, hi = int(hyp_off[j]), int(hyp_off[j + 1])
            if not keep[j]:
                assert lo == hi
                continue
            x, d, l = canonical_candidates(fwd, a, b, max_del=max_del, trim=trim)
            p, d2, l2 = to_read_frame(x, d, l, a, b, r)
            assert (owner[lo:hi] == j).all()
            assert (local[lo:hi].numpy() + a).tolist() == x.tolist()
            assert letter[lo:hi].tolist() == l.tolist()
            assert edit_pos[lo:hi].tolist() == p.tolist() and edit_del[lo:hi].tolist() == d2.tolist()
            got_letters = [ins_base[int(ins_off[h])].item() if ins_off[h + 1] > ins_off[h] else -1
                           for h in range(lo, hi)]
            assert got_letters == l2.tolist()
        assert int(hyp_off[-1]) > 0


def test_apply_edits_makes_the_mutated_genome():
    from nadavca_amd import synthetic
    g = np.array([0, 1, 2, 3, 0, 1, 2, 3, 3, 3], dtype=np.int32)
    out = synthetic.apply_edits(g, [(6, 1, []), (2, 0, [3]), (8, 2, [0, 0, 1])])
    assert out.dtype == g.dtype
    assert out.tolist() == [0, 1, 3, 2, 3, 0, 1, 3, 0, 0, 1]
    assert synthetic.apply_edits(g, []).tolist() == g.tolist()
    for bad in ([(2, 3, []), (4, 1, [])], [(-1, 1, [])], [(9, 2, [])]):
        with pytest.raises(ValueError):
            synthetic.apply_edits(g, bad)


def test_write_tsv_and_called():
    from nadavca_amd.call_indels import IndelCallBatch
    z = lambda dt: np.zeros(0, dtype=dt)
    b = IndelCallBatch(np.array([0, 0, 1], dtype=np.int32), np.array([5, 9, 2]), np.array([1, 0, 2], dtype=np.int32),
                       np.array([-1, 2, -1], dtype=np.int8), np.array([4, 3, 2]), np.array([7.5, -1.0, 0.25]),
                       np.array([4, 1, 1]), 0.0, z(np.int64), z(np.int64), z(np.int8), z(np.float64), z(np.int32),
                       z(np.int64), z(np.float64), z(np.int64), ['chrA', 'chrB'])
    assert b.called.tolist() == [0, 2] and len(b) == 3
    out = io.StringIO()
    b.write_tsv(out)
    assert out.getvalue().splitlines() == ['contig\tposition\tdel_len\tins\treads\tsupport\tllr',
                                           'chrA\t5\t1\t.\t4\t4\t7.5', 'chrB\t2\t2\t.\t2\t1\t0.25']
    out = io.StringIO()
    b.write_tsv(out, called_only=False)
    assert out.getvalue().splitlines()[2] == 'chrA\t9\t0\tG\t3\t1\t-1.0'
    e = IndelCallBatch.empty(1.0)
    assert len(e) == 0 and e.called.size == 0 and e.llr.dtype == np.float64


def test_refusals_without_a_device():
    from nadavca_amd import call_indels_batch
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match='max_del'):
            call_indels_batch(None, None, None, max_del=bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='trim'):
            call_indels_batch(None, None, None, trim=bad)
    with pytest.raises(ValueError, match='keep_rows'):
        call_indels_batch(None, None, None, keep_rows='some')
    with pytest.raises(ValueError, match='threshold'):
        call_indels_batch(None, None, None, threshold=float('nan'))
