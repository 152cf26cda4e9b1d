"""The seed aligner (nadavca_amd/seedalign.py) without a GPU:

* the CPU restatement of its extension stage (tests/host_shims/seedext_host.cpp, which the kernel is held to in
  tests/test_gpu_seed_align.py) against a brute-force full-matrix Gotoh local alignment with the same tie rules;
* its seeding (torch, run on the CPU) against a plain-Python per-read restatement with a dict k-mer index;
* seeding + the restatement against the simulated truth: error-free reads, noisy reads, random reads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -(1 << 30)


@pytest.fixture(scope='module')
def host_extend(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('seedext') / 'seedext_host.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC',
                    os.path.join(ROOT, 'tests', 'host_shims', 'seedext_host.cpp'), '-o', so], check=True)
    return _host_runner(C.CDLL(so))


def _host_runner(lib):
    f = lib.seedext_host
    f.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_int] * 6 \
        + [C.c_void_p, C.c_void_p]
    f.restype = None

    def run(query, q_off, ref, strand, diag, w, match=1, mismatch=1, gap_open=1, gap_extend=1, min_score=30):
        """-> (hit (n, 4): score, end i, end j, count; pairs list of (k, 2) arrays)"""
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        query, q_off, ref = a(query, np.int32), a(q_off, np.int64), a(ref, np.int32)
        strand, diag = a(strand, np.int32), a(diag, np.int32)
        n = q_off.size - 1
        hit = np.zeros((n, 4), dtype=np.int32)
        pairs = np.zeros((max(int(q_off[-1]), 1), 2), dtype=np.int32)
        p = lambda x: x.ctypes.data
        f(n, p(query), p(q_off), p(ref), ref.size, p(strand), p(diag), w, match, mismatch, gap_open, gap_extend,
          min_score, p(hit), p(pairs))
        return hit, [pairs[q_off[j]:q_off[j] + hit[j, 3]] for j in range(n)]
    return run


def brute_force(q, r, match, mismatch, gap_open, gap_extend):
    """Full-matrix Gotoh local alignment with the tie rules of include/nadavca_hip.h (nvk_seed_extend_dev), plain
    Python.  -> (score, end (i, j), pairs)"""
    m, G = len(q), len(r)
    O, X = gap_open + gap_extend, gap_extend
    H = [[0] * G for _ in range(m)]
    E = [[NEG] * G for _ in range(m)]
    F = [[NEG] * G for _ in range(m)]
    src = [[0] * G for _ in range(m)]
    ee = [[False] * G for _ in range(m)]
    fe = [[False] * G for _ in range(m)]
    best = (-1, -1, -1)
    for i in range(m):
        for j in range(G):
            d = (H[i - 1][j - 1] if i and j else 0) + (match if q[i] == r[j] else -mismatch)
            if j:
                E[i][j] = max(H[i][j - 1] - O, E[i][j - 1] - X)
                ee[i][j] = E[i][j - 1] - X > H[i][j - 1] - O
            if i:
                F[i][j] = max(H[i - 1][j] - O, F[i - 1][j] - X)
                fe[i][j] = F[i - 1][j] - X > H[i - 1][j] - O
            b = max(d, E[i][j], F[i][j])
            if b > 0:
                H[i][j] = b
                src[i][j] = 1 if d == b else 2 if E[i][j] == b else 3
            if H[i][j] > best[0]:
                best = (H[i][j], i, j)
    score, i, j = best
    if score < 0:
        return 0, (-1, -1), []
    pairs, state = [], 'H'
    while True:
        if state == 'H':
            s = src[i][j]
            if s == 0:
                break
            if s == 1:
                if q[i] == r[j]:
                    pairs.append((i, j))
                if i == 0 or j == 0:
                    break
                i, j = i - 1, j - 1
            else:
                state = 'E' if s == 2 else 'F'
        elif state == 'E':
            ext = ee[i][j]
            j -= 1
            state = 'E' if ext else 'H'
        else:
            ext = fe[i][j]
            i -= 1
            state = 'F' if ext else 'H'
    return score, (best[1], best[2]), pairs[::-1]


def test_restatement_equals_brute_force(host_extend):
    rng = np.random.default_rng(5)
    narrower = 0
    for trial in range(400):
        G = int(rng.integers(1, 28))
        m = int(rng.integers(1, 24))
        ref = rng.integers(0, 4, G)
        st = int(rng.integers(0, 2))
        r = 3 - ref[::-1] if st else ref
        if trial % 3 == 0:    # a read drawn from the strand, with edits: long alignments with gaps
            x = int(rng.integers(0, G))
            q = np.array(list(r[x:x + m]) or [0])
            q = np.array([b if rng.random() > 0.2 else int(rng.integers(0, 4)) for b in q])
            q = np.delete(q, rng.integers(0, q.size, int(rng.integers(0, 3)))) if q.size > 3 else q
            m = q.size
        else:
            q = rng.integers(0, 4, m)
        sc = [(1, 1, 1, 1), (2, 3, 2, 1), (1, 2, 3, 1), (3, 1, 1, 2)][trial % 4]
        exp = brute_force(list(q), list(r), *sc)
        if trial % 2 == 0:   # a band that covers the whole matrix
            w = int(rng.integers(1, 40))
            d = int(rng.integers(G - 1 - w, w - (m - 1) + 1)) if G - 1 - w <= w - (m - 1) else None
            if d is None:
                w = m + G
                d = 0
            hit, pairs = host_extend(q, [0, m], ref, [st], [d], w, *sc, min_score=1)
            assert (hit[0, 0], (hit[0, 1], hit[0, 2])) == (exp[0], exp[1]), (trial, hit, exp)
            if exp[0] >= 1:
                assert [tuple(p) for p in pairs[0]] == exp[2], trial
        else:                # a narrower band: never better than the full matrix
            w = int(rng.integers(1, 4))
            d = int(rng.integers(-m, G))
            hit, _ = host_extend(q, [0, m], ref, [st], [d], w, *sc, min_score=1)
            assert hit[0, 0] <= exp[0]
            narrower += hit[0, 0] < exp[0]
    assert narrower > 10   # (the narrow bands do lose score on some cases)


def python_seed(read, ref, k, max_occ, w, min_seeds):
    """Step 1 of seedalign.py for one read, plain Python.  -> (strand, c, votes, d*, tie flags)"""
    ref = [int(b) for b in ref]
    strands = (ref, [3 - b for b in ref[::-1]])
    best, ties = [], set()
    all_seeds = []
    for s, seq in enumerate(strands):
        index = {}
        for p in range(len(seq) - k + 1):
            index.setdefault(tuple(seq[p:p + k]), []).append(p)
        seeds = []
        for i in range(len(read) - k + 1):
            hits = index.get(tuple(int(b) for b in read[i:i + k]), [])
            if len(hits) <= max_occ:
                seeds += [(i, p) for p in hits]
            elif s == 0:
                ties.add('max_occ')
        n = {}
        for i, p in seeds:
            c = (p - i) // w
            n[c] = n.get(c, 0) + 1
            if p - i < 0:
                ties.add('negative')
        cands = sorted(set(n) | {c - 1 for c in n})
        scored = [(n.get(c, 0) + n.get(c + 1, 0), c) for c in cands]
        if scored:
            top = max(v for v, _ in scored)
            if sum(v == top for v, _ in scored) > 1:
                ties.add('window')
            c = min(c for v, c in scored if v == top)
            best.append((top, c))
        else:
            best.append((0, 0))
        all_seeds.append(seeds)
    s = 1 if best[1][0] > best[0][0] else 0
    if best[0][0] == best[1][0] and best[0][0] > 0:
        ties.add('strand')
    votes, c = best[s]
    if votes < min_seeds:
        return -1, None, votes, 0, ties
    ds = sorted(p - i for i, p in all_seeds[s] if (p - i) // w in (c, c + 1))
    assert len(ds) == votes
    return s, c, votes, ds[(len(ds) - 1) // 2], ties


def _batch(seqs):
    from nadavca_amd.readbatch import ReadBatch
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    z = np.zeros(len(seqs) + 1, dtype=np.int64)
    cat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if seqs else np.zeros(0, np.int32)
    return ReadBatch(np.zeros(0, np.int16), z, cat, off, np.zeros(0), np.zeros(0), z)


def test_seeding_equals_per_read_python():
    from nadavca_amd.seedalign import SeedAligner
    rng = np.random.default_rng(11)
    unit = rng.integers(0, 4, 9)
    # a reference with repeats (k-mers above max_occ) and palindromic pieces (reads that tie between strands)
    piece = rng.integers(0, 4, 30)
    ref = np.concatenate([rng.integers(0, 4, 300), np.tile(unit, 8), rng.integers(0, 4, 200), piece,
                          3 - piece[::-1], rng.integers(0, 4, 150)])
    rc = 3 - ref[::-1]
    seen = set()
    for k, max_occ, w, min_seeds in ((8, 3, 4, 1), (8, 32, 16, 2), (10, 1, 64, 3), (9, 5, 1, 2)):
        reads = []
        for t in range(160):
            kind = t % 8
            L = int(rng.integers(0, 120))
            if kind == 0:
                reads.append(rng.integers(0, 4, L))
            elif kind == 1:
                reads.append(rng.integers(0, 4, int(rng.integers(0, k))))          # shorter than k
            elif kind == 2:                                                         # off the left end: d < 0
                reads.append(np.concatenate([rng.integers(0, 4, 20), ref[:L]]))
            elif kind == 3:                                                         # two loci: window ties
                x, y = rng.integers(0, ref.size - 40, 2)
                reads.append(np.concatenate([ref[x:x + 20], rng.integers(0, 4, 3), ref[y:y + 20]]))
            elif kind == 4:                                                         # both strands
                x, y = rng.integers(0, ref.size - 40, 2)
                reads.append(np.concatenate([ref[x:x + 25], rc[y:y + 25]]))
            elif kind == 5:
                reads.append(ref[530:590] if t % 16 < 8 else rc[ref.size - 590:ref.size - 530])   # palindrome
            else:
                x = int(rng.integers(0, max(1, ref.size - L)))
                s = rc if t % 2 else ref
                r = s[x:x + L].copy()
                r[rng.random(r.size) < 0.05] = rng.integers(0, 4)
                reads.append(r)
        reads.append(np.tile(unit, 3))                                              # k-mers above max_occ
        rb = _batch(reads)
        al = SeedAligner(ref, device='cpu', k=k, max_occ=max_occ, band=w, min_seeds=min_seeds)
        strand, diag, votes = (x.numpy() for x in al.seed(rb))
        for j, read in enumerate(reads):
            s, c, v, d, ties = python_seed(read, ref, k, max_occ, w, min_seeds)
            seen |= ties
            assert (strand[j], votes[j]) == (s, v), (k, j)
            if s >= 0:
                assert diag[j] == d and diag[j] // w in (c, c + 1), (k, j)
        # a reference shorter than k: nothing seeds
        short = SeedAligner(ref[:k - 1], device='cpu', k=k, max_occ=max_occ, band=w, min_seeds=min_seeds)
        strand, _, votes = short.seed(rb)
        assert (strand.numpy() == -1).all() and (votes.numpy() == 0).all()
    assert seen >= {'max_occ', 'negative', 'window', 'strand'}, seen


def test_parameters_and_codes_are_checked(tmp_path):
    from nadavca_amd.seedalign import SeedAligner
    ref = np.random.default_rng(0).integers(0, 4, 100)
    for bad in (dict(k=7), dict(k=16), dict(band=0), dict(band=257), dict(max_occ=0), dict(min_seeds=0),
                dict(match=0), dict(mismatch=17), dict(gap_open=0), dict(gap_extend=17), dict(min_score=0),
                dict(bogus=1), dict(k=14.0)):
        with pytest.raises(ValueError):
            SeedAligner(ref, device='cpu', **bad)
    with pytest.raises(ValueError):
        SeedAligner(ref, device='cpu').seed(_batch([[0, 1, 4, 2]]))
    fa = tmp_path / 'two.fa'
    fa.write_text('>a\nACGT\n>b\nACGT\n')
    with pytest.raises(ValueError):
        SeedAligner(str(fa), device='cpu')
    fa = tmp_path / 'one.fa'
    fa.write_text('>a\nACGTTG\nCA\n')
    assert SeedAligner(str(fa), device='cpu').reference_num.tolist() == [0, 1, 2, 3, 3, 2, 1, 0]


def cpu_pipeline(aligner, rb, host_extend):
    """Step 1 by the aligner's torch code on the CPU, steps 2-3 by the host restatement: -> BaseAlignmentBatch
    arrays (read_idx, ref_idx, off, reverse) and the per-read hit table."""
    p = aligner.params
    strand, diag, _ = (x.numpy() for x in aligner.seed(rb))
    hit, pairs = host_extend(rb.sequence, rb.seq_off, aligner.reference_num, strand, diag, p['band'], p['match'],
                             p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'])
    off = np.concatenate([[0], np.cumsum(hit[:, 3])]).astype(np.int64)
    flat = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int32)
    reverse = (strand == 1) & (hit[:, 0] >= p['min_score'])
    return flat[:, 0].astype(np.int32), flat[:, 1].astype(np.int64), off, reverse, strand, hit


def test_error_free_reads_give_the_true_pairs(host_extend):
    from nadavca_amd import synthetic
    from nadavca_amd.seedalign import SeedAligner
    rb, truth, genome = synthetic.make_read_batch(120, synthetic.load_model_arrays(), seed=4)
    read_idx, ref_idx, off, reverse, _, _ = cpu_pipeline(SeedAligner(genome, device='cpu'), rb, host_extend)
    ba = truth.get_base_alignments(rb)
    assert reverse.any() and not reverse.all()
    for got, exp in ((read_idx, ba.read_idx), (ref_idx, ba.ref_idx), (off, ba.off), (reverse, ba.reverse)):
        assert np.array_equal(got, exp)


@pytest.mark.parametrize('length,spread,n', [(400, 40, 300), (5000, 500, 24)])
def test_noisy_reads_land_on_their_locus(host_extend, length, spread, n):
    from nadavca_amd import synthetic
    from nadavca_amd.seedalign import SeedAligner
    genome = np.random.default_rng(8).integers(0, 4, 50000)
    rb, truth, info = synthetic.make_error_read_batch(n, genome, seed=9, length=length, spread=spread,
                                                      substitution_rate=0.03, insertion_rate=0.015,
                                                      deletion_rate=0.015)
    read_idx, ref_idx, off, reverse, strand, hit = cpu_pipeline(SeedAligner(genome, device='cpu'), rb, host_extend)
    on_locus, true_pairs, emitted = 0, 0, 0
    for j in range(n):
        t = set(zip(truth.read_idx[truth.off[j]:truth.off[j + 1]].tolist(),
                    truth.ref_idx[truth.off[j]:truth.off[j + 1]].tolist()))
        got = list(zip(read_idx[off[j]:off[j + 1]].tolist(), ref_idx[off[j]:off[j + 1]].tolist()))
        emitted += len(got)
        true_pairs += sum(g in t for g in got)
        span = lambda ps: (min(r for _, r in ps), max(r for _, r in ps)) if ps else (0, -1)
        (a0, a1), (b0, b1) = span(got), span(t)
        overlap = max(0, min(a1, b1) - max(a0, b0) + 1)
        on_locus += bool(got) and strand[j] == int(info['reverse'][j]) and overlap >= 0.9 * (b1 - b0 + 1)
    # measured (seed 9): 300 / 300 short and 24 / 24 long reads on their strand and locus; of the emitted pairs
    # 98.78 % (short) and 98.82 % (long) are true pairs (the rest sit next to an indel, where a gap placed one base
    # over pairs a read base with a neighbour of its source)
    assert on_locus >= 0.98 * n          # measured 1.0
    assert true_pairs >= 0.98 * emitted  # measured 0.9878 / 0.9882


def test_random_reads_do_not_align(host_extend):
    from nadavca_amd import synthetic
    from nadavca_amd.seedalign import SeedAligner
    genome = np.random.default_rng(8).integers(0, 4, 50000)
    rb, _, info = synthetic.make_error_read_batch(200, genome, seed=2, random_fraction=1.0)
    assert (info['kind'] == 1).all()
    _, _, off, reverse, strand, hit = cpu_pipeline(SeedAligner(genome, device='cpu'), rb, host_extend)
    assert off[-1] == 0 and not reverse.any() and (hit[:, 0] < 30).all()


def test_error_read_generator_truth_is_consistent():
    from nadavca_amd import synthetic
    genome = np.random.default_rng(1).integers(0, 4, 3000)
    rc = 3 - genome[::-1]
    rb, truth, info = synthetic.make_error_read_batch(60, genome, seed=1, substitution_rate=0.05,
                                                      insertion_rate=0.05, deletion_rate=0.05,
                                                      random_fraction=0.2, overhang_fraction=0.3)
    assert set(info['kind'].tolist()) == {0, 1, 2}
    for j in range(rb.n):
        seq = rb.sequence[rb.seq_off[j]:rb.seq_off[j + 1]]
        ri = truth.read_idx[truth.off[j]:truth.off[j + 1]]
        fi = truth.ref_idx[truth.off[j]:truth.off[j + 1]]
        strand = rc if info['reverse'][j] else genome
        assert np.array_equal(seq[ri], strand[fi])
        assert (np.diff(ri) > 0).all() and (np.diff(fi) > 0).all()
