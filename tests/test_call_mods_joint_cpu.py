"""The host side of ``call_mods_batch(joint=True)`` without a GPU: the clustering (``call_mods.cluster_sites``) and the
hypothesis lists built from it (``call_mods.joint_lists``) on CPU tensors against plain loops, the marginalisation
(``call_mods.marginal_llr``) against a brute-force enumeration, ``ModCallBatch``'s TSV with and without the joint
columns, the argument refusals, the share of crowded sites the clustering rule leaves crowded, and the C-ABI's three
descriptions of the new entry."""
import io
import itertools
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT


# ---- clustering ------------------------------------------------------------------------------------------------
def _loop_clusters(owner, pos, k, max_joint):
    """The rule as a walk: -> (cluster id per site, cut flag per site)."""
    cluster, open_first, open_size, cid = [], None, 0, -1
    for i, (o, p) in enumerate(zip(owner, pos)):
        joins = (i > 0 and owner[i - 1] == o and p - pos[i - 1] <= k - 1 and p - open_first <= 14 - k
                 and open_size < max_joint)
        if joins:
            open_size += 1
        else:
            cid, open_first, open_size = cid + 1, p, 1
        cluster.append(cid)
    cut = [any(j != i and owner[j] == owner[i] and abs(pos[j] - pos[i]) <= k - 1 and cluster[j] != cluster[i]
               for j in range(max(0, i - 40), min(len(pos), i + 41))) for i in range(len(pos))]
    return cluster, cut


def _random_sites(rng, n_reads, dense):
    owner, pos = [], []
    for j in range(n_reads):
        m = int(rng.integers(0, 40))
        if j % 7 == 3:
            m = 0
        gaps = rng.integers(1, 4 if dense else 14, m) if j % 3 else rng.geometric(0.15 if dense else 0.08, m)
        p = np.cumsum(gaps) - 1 + int(rng.integers(0, 5))
        owner += [j] * m
        pos += p.tolist()
    return owner, pos


@pytest.mark.parametrize('k', [4, 6, 10, 13])
@pytest.mark.parametrize('max_joint', [2, 3, 4])
def test_cluster_sites_against_loop(k, max_joint):
    import torch
    from nadavca_amd.call_mods import cluster_sites
    total = clustered = 0
    for seed, dense in ((1, False), (2, True), (3, False)):
        owner, pos = _random_sites(np.random.default_rng([seed, k, max_joint]), 60, dense)
        cluster, first, size, cut = cluster_sites(torch.tensor(owner, dtype=torch.int64),
                                                  torch.tensor(pos, dtype=torch.int32), k, max_joint)
        exp_cluster, exp_cut = _loop_clusters(owner, pos, k, max_joint)
        assert cluster.tolist() == exp_cluster, (k, max_joint, seed)
        assert cut.tolist() == exp_cut, (k, max_joint, seed)
        assert size.tolist() == np.bincount(exp_cluster).tolist()
        assert first.tolist() == [exp_cluster.index(c) for c in range(len(size))]
        # what the rule promises the kernel: a cluster's re-run fits 14 rows, wherever the read ends
        for c in range(len(size)):
            mine = [p for p, x in zip(pos, exp_cluster) if x == c]
            assert len(mine) <= max_joint and mine[-1] - mine[0] + k <= max(14, k)
        total += len(pos)
        clustered += int((size[cluster] > 1).sum())
    assert total > 1000
    assert clustered > 50 or k == 13
    # hand-made: one read, k = 6: 0 2 4 | 9 (beyond 14 - k = 8 of 0, close to 4: a cut) | 30
    cluster, first, size, cut = cluster_sites(torch.zeros(5, dtype=torch.int64),
                                              torch.tensor([0, 2, 4, 9, 30], dtype=torch.int32), 6, 4)
    assert cluster.tolist() == [0, 0, 0, 1, 2] and cut.tolist() == [False, False, True, True, False]
    # the same positions in different reads never share a cluster; no site at all
    cluster, _, _, cut = cluster_sites(torch.tensor([0, 1, 1]), torch.tensor([5, 6, 8], dtype=torch.int32), 6, 4)
    assert cluster.tolist() == [0, 1, 1] and not cut.any()
    cluster, first, size, cut = cluster_sites(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 6, 4)
    assert cluster.numel() == first.numel() == size.numel() == cut.numel() == 0


def test_joint_lists_against_loop():
    import torch
    from nadavca_amd.call_mods import cluster_sites, joint_lists
    owner, pos = _random_sites(np.random.default_rng(8), 30, True)
    n_reads = 32                                       # two reads after the last one with sites
    to, tp = torch.tensor(owner, dtype=torch.int64), torch.tensor(pos, dtype=torch.int32)
    cluster, first, size, _ = cluster_sites(to, tp, 6, 3)
    hyp_off, sub_off, sub_pos, sub_base, hyp_cluster, hyp_mask = joint_lists(to, tp, n_reads, first, size, 4)
    exp_hyps, exp_owner, exp_cm = [], [], []
    for c in range(len(size)):
        mine = [p for p, x in zip(pos, cluster.tolist()) if x == c]
        for mask in range(1, 1 << len(mine)):
            exp_hyps.append([p for j, p in enumerate(mine) if mask >> j & 1])
            exp_owner.append(owner[int(first[c])])
            exp_cm.append((c, mask))
    assert list(zip(hyp_cluster.tolist(), hyp_mask.tolist())) == exp_cm
    assert sub_off.tolist() == np.concatenate([[0], np.cumsum([len(h) for h in exp_hyps])]).tolist()
    assert sub_pos.tolist() == [p for h in exp_hyps for p in h] and sub_pos.dtype == torch.int32
    assert (sub_base == 4).all() and sub_base.dtype == torch.int32
    assert hyp_off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(exp_owner, minlength=n_reads))]).tolist()
    assert max(len(h) for h in exp_hyps) == 3


# ---- marginalisation -------------------------------------------------------------------------------------------
def _lse(xs):
    xs = [x for x in xs if x != -math.inf]
    if not xs:
        return -math.inf
    m = max(xs)
    return m + math.log(sum(math.exp(x - m) for x in xs))


@pytest.mark.parametrize('prior', [0.5, 0.1, 0.8])
def test_marginal_llr_against_enumeration(prior):
    import torch
    from nadavca_amd.call_mods import marginal_llr
    rng = np.random.default_rng(int(prior * 100))
    J, C = 4, 200
    size = rng.integers(1, J + 1, C)
    values = rng.normal(-300.0, 8.0, (C, 1 << J))
    values[rng.random((C, 1 << J)) < 0.15] = -math.inf
    values[:, 0] = rng.normal(-300.0, 8.0, C)                 # the total of a row that is kept is finite
    values[5, 1:] = -math.inf                                  # every substitution impossible
    junk = values.copy()
    for c in range(C):
        junk[c, 1 << size[c]:] = rng.normal(0.0, 1.0, (1 << J) - (1 << size[c]))   # ignored columns
    got = marginal_llr(torch.from_numpy(junk), torch.from_numpy(size), prior).numpy()
    assert got.shape == (C, J)
    checked = 0
    for c in range(C):
        m = int(size[c])
        for j in range(m):
            num, den = [], []
            for states in itertools.product((0, 1), repeat=m):
                mask = sum(s << t for t, s in enumerate(states))
                w = sum(math.log(prior) if s else math.log(1 - prior) for t, s in enumerate(states) if t != j)
                (num if states[j] else den).append(values[c, mask] + w)
            exp = _lse(num) - _lse(den)
            if exp == -math.inf:
                assert got[c, j] == -math.inf
            else:
                assert got[c, j] == pytest.approx(exp, rel=1e-12, abs=1e-12), (c, j)
            checked += 1
    assert checked > 400 and (got[5, :size[5]] == -math.inf).all()
    # a cluster of one: the single ratio, whatever the prior
    one = marginal_llr(torch.tensor([[-7.0, -3.0]], dtype=torch.float64), torch.tensor([1]), prior)
    assert one.tolist() == [[4.0]]
    with pytest.raises(ValueError):
        marginal_llr(torch.zeros((2, 3), dtype=torch.float64), torch.tensor([1, 1]), prior)


# ---- ModCallBatch ------------------------------------------------------------------------------------------------
def _batch(joint):
    from nadavca_amd.call_mods import ModCallBatch
    more = dict(cluster=np.array([1, 2, 2], dtype=np.int32), llr_single=np.array([1.5, -0.25, -math.inf])) if joint \
        else {}
    return ModCallBatch(np.array([0, 2, 2]), np.array([0, 1, 1], dtype=np.int32), np.array([10, 7, 9]),
                        np.array([0, 1, 1], dtype=np.int8), np.array([1.5, -2.0, 0.125]), np.array([False, True, False]),
                        np.zeros(3, dtype=np.int32), np.arange(3), np.zeros(3), ['chrA', 'chrB'], **more)


def test_write_tsv_with_and_without_joint_columns(tmp_path):
    plain, joint = io.StringIO(), io.StringIO()
    _batch(False).write_tsv(plain)
    _batch(True).write_tsv(joint, names=['a', 'b', 'c'])
    assert plain.getvalue().splitlines() == [
        'read\tcontig\tposition\tstrand\tllr\tcrowded', 'read0\tchrA\t10\t+\t1.5\t0', 'read2\tchrB\t7\t-\t-2.0\t1',
        'read2\tchrB\t9\t-\t0.125\t0']
    assert joint.getvalue().splitlines() == [
        'read\tcontig\tposition\tstrand\tllr\tcrowded\tcluster\tllr_single', 'a\tchrA\t10\t+\t1.5\t0\t1\t1.5',
        'c\tchrB\t7\t-\t-2.0\t1\t2\t-0.25', 'c\tchrB\t9\t-\t0.125\t0\t2\t-inf']
    path = os.path.join(tmp_path, 'calls.tsv')
    _batch(True).write_tsv(path)
    with open(path) as f:
        assert f.read().splitlines()[1] == 'read0\tchrA\t10\t+\t1.5\t0\t1\t1.5'
    b = _batch(False)
    assert b.cluster is None and b.llr_single is None            # existing constructions keep working
    from nadavca_amd.call_mods import ModCallBatch
    e = ModCallBatch.empty(joint=True)
    assert e.cluster.dtype == np.int32 and e.llr_single.dtype == np.float64 and len(e) == 0
    assert ModCallBatch.empty().cluster is None


def test_argument_refusals():
    """Refused before anything is loaded or aligned: no GPU is touched."""
    from nadavca_amd import call_mods_batch
    for bad in (0, -1, 2.5, 9):
        with pytest.raises(ValueError, match='max_joint'):
            call_mods_batch(None, None, None, joint=True, max_joint=bad)
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='site_prior'):
            call_mods_batch(None, None, None, joint=True, site_prior=bad)


# ---- the clustering rule on genomes ------------------------------------------------------------------------------
def test_share_of_crowded_sites_left_crowded():
    """Reads of ``make_modified_read_batch``-style genomes (uniform random bases), CG, k = 6, max_joint = 4: at most a
    tenth of the crowded sites may stay crowded (measured on random sequence: 0.068)."""
    import torch
    from nadavca_amd.call_mods import find_sites, cluster_sites
    rng = np.random.default_rng(77)
    n, L, k = 3000, 400, 6
    genome = rng.integers(0, 4, 50000).astype(np.int32)
    g0 = rng.integers(0, genome.size - L, n)
    rev = rng.random(n) < 0.5
    parts = [(3 - genome[a:a + L][::-1]) if r else genome[a:a + L] for a, r in zip(g0, rev)]
    off = torch.arange(n + 1, dtype=torch.int64) * L
    _, owner, pos, _, crowded = find_sites(torch.from_numpy(np.concatenate(parts).astype(np.int32)), off,
                                           torch.from_numpy(g0), torch.from_numpy(g0 + L), torch.from_numpy(rev),
                                           [1, 2], 0, k)
    cluster, first, size, cut = cluster_sites(owner, pos, k, 4)
    assert not (cut & ~crowded).any()                         # a cut site was crowded before
    share = float(cut.sum()) / float(crowded.sum())
    print('sites %d, crowded %.3f, of those still crowded %.3f; joint hypotheses per read %.1f beside %.1f single'
          % (pos.numel(), float(crowded.float().mean()), share,
             float(((1 << size[size > 1]) - 1).sum()) / n, float((size == 1).sum()) / n))
    assert crowded.sum() > 10000
    assert share <= 0.1


# ---- the C-ABI -----------------------------------------------------------------------------------------------------
def test_joint_entry_is_declared_three_times_alike():
    from nadavca_amd import _lib
    import ctypes as C
    with open(os.path.join(ROOT, 'include', 'nadavca_hip.h')) as f:
        header = f.read()
    m = re.search(r'int nvk_estimate_joint_hypotheses_batch_dev\(([^;]*)\);', header)
    assert m, 'nvk_estimate_joint_hypotheses_batch_dev is not declared'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES['nvk_estimate_joint_hypotheses_batch_dev']
    assert res is C.c_int and len(args) == len(params) == 27
    for p, a in zip(params, args):
        want = C.c_void_p if '*' in p else C.c_int64 if p.startswith('int64_t') else C.c_int
        assert a is want, p
    names = [p.split()[-1].lstrip('*') for p in params]
    assert names[18:] == ['total_hyp', 'hyp_off', 'total_sub', 'sub_off', 'sub_pos', 'sub_base', 'out_total',
                          'out_hyp', 'out_status']
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), 'nvk_estimate_joint_hypotheses_batch_dev')
