"""``call_mods_batch(joint=True)`` on the GPU, on ``make_modified_read_batch`` with the 5-letter extension of the
packaged table (as tests/test_gpu_call_mods.py): the rows and single ratios against the ``joint=False`` run bit for
bit, the clustered rows' ratios against the marginal recomputed on the host from
``dtw.estimate_joint_hypotheses_batch`` on the same alignment stage, ``crowded`` against the cut clusters, and the
number of wrongly signed calls among the clustered rows, which the joint ratio must lower."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_READS = 1200


@pytest.fixture(scope='module')
def model5():
    """The packaged 6-mer table extended to 5 letters: an M k-mer = its C k-mer's level + N(0, 0.6^2)."""
    from nadavca_amd import synthetic, kmer_train
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
    mean5 = mean5 + np.where(has_m, np.random.default_rng(5).normal(0.0, 0.6, 5 ** k), 0.0)
    return k, central, 5, mean5, sigma5


@pytest.fixture(scope='module')
def km5(model5):
    from nadavca_amd import dtw
    return dtw.KmerModel(*model5)


def _lse(xs):
    xs = [x for x in xs if x != -math.inf]
    if not xs:
        return -math.inf
    m = max(xs)
    return m + math.log(sum(math.exp(x - m) for x in xs))


def _host_clusters(ps, k, max_joint):
    """The clustering rule as a walk over one read's ascending site positions -> list of lists of positions."""
    out = []
    for i, p in enumerate(ps):
        if i and p - ps[i - 1] <= k - 1 and p - out[-1][0] <= 14 - k and len(out[-1]) < max_joint:
            out[-1].append(p)
        else:
            out.append([p])
    return out


def _host_expectation(rb, aligner, km, config, k, max_joint, prior):
    """The alignment stage, its reads on the host, a plain walk for the clusters, every subset of every cluster
    through dtw.estimate_joint_hypotheses_batch, and the marginal by enumeration.
    -> rows (read, contig, position, strand, llr, llr_single, cluster size, cut) in the workflow's order."""
    from nadavca_amd import defaults, dtw
    from nadavca_amd.batchflow import align_batch
    from nadavca_amd.readbatch import contig_local_range
    res = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
    stage, sa, db = res.stage, res.stage.sa, res.stage.dbatch
    align_status = res.status.cpu().numpy()
    start, end = (x.cpu().numpy() for x in contig_local_range(sa, stage.reference))
    live, rev, contig = sa.live.cpu().numpy(), sa.reverse.cpu().numpy(), sa.contig.cpu().numpy()
    h = lambda t: t.cpu().numpy()
    sig, so, ref, ro = h(db.signal), h(db.sig_off), h(db.reference), h(db.ref_off)
    cb, cbo, ca, cao = h(db.context_before), h(db.cb_off), h(db.context_after), h(db.ca_off)
    anc, ao = h(db.anchors).reshape(-1, 2), h(db.anc_off)
    reads, lists, clusters = [], [], []
    for j in range(len(live)):
        part = ref[ro[j]:ro[j + 1]]
        reads.append((sig[so[j]:so[j + 1]], part, cb[cbo[j]:cbo[j + 1]], ca[cao[j]:cao[j + 1]], anc[ao[j]:ao[j + 1]]))
        ps = [q for q in range(len(part) - 1) if part[q] == 1 and part[q + 1] == 2] if align_status[j] == 0 else []
        cl = _host_clusters(ps, k, max_joint)
        clusters.append(cl)
        lists.append([np.array([[p, 4] for t, p in enumerate(c) if mask >> t & 1])
                      for c in cl for mask in range(1, 1 << len(c))])
    total, vals, status = dtw.estimate_joint_hypotheses_batch(
        reads, lists, config['bandwidth'], config['min_event_length'], km, config['model_wobbling'],
        on_error='status', return_status=True)
    lp, lq = math.log(prior), math.log(1 - prior)
    rows = []
    for j in range(len(live)):
        if align_status[j] != 0 or status[j] != 0:
            continue
        at = 0
        everyone = [p for c in clusters[j] for p in c]
        for c in clusters[j]:
            m = len(c)
            v = [total[j]] + list(vals[j][at:at + (1 << m) - 1])        # v[mask]
            at += (1 << m) - 1
            for t, p in enumerate(c):
                num, den = [], []
                for mask in range(1 << m):
                    held = bin(mask & ~(1 << t)).count('1')
                    (num if mask >> t & 1 else den).append(v[mask] + held * lp + (m - 1 - held) * lq)
                cut = any(abs(p2 - p) <= k - 1 and p2 not in c for p2 in everyone)
                f = end[j] - 1 - p if rev[j] else start[j] + p
                rows.append((int(live[j]), int(contig[j]), int(f), int(rev[j]), _lse(num) - _lse(den),
                             v[1 << t] - total[j], m, cut))
    return rows


def _check(mb, mb0, rows, k):
    """mb: joint=True, mb0: joint=False on the same batch, rows: the host expectation."""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    assert len(mb) == len(mb0) == len(rows) and len(rows) > 0
    for name in ('read', 'position', 'strand', 'contig', 'live', 'status'):
        assert np.array_equal(getattr(mb, name), getattr(mb0, name)), name
    assert np.array_equal(bits(mb.total), bits(mb0.total))
    assert mb.read.tolist() == [r[0] for r in rows] and mb.contig.tolist() == [r[1] for r in rows]
    assert mb.position.tolist() == [r[2] for r in rows] and mb.strand.tolist() == [r[3] for r in rows]
    assert mb.cluster.dtype == np.int32 and mb.cluster.tolist() == [r[6] for r in rows]
    assert not np.isnan(mb.llr).any() and not np.isnan(mb.llr_single).any()
    # the single ratio of every row, and the ratio of every row that was scored alone: the joint=False run's
    assert np.array_equal(bits(mb.llr_single), bits(mb0.llr))
    alone = mb.cluster == 1
    assert np.array_equal(bits(mb.llr[alone]), bits(mb0.llr[alone]))
    single = np.array([r[5] for r in rows])
    assert np.array_equal(np.isinf(mb.llr_single), np.isinf(single))
    assert np.allclose(mb.llr_single[np.isfinite(single)], single[np.isfinite(single)], rtol=1e-12, atol=1e-12)
    # clustered rows: the same numbers through another logsumexp order
    exp = np.array([r[4] for r in rows])
    assert np.array_equal(np.isinf(mb.llr), np.isinf(exp))
    fin = np.isfinite(exp) & ~alone
    err = float(np.max(np.abs(mb.llr[fin] - exp[fin]) / np.maximum(np.abs(exp[fin]), 1e-300)))
    print('rows %d, clustered %d, largest relative |llr - host marginal| %.3e' % (len(rows), int((~alone).sum()), err))
    assert np.allclose(mb.llr[fin], exp[fin], rtol=1e-12, atol=1e-12), err
    # crowded: exactly the cut clusters, and never a site that was not crowded before
    assert mb.crowded.tolist() == [r[7] for r in rows]
    assert not (mb.crowded & ~mb0.crowded).any()
    assert (mb0.crowded[~alone]).all() and (mb0.crowded[alone] == mb.crowded[alone]).all()


def test_joint_rows_marginals_and_wrong_calls(model5, km5):
    from nadavca_amd import call_mods_batch, defaults, synthetic
    from nadavca_amd.batchflow import load_config
    config = load_config(defaults.CONFIG_FILE)
    k = model5[0]
    rb, aligner, genome, truth = synthetic.make_modified_read_batch(N_READS, model5, seed=21)
    mb0 = call_mods_batch(rb, aligner, km5)
    mb = call_mods_batch(rb, aligner, km5, joint=True)
    assert mb0.cluster is None and mb0.llr_single is None
    rows = _host_expectation(rb, aligner, km5, config, k, 4, 0.5)
    _check(mb, mb0, rows, k)
    assert 0.3 < np.mean(mb.cluster > 1) < 0.5 and 3 <= mb.cluster.max() <= 4   # (four CG in 9 bases are rare)
    left = float(mb.crowded.sum()) / float(mb0.crowded.sum())
    print('crowded rows %.3f -> %.3f of all (%.3f of the crowded ones stay crowded)'
          % (mb0.crowded.mean(), mb.crowded.mean(), left))

    # wrongly signed calls among the clustered rows: the marginal must have fewer than the single ratio
    is_mod = np.where(mb.strand == 0, truth['forward'][mb.position], truth['reverse'][mb.position])
    sel = mb.cluster > 1
    wrong = lambda llr: int(np.sum(np.where(is_mod[sel], llr[sel] <= 0, llr[sel] >= 0)))
    w_joint, w_single = wrong(mb.llr), wrong(mb.llr_single)
    share = lambda llr, rows_: (float(np.mean(llr[rows_ & is_mod] > 0)), float(np.mean(llr[rows_ & ~is_mod] < 0)))
    print('clustered rows %d: wrong sign on %d with the joint ratio, on %d with the single one' % (sel.sum(), w_joint,
                                                                                                 w_single))
    print('correctly signed (modified / unmodified): clustered rows joint %.3f / %.3f, single %.3f / %.3f; '
          'all rows joint %.3f / %.3f, single %.3f / %.3f'
          % (share(mb.llr, sel) + share(mb.llr_single, sel) + share(mb.llr, sel | True)
             + share(mb.llr_single, sel | True)))
    assert sel.sum() > 5000
    assert w_joint < w_single

    # a smaller max_joint and another prior: the same checks, more cuts
    mb2 = call_mods_batch(rb, aligner, km5, joint=True, max_joint=2, site_prior=0.2)
    _check(mb2, mb0, _host_expectation(rb, aligner, km5, config, k, 2, 0.2), k)
    assert mb2.cluster.max() == 2 and mb2.crowded.sum() > mb.crowded.sum()
    # max_joint = 1: joint=False with the two columns
    mb1 = call_mods_batch(rb, aligner, km5, joint=True, max_joint=1)
    assert (mb1.cluster == 1).all() and np.array_equal(mb1.crowded, mb0.crowded)
    assert np.array_equal(mb1.llr.view(np.int64), mb0.llr.view(np.int64))

    # the TSV carries the two columns
    import io
    out = io.StringIO()
    mb.write_tsv(out)
    lines = out.getvalue().splitlines()
    assert lines[0].split('\t')[-2:] == ['cluster', 'llr_single'] and len(lines) == len(mb) + 1
    assert lines[1].split('\t')[-2:] == [str(mb.cluster[0]), repr(float(mb.llr_single[0]))]


def test_joint_contigs_with_seed_aligner(model5, km5):
    """Reads of three contigs through ``SeedAligner`` over a ``ReferenceSet``: contig-local positions, as the single
    form."""
    from contig_fixture import concat_batches
    from nadavca_amd import call_mods_batch, defaults, synthetic, SeedAligner, ReferenceSet
    from nadavca_amd.batchflow import load_config
    config = load_config(defaults.CONFIG_FILE)
    parts = [synthetic.make_modified_read_batch(n, model5, seed=seed, genome_length=g)
             for n, seed, g in ((300, 41, 10000), (300, 42, 4000), (200, 43, 1500))]
    names = ['chrA', 'chrB', 'chrC']
    contigs = [p[2] for p in parts]
    refset = ReferenceSet.from_arrays(names, contigs)
    rb = concat_batches([p[0] for p in parts])
    aligner = SeedAligner(refset)
    mb0 = call_mods_batch(rb, aligner, km5)
    mb = call_mods_batch(rb, aligner, km5, joint=True)
    _check(mb, mb0, _host_expectation(rb, aligner, km5, config, model5[0], 4, 0.5), model5[0])
    assert mb.contig_names == names and set(mb.contig.tolist()) == {0, 1, 2} and len(mb) > 10000
    first = np.cumsum([0, 300, 300])
    for r, c, p, s in zip(mb.read.tolist(), mb.contig.tolist(), mb.position.tolist(), mb.strand.tolist()):
        g = contigs[c]
        assert c == np.searchsorted(first, r, side='right') - 1           # the read's true contig
        assert (g[p] == 1 and g[p + 1] == 2) if s == 0 else (g[p] == 2 and g[p - 1] == 1)


def test_joint_empty_batches(model5, km5):
    from nadavca_amd import call_mods_batch, synthetic
    from nadavca_amd.readbatch import BaseAlignmentBatch, SyntheticBatchAligner
    rb, aligner, genome, truth = synthetic.make_modified_read_batch(32, model5, seed=22, genome_length=3000)
    none = SyntheticBatchAligner(genome, BaseAlignmentBatch(np.zeros(0, np.int32), np.zeros(0, np.int64),
                                                            np.zeros(rb.n + 1, np.int64), np.zeros(rb.n, bool)))
    mb = call_mods_batch(rb, none, km5, joint=True)
    assert len(mb) == 0 and mb.cluster.size == 0 and mb.llr_single.dtype == np.float64
    for pattern in ('CN', 'A' * 14):
        mb = call_mods_batch(rb, aligner, km5, pattern=pattern, joint=True)
        assert len(mb) == 0 and mb.live.size == rb.n and (mb.status == 0).all() and np.isfinite(mb.total).all()
        assert mb.cluster.size == 0 and mb.llr_single.size == 0
    assert len(call_mods_batch(rb, aligner, km5, joint=True)) > 0
