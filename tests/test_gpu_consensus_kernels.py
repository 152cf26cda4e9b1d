"""consensus_kernel and posterior_kernel (nadavca_amd/csrc/kernels_consensus.hip) against tests/consensus_ref.py: the
long-double restatement of the header's contract, with the error bound of every output derived there from the inputs
alone.  No DP runs here: log-likelihood rows are uploaded directly.  The chain tests hold both kernels, ``group_sums``
and the independent row bookkeeping to the reference's own results on constructed rows
(tests/golden/consensus_cases.npz).

Measured on an MI355X, the largest error / bound over everything below (each test prints its own): consensus_kernel
0.576 (one call 0.436 on the main layout, 0.576 at the block edges; two calls into the same sums 0.307),
posterior_kernel 0.741 (alphabet 2, k = 2; between 0.44 and 0.46 for alphabets 4, 5 and 8), the chain 0.242 against
the restatement and 0.432 against the reference's float64 results.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import consensus_ref as CR

pytestmark = pytest.mark.gpu

ALPHABETS = (2, 4, 5, 8)
PRIORS = (1e-6, 0.001, 0.01)
NELS = (1.0, 3.0, 10.0)
SKIPPED_IN_ADVANCE = set()  # (alphabet, k, snp_prior) outside the domain of positive priors: none of these


@pytest.fixture(scope='module')
def env():
    import torch
    from nadavca_amd import _lib
    ctx = _lib.default_context()
    return SimpleNamespace(torch=torch, ctx=ctx, dev=torch.device('cuda', ctx.device))


def _up(env, a, dt):
    return env.torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(env.dev)


def _dbatch(env, reference, ref_off):
    """the part of a DeviceBatch that consensus_accumulate_dev reads"""
    return SimpleNamespace(torch=env.torch, device=env.dev, n=len(ref_off) - 1, total_ref=int(ref_off[-1]),
                           reference=_up(env, reference, np.int32), ref_off=_up(env, ref_off, np.int64))


# ---- accumulate --------------------------------------------------------------------------------------------------------
def _reads(rng, alpha, spans):
    """``spans``: (start, length, reverse, status) per read -> namespace of the kernel's inputs as numpy arrays"""
    spans = np.array(spans, dtype=np.int64).reshape(-1, 4)
    ref_off = np.concatenate([[0], np.cumsum(spans[:, 1])]).astype(np.int64)
    total = int(ref_off[-1])
    return SimpleNamespace(ll=rng.normal(-30.0, 12.0, (total, alpha)), reference=rng.integers(0, alpha, total),
                           ref_off=ref_off, chunk_start=spans[:, 0].copy(), reverse=spans[:, 2].astype(np.int32),
                           status=spans[:, 3].astype(np.int32), lengths=spans[:, 1].copy())


def _accumulate(env, b, nel, ref_len, with_status=True, calls=1):
    from nadavca_amd.device import consensus_accumulate_dev
    db = _dbatch(env, b.reference, b.ref_off)
    ll, start, rev = _up(env, b.ll, np.float64), _up(env, b.chunk_start, np.int64), _up(env, b.reverse, np.int32)
    status = _up(env, b.status, np.int32) if with_status else None
    acc = cov = None
    for _ in range(calls):
        acc, cov = consensus_accumulate_dev(env.ctx, db, ll, start, rev, status, nel, ref_len, acc, cov)
    assert tuple(acc.shape) == (ref_len, b.ll.shape[1]) and tuple(cov.shape) == (ref_len,)
    return acc.cpu().numpy(), cov.cpu().numpy()


def _check_accumulate(env, b, nel, ref_len, with_status=True, calls=1):
    """coverage exact, the non-finite entries the same, the finite sums within the bound -> error / bound"""
    got, got_cov = _accumulate(env, b, nel, ref_len, with_status, calls)
    want, cov, bound = CR.accumulate(b.ll, b.reference, b.ref_off, b.chunk_start, b.reverse,
                                     b.status if with_status else None, nel, ref_len, repeat=calls)
    assert np.array_equal(got_cov, cov)
    finite = np.isfinite(want.astype(np.float64))
    assert np.array_equal(np.isfinite(got), finite)
    r = CR.ratio(got[finite], want[finite], bound[finite])
    assert r <= 1.0, r
    return r, cov, got


COUNTED = {20: 0, 21: 1, 22: 2, 23: 63, 24: 64, 25: 65, 26: 260}  # position: reads on it


def _main_layout(rng, alpha):
    """About 400 reads of 0 to 40 bases on 120 positions, shuffled: positions 20..26 under the counts of COUNTED,
    reads of status 1 and -3 over them, reads that hang over either end of the reference or lie outside it, random
    reads on 30..120, zero-length reads first, in the middle and last"""
    spans = [(21, 2, 0, 0), (22, 1, 1, 0)] + [(23, 3, i % 2, 0) for i in range(63)] + [(24, 2, 1, 0), (25, 1, 0, 0)]
    spans += [(26, 1 + i % 2, i % 2, 0) for i in range(260)]
    spans += [(20, 7, i % 2, 1) for i in range(3)] + [(19, 9, i % 2, -3) for i in range(3)]
    spans += [(-3, 8, 0, 0), (-3, 8, 1, 0), (110, 20, 0, 0), (105, 40, 1, 0), (125, 5, 0, 0), (-50, 10, 1, 0),
              (120, 1, 0, 0), (-1, 1, 1, 0)]
    for _ in range(70):
        length = int(rng.integers(0, 41))
        spans.append((int(rng.integers(30, 121 - length)), length, int(rng.integers(0, 2)), 0))
    spans = [spans[i] for i in rng.permutation(len(spans))]
    spans = [(40, 0, 0, 0)] + spans[:200] + [(0, 0, 1, 0), (119, 0, 0, 0)] + spans[200:] + [(60, 0, 1, 0)]
    return _reads(rng, alpha, spans)


@pytest.mark.parametrize('alpha,nel', list(zip(ALPHABETS, (1.0, 10.0, 3.0, 10.0))))
def test_accumulate_main_layout(env, alpha, nel):
    rng = np.random.default_rng(100 + alpha)
    b = _main_layout(rng, alpha)
    assert 380 <= len(b.lengths) <= 440 and b.lengths.min() == 0 and b.lengths.max() == 40
    r1, cov, _ = _check_accumulate(env, b, nel, 120)
    assert {p: int(cov[p]) for p in COUNTED} == COUNTED
    assert cov[0] == 2 and cov[4] == 2 and cov[5] == 0 and cov[119] >= 2   # the inside part of overhanging reads
    r2, cov_all, _ = _check_accumulate(env, b, nel, 120, with_status=False)  # status NULL: every read counts
    assert cov_all[20] == 6 and cov_all[19] == 3
    r3, cov2, _ = _check_accumulate(env, b, nel, 120, calls=2)              # a second call adds
    assert np.array_equal(cov2, 2 * cov)
    print('accumulate alphabet %d: error / bound %.3f, without status %.3f, two calls %.3f' % (alpha, r1, r2, r3))


@pytest.mark.parametrize('alpha', ALPHABETS)
def test_accumulate_block_edges_and_read_counts(env, alpha):
    rng = np.random.default_rng(200 + alpha)
    worst, turn = 0.0, 0
    for last in (15, 16, 17):  # total_ref 255, 256, 257: around the 256-thread block
        b = _reads(rng, alpha, [(int(rng.integers(0, 20)), 40, i % 2, 0) for i in range(6)] + [(3, last, 1, 0)])
        assert b.ref_off[-1] == 240 + last
        worst = max(worst, _check_accumulate(env, b, NELS[turn % 3], 60)[0])
        turn += 1
    for n in (1, 2, 3):
        b = _reads(rng, alpha, [(int(rng.integers(0, 5)), int(rng.integers(1, 8)), i % 2, 0) for i in range(n)])
        worst = max(worst, _check_accumulate(env, b, NELS[turn % 3], 12)[0])
        turn += 1
    spans = [(int(rng.integers(-2, 60)), int(rng.integers(0, 4)), int(rng.integers(0, 2)), int(rng.integers(0, 20) == 0))
             for _ in range(1001)]
    b = _reads(rng, alpha, spans)
    for nel in NELS:
        worst = max(worst, _check_accumulate(env, b, nel, 60)[0])
    print('accumulate alphabet %d, block edges and read counts: error / bound %.3f' % (alpha, worst))


def test_accumulate_empty_batches(env):
    rng = np.random.default_rng(7)
    for spans in ([], [(3, 0, 0, 0)], [(3, 0, 0, 0), (5, 0, 1, 0)]):
        b = _reads(rng, 4, spans)
        got, cov = _accumulate(env, b, 10.0, 9)
        assert not got.any() and not cov.any()


@pytest.mark.parametrize('alpha', ALPHABETS)
def test_accumulate_minus_infinite_shift_stays_in_its_read(env, alpha):
    """A read whose shift entry is -inf makes its own covered positions non-finite, as in the reference, and no
    others"""
    rng = np.random.default_rng(300 + alpha)
    spans = [(int(rng.integers(0, 50)), int(rng.integers(1, 12)), int(rng.integers(0, 2)), 0) for _ in range(40)]
    spans[17] = (-2, 9, 1, 0)
    spans[30] = (25, 6, 0, 0)
    b = _reads(rng, alpha, spans)
    for rd in (17, 30):
        r0 = b.ref_off[rd]
        b.ll[r0, b.reference[r0]] = -np.inf
    _, _, got = _check_accumulate(env, b, 3.0, 60)
    bad = np.nonzero(~np.isfinite(got).all(axis=1))[0]
    assert bad.tolist() == list(range(0, 7)) + list(range(25, 31))
    assert not np.isfinite(got[bad]).any()


# ---- posterior ---------------------------------------------------------------------------------------------------------
def _posterior_layout(rng, alpha, k):
    """One call: 300 positions with borders at 127, 128 and 129, then segments of every length around k (empty ones
    first, in the middle and last), then 1000 segments of 1 to 3 positions.  Rows: random, tied, all zero, single -inf
    entries, entries 2000 below, and next to every border of the first two parts a row 600 above everything."""
    lengths = [0, 127, 1, 1, 171] + [1, 2, k - 1, 0, k, k + 1, 2 * k - 2, 2 * k - 1, 2 * k, 40]
    marked = len(lengths)
    lengths += rng.integers(1, 4, 1000).tolist() + [0]
    seg_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(seg_off[-1])
    ll = rng.normal(-30.0, 12.0, (n, alpha)) * rng.choice([0.3, 1.0, 4.0], (n, 1))
    reference = rng.integers(0, alpha, n).astype(np.int32)
    kind = rng.integers(0, 12, n)
    ll[kind == 0] = np.round(ll[kind == 0][:, :1])           # tied rows
    ll[kind == 1] = 0.0                                      # uncovered positions
    at = np.nonzero(kind == 2)[0]
    ll[at, rng.integers(0, alpha, at.size)] = -np.inf         # contributes exactly 0
    at = np.nonzero(kind == 3)[0]
    ll[at, rng.integers(0, alpha, at.size)] -= 2000.0         # exp is exactly 0
    strong = []
    for j, border in enumerate(seg_off[1:marked]):
        row = int(border) - 1 if j % 2 else int(border)       # the row before the border, or the one after it
        if 0 <= row < seg_off[marked] and row not in strong:
            ll[row] = rng.normal(600.0, 5.0, alpha)
            strong.append(row)
    return ll, reference, seg_off, strong


def _posterior(env, ll, reference, seg_off, k, snp_prior):
    from nadavca_amd.device import posterior_segments_dev
    out = posterior_segments_dev(env.ctx, _up(env, ll, np.float64), _up(env, reference, np.int32),
                                 _up(env, seg_off, np.int64), k, snp_prior)
    return out.cpu().numpy()


def _check_posterior(got, post, reference):
    """within the bound; exact zeros where a single term underflows; finite rows sum to 1 -> error / bound"""
    finite = np.isfinite(post.want.astype(np.float64)).all(axis=1)
    assert finite.all()
    assert np.isfinite(got).all() and (got >= 0).all()
    r = CR.ratio(got, post.want, CR.tolerance(post))
    assert r <= 1.0, r
    single = np.ones(got.shape, dtype=bool)
    single[np.arange(len(reference)), reference] = False
    gone = single & (post.x.astype(np.float64) < -746.0)
    assert (got[gone] == 0).all()
    assert np.max(np.abs(got.astype(CR.LD).sum(axis=1) - 1)) <= 4 * CR.EPS
    return r, int(gone.sum())


@pytest.mark.parametrize('k', range(1, 7))
@pytest.mark.parametrize('alpha', ALPHABETS)
def test_posterior_segments(env, alpha, k):
    rng = np.random.default_rng(1000 + 10 * alpha + k)
    ll, reference, seg_off, strong = _posterior_layout(rng, alpha, k)
    assert {127, 128, 129} <= set(seg_off.tolist()) and len(strong) >= 8
    worst, zeros, skipped = 0.0, 0, set()
    for snp_prior in PRIORS:
        if not CR.priors_positive(snp_prior, k, alpha):
            skipped.add((alpha, k, snp_prior))
            continue
        post = CR.posterior(ll, reference, seg_off, k, snp_prior)
        r, gone = _check_posterior(_posterior(env, ll, reference, seg_off, k, snp_prior), post, reference)
        worst, zeros = max(worst, r), zeros + gone
    assert skipped <= SKIPPED_IN_ADVANCE
    assert zeros > 0
    print('posterior alphabet %d k %d: error / bound %.3f, %d exact zeros' % (alpha, k, worst, zeros))


def test_posterior_window_stops_at_the_border_next_to_a_strong_row(env):
    """The layout's strong rows do what they are there for: in the restatement, a window one position wider than the
    segment allows moves a neighbour across the border by orders of magnitude."""
    rng = np.random.default_rng(77)
    ll, reference, seg_off, strong = _posterior_layout(rng, 4, 3)
    post = CR.posterior(ll, reference, seg_off, 3, 0.001)
    merged = CR.posterior(ll, reference, np.array([0, seg_off[-1]]), 3, 0.001)
    assert CR.ratio(merged.want, post.want, CR.tolerance(post)) > 1e9
    got = _posterior(env, ll, reference, seg_off, 3, 0.001)
    assert CR.ratio(got, post.want, CR.tolerance(post)) <= 1.0


def test_posterior_non_finite_sums_spoil_exactly_the_windows_that_hold_them(env):
    """Rows as a read with a -inf shift leaves them (+inf, NaN in its reference column): NaN on every position whose
    window, clipped at the segment's borders, holds such a row, as in the reference, and the others within the bound"""
    rng = np.random.default_rng(78)
    k, seg_off = 3, np.array([0, 30, 35, 65], dtype=np.int64)
    ll = rng.normal(-30.0, 12.0, (65, 4))
    reference = rng.integers(0, 4, 65).astype(np.int32)
    for row in (12, 34):
        ll[row] = np.inf
        ll[row, reference[row]] = np.nan
    spoiled = np.zeros(65, dtype=bool)
    spoiled[[10, 11, 12, 13, 14, 32, 33, 34]] = True
    post = CR.posterior(ll, reference, seg_off, k, 0.001)
    assert np.array_equal(np.isnan(post.want.astype(np.float64)), np.repeat(spoiled[:, None], 4, axis=1))
    got = _posterior(env, ll, reference, seg_off, k, 0.001)
    assert np.array_equal(np.isnan(got), np.repeat(spoiled[:, None], 4, axis=1))
    assert CR.ratio(got[~spoiled], post.want[~spoiled], CR.tolerance(post)[~spoiled]) <= 1.0


# ---- the chain against the reference's own results -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    return [(c, CR.expected_consensus(c), CR.expected_independent(c)) for c in CR.load_cases()]


def test_chain_reproduces_the_reference_consensus_chunks(env, golden):
    from nadavca_amd import estimator as E
    from nadavca_amd.device import consensus_accumulate_dev
    worst_ref = worst = 0.0
    for c, (groups, cov, post, seg_off), _ in golden:
        db = _dbatch(env, c.reference, c.ref_off)
        acc, dcov = consensus_accumulate_dev(env.ctx, db, _up(env, c.ll, np.float64), _up(env, c.chunk_start, np.int64),
                                             _up(env, c.reverse, np.int32), None, c.nel, len(c.codes))
        model = SimpleNamespace(context=env.ctx, get_k=lambda k=c.k: k)
        chunks = E.consensus_chunks(model, c.snp_prior, c.codes, acc, dcov, c.ranges)
        assert [(ch.start, ch.end) for ch in chunks] == [tuple(r) for r in c.cons_ranges.tolist()]
        assert np.array_equal(np.concatenate([ch.coverage for ch in chunks]), c.cons_coverage)
        values = np.concatenate([ch.values for ch in chunks])
        tol = CR.tolerance(post)
        worst = max(worst, CR.ratio(values, post.want, tol))
        worst_ref = max(worst_ref, CR.ratio(values, c.cons_values.astype(CR.LD), tol))
    print('chain, consensus chunks: error / bound %.3f against the restatement, %.3f against the reference'
          % (worst, worst_ref))
    assert worst <= 1.0 and worst_ref <= 1.0


def test_chain_reproduces_the_reference_independent_chunks(env, golden):
    from nadavca_amd import estimator as E
    worst_ref = worst = 0.0
    for c, _, post in golden:
        db = _dbatch(env, c.reference, c.ref_off)
        status = np.zeros(len(c.ranges), dtype=np.int32)
        status[1::5] = 1  # such reads yield no rows, the others keep theirs
        codes = np.concatenate([c.codes[s:e] for s, e in c.ranges])
        model = SimpleNamespace(context=env.ctx, get_k=lambda k=c.k: k)
        ok, values, row_off = E.independent_posteriors(model, c.snp_prior, c.nel, db, _up(env, c.ll, np.float64),
                                                       _up(env, status, np.int32), _up(env, c.reverse, np.int32),
                                                       _up(env, codes, np.int32))
        assert np.array_equal(ok, status == 0)
        lengths = np.diff(c.ref_off)
        assert np.array_equal(row_off, np.concatenate([[0], np.cumsum(lengths[ok])]))
        rows = np.repeat(ok, lengths)
        tol = CR.tolerance(post)[rows]
        worst = max(worst, CR.ratio(values, post.want[rows], tol))
        worst_ref = max(worst_ref, CR.ratio(values, c.ind_values[rows].astype(CR.LD), tol))
    print('chain, independent chunks: error / bound %.3f against the restatement, %.3f against the reference'
          % (worst, worst_ref))
    assert worst <= 1.0 and worst_ref <= 1.0


# ---- argument checks -----------------------------------------------------------------------------------------------------
def test_accumulate_rejects_bad_arguments(env):
    from nadavca_amd import _lib
    from nadavca_amd.device import consensus_accumulate_dev
    lib = _lib.load()
    rng = np.random.default_rng(5)
    b = _reads(rng, 4, [(0, 5, 0, 0), (2, 4, 1, 0)])
    db = _dbatch(env, b.reference, b.ref_off)
    ll, start, rev = _up(env, b.ll, np.float64), _up(env, b.chunk_start, np.int64), _up(env, b.reverse, np.int32)
    acc, cov = consensus_accumulate_dev(env.ctx, db, ll, start, rev, None, 10.0, 8)
    before = acc.cpu().numpy().copy()
    for nel in (0.0, -0.0, float('nan'), float('inf'), float('-inf')):
        with pytest.raises(ValueError):
            consensus_accumulate_dev(env.ctx, db, ll, start, rev, None, nel, 8, acc, cov)
    for alpha in (1, 9):
        wide = _up(env, rng.normal(0, 1, (9, alpha)), np.float64)
        with pytest.raises(ValueError):
            consensus_accumulate_dev(env.ctx, db, wide, start, rev, None, 10.0, 8)
    p = lambda t: t.data_ptr()
    args = lambda: [env.ctx.handle, 2, 9, 4, p(ll), p(db.reference), p(db.ref_off), p(start), p(rev), None, 10.0, 8,
                    p(acc), p(cov)]
    for at, value in ((0, None), (1, -1), (2, -1), (11, -1)):  # NULL context, negative counts and length
        a = args()
        a[at] = value
        assert lib.nvk_consensus_accumulate_dev(*a) == _lib.NVK_ERR_INVALID
    assert np.array_equal(acc.cpu().numpy(), before) and cov.sum().item() == 9
    assert lib.nvk_consensus_accumulate_dev(*args()) == _lib.NVK_OK


def test_posterior_rejects_bad_arguments(env):
    from nadavca_amd import _lib
    from nadavca_amd.device import posterior_segments_dev
    lib = _lib.load()
    rng = np.random.default_rng(6)
    ll, ref = _up(env, rng.normal(-30, 12, (7, 4)), np.float64), _up(env, rng.integers(0, 4, 7), np.int32)
    seg = _up(env, [0, 3, 7], np.int64)
    with pytest.raises(ValueError):
        posterior_segments_dev(env.ctx, ll, ref, seg, 0, 0.001)
    for alpha in (1, 9):
        with pytest.raises(ValueError):
            posterior_segments_dev(env.ctx, _up(env, np.zeros((7, alpha)), np.float64), ref, seg, 3, 0.001)
    out = env.torch.empty_like(ll)
    p = lambda t: t.data_ptr()
    args = lambda: [env.ctx.handle, 7, 2, p(seg), 4, 3, 0.001, p(ll), p(ref), p(out)]
    for at, value in ((0, None), (1, -1), (2, -1), (3, None)):  # NULL context, negative counts, NULL seg_off
        a = args()
        a[at] = value
        assert lib.nvk_posterior_segments_dev(*a) == _lib.NVK_ERR_INVALID
    assert lib.nvk_posterior_segments_dev(*args()) == _lib.NVK_OK
