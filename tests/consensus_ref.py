"""The CPU side of the consensus tests: nvk_consensus_accumulate_dev and nvk_posterior_segments_dev
(include/nadavca_hip.h, nadavca_amd/csrc/kernels_consensus.hip) restated in numpy ``longdouble`` (80-bit on x86: 64
bits of mantissa, exponents to 2^-16445), the error bound of every output computed from the inputs alone, and the
reading of tests/golden/consensus_cases.npz (oracle/make_golden_consensus.py: the reference's own
``ProbabilityEstimator.estimate_probabilities`` on constructed log-likelihoods).

The rules
---------
Accumulation, per read with status 0 (or every read without a status): ``rows = (ll - ll[0][reference[0]]) / nel``;
on the reverse strand column b -> alphabet - 1 - b and the rows flipped; ``acc[chunk_start + p] += rows[p]`` and
``coverage[chunk_start + p] += 1`` for the positions inside [0, ref_len).

Posterior, per position i of a segment [s0, s1): the window is [max(s0, i - k + 1), min(s1, i + k)), ``mx`` the largest
entry in it, ``snp_h = 1 / (p1 / p2 + (1 - (W - 1)) * c)`` and ``non_h = 1 - snp_h * c`` with W the window's positions,
c = alphabet - 1, p1 = 1 - snp_prior, p2 = snp_prior / c.  ``pr[j] = exp(ll[i][j] - mx) * snp_h`` for the other bases,
``pr[ref] = exp(ll[i][ref] - mx) * non_h + snp_h * sum of exp(ll[q][b] - mx)`` over the window's other positions q and
their non-reference bases b; the output is ``pr / sum(pr)``.

The bounds (u = 2^-53, eps = 2^-52)
-----------------------------------
Sums.  A term is (ll - shift) / nel.  The kernel rounds the subtraction, 1 / nel and the product: at most 3u relative
on the term.  ``n`` terms meet in n - 1 rounded additions in any order (the atomics fix none), each off by at most u
times a partial sum, which is at most the sum of the terms' magnitudes.  So

    |got - want| <= (coverage + 2) * u * sum |terms|        per entry,

to first order in u (the second order is below 2^-90 relative at the coverages used).  The reference divides by nel
(2 roundings per term) and adds in sorted chunk order: inside the same bound.  A second call into the same sums
doubles the term list; the bound is the one of the doubled list.

Posterior, from the same float64 ``ll`` as the kernel gets.  Every term is a non-negative exp(x) * prior, so nothing
cancels and relative errors carry through the additions and the division:
  * x = ll - mx is rounded once: |x| u absolute in x, hence |x| u relative in exp(x).  X, the largest |x| among the
    terms of the row's sum that do not underflow (x >= -745.2), covers it for the numerator and the denominator.
  * T, the number of terms added into the row (alphabet + (W - 1) (alphabet - 1)), covers the additions, u each.
  * the constant covers an exp good to 2 ulp, the priors (five roundings in snp_h; non_h is 1 - snp_h c with
    snp_h c < 0.1 on the domain below, so it inherits less than one u), the prior products and the division.

    |got - want| <= (X + T + 8) * eps * |want|              per entry with |want| >= 2^-1000.

The factor eps where the count above is in u leaves the correlated errors of numerator and denominator their room.
Below 2^-1000 the same factor applies to 2^-1000: such values come from denormal terms, which have no relative
precision.  One more absolute term covers what denormals do to larger outputs when the row's sum itself is tiny
(the window's maximum may sit in a neighbour's reference column, which is in no sum): each of the T terms may lose
2^-1074 twice (exp, product), in units of the row's sum s, so T * 2^-1073 / s is added.  It also covers the restatement
keeping what float64 flushes to 0 (exp below -745.13), which is why nothing here has to imitate the underflow.  With s
near 1 it is below 2^-1060 and plays no part.

The domain: both corrected priors positive, p1 / p2 > W_max * c with W_max = 2k - 2 context positions
(``priors_positive``; p1 / p2 > (W_max - 1) c keeps snp_h positive, one more c keeps non_h positive).  Outside it
the reference's own arithmetic cancels and no bound holds.

The chain against the golden.  The golden's posterior comes from float64 sums added in another order: entries off by
at most the sums bound d.  In exact arithmetic mx cancels in pr / sum(pr), each term moves by a factor within
exp(+-d), the ratio within exp(+-2 d_max): the posterior bound plus twice the largest sums bound in the window.

Measured (tests/test_consensus_cpu.py prints them): the reference's own float64 results in the golden reach at most
0.233 of the chain bound on the consensus chunks and 0.254 on the independent chunks, so a correct float64 evaluation
stays well inside.
"""
import os
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'consensus_cases.npz')
LD = np.longdouble
U = LD(2) ** -53
EPS = LD(2) ** -52
TINY = LD(2) ** -1000
DENORMAL = LD(2) ** -1073
UNDERFLOW = -745.2  # exp(x) is 0 in float64 below -745.13


def corrected_priors(context_positions, snp_prior, alpha):
    """``_corrected_priors`` in long double -> (snp_h, non_h)"""
    c = LD(alpha - 1)
    p1, p2 = 1 - LD(snp_prior), LD(snp_prior) / c
    snp_h = 1 / (p1 / p2 + (1 - LD(context_positions)) * c)
    return snp_h, 1 - snp_h * c


def priors_positive(snp_prior, k, alpha):
    """The domain of the posterior bound: both corrected priors positive for every window of up to 2k - 1 positions"""
    c = alpha - 1
    ratio = (1 - snp_prior) / (snp_prior / c)
    return ratio > (2 * k - 3) * c and ratio > (2 * k - 2) * c


def accumulate(ll, reference, ref_off, chunk_start, reverse, status, nel, ref_len, repeat=1):
    """-> (acc (ref_len, alpha) long double, coverage (ref_len,) i64, bound (ref_len, alpha) long double) after
    ``repeat`` calls into the same sums"""
    ll = np.asarray(ll, dtype=np.float64)
    alpha = ll.shape[1]
    acc, mag = np.zeros((ref_len, alpha), dtype=LD), np.zeros((ref_len, alpha), dtype=LD)
    cov = np.zeros(ref_len, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for rd in range(len(ref_off) - 1):
            r0, r1 = int(ref_off[rd]), int(ref_off[rd + 1])
            if r1 == r0 or (status is not None and status[rd] != 0):
                continue
            rows = (ll[r0:r1].astype(LD) - LD(ll[r0, reference[r0]])) / LD(nel)
            if reverse[rd]:
                rows = rows[::-1, ::-1]
            pos = int(chunk_start[rd]) + np.arange(r1 - r0)
            keep = (pos >= 0) & (pos < ref_len)
            acc[pos[keep]] += rows[keep]  # a read covers a position once
            mag[pos[keep]] += np.abs(rows[keep])
            cov[pos[keep]] += 1
        acc, mag, cov = acc * repeat, mag * repeat, cov * repeat
        return acc, cov, (cov + 2)[:, None] * U * mag


def posterior(ll, reference, seg_off, k, snp_prior, ll_bound=None):
    """``ll`` (n, alpha), ``reference`` (n,) codes, ``seg_off`` (segments + 1,) -> namespace of
    want (n, alpha) long double, rel (n,): the relative bound (X + T + 8) eps — plus twice the largest entry of
    ``ll_bound`` in the window, where given —, floor (n,): the absolute term T 2^-1073 / s, x (n, alpha): ll[i] - mx."""
    ll = np.asarray(ll, dtype=LD)
    n, alpha = ll.shape
    want, x_row = np.full((n, alpha), np.nan, dtype=LD), np.full((n, alpha), np.nan, dtype=LD)
    rel, floor = np.full(n, np.nan, dtype=LD), np.full(n, np.nan, dtype=LD)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        for s0, s1 in zip(seg_off[:-1], seg_off[1:]):
            for i in range(int(s0), int(s1)):
                cs, ce = max(int(s0), i - k + 1), min(int(s1), i + k)
                x = ll[cs:ce] - ll[cs:ce].max()
                e = np.exp(x)
                snp_h, non_h = corrected_priors(ce - cs - 1, snp_prior, alpha)
                context = np.ones(x.shape, dtype=bool)  # the other positions' non-reference bases
                context[np.arange(ce - cs), reference[cs:ce]] = False
                context[i - cs] = False
                ri = reference[i]
                pr = e[i - cs] * snp_h
                pr[ri] = e[i - cs, ri] * non_h + e[context].sum() * snp_h
                s = pr.sum()
                want[i], x_row[i] = pr / s, x[i - cs]
                terms = np.concatenate([x[i - cs], x[context]])
                live = terms[terms >= UNDERFLOW]
                rel[i] = ((np.abs(live).max() if live.size else 0) + terms.size + 8) * EPS
                if ll_bound is not None:
                    rel[i] += 2 * np.max(ll_bound[cs:ce])
                floor[i] = terms.size * DENORMAL / s
    return SimpleNamespace(want=want, rel=rel, floor=floor, x=x_row)


def tolerance(post):
    """The absolute error allowed per entry of ``posterior``'s result"""
    return post.rel[:, None] * np.maximum(np.abs(post.want), TINY) + post.floor[:, None]


def ratio(got, want, bound):
    """The largest |got - want| / bound over the entries (0 for none)"""
    err = np.abs(np.asarray(got, dtype=LD) - want)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def group_ranges(ranges):
    """estimator.py:205-220 once more, plainly: sorted intervals merge while the next one starts before the group's
    end -> [(start, end)]"""
    groups = []
    for s, e in sorted(ranges):
        if groups and s < groups[-1][1]:
            groups[-1][1] = max(groups[-1][1], e)
        else:
            groups.append([s, e])
    return [tuple(g) for g in groups]


# ---- the golden ------------------------------------------------------------------------------------------------------
def load_cases():
    """tests/golden/consensus_cases.npz -> list of namespaces: the stored arrays plus what the kernels take — codes
    (genome as base codes), reference (the reads' strand-corrected codes end to end), ref_off, chunk_start, reverse"""
    z = np.load(GOLDEN, allow_pickle=False)
    cases = []
    for c in range(int(z['n_cases'])):
        pre = 'c%d_' % c
        d = {key[len(pre):]: np.array(z[key]) for key in z.files if key.startswith(pre)}
        case = SimpleNamespace(**d)
        case.k, case.snp_prior, case.nel = int(case.k), float(case.snp_prior), float(case.nel)
        case.codes = np.array(['ACGT'.index(b) for b in str(case.genome)], dtype=np.int32)
        parts = [case.codes[s:e] if not rev else (3 - case.codes[s:e])[::-1] for s, e, rev in case.reads]
        case.reference = np.concatenate(parts).astype(np.int32)
        case.ref_off = np.concatenate([[0], np.cumsum(case.reads[:, 1] - case.reads[:, 0])]).astype(np.int64)
        case.chunk_start = case.reads[:, 0].astype(np.int64)
        case.reverse = case.reads[:, 2].astype(np.int32)
        case.ranges = [(int(s), int(e)) for s, e, _ in case.reads]
        cases.append(case)
    return cases


def expected_consensus(case):
    """The restatement's chunks of a golden case: -> (groups, coverage (L,), posterior namespace over the groups end
    to end with the chain bound, seg_off)"""
    L = len(case.codes)
    acc, cov, bound = accumulate(case.ll, case.reference, case.ref_off, case.chunk_start, case.reverse, None,
                                 case.nel, L)
    groups = group_ranges(case.ranges)
    seg_off = np.cumsum([0] + [e - s for s, e in groups])
    pos = np.concatenate([np.arange(s, e) for s, e in groups])
    return groups, cov, posterior(acc[pos], case.codes[pos], seg_off, case.k, case.snp_prior, bound[pos]), seg_off


def expected_independent(case):
    """Every read its own segment, laid out as ``case.ll``: -> posterior namespace with the chain bound"""
    n = int(case.ref_off[-1])
    acc, _, bound = accumulate(case.ll, case.reference, case.ref_off, case.ref_off[:-1], case.reverse, None,
                               case.nel, n)
    codes = np.concatenate([case.codes[s:e] for s, e in case.ranges])
    return posterior(acc, codes, case.ref_off, case.k, case.snp_prior, bound)
