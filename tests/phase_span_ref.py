"""The span contract of include/nadavca_hip.h (nvk_phase_span_links_dev / nvk_phase_tag_blocks_dev and the forest
between them) restated in plain numpy float64, on the (has, E) of ``phase_ref.evidence``.  As in tests/phase_ref.py
every function returns the margin of each decision it takes.  The yardstick of the CPU and the GPU tests of
``phase_reads_batch(span=...)``; nothing here touches the package's kernels."""
import numpy as np

import phase_ref
from phase_ref import link_term, sum64, votes


def first_of_chain(chain_flag):
    """chain flags -> site_first: the last site at or before s whose flag is 0 (site 0 opens a chain whatever its
    flag)."""
    first, cur = np.zeros(len(chain_flag), dtype=np.int64), 0
    for s in range(len(chain_flag)):
        if s == 0 or not chain_flag[s]:
            cur = s
        first[s] = cur
    return first


def span_links(has, E, site_first, span):
    """-> (link (S, span), shared (S, span) int64): column w - 1 of row s over the rows of site s (its reads,
    ascending), those shared with s - w; 0 where s - w < site_first[s]."""
    S = has.shape[1]
    link, shared = np.zeros((S, span)), np.zeros((S, span), dtype=np.int64)
    for s in range(S):
        rows = np.nonzero(has[:, s])[0]
        for w in range(1, span + 1):
            p = s - w
            if p < site_first[s] or p < 0:
                continue
            both = has[rows, p]
            terms = np.where(both, link_term(E[rows, p], E[rows, s]), 0.0)
            link[s, w - 1], shared[s, w - 1] = sum64(terms), int(both.sum())
    return link, shared


def forest(link, shared, site_first, min_shared, min_link):
    """Sequential.  -> (parent (S,), block (S,), sigma (S,) int64, margins): margins['join'] the smallest
    | |link| - min_link | over the candidates whose qualification the link decides, margins['sign'] the smallest |link|
    of a chosen candidate, margins['choice'] the smallest gap between a site's best and second-best qualifying |link|
    (0 on a tie, which the smaller w wins)."""
    S, span = link.shape
    parent, block = np.full(S, -1, dtype=np.int64), np.arange(S, dtype=np.int64)
    sigma = np.ones(S, dtype=np.int64)
    join = sign = choice = np.inf
    for s in range(S):
        best = None
        mags = []
        for w in range(1, span + 1):
            if s - w < site_first[s] or s - w < 0 or shared[s, w - 1] < min_shared:
                continue
            mag = abs(link[s, w - 1])
            join = min(join, abs(mag - min_link))
            if not mag >= min_link:
                continue
            mags.append(mag)
            if best is None or mag > abs(link[s, best - 1]):
                best = w
        if best is None:
            continue
        mags.sort()
        if len(mags) > 1:
            choice = min(choice, mags[-1] - mags[-2])
        sign = min(sign, mags[-1])
        parent[s] = s - best
        block[s] = block[s - best]
        sigma[s] = sigma[s - best] * (1 if link[s, best - 1] > 0 else -1)
    return parent, block, sigma, dict(join=join, sign=sign, choice=choice)


def tag_blocks(has, E, block, sigma):
    """-> (read_block (n,) int64, read_llr (n,), read_sites (n,) int64, margins): per read and block the left-to-right
    sum of sigma_s * e_is over ALL of the read's sites in that block, ascending s; the block with the largest |H|, the
    smallest block index on ties.  Margins as ``phase_ref.tag``."""
    n = has.shape[0]
    read_block, read_llr = np.full(n, -1, dtype=np.int64), np.zeros(n)
    read_sites = np.zeros(n, dtype=np.int64)
    gap = llr = np.inf
    for i in range(n):
        sums = {}                    # block -> [H, sites]
        for s in np.nonzero(has[i])[0]:
            acc = sums.setdefault(int(block[s]), [0.0, 0])
            acc[0] = acc[0] + float(sigma[s]) * E[i, s]
            acc[1] += 1
        best = None
        for b in sorted(sums):
            if best is None or abs(sums[b][0]) > abs(sums[best][0]):
                best = b
        if best is not None:
            read_block[i], (read_llr[i], read_sites[i]) = best, sums[best]
            rest = [abs(v[0]) for b, v in sums.items() if b != best]
            if rest:
                gap = min(gap, abs(sums[best][0]) - max(rest))
            llr = min(llr, abs(sums[best][0]))
    return read_block, read_llr, read_sites, dict(gap=gap, llr=llr)


def refine_span(has, E, site_first, min_shared, min_link, rounds, span):
    """The whole back half under ``span``: span links, forest, ``rounds`` rounds of tag / vote / flip, the final tag and
    vote.  -> dict with the outputs of ``phase_ref.refine`` (link and shared: column w = 1) plus parent, span_link,
    span_shared, parent_link, parent_shared; 'margins' the smallest margin of every kind over all rounds."""
    span_link, span_shared = span_links(has, E, site_first, span)
    parent, block, sigma, margins = forest(span_link, span_shared, site_first, min_shared, min_link)
    flips = []

    def fold(m):
        for k, v in m.items():
            margins[k] = min(margins.get(k, np.inf), v)

    for r in range(rounds + 1):
        read_block, read_llr, read_sites, m = tag_blocks(has, E, block, sigma)
        fold(m)
        vote, agree, against, m = votes(has, E, block, sigma, read_block, read_llr, read_sites)
        if r == rounds:
            m.pop('vote')               # the final vote decides nothing
        fold(m)
        if r == rounds:
            break
        flip = vote * sigma < 0
        flips.append(int(flip.sum()))
        sigma = np.where(flip, -sigma, sigma)
        sigma = sigma * sigma[block]
    haplotype = np.where(read_llr > 0, 1, np.where(read_llr < 0, 2, 0)).astype(np.int8)
    # the link every site was joined by (0 at a root)
    S = has.shape[1]
    col = np.clip(np.arange(S) - parent - 1, 0, span - 1)
    parent_link = np.where(parent >= 0, span_link[np.arange(S), col], 0.0)
    parent_shared = np.where(parent >= 0, span_shared[np.arange(S), col], 0)
    return dict(link=span_link[:, 0].copy(), shared=span_shared[:, 0].copy(), span_link=span_link,
                span_shared=span_shared, parent=parent, parent_link=parent_link, parent_shared=parent_shared,
                block=block, sigma=sigma, joined=parent >= 0,
                read_block=read_block, read_llr=read_llr, read_sites=read_sites, haplotype=haplotype, vote=vote,
                n_agree=agree, n_against=against, flips_per_round=flips, margins=margins)


def close(a, b):
    """The project's tolerance for device exp / log1p against numpy's: 1e-9 relative + 1e-9 absolute."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.abs(a - b) <= 1e-9 + 1e-9 * np.abs(b))


def check_against(ref, got, label='', exact=()):
    """``phase_ref.check_against``'s rules for ``refine_span``'s result ``ref`` and a dict ``got`` of numpy arrays with
    the keys of ``device.phase_sites_dev(span > 1)`` (span_link, span_shared: every column) or of a PhaseBatch
    (parent_link, parent_shared: the chosen column): no decision of ``ref`` within 1e-6 of its threshold unless the
    caller names its kind in ``exact``; the integers, parent and block equal; read_llr bit for bit; the links and the
    votes within 1e-9 relative + 1e-9 absolute."""
    assert np.array_equal(np.asarray(got['parent'], dtype=np.int64), ref['parent']), \
        '%s parent: %r vs %r' % (label, got['parent'], ref['parent'])
    phase_ref.check_against(ref, got, label, exact)
    kind = 'span' if 'span_link' in got else 'parent'
    count, link = kind + '_shared', kind + '_link'
    assert np.array_equal(np.asarray(got[count], dtype=np.int64), ref[count]), '%s %s' % (label, count)
    same = close(got[link], ref[link])
    assert same.all(), '%s %s: %r vs %r' % (label, link, np.asarray(got[link])[~same][:4], ref[link][~same][:4])


def weak_site_case(seed=11):
    """Six sites, 60 reads of 3 - 4 consecutive sites each drawn from two haplotypes: evidence +-6 with noise at the
    real sites 0, 1, 3, 5, +-0.01 at the weak site 2, and a decoy at site 4 where every read says "reference" (-5 with
    noise).  -> (has, E, truth): truth the planted sigma of the real sites relative to site 0 (0 at site 4)."""
    rng = np.random.default_rng(seed)
    S, n = 6, 60
    truth = np.array([1, -1, 1, 1, 0, -1])
    rows = []
    for i in range(n):
        hap = 1 if rng.random() < 0.5 else -1
        length = 3 + int(rng.integers(0, 2))
        first = int(rng.integers(0, S - length + 1))
        row = [None] * S
        for s in range(first, first + length):
            if s == 2:
                row[s] = 0.01 * hap * truth[s]
            elif s == 4:
                row[s] = -5.0 + float(rng.normal(0, 1.0))
            else:
                row[s] = hap * truth[s] * 6.0 + float(rng.normal(0, 1.5))
        rows.append(tuple(row))
    has, E = phase_ref.dense(rows, S)
    return has, E, truth
