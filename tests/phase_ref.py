"""The phasing contract of include/nadavca_hip.h (nvk_phase_links_dev / nvk_phase_tag_dev / nvk_phase_votes_dev and the
integer work between them) restated in plain numpy float64 from the read-major (key, val) of ``allele_ref.rows``.  Every
function also returns the margin of each decision it takes, so that a test can tell which discrete answers a rounding
difference could change.  The yardstick of the CPU and the GPU tests of ``phase_reads_batch``; nothing here touches the
package's kernels."""
import numpy as np


def clip_value(d, clip):
    """min(max(d, -clip), clip); -inf and a value that is not a number become -clip."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(d > -clip, np.where(d < clip, d, clip), -clip)


def lae(a, b):
    return np.maximum(a, b) + np.log1p(np.exp(-np.abs(a - b)))


def link_term(e1, e2):
    """Log-likelihood ratio of "both alternatives on one haplotype" against "on different ones" for one read."""
    return lae(e1 + e2, 0.0) - lae(e1, e2)


def sum64(terms):
    """The kernels' sum: term j into partial j mod 64 in ascending j (every partial starts at +0.0), then wave_sum's
    butterfly (lane l adds lane l ^ 32, l ^ 16, ... l ^ 1)."""
    terms = np.asarray(terms, dtype=np.float64)
    m = -(-terms.size // 64)
    buf = np.zeros((m + 1) * 64)
    buf[64:64 + terms.size] = terms
    p = np.cumsum(buf.reshape(m + 1, 64), axis=0)[-1]
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ d]
    return float(p[0])


def evidence(key, val, ref_off, chunk_start, reverse, site_pos, site_alt, clip):
    """-> (has (n, S) bool, E (n, S) f64, 0 where the read has no evidence): read i has evidence at site s where the
    read-major row of (i, P_s) holds the key P_s; the value is the clipped forward column alt_s of that row."""
    ref_off = np.asarray(ref_off, dtype=np.int64)
    n, S = ref_off.size - 1, len(site_pos)
    has, E = np.zeros((n, S), dtype=bool), np.zeros((n, S))
    for i in range(n):
        r0, R = int(ref_off[i]), int(ref_off[i + 1] - ref_off[i])
        c0 = int(chunk_start[i])
        for s in range(S):
            P = int(site_pos[s])
            if not c0 <= P < c0 + R:
                continue
            p = R - 1 - (P - c0) if reverse[i] else P - c0
            if key[r0 + p] == P:
                has[i, s] = True
                E[i, s] = clip_value(val[r0 + p, site_alt[s]], clip)
    return has, E


def links(has, E, chain_flag):
    """-> (link (S,), shared (S,) int64): over the rows of site s (its reads, ascending), those shared with s - 1."""
    S = has.shape[1]
    link, shared = np.zeros(S), np.zeros(S, dtype=np.int64)
    for s in range(1, S):
        if not chain_flag[s]:
            continue
        rows = np.nonzero(has[:, s])[0]
        both = has[rows, s - 1]
        terms = np.where(both, link_term(E[rows, s - 1], E[rows, s]), 0.0)
        link[s], shared[s] = sum64(terms), int(both.sum())
    return link, shared


def chain(link, shared, chain_flag, min_shared, min_link):
    """-> (block (S,) int64, sigma (S,) int64, joined (S,) bool, margins): margins['join'] the smallest
    | |link| - min_link | over the sites whose join the link decides, margins['sign'] the smallest |link| of a join."""
    S = link.size
    block, sigma, joined = np.zeros(S, dtype=np.int64), np.ones(S, dtype=np.int64), np.zeros(S, dtype=bool)
    join_margin = sign_margin = np.inf
    for s in range(S):
        decides = s >= 1 and bool(chain_flag[s]) and shared[s] >= min_shared
        if decides:
            join_margin = min(join_margin, abs(abs(link[s]) - min_link))
        joined[s] = decides and abs(link[s]) >= min_link
        if joined[s]:
            sign_margin = min(sign_margin, abs(link[s]))
            block[s], sigma[s] = block[s - 1], sigma[s - 1] * (1 if link[s] > 0 else -1)
        else:
            block[s] = s
    return block, sigma, joined, dict(join=join_margin, sign=sign_margin)


def tag(has, E, block, sigma):
    """-> (read_block (n,) int64, read_llr (n,), read_sites (n,) int64, margins): per read the run of its sites inside
    one block with the largest |H|, the first on ties; H the left-to-right sum of sigma_s * e_is.  margins['gap'] the
    smallest difference between a read's best and second |H|, margins['llr'] the smallest |H| of a chosen run."""
    n = has.shape[0]
    read_block, read_llr = np.full(n, -1, dtype=np.int64), np.zeros(n)
    read_sites = np.zeros(n, dtype=np.int64)
    gap = llr = np.inf
    for i in range(n):
        runs = []                    # [block, H, sites]
        for s in np.nonzero(has[i])[0]:
            if not runs or runs[-1][0] != block[s]:
                runs.append([int(block[s]), 0.0, 0])
            runs[-1][1] = runs[-1][1] + float(sigma[s]) * E[i, s]
            runs[-1][2] += 1
        best = None
        for run in runs:
            if best is None or abs(run[1]) > abs(best[1]):
                best = run
        if best is not None:
            read_block[i], read_llr[i], read_sites[i] = best
            rest = [abs(r[1]) for r in runs if r is not best]
            if rest:
                gap = min(gap, abs(best[1]) - max(rest))
            llr = min(llr, abs(best[1]))
    return read_block, read_llr, read_sites, dict(gap=gap, llr=llr)


def votes(has, E, block, sigma, read_block, read_llr, read_sites=None):
    """-> (vote (S,), n_agree (S,), n_against (S,) int64, margins): the leave-one-out vote of every site.
    margins['h'] the smallest |h| over the rows of reads with more than one site in their run (a read's only site has
    h = 0 exactly), margins['vote'] the smallest |vote| of a site with a counted row, margins['agree'] the smallest |e|
    of a counted row."""
    S = has.shape[1]
    vote, agree, against = np.zeros(S), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    h_margin = e_margin = np.inf
    for s in range(S):
        rows = np.nonzero(has[:, s])[0]
        mine = read_block[rows] == block[s]
        e = E[rows, s]
        h = np.where(mine, read_llr[rows] - float(sigma[s]) * e, 0.0)
        counted = mine & (h != 0)
        vote[s] = sum64(np.where(counted, np.sign(h) * e, 0.0))
        side = np.sign(h) * float(sigma[s]) * e
        agree[s], against[s] = int((counted & (side > 0)).sum()), int((counted & (side < 0)).sum())
        if read_sites is not None and (mine & (read_sites[rows] > 1)).any():
            h_margin = min(h_margin, float(np.abs(h[mine & (read_sites[rows] > 1)]).min()))
        if counted.any():
            e_margin = min(e_margin, float(np.abs(e[counted]).min()))
    decided = (agree + against) > 0       # (a site without a counted row has vote 0 exactly, here and in the kernel)
    return vote, agree, against, dict(h=h_margin, vote=float(np.abs(vote[decided]).min()) if decided.any() else np.inf,
                                      agree=e_margin)


def refine(has, E, chain_flag, min_shared, min_link, rounds):
    """The whole back half: links, blocks and starting phase, ``rounds`` rounds of tag / vote / flip, the final tag and
    vote.  -> dict with every output and 'margins': the smallest margin of every kind over all rounds."""
    link, shared = links(has, E, chain_flag)
    block, sigma, joined, margins = chain(link, shared, chain_flag, min_shared, min_link)
    flips = []

    def fold(m):
        for k, v in m.items():
            margins[k] = min(margins.get(k, np.inf), v)

    for r in range(rounds + 1):
        read_block, read_llr, read_sites, m = tag(has, E, block, sigma)
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
    return dict(link=link, shared=shared, block=block, sigma=sigma, joined=joined, read_block=read_block,
                read_llr=read_llr, read_sites=read_sites, haplotype=haplotype, vote=vote, n_agree=agree,
                n_against=against, flips_per_round=flips, margins=margins)


def smallest_margin(margins):
    return min(margins.values())


def phasing_likelihood(has, E, sigma):
    """Brute force: log of prod_i [ 1/2 prod_s p(read i | s on its haplotype) + 1/2 prod_s p(... on the other) ] up to a
    constant that does not depend on sigma.  With e = log p(alt) - log p(ref) and the read on haplotype 1, site s shows
    the alternative where sigma_s = +1: the read's log-likelihood is the sum of e over sigma_s = +1; on haplotype 2
    over sigma_s = -1."""
    total = 0.0
    for i in range(has.shape[0]):
        s = has[i]
        a = float(np.sum(E[i, s & (sigma > 0)]))
        b = float(np.sum(E[i, s & (sigma < 0)]))
        total += lae(a, b) + np.log(0.5)
    return total


def check_against(ref, got, label='', exact=()):
    """The tolerances of the phase kernels against ``refine``'s result ``ref`` for the same rows; ``got``: a dict of
    numpy arrays with the keys of ``device.phase_sites_dev``.  No decision of ``ref`` may lie within 1e-6 of its
    threshold (asserted: then every discrete output is compared; ``exact``: the kinds of margin that the caller's
    inputs decide in exact arithmetic, such as a sum of 10.0 and -10.0); the integers and every block are equal,
    read_llr is equal bit for bit (a sequential sum of exact terms), link and vote agree within 1e-9 relative + 1e-9
    absolute (the tolerance of ``allele_ref.check_against``: exp and log1p differ between the device's library and
    numpy's)."""
    small = {k: v for k, v in ref['margins'].items() if not v > 1e-6 and k not in exact}
    assert not small, '%s decisions within 1e-6 of their threshold: %r' % (label, small)
    for f in ('shared', 'block', 'sigma', 'read_block', 'read_sites', 'n_agree', 'n_against'):
        same = np.array_equal(np.asarray(got[f], dtype=np.int64), ref[f])
        assert same, '%s %s: %r vs %r' % (label, f, got[f], ref[f])
    assert np.array_equal(got['read_llr'], ref['read_llr']), label + ' read_llr differs in some bit'
    for f in ('link', 'vote'):
        a, b = np.asarray(got[f]), ref[f]
        same = (a == b) | (np.abs(a - b) <= 1e-9 + 1e-9 * np.abs(b))
        assert same.all(), '%s %s: %r vs %r' % (label, f, a[~same][:4], b[~same][:4])
    assert [int(x) for x in got['flips']] == ref['flips_per_round'], label + ' flips'


# ---- constructed cases ---------------------------------------------------------------------------------------------
def dense(rows, S):
    """[(evidence per site or None, ...)] per read -> (has, E)."""
    has = np.array([[v is not None for v in r] for r in rows], dtype=bool).reshape(len(rows), S)
    E = np.array([[0.0 if v is None else float(v) for v in r] for r in rows]).reshape(len(rows), S)
    return has, E


def refinement_case():
    """Three sites a < b < c: 10 + 10 reads over a, b with (+-10, +-10), 3 reads over b, c with (+10, -10), 4 + 4 reads
    over a, b, c with (+-10, +-0.1, +-10)."""
    rows = [(10.0, 10.0, None)] * 10 + [(-10.0, -10.0, None)] * 10 + [(None, 10.0, -10.0)] * 3 \
        + [(10.0, 0.1, 10.0)] * 4 + [(-10.0, -0.1, -10.0)] * 4
    return dense(rows, 3)
