"""The contract of nvk_mod_site_solve_dev (include/nadavca_hip.h) restated in plain numpy float64 on the allele
restatement's ``t_term`` / ``u_term`` / ``solve`` (tests/allele_ref.py; sums left to right), and the phase-set rule of
``phase_mods.phase_mods_of_rows`` with a loop per site.  The yardstick of the CPU and the GPU tests of
``phase_mods_batch``; nothing here touches the package's kernels or its torch code."""
import numpy as np

from allele_ref import pad, solve as allele_solve, t_term, u_term   # noqa: F401  (t_term, u_term: for the tests)

MASKS = (0b111, 0b010, 0b100, 0b110)   # the workflow's sets: all rows, haplotype 1, haplotype 2, tagged


def members(val, group, mask):
    """Which rows are in the set ``mask``: the value is a number, the group lies in 0 .. 31 and its bit is set."""
    val = np.asarray(val, dtype=np.float64)
    group = np.zeros(val.size, dtype=np.int64) if group is None else np.asarray(group).astype(np.int64)
    ok = ~np.isnan(val) & (group >= 0) & (group < 32)
    return ok & (((int(mask) >> np.where(ok, group, 0)) & 1) != 0)


def clipped(val, clip):
    with np.errstate(invalid='ignore'):
        return np.minimum(np.maximum(np.asarray(val, dtype=np.float64), -clip), clip)


def site_vectors(site_lo, site_hi, val, group, set_mask, clip):
    """The clipped values of every (site, set) in row order: a list of S * Q vectors, laid out [site][set]."""
    val = np.asarray(val, dtype=np.float64)
    out = []
    for lo, hi in zip(np.asarray(site_lo).tolist(), np.asarray(site_hi).tolist()):
        v = val[lo:hi]
        g = None if group is None else np.asarray(group)[lo:hi]
        for m in set_mask:
            out.append(clipped(v[members(v, g, m)], clip))
    return out


def solve(site_lo, site_hi, val, group, set_mask, clip, full=False):
    """nvk_mod_site_solve_dev: -> (count int64, fraction, ll), each (S, Q).  ``full``: also the dict of
    ``allele_ref.solve`` and the padded (D, valid) it was given, rows laid out [site][set], for ``check_against``."""
    S, Q = len(site_lo), len(set_mask)
    vectors = site_vectors(site_lo, site_hi, val, group, set_mask, clip)
    D, valid = pad(vectors)
    ref = allele_solve(D, valid)
    count = np.array([v.size for v in vectors], dtype=np.int64).reshape(S, Q)
    fraction = ref['fraction'].reshape(S, Q)
    ll = (ref['lrt'] / 2.0).reshape(S, Q)     # lrt = 2 L(f^) where f^ > 0, else 0: halving is exact
    return (count, fraction, ll, ref, D, valid) if full else (count, fraction, ll)


def site_rows(contig, position, strand):
    """The stable order of the rows by (contig, position, strand) and the sites' ranges in it:
    -> (order, site_lo, site_hi, site_of_sorted_row)."""
    key = np.stack([np.asarray(contig, dtype=np.int64), np.asarray(position, dtype=np.int64),
                    np.asarray(strand, dtype=np.int64)], 1)
    order = np.lexsort((key[:, 2], key[:, 1], key[:, 0])) if key.shape[0] else np.zeros(0, dtype=np.int64)
    k = key[order]
    new = np.ones(k.shape[0], dtype=bool)
    new[1:] = (k[1:] != k[:-1]).any(1)
    lo = np.nonzero(new)[0]
    hi = np.append(lo[1:], k.shape[0]).astype(np.int64) if lo.size else lo
    return order, lo.astype(np.int64), hi, np.cumsum(new) - 1


def phase_sets(mods, phase):
    """The phase set of every site and the group of every row (in the sorted order), one site at a time: among the
    site's rows whose read has haplotype 1 or 2 on the site's contig, the ``read_phase_set`` with the most rows (the
    smallest on ties), -1 without such a row; a row's group is its read's haplotype when the read's phase set is the
    site's, else 0.  -> (order, site_lo, site_hi, phase_set (S,), group (rows,) int32)."""
    order, lo, hi, _ = site_rows(mods.contig, mods.position, mods.strand)
    read, contig = mods.read[order], mods.contig[order]
    hap = phase.haplotype[read].astype(np.int64)
    ps = phase.read_phase_set[read]
    tagged = ((hap == 1) | (hap == 2)) & (phase.read_contig[read] == contig)
    group = np.zeros(order.size, dtype=np.int32)
    site_ps = np.full(lo.size, -1, dtype=np.int64)
    for s, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        sets = ps[a:b][tagged[a:b]]
        if sets.size == 0:
            continue
        values, counts = np.unique(sets, return_counts=True)
        site_ps[s] = values[np.argmax(counts)]          # unique ascends and argmax takes the first: smallest on ties
        own = tagged[a:b] & (ps[a:b] == site_ps[s])
        group[a:b] = np.where(own, hap[a:b], 0)
    return order, lo, hi, site_ps, group
