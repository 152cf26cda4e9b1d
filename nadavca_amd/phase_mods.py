"""``phase_mods_batch`` — per-haplotype modification frequencies per site (allele-specific modification).

``phase_reads_batch`` tags every read with a haplotype and ``call_mods_batch`` gives every read a log-likelihood ratio
at every occurrence of a pattern.  This workflow joins them: the rows of the calls are grouped per (contig, position,
strand), every row gets the haplotype of its read, and ONE operator call (include/nadavca_hip.h:
nvk_mod_site_solve_dev, csrc/kernels_modsites.hip) solves four mixtures per site: all rows, haplotype 1, haplotype 2
and both tagged haplotypes pooled.  The frequency of a set is the f^ that maximises the two-component mixture
likelihood L(f) = sum t(f, d_i) of the rows' ratios, the estimator of ``estimate_allele_fractions_batch``; the
haplotype contrast is the likelihood ratio ``asm_lrt`` = 2 ((L_1 + L_2) - L_tagged) with one degree of freedom.

``mod_site_frequencies`` is the same estimate for any ``ModCallBatch`` without haplotypes: the likelihood-based
counterpart of ``ModCallBatch.site_table``, which counts the ratios beyond a threshold and drops their sizes.

NOTHING here is calibrated on real data: ``clip`` (the bound on one row's ratio), ``min_tagged`` and any use of ``p``
have only been scored on synthetic levels.  ``p`` is the chi^2_1 survival of ``asm_lrt`` per site; there is no default
call and no correction for the number of sites."""
import os

import numpy as np

from . import defaults

SET_MASKS = (0b111, 0b010, 0b100, 0b110)   # groups 0 (untagged here), 1, 2: all rows, haplotype 1, haplotype 2, tagged


class PhasedModBatch:
    """What ``phase_mods_batch`` returns: one entry per distinct (contig, position, strand) of the calls, sorted by
    them (the sites and the order of ``ModCallBatch.site_table``).
    ``contig`` (an index into ``contig_names`` over a ``refset.ReferenceSet``; 0 and None otherwise), ``position``
    (forward, contig-local), ``strand`` (0 forward, 1 reverse), ``phase_set`` (the phase set the site's haplotype
    labels belong to: among the site's rows whose read is tagged, the ``read_phase_set`` with the most rows, the
    smallest on ties; -1 for a site without a tagged row), ``reads`` (rows whose ratio is a number), ``n_h1``,
    ``n_h2`` (the rows of the reads tagged 1 / 2 in that phase set) and ``n_untagged`` (the rest: a read tagged in
    ANOTHER phase set counts here, since labels mean nothing across phase sets).
    ``fraction`` and ``lrt`` = 2 L(f^): the modification frequency of all rows and its likelihood ratio against
    f = 0; ``fraction_h1``, ``fraction_h2``, ``fraction_tagged``: of the rows of haplotype 1, 2 and both pooled (0 for
    an empty set); ``delta`` = fraction_h1 - fraction_h2; ``asm_lrt`` = max(2 ((L_1 + L_2) - L_tagged), 0) and ``p``
    its chi^2_1 survival, both NaN where ``n_h1`` or ``n_h2`` is below ``min_tagged``; ``near_variant``: a phased site
    of ``phase`` lies within k - 1 bases on the same contig, so that a substitution on one haplotype changes the
    k-mers the ratios were computed from — a contrast there may be the variant's, not the modification's.
    ``phase`` and ``mods``: the PhaseBatch and the ModCallBatch the table was made from; ``clip``, ``min_tagged``: as
    given.  ``p`` is uncalibrated and not corrected for the number of sites."""

    FIELDS = ('contig', 'position', 'strand', 'phase_set', 'reads', 'n_h1', 'n_h2', 'n_untagged', 'fraction', 'lrt',
              'fraction_h1', 'fraction_h2', 'fraction_tagged', 'asm_lrt', 'p', 'delta', 'near_variant')
    _DTYPES = dict(contig=np.int32, position=np.int64, strand=np.int8, phase_set=np.int64, reads=np.int64,
                   n_h1=np.int64, n_h2=np.int64, n_untagged=np.int64, near_variant=bool)

    def __init__(self, table, phase, mods, contig_names=None, clip=30.0, min_tagged=4):
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(table[f], dtype=self._DTYPES.get(f, np.float64)))
        self.phase, self.mods, self.contig_names = phase, mods, contig_names
        self.clip, self.min_tagged = float(clip), int(min_tagged)

    @classmethod
    def empty(cls, phase, mods, contig_names=None, clip=30.0, min_tagged=4):
        return cls({f: np.zeros(0) for f in cls.FIELDS}, phase, mods, contig_names, clip, min_tagged)

    def __len__(self):
        return int(self.position.size)

    def write_tsv(self, file):
        """Header, then one tab-separated row per site: contig (by name where the batch has names), position, strand
        (``+`` / ``-``), phase_set, reads, n_h1, n_h2, n_untagged, fraction, lrt, fraction_h1, fraction_h2,
        fraction_tagged, delta, asm_lrt, p (floats as ``repr`` gives them), near_variant (0 / 1), to ``file``, a path
        or a text file."""
        label = (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])
        floats = ('fraction', 'lrt', 'fraction_h1', 'fraction_h2', 'fraction_tagged', 'delta', 'asm_lrt', 'p')
        out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
        try:
            out.write('contig\tposition\tstrand\tphase_set\treads\tn_h1\tn_h2\tn_untagged\t%s\tnear_variant\n'
                      % '\t'.join(floats))
            out.writelines('%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n'
                           % (label(int(self.contig[t])), self.position[t], '-' if self.strand[t] else '+',
                              self.phase_set[t], self.reads[t], self.n_h1[t], self.n_h2[t], self.n_untagged[t],
                              '\t'.join(repr(float(getattr(self, f)[t])) for f in floats), self.near_variant[t])
                           for t in range(len(self)))
        finally:
            if out is not file:
                out.close()


def _host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def site_ranges(mods, device):
    """The rows of a ModCallBatch on ``device`` in the STABLE order of (contig, position, strand), and the sites'
    ranges there.  Needs ``len(mods) > 0``.  -> (order, site_lo, site_hi, site_of_row: of every sorted row), int64
    tensors."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)
    contig, position, strand = up(mods.contig), up(mods.position), up(mods.strand)
    n = int(position.numel())
    if bool((position < 0).any()) or bool((contig < 0).any()) or bool(((strand != 0) & (strand != 1)).any()):
        raise ValueError('phase_mods: a row of the ModCallBatch has a negative contig or position, or a strand that is '
                         'neither 0 nor 1')
    key = (contig * (int(position.max()) + 1) + position) * 2 + strand
    skey, order = torch.sort(key, stable=True)
    new = torch.ones(n, dtype=torch.bool, device=device)
    new[1:] = skey[1:] != skey[:-1]
    site_lo = torch.nonzero(new).reshape(-1)
    site_hi = torch.cat([site_lo[1:], torch.full((1,), n, dtype=torch.int64, device=device)])
    return order, site_lo, site_hi, torch.cumsum(new.to(torch.int64), 0) - 1


def site_phase_sets(order, site_of, n_sites, mods, phase, device):
    """The phase set of every site and the group of every sorted row (integer work in torch, no loop over sites).
    A row is TAGGED when its read has haplotype 1 or 2 in a block of the row's contig.  The site takes the
    ``read_phase_set`` with the most tagged rows, the smallest on ties (-1 without a tagged row); a row's group is its
    read's haplotype when the read's phase set is the site's, else 0.  -> (phase_set int64 (S,), group int32 (rows,))."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)
    read = up(mods.read)[order]
    if int(read.numel()) and not 0 <= int(read.min()) <= int(read.max()) < int(phase.haplotype.size):
        raise ValueError('phase_mods: a row of the ModCallBatch names a read the PhaseBatch does not have')
    hap, ps, rc = up(phase.haplotype)[read], up(phase.read_phase_set)[read], up(phase.read_contig)[read]
    tagged = ((hap == 1) | (hap == 2)) & (rc == up(mods.contig)[order]) & (ps >= 0)
    site_ps = torch.full((n_sites,), -1, dtype=torch.int64, device=device)
    at = torch.nonzero(tagged).reshape(-1)
    if int(at.numel()):
        span = int(ps[at].max()) + 1
        pair, rows = torch.unique(site_of[at] * span + ps[at], return_counts=True)     # ascending (site, phase set)
        pair_site, pair_ps = torch.div(pair, span, rounding_mode='floor'), pair % span
        most = torch.zeros(n_sites, dtype=torch.int64, device=device)
        most.scatter_reduce_(0, pair_site, rows, 'amax', include_self=True)
        top = rows == most[pair_site]
        best = torch.full((n_sites,), span, dtype=torch.int64, device=device)
        best.scatter_reduce_(0, pair_site[top], pair_ps[top], 'amin', include_self=True)
        site_ps = torch.where(best < span, best, site_ps)
    group = torch.where(tagged & (ps == site_ps[site_of]), hap, torch.zeros_like(hap)).to(torch.int32)
    return site_ps, group


def phase_mods_of_rows(mods, phase, solve, k, clip=30.0, min_tagged=4, device='cpu'):
    """The part of ``phase_mods_batch`` behind the two workflows: from a ModCallBatch ``mods`` and the PhaseBatch
    ``phase`` of the same ReadBatch to the per-site table.  ``solve(site_lo, site_hi, val, group, set_mask, clip)`` ->
    (count, fraction, ll), each (S, len(set_mask)), tensors or numpy arrays: whatever runs nvk_mod_site_solve_dev's
    contract on the tensors it is given (``device.mod_site_solve_dev`` with a context in front, or the numpy
    restatement of the tests); ``device``: where the torch work runs; ``k``: the k-mer length (``near_variant``).
    -> PhasedModBatch."""
    import torch
    from scipy.special import chdtrc
    clip, min_tagged = float(clip), int(min_tagged)
    if not 0.0 < clip < float('inf'):
        raise ValueError('phase_mods: clip %r is not a positive finite number' % clip)
    if min_tagged < 0:
        raise ValueError('phase_mods: min_tagged %r is negative' % min_tagged)
    names = mods.contig_names
    if len(mods) == 0:
        return PhasedModBatch.empty(phase, mods, names, clip, min_tagged)
    device = torch.device(device)
    order, site_lo, site_hi, site_of = site_ranges(mods, device)
    S = int(site_lo.numel())
    site_ps, group = site_phase_sets(order, site_of, S, mods, phase, device)
    val = torch.from_numpy(np.ascontiguousarray(mods.llr, dtype=np.float64)).to(device)[order].contiguous()
    count, fraction, ll = (_host(t) for t in solve(site_lo, site_hi, val, group.contiguous(), SET_MASKS, clip))
    first = _host(order[site_lo])
    t = dict(contig=mods.contig[first], position=mods.position[first], strand=mods.strand[first],
             phase_set=_host(site_ps), reads=count[:, 0], n_h1=count[:, 1], n_h2=count[:, 2],
             n_untagged=count[:, 0] - count[:, 1] - count[:, 2], fraction=fraction[:, 0], lrt=2.0 * ll[:, 0],
             fraction_h1=fraction[:, 1], fraction_h2=fraction[:, 2], fraction_tagged=fraction[:, 3],
             delta=fraction[:, 1] - fraction[:, 2])
    enough = (count[:, 1] >= min_tagged) & (count[:, 2] >= min_tagged)
    # the raw statistic goes below 0 by rounding only (the pooled maximum cannot exceed the two free ones' sum)
    stat = np.maximum(2.0 * ((ll[:, 1] + ll[:, 2]) - ll[:, 3]), 0.0)
    t['asm_lrt'] = np.where(enough, stat, np.nan)
    t['p'] = np.where(enough, chdtrc(1.0, stat), np.nan)
    t['near_variant'] = near_sites(t['contig'], t['position'], phase.contig, phase.position, int(k) - 1)
    return PhasedModBatch(t, phase, mods, names, clip, min_tagged)


def near_sites(contig, position, other_contig, other_position, reach):
    """Per (contig, position): whether one of the other (contig, position) pairs, which ascend, lies within ``reach``
    bases on the same contig."""
    contig, position = np.asarray(contig, dtype=np.int64), np.asarray(position, dtype=np.int64)
    oc, op = np.asarray(other_contig, dtype=np.int64), np.asarray(other_position, dtype=np.int64)
    if op.size == 0 or position.size == 0:
        return np.zeros(position.size, dtype=bool)
    span = int(max(position.max(), op.max())) + int(reach) + 2       # two contigs are further apart than reach
    here, there = contig * span + position, oc * span + op
    at = np.searchsorted(there, here)
    below = np.abs(here - there[np.maximum(at - 1, 0)]) <= reach
    above = np.abs(there[np.minimum(at, there.size - 1)] - here) <= reach
    return below | above


def mod_site_frequencies(mods, clip=30.0, context=None):
    """The likelihood-based modification frequency of every site of a ModCallBatch: a dict of arrays, one entry per
    distinct (contig, position, strand), sorted by them as ``ModCallBatch.site_table`` sorts its own: ``contig``,
    ``position``, ``strand``, ``reads`` (rows whose ratio is a number), ``fraction`` (the f^ that maximises the
    mixture likelihood of the rows' ratios, each clipped to +-``clip``) and ``lrt`` = 2 L(f^) against f = 0.  One set
    without groups of nvk_mod_site_solve_dev on the device of ``context`` (default: the process's).  ``clip`` has no
    calibrated value."""
    from . import _lib
    from .device import mod_site_solve_dev
    context = _lib.default_context() if context is None else context
    return mod_site_frequencies_of_rows(mods, lambda *a: mod_site_solve_dev(context, *a), clip,
                                        'cuda:%d' % context.device)


def mod_site_frequencies_of_rows(mods, solve, clip=30.0, device='cpu'):
    """``mod_site_frequencies`` over whatever runs the operator: ``solve`` and ``device`` as for
    ``phase_mods_of_rows``."""
    import torch
    clip = float(clip)
    if not 0.0 < clip < float('inf'):
        raise ValueError('mod_site_frequencies: clip %r is not a positive finite number' % clip)
    if len(mods) == 0:
        z = lambda dt: np.zeros(0, dtype=dt)
        return dict(contig=z(np.int32), position=z(np.int64), strand=z(np.int8), reads=z(np.int64),
                    fraction=z(np.float64), lrt=z(np.float64))
    device = torch.device(device)
    order, site_lo, site_hi, _ = site_ranges(mods, device)
    val = torch.from_numpy(np.ascontiguousarray(mods.llr, dtype=np.float64)).to(device)[order].contiguous()
    count, fraction, ll = (_host(t) for t in solve(site_lo, site_hi, val, None, (1,), clip))
    first = _host(order[site_lo])
    return dict(contig=mods.contig[first].astype(np.int32), position=mods.position[first].astype(np.int64),
                strand=mods.strand[first].astype(np.int8), reads=count[:, 0].copy(), fraction=fraction[:, 0].copy(),
                lrt=2.0 * ll[:, 0])


def phase_mods_batch(reference_num, read_batch, aligner, kmer_model, mod_model, pattern='CG', mod_offset=0, mod_code=4,
                     config=defaults.CONFIG_FILE, renorm_rounds=defaults.RENORM_ROUNDS, joint=True, max_joint=4,
                     site_prior=0.5, clip=30.0, min_tagged=4, threshold=None, sites=None, min_fraction=0.25,
                     min_coverage=8, min_shared=3, min_link=2.0, rounds=2, span=1):
    """Per occurrence of ``pattern`` and strand: the modification frequency of all reads, of the reads of haplotype 1
    and of haplotype 2, and the likelihood-ratio contrast of the two.
    ``phase_reads_batch`` runs with the canonical 4-letter ``kmer_model`` (``threshold``, ``sites``, ``min_fraction``,
    ``min_coverage``, ``min_shared``, ``min_link``, ``rounds``, ``span``: its arguments) and ``call_mods_batch`` with
    the 5-letter ``mod_model`` (``pattern``, ``mod_offset``, ``mod_code``, ``renorm_rounds``, ``joint``, ``max_joint``,
    ``site_prior``: its arguments), both unchanged, on the same ``aligner`` and the same ``read_batch``, which
    neither alters: two front ends per batch.  Then the calls' rows go to the device, are sorted stably by (contig,
    position, strand) and tagged with their read's haplotype (``site_phase_sets``), and one call of
    nvk_mod_site_solve_dev solves the four sets of every site (``phase_mods_of_rows``).
    ``reference_num``: base codes, or a ``refset.ReferenceSet`` with an aligner over the same set — sites, phase sets
    and ``near_variant`` are then contig-local.  ``clip`` bounds one row's ratio (nats); ``asm_lrt`` and ``p`` are
    given where both haplotypes have at least ``min_tagged`` rows.  ``clip``, ``min_tagged`` and any use of ``p``
    are UNCALIBRATED; there is no default call and no correction for the number of sites.  An empty batch, a batch in
    which no read aligns or no site is phased and a batch without the pattern give an empty or an all-untagged table,
    not an error.  Single process only.  -> PhasedModBatch."""
    from .batchflow import load_config, load_kmer_model
    from .call_mods import call_mods_batch
    from .device import check_span, mod_site_solve_dev
    from .phase import phase_reads_batch
    clip, span = float(clip), check_span('phase_mods_batch', span)
    if not 0.0 < clip < float('inf'):
        raise ValueError('phase_mods_batch: clip %r is not a positive finite number' % clip)
    if isinstance(min_tagged, bool) or int(min_tagged) != min_tagged or min_tagged < 0:
        raise ValueError('phase_mods_batch: min_tagged %r is not an integer >= 0' % (min_tagged,))
    config, kmer_model, mod_model = load_config(config), load_kmer_model(kmer_model), load_kmer_model(mod_model)
    # neither workflow alters the batch it is given (``batchflow.device_stage`` normalises its device copy of the raw
    # signal), so both read the caller's
    phase = phase_reads_batch(reference_num, read_batch, config=config, kmer_model=kmer_model, aligner=aligner,
                              threshold=threshold, sites=sites, min_fraction=min_fraction, min_coverage=min_coverage,
                              min_shared=min_shared, min_link=min_link, rounds=rounds, span=span)
    mods = call_mods_batch(read_batch, aligner, mod_model, pattern=pattern, mod_offset=mod_offset, mod_code=mod_code,
                           config=config, renorm_rounds=renorm_rounds, joint=joint, max_joint=max_joint,
                           site_prior=site_prior)
    context = mod_model.context
    return phase_mods_of_rows(mods, phase, lambda *a: mod_site_solve_dev(context, *a), kmer_model.get_k(), clip,
                              int(min_tagged), 'cuda:%d' % context.device)
