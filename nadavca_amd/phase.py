"""``phase_reads_batch`` — phase the heterozygous sites of a sample and tag its reads by haplotype.

``estimate_allele_fractions_batch`` computes a log-likelihood ratio d for every read over every site and keeps only
the per-site mixture.  This workflow keeps which read carried which base: adjacent sites are linked through the reads
that cover both, linked sites form blocks with a phase per site, every read is tagged with the block and haplotype its
evidence supports, and the phases are refined by the leave-one-out votes of the tagged reads.  With ``span`` > 1 a site
is linked to the ``span`` sites before it and joined to the strongest of them, so that a weak site neither cuts a block
nor passes a random sign on.  The contract is in include/nadavca_hip.h (nvk_phase_links_dev,
nvk_phase_span_links_dev), the kernels of either span in csrc/kernels_phase.hip, the loop in
``device.phase_sites_dev``.  Single process only, as the allele workflow."""
import os

import numpy as np

from . import defaults
from .allele_fractions import AlleleFractionBatch


class PhaseBatch:
    """What ``phase_reads_batch`` returns.
    Site arrays, one entry per site, ascending in global position: ``contig`` (an index into ``contig_names`` for a
    ``refset.ReferenceSet``; 0 and None otherwise), ``position`` (forward, contig-local), ``ref_base``, ``alt_base``
    (codes 0..3), ``phase`` (int8: +1 where the alternative lies on haplotype 1 of the site's block, the haplotype that
    carries the alternative of the block's first site; -1 on haplotype 2), ``block`` (the index of the block's first
    site, the root of the site's tree), ``phase_set`` (the contig-local position of that site), ``block_size``,
    ``link`` and ``shared`` (the log-likelihood ratio "same haplotype as the previous site" against "the other one" and
    the reads it rests on; both 0 at the first site of a contig), ``parent`` (the index of the site this one was
    joined to: the site before it with ``span`` = 1, one of the ``span`` sites before it otherwise; -1 at a block's
    first site), ``parent_link`` and ``parent_shared`` (the link to that site and its reads; 0 without a parent),
    ``vote``, ``n_agree``, ``n_against`` (the leave-one-out vote of the
    reads tagged in the block, under the final phases), ``fraction``, ``lrt``, ``coverage`` (of the (position,
    alternative) row of ``fractions``; fraction and lrt 0 where that row has fraction 0).  ``gt``: '1|0' for phase +1,
    '0|1' for -1.
    Read arrays, one entry per read of the ReadBatch: ``haplotype`` (int8: 1, 2, or 0 for none), ``read_contig`` and
    ``read_phase_set`` (of the read's block; -1 without one), ``read_llr`` (the signed evidence H for haplotype 1),
    ``read_sites`` (the read's sites in its block).  A read that is not live or meets no site has 0 / -1 / -1 / 0 / 0.
    ``fractions``: the AlleleFractionBatch of the same rows; ``flips_per_round``: the sites flipped in each round of
    the refinement; ``span``: the ``span`` the batch was made with (with ``span`` > 1 a block need not be an interval
    of sites: a site without a strong link stays a block of its own inside the block of its neighbours)."""

    SITE_FIELDS = ('contig', 'position', 'ref_base', 'alt_base', 'phase', 'block', 'phase_set', 'block_size', 'link',
                   'shared', 'vote', 'n_agree', 'n_against', 'fraction', 'lrt', 'coverage', 'parent', 'parent_link',
                   'parent_shared')
    READ_FIELDS = ('haplotype', 'read_contig', 'read_phase_set', 'read_llr', 'read_sites')

    def __init__(self, sites, reads, fractions, flips_per_round, contig_names=None, span=1):
        for f in self.SITE_FIELDS:
            setattr(self, f, sites[f])
        for f in self.READ_FIELDS:
            setattr(self, f, reads[f])
        self.fractions, self.flips_per_round, self.contig_names = fractions, list(flips_per_round), contig_names
        self.span = int(span)

    @classmethod
    def empty(cls, n_reads, ref_len=0, rounds=0, threshold=None, contig_names=None, fractions=None, span=1):
        """No site; every read untagged."""
        if fractions is None:
            fractions = AlleleFractionBatch.empty(ref_len, threshold, contig_names)
        return cls(_site_table(0), _read_table(int(n_reads)), fractions, [0] * int(rounds), contig_names, span)

    def __len__(self):
        return int(self.position.size)

    @property
    def gt(self):
        return np.where(self.phase > 0, '1|0', '0|1')

    @property
    def n_blocks(self):
        return int(np.unique(self.block).size)

    def _label(self):
        return (lambda c: str(c)) if self.contig_names is None else (lambda c: self.contig_names[c])

    def write_sites_tsv(self, file):
        """Header, then one tab-separated row per site: contig (by name where the batch has names), position, ref, alt,
        gt, phase_set, block_size, link, shared, vote, n_agree, n_against, fraction, lrt (floats as ``repr`` gives
        them), coverage, to ``file``, a path or a text file.  A batch made with ``span`` > 1 appends parent (the
        contig-local position of the site this one was joined to, '.' without one) and parent_link."""
        label, gt = self._label(), self.gt
        if self.span > 1:
            more = lambda t: '\t%s\t%r' % ('.' if self.parent[t] < 0 else str(int(self.position[self.parent[t]])),
                                            float(self.parent_link[t]))
        else:
            more = lambda t: ''
        _write(file, 'contig\tposition\tref\talt\tgt\tphase_set\tblock_size\tlink\tshared\tvote\tn_agree\tn_against\t'
                     'fraction\tlrt\tcoverage%s\n' % ('\tparent\tparent_link' if self.span > 1 else ''),
               ('%s\t%d\t%s\t%s\t%s\t%d\t%d\t%r\t%d\t%r\t%d\t%d\t%r\t%r\t%d%s\n'
                % (label(int(self.contig[t])), self.position[t], 'ACGT'[self.ref_base[t]], 'ACGT'[self.alt_base[t]],
                   gt[t], self.phase_set[t], self.block_size[t], float(self.link[t]), self.shared[t],
                   float(self.vote[t]), self.n_agree[t], self.n_against[t], float(self.fraction[t]),
                   float(self.lrt[t]), self.coverage[t], more(t)) for t in range(len(self))))

    def write_reads_tsv(self, file):
        """Header, then one tab-separated row per read of the ReadBatch: its index, ``H1`` / ``H2`` / ``none``, the
        phase set and the contig of its block ('.' for both without one), to ``file``, a path or a text file."""
        label = self._label()
        tag = ('none', 'H1', 'H2')
        _write(file, 'read\thaplotype\tphase_set\tcontig\n',
               ('%d\t%s\t%s\t%s\n' % ((i, tag[self.haplotype[i]]) + (('.', '.') if self.read_phase_set[i] < 0 else
                                      (str(int(self.read_phase_set[i])), label(int(self.read_contig[i])))))
                for i in range(self.haplotype.size)))


def _write(file, header, lines):
    out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
    try:
        out.write(header)
        out.writelines(lines)
    finally:
        if out is not file:
            out.close()


_SITE_DTYPES = dict(contig=np.int32, position=np.int64, ref_base=np.int8, alt_base=np.int8, phase=np.int8,
                    block=np.int64, phase_set=np.int64, block_size=np.int64, link=np.float64, shared=np.int64,
                    vote=np.float64, n_agree=np.int64, n_against=np.int64, fraction=np.float64, lrt=np.float64,
                    coverage=np.int64, parent=np.int64, parent_link=np.float64, parent_shared=np.int64)


def _site_table(S):
    return {f: np.zeros(S, dtype=_SITE_DTYPES[f]) for f in PhaseBatch.SITE_FIELDS}


def _read_table(n):
    return dict(haplotype=np.zeros(n, dtype=np.int8), read_contig=np.full(n, -1, dtype=np.int32),
                read_phase_set=np.full(n, -1, dtype=np.int64), read_llr=np.zeros(n), read_sites=np.zeros(n, np.int64))


def select_sites(fractions, threshold, min_fraction=0.25, min_coverage=8):
    """The heterozygous sites among the rows of an AlleleFractionBatch: the rows with lrt >= threshold, min_fraction <=
    fraction <= 1 - min_fraction, coverage >= min_coverage that are not shadowed, ONE per position (the largest lrt, the
    first on ties).  -> the indices of the kept rows, ascending."""
    f = fractions
    ok = (f.lrt >= threshold) & (f.fraction >= min_fraction) & (f.fraction <= 1.0 - min_fraction) \
        & (f.coverage >= min_coverage) & ~f.shadowed
    rows = np.nonzero(ok)[0]
    kept = []
    for t in rows:      # rows ascend in (contig, position): the rows of one position are neighbours
        if kept and f.contig[kept[-1]] == f.contig[t] and f.position[kept[-1]] == f.position[t]:
            if f.lrt[t] > f.lrt[kept[-1]]:
                kept[-1] = t
        else:
            kept.append(t)
    return np.array(kept, dtype=np.int64)


def _check_sites(sites, reference_num, refset):
    """``sites`` = (positions, alt_bases) as ``phase_reads_batch`` takes them -> (global positions int64 strictly
    ascending, alternative bases int32), or ValueError."""
    what = 'phase_reads_batch: sites'
    try:
        positions, alts = sites
    except (TypeError, ValueError):
        raise ValueError('%s is not a pair (positions, alt_bases)' % what)
    alts = np.asarray(alts)
    if refset is not None:
        try:
            contig, local = positions
        except (TypeError, ValueError):
            raise ValueError('%s: positions over a ReferenceSet are a pair (contig, local)' % what)
        contig, local = np.asarray(contig), np.asarray(local)
        if contig.ndim != 1 or contig.shape != local.shape or (contig.size and contig.dtype.kind not in 'iu') \
                or (local.size and local.dtype.kind not in 'iu'):
            raise ValueError('%s: contig and local are not integer vectors of one length' % what)
        contig, local = contig.astype(np.int64), local.astype(np.int64)
        if ((contig < 0) | (contig >= len(refset.names))).any():
            raise ValueError('%s: contig index outside 0 .. %d' % (what, len(refset.names) - 1))
        if ((local < 0) | (local >= np.diff(refset.offsets)[contig])).any():
            raise ValueError('%s: position outside its contig' % what)
        P = refset.offsets[contig] + local
    else:
        P = np.asarray(positions)
        if P.ndim != 1 or (P.size and P.dtype.kind not in 'iu'):
            raise ValueError('%s: positions are not an integer vector' % what)
        P = P.astype(np.int64)
        if ((P < 0) | (P >= reference_num.size)).any():
            raise ValueError('%s: position outside the reference' % what)
    if alts.shape != P.shape or (alts.size and alts.dtype.kind not in 'iu'):
        raise ValueError('%s: alt_bases is not an integer vector as long as the positions' % what)
    if ((alts < 0) | (alts > 3)).any():
        raise ValueError('%s: alternative base outside 0 .. 3' % what)
    if (np.diff(P) <= 0).any():
        raise ValueError('%s: positions do not ascend strictly' % what)
    if (reference_num[P] == alts).any():
        raise ValueError("%s: an alternative base equals the reference's" % what)
    return P, alts.astype(np.int32)


def phase_reads_batch(reference_num, read_batch, config=defaults.CONFIG_FILE, kmer_model=defaults.KMER_MODEL_FILE,
                      aligner=None, threshold=None, sites=None, min_fraction=0.25, min_coverage=8, event_length=1.0,
                      clip=30.0, min_shared=3, min_link=2.0, rounds=2, span=1):
    """Phase the heterozygous sites of the sample and tag every read with its haplotype.
    The front end is ``estimate_allele_fractions_batch``'s (``batchflow.device_stage`` 'pooled', then
    ``batchflow.likelihood_rows``); the rows are normalised, strand-corrected and sorted ONCE and serve both the
    per-position mixture solve and the phase kernels.  The sites are the rows ``select_sites`` keeps (on the host), or
    ``sites = (positions, alt_bases)``: known variants, positions global and strictly ascending, or a pair (contig,
    local) for a ``refset.ReferenceSet``; ``threshold`` may then be None.  Then ``device.phase_sites_dev`` (links,
    blocks, ``rounds`` rounds of tag / vote / flip: include/nadavca_hip.h, nvk_phase_links_dev) and one copy of its
    results to the host.  Over a ReferenceSet a chain never crosses a contig, and positions are contig-local and named.
    ``clip`` bounds one read's evidence at one site (nats); two sites are joined when at least ``min_shared``
    reads cover both and |link| >= ``min_link``.  ``span`` (1 .. 8): a site is linked to the ``span`` sites before it
    in its contig and joined to the one with the largest |link| among those that qualify (the nearest on ties); with
    the default 1 only to the site before it, so that a weak site splits a block.  ``clip``, ``min_link``,
    ``min_shared``, ``span`` and ``threshold`` have NO calibrated values: only synthetic levels have been scored with
    them.  ``event_length``, ``min_fraction``,
    ``min_coverage``: as for ``estimate_allele_fractions_batch`` (``min_fraction`` bounds the fraction on both sides).
    The joining is greedy (every site takes its strongest earlier neighbour inside ``span``; no maximum spanning tree
    is sought), blocks are neither merged nor split during the refinement, and two variants inside one k-mer still
    bias each other's evidence.
    Alphabet 4 only; single process only.  -> PhaseBatch."""
    what = 'phase_reads_batch'
    event_length, clip, min_fraction, min_link = float(event_length), float(clip), float(min_fraction), float(min_link)
    if not 0.0 < event_length < float('inf'):
        raise ValueError('%s: event_length %r is not a positive finite number' % (what, event_length))
    if not 0.0 < clip < float('inf'):
        raise ValueError('%s: clip %r is not a positive finite number' % (what, clip))
    if not 0.0 <= min_fraction <= 0.5:
        raise ValueError('%s: min_fraction %r outside 0 .. 0.5' % (what, min_fraction))
    if not 0.0 <= min_link < float('inf'):
        raise ValueError('%s: min_link %r is not a finite number >= 0' % (what, min_link))
    for name, v in (('min_coverage', min_coverage), ('min_shared', min_shared), ('rounds', rounds)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError('%s: %s %r is not an integer >= 0' % (what, name, v))
    from .device import check_span
    span = check_span(what, span)
    if threshold is None:
        if sites is None:
            raise ValueError('%s needs a threshold to select sites with, or sites' % what)
    else:
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError('%s: threshold is NaN' % what)
    if aligner is None:
        raise ValueError('%s needs a batch aligner (BWA has no batch adapter offline)' % what)
    from .batchflow import device_stage, likelihood_rows, load_config, load_kmer_model
    config, kmer_model = load_config(config), load_kmer_model(kmer_model)
    if kmer_model.alphabet_size != 4:
        raise ValueError('%s: alphabet %d (the strand flip and the rows are those of ACGT)'
                         % (what, kmer_model.alphabet_size))
    from .refset import ReferenceSet
    refset = reference_num if isinstance(reference_num, ReferenceSet) else None
    if refset is not None:
        if not np.array_equal(refset.codes, np.asarray(aligner.reference_num).reshape(-1)):
            raise ValueError("%s: the ReferenceSet's concatenation differs from the aligner's reference_num" % what)
        reference_num = refset.codes
    reference_num = np.ascontiguousarray(reference_num, dtype=np.int32)
    if sites is not None:
        sites = _check_sites(sites, reference_num, refset)
    L, n_reads = reference_num.size, int(read_batch.n)
    names = None if refset is None else list(refset.names)
    stage = device_stage(read_batch, reference_num if refset is None else refset, config, kmer_model, aligner,
                         'pooled')
    if stage.n_live == 0 or L == 0:
        return PhaseBatch.empty(n_reads, L, rounds, threshold, names, span=span)
    ll, status, _ = likelihood_rows(stage, config, kmer_model)
    return phase_of_rows(stage, ll, status, reference_num, refset, kmer_model, n_reads, threshold, sites, min_fraction,
                         int(min_coverage), event_length, clip, int(min_shared), min_link, int(rounds), span)


def phase_of_rows(stage, ll, status, reference_num, refset, kmer_model, n_reads, threshold=None, sites=None,
                  min_fraction=0.25, min_coverage=8, event_length=1.0, clip=30.0, min_shared=3, min_link=2.0, rounds=2,
                  span=1):
    """The back half of ``phase_reads_batch``, from the log-likelihood rows ``ll`` and the per-read ``status`` of a
    ``batchflow.DeviceStage`` with live reads (device tensors, as ``batchflow.likelihood_rows`` returns them).
    ``reference_num``: int32 base codes of the whole reference; ``refset``: its ReferenceSet or None; ``n_reads``: the
    reads of the ReadBatch; ``sites``: None or (global positions, alternative bases) as checked there; the other
    arguments as checked there.  -> PhaseBatch."""
    import torch
    from .allele_fractions import allele_fractions_of_rows
    from .device import allele_sorted_rows_dev, check_span, phase_sites_dev, to_host
    span = check_span('phase_of_rows', span)
    sa, context = stage.sa, kmer_model.context
    device = torch.device('cuda', context.device)
    L = reference_num.size
    names = None if refset is None else list(refset.names)
    chunk_start, reverse = sa.ref_start.contiguous(), sa.reverse.to(torch.int32)
    key, val, sorted_key, order = allele_sorted_rows_dev(context, stage.dbatch, ll, chunk_start, reverse, status,
                                                         event_length, L)
    sorted_val = val[order]
    fractions = allele_fractions_of_rows(stage, ll, status, reference_num, refset, kmer_model, event_length,
                                         min_coverage, min_fraction, threshold, 'positive', (sorted_key, sorted_val))
    offsets = None if refset is None else refset.offsets
    row_global = fractions.position if refset is None else offsets[fractions.contig] + fractions.position
    if sites is None:
        picked = select_sites(fractions, threshold, min_fraction, min_coverage)
        P, alt = row_global[picked], fractions.alt_base[picked].astype(np.int32)
    else:
        P, alt = sites
    S = int(P.size)
    if S == 0:
        return PhaseBatch.empty(n_reads, L, rounds, threshold, names, fractions, span)
    contig = np.zeros(S, dtype=np.int32)
    local = P
    if refset is not None:
        contig, local = refset.locate(P)
        contig = contig.astype(np.int32)
    chain = np.ones(S, dtype=np.int32)
    chain[0] = 0
    chain[1:][contig[1:] != contig[:-1]] = 0        # a chain never crosses a contig
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    got = phase_sites_dev(context, stage.dbatch.ref_off, chunk_start, reverse, key, val, sorted_key, sorted_val, order,
                          up(P), up(alt), up(chain), clip, min_shared, min_link, rounds, span=span)
    # one copy to the host (every integer here is exact in a double)
    site_cols = ('link', 'shared', 'block', 'sigma', 'vote', 'n_agree', 'n_against')
    if span > 1:
        # the link a site was joined by: column parent's distance - 1 of its row (a root reads column 0 and is masked)
        at = (torch.arange(S, device=device) - got['parent'] - 1).clamp(0, span - 1)[:, None]
        got['parent_link'], got['parent_shared'] = got['span_link'].gather(1, at)[:, 0], \
            got['span_shared'].gather(1, at)[:, 0]
        site_cols += ('parent', 'parent_link', 'parent_shared')
    read_cols = ('read_block', 'read_llr', 'read_sites')
    n_live = int(sa.live.numel())
    flat = to_host(torch.cat([got[c].double() for c in site_cols + read_cols]
                             + [sa.live.to(device).double(), got['flips'].double()]))
    site = {c: flat[j * S:(j + 1) * S] for j, c in enumerate(site_cols)}
    base = len(site_cols) * S
    read = {c: flat[base + j * n_live:base + (j + 1) * n_live] for j, c in enumerate(read_cols)}
    base += len(read_cols) * n_live
    live = flat[base:base + n_live].astype(np.int64)
    flips = [int(x) for x in flat[base + n_live:]]

    t = _site_table(S)
    t['contig'], t['position'], t['alt_base'] = contig, np.ascontiguousarray(local, dtype=np.int64), alt.astype(np.int8)
    t['ref_base'] = reference_num[P].astype(np.int8)
    t['phase'] = site['sigma'].astype(np.int8)
    block = site['block'].astype(np.int64)
    t['block'], t['phase_set'] = block, t['position'][block]
    t['block_size'] = np.bincount(block, minlength=S)[block].astype(np.int64)
    for c in ('link', 'vote'):
        t[c] = np.ascontiguousarray(site[c])
    for c in ('shared', 'n_agree', 'n_against'):
        t[c] = site[c].astype(np.int64)
    if span > 1:
        t['parent'] = site['parent'].astype(np.int64)
    else:
        t['parent'] = np.where(block != np.arange(S), np.arange(S) - 1, -1).astype(np.int64)
        site['parent_link'], site['parent_shared'] = site['link'], site['shared']
    joined = t['parent'] >= 0
    t['parent_link'] = np.where(joined, site['parent_link'], 0.0)
    t['parent_shared'] = np.where(joined, site['parent_shared'], 0).astype(np.int64)
    # the (position, alternative) rows of the fractions; a pair without a row has fraction 0
    t['coverage'] = fractions.position_coverage[P].astype(np.int64)
    code = row_global * 4 + fractions.alt_base
    at = np.searchsorted(code, P * 4 + alt)
    hit = (at < code.size) & (code[np.minimum(at, max(code.size - 1, 0))] == P * 4 + alt) if code.size else \
        np.zeros(S, dtype=bool)
    t['fraction'][hit], t['lrt'][hit] = fractions.fraction[at[hit]], fractions.lrt[at[hit]]

    r = _read_table(int(n_reads))
    rb = read['read_block'].astype(np.int64)
    has = rb >= 0
    r['read_llr'][live] = read['read_llr']
    r['read_sites'][live] = read['read_sites'].astype(np.int64)
    r['haplotype'][live] = np.where(read['read_llr'] > 0, 1, np.where(read['read_llr'] < 0, 2, 0))
    r['read_contig'][live[has]] = contig[rb[has]]
    r['read_phase_set'][live[has]] = t['position'][rb[has]]
    return PhaseBatch(t, r, fractions, flips, names, span)
