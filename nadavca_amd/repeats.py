"""``count_repeats_batch``: the copy number of a short tandem repeat in every read of a ``ReadBatch``, from raw signal.

A repeat is where base-space methods fail: the basecaller's calls inside it are not a count, and an alignment needs a
sequence of the right length, which is the unknown.  The signal-level answer (STRique's class) is a small HMM over the
read's events: the k-mers of the left flank, of the repeat and of the right flank as a chain of states, with one back
edge from the end of the repeat's first copy to its start.  The Viterbi path goes round that loop once per copy the read
holds beyond those the chain spells out.  On the device:

1. normalisation and event detection (``rawsignal.signal_events_dev``, ``signal_map_batch``'s);
2. the rescale of every read's events onto the table's pooled means (``rescale_by_moments_dev``, as ``decode_batch``);
   a read with fewer than ``min_events`` events or a zero MAD is ``REP_NO_EVENTS``;
3. the chains' tables (``decode.tables_dev`` of the chains' k-mers), forward and reverse per locus;
4. the items: per (read, locus) the read's events against both strands' chains, or, with ``items``, the one strand and
   sample window each entry names (``repeat_items`` makes them from base alignments);
5. the operator (``nvk_repeat_count_dev``, contract in include/nadavca_hip.h): per item the best path's score, how
   often it went round the loop, and where and with what score it crossed into the repeat and out of it;
6. the better strand per (read, locus), forward on ties, and the per-part scores, in numpy on the host;
7. with ``layers=n``: the likelihood of every count c0 .. c0 + n - 1 for the chosen item of every pair
   (``nvk_repeat_likelihoods_dev``: the forward sum over all paths that go round the loop exactly c times, the count
   as a second dimension of the trellis), and from it, in numpy on the host, the posterior over the window under a
   flat prior, its mode, mean and confidence; ``RepeatCountBatch.genotypes`` combines the reads of a locus into
   diploid genotype likelihoods through a stutter kernel.

The copy number of a path is ``c0 + loops``, c0 = ceil(k / u) + 1 the copies the chain spells out (u the unit's length):
alleles below c0 copies all count as c0.

Limits: the per-count posterior is ordered, not calibrated (on the tests' batch the true count has a posterior below
0.01 on 9 of 64 reads), and the most likely count is no better a count than Viterbi's; the window of counts starts at
c0; ``genotypes`` is diploid only, its three parameters are uncalibrated, and a read cut off inside the repeat is left
out rather than used as a lower bound; one repeat unit per locus, no interruptions; the loop is taken by a
step only; alleles below c0 are not told apart; 4-letter tables, no RNA; the defaults are uncalibrated (the values at
which the simulated reads of the test suite count best); the event detector makes about two events per base, and an
extra event sometimes goes round the loop instead of staying: counts lean upwards a little (25 copies: median 25.5
over the 32 reads of the tests' batch, 25 over 5 000 reads of tools/bench_repeats.py, range 21-34).
"""
import math

import numpy as np

from . import _lib, defaults
from .rawsignal import (rescale_by_moments_dev, resolve_kmer_model, signal_events_dev, transition_costs,
                        transition_weights)

REP_OK, REP_NO_EVENTS, REP_NO_PATH = _lib.REP_OK, _lib.REP_NO_EVENTS, _lib.REP_NO_PATH
MAX_STATES, MAX_LAYERS = _lib.REP_MAX_STATES, _lib.REP_MAX_LAYERS
_LETTERS = {'A': 0, 'C': 1, 'G': 2, 'T': 3}


def _codes(x, what):
    """A base string or code array -> int32 codes 0..3"""
    if isinstance(x, str):
        try:
            return np.array([_LETTERS[c] for c in x.upper()], dtype=np.int32)
        except KeyError:
            raise ValueError('RepeatLocus: %s holds a letter outside ACGT' % what)
    x = np.asarray(x)
    if x.ndim != 1 or (x.size and (x.min() < 0 or x.max() > 3)):
        raise ValueError('RepeatLocus: %s must be a flat array of base codes 0..3' % what)
    return x.astype(np.int32)


class RepeatLocus:
    """A tandem repeat: ``left`` flank, repeat ``unit``, ``right`` flank, as strings over ACGT or base codes, in the
    forward strand's order.  ``start`` / ``end`` / ``contig`` / ``ref_length`` (None unless ``from_reference`` made it):
    where the repeat lies in the reference, and that contig's length.  Refused: a unit shorter than 2 (a homopolymer's
    loop is indistinguishable from a stay) and a unit that is itself a repetition of a shorter one (``CACA``)."""

    def __init__(self, name, left, unit, right, start=None, end=None, contig=0, ref_length=None):
        self.name = str(name)
        self.left, self.unit, self.right = _codes(left, 'left'), _codes(unit, 'unit'), _codes(right, 'right')
        u = self.unit.size
        if u < 2:
            raise ValueError('RepeatLocus %s: the unit has %d bases; a unit has at least 2' % (self.name, u))
        for p in range(1, u):
            if u % p == 0 and np.array_equal(self.unit, np.tile(self.unit[:p], u // p)):
                raise ValueError('RepeatLocus %s: the unit is itself %d copies of a unit of %d bases'
                                 % (self.name, u // p, p))
        self.start, self.end, self.contig, self.ref_length = start, end, int(contig), ref_length

    @classmethod
    def from_reference(cls, reference, start, end, unit, flank=30, contig=0, name=None):
        """The locus whose repeat is [``start``, ``end``) of ``reference`` (base codes, or a ``ReferenceSet`` and
        ``contig``), with ``flank`` bases either side.  ValueError unless that range is whole copies of ``unit`` and
        the flanks lie inside the sequence."""
        from .refset import ReferenceSet
        seq = reference.contig_codes(contig) if isinstance(reference, ReferenceSet) else np.asarray(reference)
        unit = _codes(unit, 'unit')
        start, end, flank = int(start), int(end), int(flank)
        if not (0 <= start - flank and end + flank <= seq.size and start < end):
            raise ValueError('RepeatLocus.from_reference: [%d, %d) with flanks of %d does not lie inside the %d bases'
                             % (start, end, flank, seq.size))
        if (end - start) % unit.size or not np.array_equal(seq[start:end], np.tile(unit, (end - start) // unit.size)):
            raise ValueError('RepeatLocus.from_reference: [%d, %d) is not whole copies of the unit' % (start, end))
        return cls(name if name is not None else 'locus_%d_%d' % (contig, start), seq[start - flank:start], unit,
                   seq[end:end + flank], start=start, end=end, contig=contig, ref_length=int(seq.size))


def repeat_chain(locus, kmer_model, reverse=False):
    """The chain of ``locus`` on one strand -> (ids, lp_from, lp_to, m1, m2, c0).  With T = left + unit * c0 + right, c0 =
    ceil(k / u) + 1, the states are the k-mers T[j .. j + k) (``ids``: int64, numbered as the table numbers them, first
    base most significant); the back edge goes from the last state of the first copy (lp_from = a + u - 1, a =
    len(left)) to its first (lp_to = a), whose k-mer is also that of state lp_from + 1; the marks are the repeat's first
    state (m1 = a) and the first state that holds a base of the right flank (m2 = a + c0 u - k + 1).  ``reverse``: the
    chain of the reverse complement of T.  ValueError for a flank shorter than k or a chain above 256 states."""
    k, alphabet = kmer_model.get_k(), kmer_model.get_alphabet_size()
    if alphabet != 4:
        raise ValueError('repeat_chain: the table has %d letters; only 4-letter tables serve' % alphabet)
    left, unit, right = locus.left, locus.unit, locus.right
    if reverse:
        left, unit, right = 3 - right[::-1], 3 - unit[::-1], 3 - left[::-1]
    a, u = int(left.size), int(unit.size)
    if a < k or right.size < k:
        raise ValueError('repeat_chain: locus %s has flanks of %d and %d bases; a flank has at least k = %d'
                         % (locus.name, locus.left.size, locus.right.size, k))
    c0 = -(-k // u) + 1
    T = np.concatenate([left, np.tile(unit, c0), right]).astype(np.int64)
    n = T.size - k + 1
    if n > MAX_STATES:
        raise ValueError('repeat_chain: locus %s makes a chain of %d states; the operator takes %d'
                         % (locus.name, n, MAX_STATES))
    ids = np.zeros(n, dtype=np.int64)
    for t in range(k):
        ids = ids * 4 + T[t:t + n]
    return ids, a + u - 1, a, a, a + c0 * u - k + 1, c0


class RepeatItems:
    """Which (read, locus) pairs to count, on which strand and in which samples (numpy, one entry per item):
    ``read``, ``locus`` (int64), ``reverse`` (bool), ``sig_lo`` / ``sig_hi`` (int64: the samples [sig_lo, sig_hi)
    inside the read)."""

    def __init__(self, read, locus, reverse, sig_lo, sig_hi):
        self.read, self.locus = np.asarray(read, dtype=np.int64), np.asarray(locus, dtype=np.int64)
        self.reverse = np.asarray(reverse, dtype=bool)
        self.sig_lo, self.sig_hi = np.asarray(sig_lo, dtype=np.int64), np.asarray(sig_hi, dtype=np.int64)
        self.n = int(self.read.size)
        if any(x.shape != (self.n,) for x in (self.locus, self.reverse, self.sig_lo, self.sig_hi)):
            raise ValueError('RepeatItems: the five arrays hold one entry per item')


def repeat_items(read_batch, aligner, loci, pad=50):
    """The items of a whole-genome batch: the (read, locus) pairs whose base alignment
    (``aligner.get_base_alignments``) spans the locus, each with the read's strand and the samples between the
    anchors that bracket it, widened by ``pad``.  An anchor is a matched pair whose read base has a row in the batch's
    ``map_base`` / ``map_sig``.  A pair is kept when the read has an anchor at or before ``start - len(left)`` and one
    at or after ``end + len(right)`` (forward positions in the locus's contig; the nearest such anchors bound the
    window).  The loci must carry ``start`` / ``end`` / ``ref_length`` (``RepeatLocus.from_reference``).
    -> RepeatItems, by read, then locus."""
    rb, ba = read_batch, aligner.get_base_alignments(read_batch)
    n = rb.n
    seq_len = np.diff(rb.seq_off)
    sig_of_base = np.full(int(rb.seq_off[-1]) + 1, -1, dtype=np.int64)
    m_owner = np.repeat(np.arange(n), np.diff(rb.map_off))
    ok = (rb.map_base >= 0) & (rb.map_base < seq_len[m_owner])
    sig_of_base[(rb.seq_off[:-1][m_owner] + rb.map_base)[ok]] = rb.map_sig[ok]
    owner = np.repeat(np.arange(n), np.diff(ba.off))
    inside = (ba.read_idx >= 0) & (ba.read_idx < seq_len[owner])
    sig = sig_of_base[np.where(inside, rb.seq_off[:-1][owner] + ba.read_idx, rb.seq_off[-1])]
    anchored = sig >= 0
    rev = ba.reverse[owner]
    contig = np.zeros(n, dtype=np.int64) if ba.contig is None else ba.contig.astype(np.int64)
    sig_len = np.diff(rb.sig_off)
    far = np.iinfo(np.int64).max
    out = [[] for _ in range(5)]
    for li, locus in enumerate(loci):
        if locus.start is None or locus.ref_length is None:
            raise ValueError('repeat_items: locus %s has no reference position (RepeatLocus.from_reference)'
                             % locus.name)
        fwd = np.where(rev, locus.ref_length - 1 - ba.ref_idx, ba.ref_idx)
        here = anchored & (contig[owner] == locus.contig)
        before, after = here & (fwd <= locus.start - locus.left.size), here & (fwd >= locus.end + locus.right.size)
        # per read the nearest anchor on either side, as (distance, sample) so that one minimum finds both
        near_b, near_a = np.full(n, far), np.full(n, far)
        np.minimum.at(near_b, owner[before], (locus.start - fwd[before]) * (1 << 32) + sig[before])
        np.minimum.at(near_a, owner[after], (fwd[after] - locus.end) * (1 << 32) + sig[after])
        keep = np.nonzero((near_b < far) & (near_a < far))[0]
        s_b, s_a = near_b[keep] & 0xffffffff, near_a[keep] & 0xffffffff
        out[0].append(keep)
        out[1].append(np.full(keep.size, li, dtype=np.int64))
        out[2].append(ba.reverse[keep])
        out[3].append(np.maximum(np.minimum(s_b, s_a) - int(pad), 0))
        out[4].append(np.minimum(np.maximum(s_b, s_a) + int(pad), sig_len[keep]))
    cat = [np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in out]
    order = np.lexsort((cat[1], cat[0]))
    return RepeatItems(*(x[order] for x in cat))


def split_counts(counts, min_gain=8.0):
    """The exact two-class split of ``counts`` that minimises the within-class sum of squares, every cut of the sorted
    values tried -> [(median, support), ...]: two classes when the split cuts the sum of squares about the single mean
    by at least the factor ``min_gain``, else one (none for no counts).  A normal sample cut at its mean gains the
    factor 2.75, a uniform one 4: one allele's counts stay one class."""
    x = np.sort(np.asarray(counts, dtype=np.float64))
    if x.size == 0:
        return []
    one = [(float(np.median(x)), int(x.size))]
    total = float(((x - x.mean()) ** 2).sum())
    if x.size < 2 or total == 0.0:
        return one
    sse = [float(((x[:c] - x[:c].mean()) ** 2).sum() + ((x[c:] - x[c:].mean()) ** 2).sum()) for c in range(1, x.size)]
    c = int(np.argmin(sse)) + 1
    if sse[c - 1] * float(min_gain) > total:
        return one
    return [(float(np.median(x[:c])), c), (float(np.median(x[c:])), int(x.size) - c)]


def genotype_table(post, stutter=0.5, decay=0.5, outlier=0.01):
    """The log-likelihood of every diploid genotype over a window of n counts, from the reads' posteriors ``post``
    (f64 (reads, n), rows summing to 1) -> G f64 (n, n), [a1, a2] for a1 <= a2 and -inf below the diagonal.  A read
    of allele a shows count c with K[c | a] = 1 - stutter at c = a and stutter / 2 * (1 - decay) * decay^(|c - a| - 1)
    elsewhere, each column renormalised over the window; l_r(a) = (1 - outlier) * SUM_c K[c | a] post_r[c] +
    outlier / n; G(a1, a2) = SUM_r log(l_r(a1) / 2 + l_r(a2) / 2), the reads summed in ascending order."""
    post = np.asarray(post, dtype=np.float64)
    n = post.shape[1]
    if not (0.0 <= stutter < 1.0 and 0.0 < decay < 1.0 and 0.0 <= outlier < 1.0):
        raise ValueError('genotype_table: stutter and outlier lie in [0, 1), decay in (0, 1)')
    d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])        # [c, a]
    K = np.where(d == 0, 1.0 - stutter, stutter / 2.0 * (1.0 - decay) * decay ** np.maximum(d - 1, 0))
    K = K / K.sum(axis=0, keepdims=True)
    like = (1.0 - outlier) * (post @ K) + outlier / n                # [r, a]
    G = np.full((n, n), -np.inf)
    for a1 in range(n):
        with np.errstate(divide='ignore'):
            terms = np.log(0.5 * like[:, a1:a1 + 1] + 0.5 * like[:, a1:])
        G[a1, a1:] = np.cumsum(terms, axis=0)[-1] if terms.shape[0] else 0.0
    return G


def likelihood_fields(c0_of_pair, status, z, x, lik_status):
    """The per-pair fields ``count_repeats_batch(layers=n)`` adds, numpy on the host, from the likelihood operator's
    outputs (``z`` (pairs, n), ``x`` (pairs,), ``lik_status``) -> dict of RepeatCountBatch.LIK_FIELDS.  log L =
    np.log(z) + x * log 2; the posterior: the row less its largest value, np.exp, divided by the sum in ascending
    order."""
    n, L = z.shape
    ok = (status == REP_OK) & (lik_status == REP_OK)
    with np.errstate(divide='ignore'):
        loglik = np.where(ok[:, None], np.log(z) + x[:, None] * math.log(2.0), np.nan)
    safe = np.where(ok[:, None], loglik, 0.0)
    w = np.exp(safe - safe.max(axis=1, keepdims=True)) if n else np.zeros((0, L))
    post = w / np.cumsum(w, axis=1)[:, -1:]
    counts = c0_of_pair[:, None] + np.arange(L)[None, :]
    top = post.argmax(axis=1) if n else np.zeros(0, dtype=np.int64)
    nan = lambda v: np.where(ok, v, np.nan)
    return dict(count_loglik=loglik, count_post=np.where(ok[:, None], post, np.nan),
                count_map=np.where(ok, c0_of_pair + top, -1),
                count_mean=nan(np.cumsum(post * counts, axis=1)[:, -1] if n else np.zeros(0)),
                count_conf=nan(post[np.arange(n), top]),
                clipped=ok & ((top == L - 1) | (post[:, L - 1] > 1e-3)))


class RepeatCountBatch:
    """What ``count_repeats_batch`` returns, numpy arrays with one entry per (read, locus) pair: ``read``, ``locus``,
    ``strand`` (0 forward, 1 reverse: the better-scoring one, forward on ties, or the one the item named), ``status``
    (REP_OK; REP_NO_EVENTS: fewer than ``min_events`` events, events of one level, or none in the window; REP_NO_PATH:
    fewer events than the chain needs), ``count`` (c0 + loops; -1 unless REP_OK), ``loops``, ``n_events``, ``first`` /
    ``last`` (the path's events inside the item), ``score`` (the path's log-likelihood per aligned event, trimmed ends
    left out), ``margin`` (nats by which the chosen strand's end value beats the other's; NaN if only one was scored),
    ``left_score`` / ``repeat_score`` / ``right_score`` (per event: before the repeat, inside it, after it, in the order
    the read passes them), ``repeat_start`` / ``repeat_end`` (the samples, inside the read, of the events with which
    the path enters the repeat and leaves it; -1 unless REP_OK), ``spanning`` (REP_OK, both marks crossed and, when
    ``min_flank_score`` was given, both flank scores at or above it).  ``loci``: the loci, ``c0``: per locus.

    With ``layers=n`` (else ``layers`` is 0 and these are None), per pair over the window of the n counts c0 .. c0 + n -
    1: ``count_loglik`` (f64 (pairs, n): the log-likelihood of the pair's events summed over all paths of that count,
    -inf where the sum is 0; NaN rows unless REP_OK), ``count_post`` (the same normalised per row under a flat prior
    over the window), ``count_map`` (the most likely count, the smallest of equal ones; -1 unless REP_OK),
    ``count_mean`` (the posterior mean), ``count_conf`` (the posterior of ``count_map``: it orders reads by how far the
    count can be trusted and is not a calibrated probability), ``clipped`` (``count_map`` is the window's last count,
    or the last count's posterior exceeds 1e-3: the window was too small for this read)."""

    FIELDS = ('read', 'locus', 'strand', 'status', 'count', 'loops', 'n_events', 'first', 'last', 'score', 'margin',
              'left_score', 'repeat_score', 'right_score', 'repeat_start', 'repeat_end', 'spanning')
    LIK_FIELDS = ('count_loglik', 'count_post', 'count_map', 'count_mean', 'count_conf', 'clipped')

    def __init__(self, loci, c0, kernel_ms=None, layers=0, lik_ms=None, **fields):
        self.loci, self.c0, self.kernel_ms = list(loci), np.asarray(c0, dtype=np.int64), kernel_ms
        self.layers, self.lik_ms = int(layers), lik_ms
        for f in self.FIELDS:
            setattr(self, f, fields[f])
        for f in self.LIK_FIELDS:
            setattr(self, f, fields[f] if self.layers else None)
        self.n = int(self.read.size)

    def locus_table(self):
        """-> per locus a dict: name, reads (pairs with REP_OK), spanning, histogram {count: spanning reads}"""
        out = []
        for li, locus in enumerate(self.loci):
            here = self.locus == li
            counts = self.count[here & self.spanning]
            values, n = np.unique(counts, return_counts=True)
            out.append(dict(name=locus.name, reads=int((here & (self.status == REP_OK)).sum()),
                            spanning=int(counts.size), histogram={int(v): int(c) for v, c in zip(values, n)}))
        return out

    def alleles(self, max_alleles=2, min_gain=8.0):
        """-> per locus [(allele count, supporting reads), ...] from the spanning reads' counts: ``split_counts``
        (class medians; one class unless two cut the sum of squares by ``min_gain``).  ``max_alleles``: 1 or 2."""
        if max_alleles not in (1, 2):
            raise ValueError('RepeatCountBatch.alleles: max_alleles is 1 or 2')
        out = []
        for li in range(len(self.loci)):
            counts = self.count[(self.locus == li) & self.spanning]
            out.append(split_counts(counts, min_gain if max_alleles == 2 else float('inf')))
        return out

    def genotypes(self, stutter=0.5, decay=0.5, outlier=0.01):
        """The diploid genotype of every locus from the per-count posteriors of its spanning, unclipped pairs
        (``genotype_table``; a batch made with ``layers``, else ValueError).  -> per locus None (no usable pair) or a
        dict: ``alleles`` (the best pair of counts, a1 <= a2), ``loglik`` (its G), ``margin`` (nats over the second-best
        pair; inf in a window of one count), ``het_margin`` (the best heterozygote's G less the best homozygote's; -inf
        in a window of one count), ``reads`` (the pairs used), ``table`` (G, f64 (n, n): [a1 - c0, a2 - c0], -inf below
        the diagonal).  ``stutter``, ``decay`` and ``outlier`` are UNCALIBRATED: round numbers at which the simulated
        batch of the test suite genotypes right, fitted to no real data.  A read cut off inside the repeat is left
        out, not used as a lower bound."""
        if not self.layers:
            raise ValueError('RepeatCountBatch.genotypes: the batch was made without layers')
        out = []
        for li in range(len(self.loci)):
            use = (self.locus == li) & self.spanning & ~self.clipped & (self.count_map >= 0)
            if not use.any():
                out.append(None)
                continue
            table = genotype_table(self.count_post[use], stutter, decay, outlier)
            n, c0 = self.layers, int(self.c0[li])
            order = np.argsort(-table, axis=None, kind='stable')
            a1, a2 = divmod(int(order[0]), n)
            het = np.triu(np.ones((n, n), dtype=bool), 1)
            best_het = float(table[het].max()) if n > 1 else -np.inf
            out.append(dict(alleles=(c0 + a1, c0 + a2), loglik=float(table[a1, a2]),
                            margin=float(table[a1, a2] - table.flat[order[1]]) if n > 1 else np.inf,
                            het_margin=best_het - float(np.diag(table).max()), reads=int(use.sum()), table=table))
        return out

    def write_tsv(self, path, names=None):
        """One line per (read, locus) pair -> lines written.  ``names``: one per read (default ``read_<index>``).  A
        batch made with ``layers`` appends ``count_map``, ``count_mean``, ``count_conf`` and ``clipped``."""
        cols = ('status', 'count', 'loops', 'n_events', 'score', 'margin', 'left_score', 'repeat_score',
                'right_score', 'repeat_start', 'repeat_end', 'spanning')
        if self.layers:
            cols += ('count_map', 'count_mean', 'count_conf', 'clipped')
        with open(path, 'w') as out:
            out.write('\t'.join(('read', 'locus', 'strand') + cols) + '\n')
            for p in range(self.n):
                r = int(self.read[p])
                row = [names[r] if names is not None else 'read_%d' % r, self.loci[int(self.locus[p])].name,
                       '+-'[int(self.strand[p])]]
                for c in cols:
                    v = getattr(self, c)[p]
                    row.append('%.4f' % v if isinstance(v, np.floating) else str(int(v)))
                out.write('\t'.join(row) + '\n')
        return self.n


def chain_tables(loci, kmer_model):
    """The chains of ``loci``, forward then reverse per locus (chain 2 l + strand) -> (ids int64 flat, st_off int64,
    chain_par int32 (chains, 4): lp_from, lp_to, m1, m2, c0 int64 per locus), numpy"""
    ids, par, c0 = [], [], []
    for locus in loci:
        for reverse in (False, True):
            chain = repeat_chain(locus, kmer_model, reverse)
            ids.append(chain[0])
            par.append(chain[1:5])
        c0.append(chain[5])
    st_off = np.concatenate([[0], np.cumsum([x.size for x in ids])]).astype(np.int64)
    return (np.concatenate(ids) if ids else np.zeros(0, np.int64), st_off,
            np.array(par, dtype=np.int32).reshape(-1, 4), np.array(c0, dtype=np.int64))


def pair_results(loci, c0, read, locus, strand_of, hit, score, ev_lo, ev_start, trim_cost, min_flank_score,
                 kernel_ms=None, layers=0, likelihoods=None):
    """Stage 6, numpy: the operator's per-item outputs -> RepeatCountBatch.  ``strand_of``: None when every pair owns
    two items (forward, reverse: items 2 p and 2 p + 1), else the strand of each pair's single item; ``ev_lo``: the
    items' first events in the flat ``ev_start``.  With ``layers``, ``likelihoods(pick, status)`` runs the likelihood
    operator on every pair's chosen item (``pick``: its index; ``status``: the pair's, its ``status_in``) -> (z, x,
    status, milliseconds or None), numpy."""
    n = int(read.size)
    if strand_of is None:
        end = score[:, 0].reshape(n, 2)
        strand = (end[:, 1] > end[:, 0]).astype(np.int64)      # forward on ties
        pick = 2 * np.arange(n) + strand
        both = (hit[0::2, 0] == REP_OK) | (hit[1::2, 0] == REP_OK)
        with np.errstate(invalid='ignore'):
            margin = np.where(both, end[np.arange(n), strand] - end[np.arange(n), 1 - strand], np.nan)
    else:
        strand, pick, margin = np.asarray(strand_of, dtype=np.int64), np.arange(n), np.full(n, np.nan)
    h, s, lo = hit[pick].astype(np.int64), score[pick], ev_lo[pick]
    status, first, last, loops, i1, i2 = h[:, 0], h[:, 2], h[:, 3], h[:, 4], h[:, 5], h[:, 6]
    ok = status == REP_OK
    f = first.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        nan = lambda x: np.where(ok, x, np.nan)
        path = nan((s[:, 1] - f * trim_cost) / (last - first + 1).astype(np.float64))
        left = nan((s[:, 2] - f * trim_cost) / (i1 - first).astype(np.float64))
        inner = nan((s[:, 3] - s[:, 2]) / (i2 - i1).astype(np.float64))
        right = nan((s[:, 1] - s[:, 3]) / (last - i2 + 1).astype(np.float64))
    sample = lambda i: np.where(ok, ev_start[np.where(ok, lo + i, 0)], -1).astype(np.int64) if ev_start.size \
        else np.full(n, -1, dtype=np.int64)
    spanning = ok & (i1 >= 0) & (i2 >= 0)
    if min_flank_score is not None:
        with np.errstate(invalid='ignore'):
            spanning &= (left >= min_flank_score) & (right >= min_flank_score)
    extra, lik_ms = {}, None
    if layers:
        z, x, lik_status, lik_ms = likelihoods(pick, status)
        extra = likelihood_fields(c0[locus], status, z, x, lik_status)
    return RepeatCountBatch(loci, c0, kernel_ms, layers, lik_ms, **extra, read=read, locus=locus, strand=strand,
                            status=status,
                            count=np.where(ok, c0[locus] + loops, -1) if n else np.zeros(0, np.int64), loops=loops,
                            n_events=h[:, 1], first=first, last=last, score=path, margin=margin, left_score=left,
                            repeat_score=inner, right_score=right, repeat_start=sample(i1), repeat_end=sample(i2),
                            spanning=spanning)


def count_repeats_batch(read_batch, loci, kmer_model=defaults.KMER_MODEL_FILE, items=None, p_stay=0.8, p_skip=0.01,
                        sigma_scale=0.5, trim_cost=math.log(0.01), min_events=32, window=2, threshold=5.0,
                        var_floor=0.02, min_flank_score=None, context=None, timer=None, layers=0):
    """The copy number of every locus of ``loci`` (``RepeatLocus``) in every read of ``read_batch``, from its raw
    signal alone (module docstring); any sequence or table the batch carries is ignored.  ``kmer_model``: a KmerModel
    or a path (4 letters); ``context``: the context a model loaded from a path is made on.  ``items``: None — every
    read against every locus, the whole read's events, both strands — or a ``RepeatItems`` (``repeat_items``): only
    those pairs, each on its strand and in its sample window.  ``p_stay`` / ``p_skip``: the chances that an event
    stays in its k-mer or passes one; ``sigma_scale``: the model's sigma is multiplied by it (above 0.5 the loop
    swallows unrelated signal); ``trim_cost`` (a log, <= 0): per event left out before or after the path;
    ``min_events`` (>= 1): a read with fewer is not counted; ``window``, ``threshold``, ``var_floor``: the event
    detector's; ``min_flank_score``: None, or the least per-event score of either flank for a read to count as
    spanning (a read that ends inside the repeat is not told by its path's score, which the repeat's events dominate,
    but by its worse flank).  The defaults are uncalibrated: the values at which the simulated reads of the test suite
    (dwell 3-17 samples, noise 0.35, the packaged 6-mer table) count best.  ``timer(name)``: called after each stage
    (bench tool).  ``layers``: 0, or the number n <= 128 of counts c0 .. c0 + n - 1 whose likelihoods, summed over all
    paths, the chosen item of every pair gets beside its Viterbi count (``nvk_repeat_likelihoods_dev``, with
    exp(trim_cost) as the trim's weight): the ``count_*`` fields and ``clipped`` of the result, and what
    ``RepeatCountBatch.genotypes`` stands on.  -> RepeatCountBatch."""
    import torch
    from .decode import tables_dev
    from .device import repeat_count_dev, repeat_likelihoods_dev
    kmer_model = resolve_kmer_model(kmer_model, context)
    layers = int(layers)
    if not 0 <= layers <= MAX_LAYERS:
        raise ValueError('count_repeats_batch: layers is 0 (no likelihoods) or at most %d' % MAX_LAYERS)
    if int(min_events) < 1:
        raise ValueError('count_repeats_batch: min_events is at least 1')
    if not (trim_cost <= 0.0 and math.isfinite(trim_cost)):
        raise ValueError('count_repeats_batch: trim_cost is a finite log, at most 0')
    costs = transition_costs(p_stay, p_skip, 'count_repeats_batch')
    loci = list(loci)
    ids, st_off, chain_par, c0 = chain_tables(loci, kmer_model)
    rb, m = read_batch, len(loci)
    if items is None:
        read, locus = np.repeat(np.arange(rb.n, dtype=np.int64), m), np.tile(np.arange(m, dtype=np.int64), rb.n)
    else:
        read, locus = items.read, items.locus
        if items.n and (read.min() < 0 or read.max() >= rb.n or locus.min() < 0 or locus.max() >= m
                        or (items.sig_lo < 0).any() or (items.sig_hi < items.sig_lo).any()
                        or (items.sig_hi > np.diff(rb.sig_off)[read]).any()):
            raise ValueError('count_repeats_batch: an item names a read, a locus or samples that do not exist')
    n = int(read.size)
    n_items = 2 * n if items is None else n
    if n == 0 or rb.raw_signal.size == 0:      # nothing to run: every item is REP_NO_EVENTS
        hit = np.tile(np.array([REP_NO_EVENTS, 0, -1, -1, -1, -1, -1, 0], dtype=np.int32), (n_items, 1))
        return pair_results(loci, c0, read, locus, None if items is None else items.reverse, hit,
                            np.full((n_items, 4), -np.inf), np.zeros(n_items, dtype=np.int64),
                            np.zeros(0, dtype=np.int64), trim_cost, min_flank_score, None, layers,
                            lambda pick, status: (np.zeros((n, layers)), np.zeros(n), status, None))
    ctx = kmer_model.context
    device = torch.device('cuda', ctx.device)
    tick = timer if timer is not None else (lambda name: None)
    ev = signal_events_dev(rb, ctx, window, threshold, var_floor, tick)
    mean = torch.from_numpy(np.ascontiguousarray(kmer_model.mean, dtype=np.float64)).to(device)
    pool_off = torch.tensor([0, int(mean.numel())], dtype=torch.int64, device=device)
    scaled, _, _, ok = rescale_by_moments_dev(ctx, ev.ev_level, ev.ev_off, mean, pool_off, min_events=min_events)
    tick('rescale')
    mu, ac, mc = tables_dev(np.asarray(kmer_model.mean)[ids], np.asarray(kmer_model.sigma)[ids], sigma_scale, device)
    d_read = torch.from_numpy(read).to(device)
    if items is None:
        chain = 2 * torch.from_numpy(locus).to(device)
        ev_lo, ev_hi = ev.ev_off[:-1][d_read], ev.ev_off[1:][d_read]
        triples = torch.stack([torch.stack([chain, chain + 1], 1), torch.stack([ev_lo, ev_lo], 1),
                               torch.stack([ev_hi, ev_hi], 1)], 2).reshape(-1, 3)
        item_read = d_read.repeat_interleave(2)
    else:
        chain = torch.from_numpy(2 * locus + items.reverse).to(device)
        base = ev.sig_off[:-1][d_read]
        # the events that start inside the window: the flat positions of the borders ascend over the whole batch
        ev_lo = torch.searchsorted(ev.ev_pos, base + torch.from_numpy(items.sig_lo).to(device))
        ev_hi = torch.searchsorted(ev.ev_pos, base + torch.from_numpy(items.sig_hi).to(device))
        triples, item_read = torch.stack([chain, ev_lo, ev_hi], 1), d_read
    status_in = torch.where(ok[item_read], REP_OK, REP_NO_EVENTS).to(torch.int32)
    tick('items')
    out = repeat_count_dev(ctx, scaled, triples.contiguous(), mu, ac, mc, torch.from_numpy(st_off).to(device),
                           torch.from_numpy(chain_par).to(device), *costs, trim_cost, status_in,
                           timing=timer is not None)
    tick('count')
    host = lambda t: t.cpu().numpy()

    def likelihoods(pick, status):
        lik = repeat_likelihoods_dev(ctx, scaled, triples[torch.from_numpy(pick).to(device)].contiguous(), mu, ac, mc,
                                     torch.from_numpy(st_off).to(device), torch.from_numpy(chain_par).to(device),
                                     *transition_weights(p_stay, p_skip), math.exp(trim_cost), layers,
                                     torch.from_numpy(status.astype(np.int32)).to(device), timing=timer is not None)
        tick('likelihoods')
        return host(lik[0]), host(lik[1]), host(lik[2]), lik[3] if timer is not None else None

    res = pair_results(loci, c0, read, locus, None if items is None else items.reverse, host(out[0]), host(out[1]),
                       host(triples[:, 1]), host(ev.ev_start), trim_cost, min_flank_score,
                       out[2] if timer is not None else None, layers, likelihoods)
    tick('results')
    return res
