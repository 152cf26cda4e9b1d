"""``SeedAligner`` — a device-resident batch aligner: basecalled reads to matched (read base, reference base) pairs,
the ``BaseAlignmentBatch`` that ``align_signal_batch``, ``estimate_snps_batch`` and ``detect_meth_batch`` take from
their ``aligner``, with no BWA and no per-read Python.

It is not BWA and does not reproduce BWA's hits; what it computes is specified exactly, so that a CPU restatement and
the kernel agree bit for bit.  Scoring defaults to what the reference asks of BWA (``-x ont2d``: match 1, mismatch 1,
gap open 1, gap extend 1: the reference's nadavca/alignment.py:36), and pairs follow the reference's CIGAR rule:
only aligned columns whose two bases are equal (alignment.py:118-138, ``alignment._get_base_alignment``).

1. Seeds and vote (torch, on the aligner's device).  Per strand (0: the reference, 1: its reverse complement
   ``rc[x] = 3 - ref[G-1-x]``) a seed is a pair (i, p) with read k-mer i equal to strand k-mer p; a read k-mer that
   occurs more than ``max_occ`` times in the strand gives none.  Seed diagonal d = p - i, window c = floor(d / w);
   window c scores n(c) + n(c+1) seeds (diagonals [c w, (c+2) w)).  Each strand takes its best window (smallest c on a
   tie), the read its better strand (forward on a tie); below ``min_seeds`` the read is unaligned, else the band
   centre d* is the lower median of the window's seed diagonals (index (n-1)//2 of them sorted).
   Several contigs (a ``refset.ReferenceSet``): the strands are those of the concatenation, in its global coordinates;
   a strand k-mer whose k bases do not lie in one contig is not indexed, and seeding and the vote are otherwise the
   same, on global diagonals.  The read's contig: on the chosen strand x* = clamp(d* + (m - 1) // 2, 0, G - 1), m the
   read's length — where its middle base lands on the voted diagonal — and the contig is the one whose range on that
   strand, [lo, hi), contains x* (``contig_of``).  The extension sees only the columns lo <= j < hi.
2. Banded affine-gap local alignment around d* and 3. traceback, in the HIP kernel ``nvk_seed_extend_dev``
   (include/nadavca_hip.h states the rules; nadavca_amd/csrc/kernels_seedext.hip; with a ReferenceSet
   ``nvk_seed_extend_bounded_dev``, the same kernel held to the read's contig).  A read whose score is below
   ``min_score`` is unaligned.  There is no CPU form of steps 2 and 3 in the package.

``chain=1`` (off by default) lets the band follow the read instead of standing on d*: a read whose insertions and
deletions do not cancel drifts off any one diagonal by about (deletion rate - insertion rate) x its length, and a
fixed band keeps only the piece that fits.  Between steps 1 and 2 the seeds of the voted strand (``strand_seeds``;
over a ReferenceSet those inside the read's contig), sorted by (p, i) (``sort_seeds``), are chained by the HIP kernel
``nvk_seed_chain_dev`` (kernels_seedchain.hip): f[t] = max(k, max_u f[u] + min(di, dp, k) - |dp - di|) over the 64
seeds before t with 0 < di, dp <= ``max_gap`` and |dp - di| <= band; the best chain's anchors give every strip of 64
read rows its own centre, p - i of the anchor nearest the strip's middle.  Steps 2 and 3 then run in
``nvk_seed_extend_path_dev``, the same kernel body with the centre taken per strip.  Strand, vote, contig and
``min_score`` keep their rules; a read without a chain keeps d* in every strip.  include/nadavca_hip.h states both
contracts."""
import numpy as np

from . import _lib
from .batchflow import seg_index
from .readbatch import BaseAlignmentBatch
from .refset import ReferenceSet

PARAMS = dict(k=14, max_occ=32, band=64, min_seeds=2, match=1, mismatch=1, gap_open=1, gap_extend=1, min_score=30,
              chain=0, max_gap=500)


def _check_params(p):
    unknown = sorted(set(p) - set(PARAMS))
    if unknown:
        raise ValueError('SeedAligner: unknown parameter(s) %s' % ', '.join(unknown))
    q = dict(PARAMS)
    q.update(p)
    ranges = dict(k=(8, 15), max_occ=(1, None), band=(1, 256), min_seeds=(1, None), match=(1, 16),
                  mismatch=(1, 16), gap_open=(1, 16), gap_extend=(1, 16), min_score=(1, None), chain=(0, 1),
                  max_gap=(1, 1 << 26))
    for name, (lo, hi) in ranges.items():
        v = q[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
            raise ValueError('SeedAligner: %s = %r is outside %d..%s' % (name, v, lo, hi if hi is not None else ''))
        q[name] = int(v)
    return q


def _load_reference(reference):
    import os
    if isinstance(reference, (str, os.PathLike)):
        from .genome import Genome
        records = Genome.load_from_fasta(os.fspath(reference))
        if len(records) != 1:
            raise ValueError('SeedAligner: %s holds %d FASTA records; a path stands for exactly one, several go in as '
                             'ReferenceSet.from_fasta(path)' % (os.fspath(reference), len(records)))
        return np.ascontiguousarray(Genome.to_numerical(records[0].bases), dtype=np.int32)
    return np.ascontiguousarray(np.asarray(reference).reshape(-1), dtype=np.int32)


class SeedHits:
    """What ``SeedAligner.align`` returns, numpy arrays: per read ``reverse`` (bool: the chosen strand, False for an
    unaligned read), ``strand`` (int32: 0, 1, or -1 where the seeds did not vote for any), ``diagonal`` (int64 d*,
    0 without a strand), ``votes`` (int64: the chosen window's seeds), ``score`` (int32), ``end`` (int32 (n, 2): the
    end cell (i, j), -1 where there was no cell), ``aligned`` (bool); and the pairs of read j,
    ``read_idx`` / ``ref_idx`` [off[j], off[j+1]), ascending — ``ref_idx`` on the chosen strand, counted from the
    reference's end on strand 1.  ``contig`` (int32): 0 for an aligned read, -1 for an unaligned one.
    From an aligner over a ReferenceSet (``reference_set``, else None): ``contig`` is the read's contig, ``ref_idx``
    is contig-local — the strand coordinate less the contig's first one, i.e. counted from the contig's end on strand
    1 — while ``diagonal`` and ``end`` stay in the concatenation's strand coordinates.
    From an aligner with ``chain=1`` (else all four are None): ``chain_score`` and ``chain_anchors`` (int32: the score
    of the read's seed chain and the number of seeds on it, 0 where there is none), ``strip_off`` (int64 (n + 1,)) and
    ``strip_diagonal`` (int32): the band centre of rows 64 s .. 64 s + 63 of read j is
    ``strip_diagonal[strip_off[j] + s]``, in the coordinates of ``diagonal``, and equals ``diagonal[j]`` for a read
    without a chain."""

    def __init__(self, strand, diagonal, votes, score, end, aligned, off, read_idx, ref_idx, contig=None,
                 reference_set=None, chain_score=None, chain_anchors=None, strip_off=None, strip_diagonal=None):
        self.strand, self.diagonal, self.votes, self.score, self.end = strand, diagonal, votes, score, end
        self.chain_score, self.chain_anchors = chain_score, chain_anchors
        self.strip_off, self.strip_diagonal = strip_off, strip_diagonal
        self.aligned, self.off, self.read_idx, self.ref_idx = aligned, off, read_idx, ref_idx
        self.reverse = aligned & (strand == 1)
        self.contig = np.where(aligned, 0, -1).astype(np.int32) if contig is None else contig
        self.reference_set = reference_set

    @property
    def n(self):
        return self.strand.size

    def base_alignments(self):
        return BaseAlignmentBatch(self.read_idx, self.ref_idx, self.off, self.reverse,
                                  contig=None if self.reference_set is None else self.contig)


class SeedAligner:
    """``SeedAligner(reference, device=None, **params)``: ``reference`` is base codes 0..3, the path of a FASTA
    file with exactly one record, or a ``refset.ReferenceSet`` (several contigs: ``reference_set`` is then that set,
    else None, and ``reference_num`` its concatenation; a FASTA file of several records goes in as
    ``ReferenceSet.from_fasta(path)``); ``params`` as in ``PARAMS`` (``k`` 8..15, ``max_occ`` >= 1, ``band`` (the
    half-width w, in diagonals) 1..256, ``min_seeds`` >= 1, ``match`` / ``mismatch`` / ``gap_open`` / ``gap_extend``
    1..16 (a gap of length l costs gap_open + l * gap_extend), ``min_score`` >= 1, ``chain`` 0 or 1 (1: the band
    follows the read's seed chain, see the module's text) and ``max_gap`` >= 1 (the chain's largest step between two
    seeds, in read and in reference bases)); out of range raises ValueError.
    ``device``: where the reference, its k-mer index and the seeding live (default: the library's default GPU).  The
    index of both strands is built once, here.  ``align`` and ``get_base_alignments`` need a GPU device; ``seed``
    (step 1 alone) runs on any."""

    def __init__(self, reference, device=None, **params):
        import torch
        self.params = _check_params(params)
        self.reference_set = reference if isinstance(reference, ReferenceSet) else None
        self.reference_num = _load_reference(reference if self.reference_set is None else reference.codes)
        if device is None:
            device = torch.device('cuda', _lib.default_context().device)
        self.device = torch.device(device)
        ref = torch.from_numpy(self.reference_num).to(self.device).to(torch.int64)
        self._ref = ref.to(torch.int32)
        G = int(ref.numel())
        rc = 3 - ref.flip(0) if G else ref
        if self.reference_set is None:
            self._offsets = None
            self._index = [self._build_index(ref), self._build_index(rc)]
        else:
            # the contigs' boundaries on each strand, ascending (on strand 1 the contigs run backwards)
            self._offsets = torch.from_numpy(self.reference_set.offsets).to(self.device)
            self._index = [self._build_index(ref, self._offsets), self._build_index(rc, (G - self._offsets).flip(0))]

    # ---- step 1 ---------------------------------------------------------------------------------------------
    def _kmers(self, seq, length):
        """k-mer codes (2 bits per base) of positions 0 .. length-1 of int64 ``seq`` (which holds at least
        length + k - 1 elements) and whether all their bases are 0..3."""
        import torch
        k = self.params['k']
        code = torch.zeros(length, dtype=torch.int64, device=self.device)
        ok = torch.ones(length, dtype=torch.bool, device=self.device)
        for u in range(k):
            x = seq[u:u + length]
            ok &= (x >= 0) & (x <= 3)
            code = code * 4 + x.clamp(0, 3)
        return code, ok

    def _build_index(self, strand_seq, bounds=None):
        """``bounds``: the contigs' boundaries on this strand, ascending; a k-mer that crosses one is left out."""
        import torch
        k = self.params['k']
        n_pos = int(strand_seq.numel()) - k + 1
        if n_pos <= 0:
            return (torch.zeros(0, dtype=torch.int64, device=self.device),) * 2
        code, ok = self._kmers(strand_seq, n_pos)
        pos = torch.arange(n_pos, dtype=torch.int64, device=self.device)
        if bounds is not None:
            ok &= torch.searchsorted(bounds, pos, right=True) == torch.searchsorted(bounds, pos + (k - 1), right=True)
        pos = pos[ok]
        keys, order = torch.sort(code[ok], stable=True)
        return keys, pos[order]

    def _check_reads(self, read_batch):
        seq = read_batch.sequence
        if seq.size and (int(seq.min()) < 0 or int(seq.max()) > 3):
            raise ValueError('SeedAligner: read sequences hold base codes outside 0..3')

    def seed(self, read_batch):
        """Step 1 for every read of ``read_batch``, on the aligner's device: -> (strand int32, diagonal int64,
        votes int64), torch tensors of n reads; strand -1 (diagonal 0) where the read did not reach ``min_seeds``."""
        return self._seed(read_batch)[:3]

    def strand_seeds(self, read_batch):
        """Step 1 and the seeds it voted with: -> (strand, diagonal, votes, seed_read, seed_i, seed_p): the first
        three as ``seed`` returns them, then every seed (i, p) of each read on the strand its vote chose (all of them,
        not only the winning window's), int64 tensors in no particular order; a read without a strand has none.  From
        an aligner over a ReferenceSet only the seeds inside the read's contig (``contig_of``):
        ref_lo <= p < ref_hi."""
        import torch
        strand, diagonal, votes, seeds = self._seed(read_batch)
        voted = [strand[x[0]] == s for s, x in enumerate(seeds)]
        rd, si, sp = (torch.cat([x[f][v] for x, v in zip(seeds, voted)]) for f in (0, 3, 4))
        if self.reference_set is not None:
            _, ref_lo, ref_hi = self.contig_of(read_batch, strand, diagonal)
            keep = (sp >= ref_lo[rd]) & (sp < ref_hi[rd])
            rd, si, sp = rd[keep], si[keep], sp[keep]
        return strand, diagonal, votes, rd, si, sp

    @staticmethod
    def sort_seeds(n, seed_read, seed_i, seed_p):
        """The seeds of ``strand_seeds`` in the order the chaining takes them: by read, then p, then i.
        -> (seed_off int64 (n + 1,), seed_i int32, seed_p int32)."""
        import torch
        span = int(seed_i.max()) + 1 if seed_i.numel() else 1
        order = torch.sort(seed_p * span + seed_i).indices       # p < 2^30, i < 2^26
        order = order[torch.sort(seed_read[order], stable=True).indices]
        off = torch.zeros(n + 1, dtype=torch.int64, device=seed_read.device)
        torch.cumsum(torch.bincount(seed_read, minlength=n)[:n], 0, out=off[1:])
        return off, seed_i[order].to(torch.int32), seed_p[order].to(torch.int32)

    def _seed(self, read_batch):
        """-> ``seed``'s three, and per strand the seeds (read, diagonal, window, i, p)."""
        import torch
        self._check_reads(read_batch)
        p = self.params
        k, w, dev, i64 = p['k'], p['band'], self.device, torch.int64
        n = read_batch.n
        G = int(self.reference_num.size)
        q_off = torch.from_numpy(read_batch.seq_off).to(dev)
        seq = torch.from_numpy(read_batch.sequence).to(dev).to(i64)
        total = int(seq.numel())
        lens = q_off[1:] - q_off[:-1]
        max_m = int(lens.max()) if n else 0
        owner, inner = seg_index(q_off, total)
        code, _ = self._kmers(torch.cat([seq, torch.zeros(k, dtype=i64, device=dev)]), total)
        starts = torch.nonzero(inner <= lens[owner] - k).reshape(-1)   # read k-mers (codes are checked above)
        q_code = code[starts]
        # windows are keyed read * CR + (c + C0): c runs over [-(max_m // w) - 1, (G - 1) // w], so c - 1 and c + 1
        # stay inside a read's key range
        C0 = max_m // w + 3
        CR = C0 + G // w + 3
        votes, cstar, seeds = [], [], []
        for keys, pos in self._index:
            lo = torch.searchsorted(keys, q_code)
            cnt = torch.searchsorted(keys, q_code, right=True) - lo
            use = (cnt >= 1) & (cnt <= p['max_occ'])
            t, lo, cnt = starts[use], lo[use], cnt[use]
            n_seeds = int(cnt.sum()) if cnt.numel() else 0
            best = torch.zeros(n, dtype=i64, device=dev)
            best_c = torch.zeros(n, dtype=i64, device=dev)
            if n_seeds == 0:
                votes.append(best)
                cstar.append(best_c)
                seeds.append((torch.zeros(0, dtype=i64, device=dev),) * 5)
                continue
            sk = torch.repeat_interleave(torch.arange(t.numel(), dtype=i64, device=dev), cnt, output_size=n_seeds)
            within = torch.arange(n_seeds, dtype=i64, device=dev) - (torch.cumsum(cnt, 0) - cnt)[sk]
            rd, si, sp = owner[t][sk], inner[t][sk], pos[lo[sk] + within]
            d = sp - si
            c = torch.div(d, w, rounding_mode='floor')
            uk, un = torch.unique(rd * CR + c + C0, return_counts=True)
            cand = torch.unique(torch.cat([uk, uk - 1]))

            def n_of(x):
                j = torch.searchsorted(uk, x).clamp(max=uk.numel() - 1)
                return torch.where(uk[j] == x, un[j], torch.zeros_like(un[j]))

            score = n_of(cand) + n_of(cand + 1)
            cread = torch.div(cand, CR, rounding_mode='floor')
            best.scatter_reduce_(0, cread, score, 'amax')
            first = torch.full((n,), torch.iinfo(i64).max, dtype=i64, device=dev)
            first.scatter_reduce_(0, cread, torch.where(score == best[cread], cand, first[cread]), 'amin')
            best_c = torch.where(best > 0, first - torch.arange(n, dtype=i64, device=dev) * CR - C0, best_c)
            votes.append(best)
            cstar.append(best_c)
            seeds.append((rd, d, c, si, sp))
        rev = votes[1] > votes[0]
        n_votes = torch.where(rev, votes[1], votes[0])
        c_win = torch.where(rev, cstar[1], cstar[0])
        aligned = n_votes >= p['min_seeds']
        strand = torch.where(aligned, rev.to(torch.int32), torch.full_like(rev, -1, dtype=torch.int32))
        # d*: the lower median of the chosen window's seed diagonals
        D0 = max_m + 1
        DR = D0 + G + 1
        sel_r, sel_d = [], []
        for s, (rd, d, c, _, _) in enumerate(seeds):
            if rd.numel() == 0:
                continue
            keep = (strand[rd] == s) & ((c == c_win[rd]) | (c == c_win[rd] + 1))
            sel_r.append(rd[keep])
            sel_d.append(d[keep])
        diagonal = torch.zeros(n, dtype=i64, device=dev)
        if sel_r and sum(int(x.numel()) for x in sel_r):
            rd, d = torch.cat(sel_r), torch.cat(sel_d)
            key, _ = torch.sort(rd * DR + d + D0)
            per = torch.bincount(rd, minlength=n)
            start = torch.cumsum(per, 0) - per
            mid = (start + torch.div(per - 1, 2, rounding_mode='floor')).clamp(min=0, max=key.numel() - 1)
            med = key[mid] - torch.arange(n, dtype=i64, device=dev) * DR - D0
            diagonal = torch.where(aligned, med, diagonal)
        return strand, diagonal, n_votes, seeds

    def contig_of(self, read_batch, strand, diagonal):
        """The contig rule of step 1 for a ReferenceSet aligner, on the aligner's device: ``strand`` / ``diagonal`` as
        ``seed`` returns them -> (contig int32, -1 without a strand; ref_lo, ref_hi int32: the contig's range on the
        read's strand, [0, G) without one)."""
        import torch
        dev, i64 = self.device, torch.int64
        off = self._offsets
        G = int(self.reference_num.size)
        n = read_batch.n
        m = torch.from_numpy(np.diff(read_batch.seq_off)).to(dev)
        has = (strand >= 0) & (G > 0)
        x = (diagonal + torch.div(m - 1, 2, rounding_mode='floor')).clamp(min=0, max=max(G - 1, 0))
        fwd = torch.where(strand == 1, G - 1 - x, x)       # x* as a forward position
        c = (torch.searchsorted(off, fwd.contiguous(), right=True) - 1).clamp(min=0, max=max(off.numel() - 2, 0))
        if off.numel() < 2:
            has = torch.zeros(n, dtype=torch.bool, device=dev)
            off = torch.zeros(2, dtype=i64, device=dev)
        lo = torch.where(strand == 1, G - off[c + 1], off[c])
        hi = torch.where(strand == 1, G - off[c], off[c + 1])
        zero = torch.zeros_like(lo)
        return (torch.where(has, c, zero - 1).to(torch.int32), torch.where(has, lo, zero).to(torch.int32),
                torch.where(has, hi, zero + G).to(torch.int32))

    # ---- steps 2 and 3 ----------------------------------------------------------------------------------------
    def align(self, read_batch):
        """-> SeedHits for every read of ``read_batch``: step 1 here, steps 2 and 3 in the kernel."""
        import torch
        from .device import seed_extend_dev
        if self.device.type != 'cuda':
            raise _lib.NadavcaHipError('SeedAligner.align: the extension stage runs only in the HIP kernel; this '
                                       'aligner was built on %s' % self.device)
        p, dev, i64 = self.params, self.device, torch.int64
        ctx = _lib.default_context(dev.index or 0)
        n = read_batch.n
        q_off = torch.from_numpy(read_batch.seq_off).to(dev)
        query = torch.from_numpy(read_batch.sequence).to(dev)
        chain = {}
        if p['chain']:
            strand, diagonal, votes, seed_read, seed_i, seed_p = self.strand_seeds(read_batch)
        else:
            strand, diagonal, votes = self.seed(read_batch)
        contig = ref_lo = ref_hi = None
        if self.reference_set is not None:
            contig, ref_lo, ref_hi = self.contig_of(read_batch, strand, diagonal)
        scoring = (p['band'], p['match'], p['mismatch'], p['gap_open'], p['gap_extend'], p['min_score'])
        if p['chain']:
            from .device import seed_chain_dev, seed_extend_path_dev
            seed_off, seed_i, seed_p = self.sort_seeds(n, seed_read, seed_i, seed_p)
            strips = torch.div(q_off[1:] - q_off[:-1] + 63, 64, rounding_mode='floor')
            strip_off = torch.zeros(n + 1, dtype=i64, device=dev)
            torch.cumsum(strips, 0, out=strip_off[1:])
            # every strip starts at the voted d*: what a read keeps whose seeds give no chain
            strip_diag = torch.repeat_interleave(diagonal.to(torch.int32), strips).contiguous()
            chain_score, anchors = seed_chain_dev(ctx, q_off, strand, seed_off, seed_i, seed_p, strip_off, strip_diag,
                                                  p['k'], p['band'], p['max_gap'])
            score, end, count, pairs = seed_extend_path_dev(ctx, query, q_off, self._ref, strand, strip_off,
                                                            strip_diag, *scoring, ref_lo, ref_hi)
            chain = dict(chain_score=chain_score.cpu().numpy(), chain_anchors=anchors.cpu().numpy(),
                         strip_off=strip_off.cpu().numpy(), strip_diagonal=strip_diag.cpu().numpy())
        else:
            score, end, count, pairs = seed_extend_dev(ctx, query, q_off, self._ref, strand, diagonal, *scoring,
                                                       ref_lo, ref_hi)
        count = count.to(i64)
        off = torch.zeros(n + 1, dtype=i64, device=dev)
        torch.cumsum(count, 0, out=off[1:])
        owner, inner = seg_index(off)
        got = pairs[q_off[:-1][owner] + inner]
        aligned = (strand >= 0) & (score >= p['min_score'])
        h = lambda t: t.cpu().numpy()
        ref_idx = got[:, 1].to(i64)
        if contig is not None:
            ref_idx = ref_idx - ref_lo.to(i64)[owner]
            contig = h(torch.where(aligned, contig, torch.full_like(contig, -1)))
        return SeedHits(h(strand), h(diagonal), h(votes), h(score), h(end), h(aligned), h(off), h(got[:, 0]),
                        h(ref_idx), contig, self.reference_set, **chain)

    def get_base_alignments(self, read_batch):
        """The aligner contract of the batch workflows: -> BaseAlignmentBatch."""
        return self.align(read_batch).base_alignments()
