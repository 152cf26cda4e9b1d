"""``ReferenceSet`` — a reference of several contigs (FASTA records) and the one coordinate system the batch path
uses for it.

The contigs are laid end to end with nothing between them: ``names`` (list of str), ``offsets`` (int64[C+1],
``offsets[0] = 0``) and ``codes`` (int32[G], ``G = offsets[C] <= 2^30``, the limit of the seed aligner's extension
kernel).  Zero-length contigs are allowed; no position belongs to them.

Global coordinates.  On strand 0 contig c occupies [offsets[c], offsets[c+1]).  Strand 1 is the reverse complement
of the whole concatenation, ``rc[x] = 3 - codes[G-1-x]``, so contig c occupies [G - offsets[c+1], G - offsets[c])
there and a contig-local oriented index y (counted from the contig's end, as the reference's alignment.py:128-134
counts it) is the strand coordinate ``G - offsets[c+1] + y``.  In these coordinates the ``L - x`` mirror of
``readbatch.signal_alignments`` and the consensus over forward positions hold as for one sequence: chunks of
different contigs can only touch, and touching chunks do not merge (``ProbabilityEstimator.group_ranges``)."""
import os

import numpy as np

MAX_TOTAL = 1 << 30


class ReferenceSet:
    def __init__(self, names, offsets, codes):
        self.names = [str(x) for x in names]
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if self.offsets.size != len(self.names) + 1 or self.offsets[0] != 0 or (np.diff(self.offsets) < 0).any():
            raise ValueError('ReferenceSet: offsets must hold one more entry than names, start at 0 and never decrease')
        if len(set(self.names)) != len(self.names):
            seen = set()
            twice = sorted({x for x in self.names if x in seen or seen.add(x)})
            raise ValueError('ReferenceSet: duplicate contig name(s) %s' % ', '.join(map(repr, twice[:8])))
        if int(self.offsets[-1]) > MAX_TOTAL:
            raise ValueError('ReferenceSet: %d bases over all contigs, above the limit 2^30' % int(self.offsets[-1]))
        self.codes = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        if self.codes.size != int(self.offsets[-1]):
            raise ValueError('ReferenceSet: codes hold %d bases, the offsets end at %d'
                             % (self.codes.size, int(self.offsets[-1])))

    @classmethod
    def from_arrays(cls, names, arrays):
        """``arrays``: per contig its base codes 0..3."""
        arrays = [np.asarray(a).reshape(-1) for a in arrays]
        offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
        np.cumsum([a.size for a in arrays], out=offsets[1:])
        codes = np.concatenate([a.astype(np.int32) for a in arrays]) if arrays else np.zeros(0, dtype=np.int32)
        return cls(names, offsets, codes)

    @classmethod
    def from_fasta(cls, path):
        """One contig per record, named as ``load_model_and_estimator`` keys its ``references_dict``: the description
        line without its '>'."""
        from .genome import Genome
        records = Genome.load_from_fasta(os.fspath(path))
        return cls.from_arrays([r.description[1:] for r in records], [Genome.to_numerical(r.bases) for r in records])

    @property
    def n_contigs(self):
        return len(self.names)

    @property
    def total(self):
        return int(self.offsets[-1])

    def contig_codes(self, c):
        return self.codes[self.offsets[c]:self.offsets[c + 1]]

    def locate(self, x):
        """Forward global position(s) ``x`` (0 <= x < G; numpy or torch, any shape) -> (contig, local).  An end
        position e maps through ``locate(e - 1)``: (contig, local + 1)."""
        if hasattr(x, 'device') and hasattr(x, 'numel'):
            import torch
            off = torch.from_numpy(self.offsets).to(x.device)
            c = torch.searchsorted(off, x.to(torch.int64).contiguous(), right=True) - 1
            return c, x - off[c]
        x = np.asarray(x)
        c = np.searchsorted(self.offsets, x, side='right') - 1
        return c, x - self.offsets[c]

    def locate_range(self, start, end):
        """A non-empty forward global range [start, end) inside one contig -> (contig, local start, local end)."""
        c, s = self.locate(start)
        return c, s, s + (end - start)
