"""The multi-contig fixture of tests/test_contigs_cpu.py and tests/test_gpu_contigs.py: five contigs — 10 000, 4 000
and 400 bases with 48 simulated reads each (``synthetic.make_read_batch``, seeds 31, 32, 33; the reads of the 400-base
contig cover it end to end, so they sit flush against both of its joins), then one of 9 bases (shorter than k) and one
of length 0, which no read comes from.  Truth: each read's contig and the per-contig ``SyntheticBatchAligner`` pairs.
Also ``two_contig_samples``, the two samples over two contigs of tests/test_gpu_site_ranks.py and
tests/test_gpu_site_mixtures.py."""
import numpy as np

NAMES = ['chrA', 'chrB', 'flush400', 'tiny9', 'empty']
SEEDS = (31, 32, 33)
LENGTHS = (10000, 4000, 400)
READS_PER_CONTIG = 48


def concat_batches(batches):
    from nadavca_amd.readbatch import ReadBatch
    off = lambda name: np.concatenate([[0]] + [np.diff(getattr(b, name)) for b in batches]).cumsum().astype(np.int64)
    cat = lambda name: np.concatenate([getattr(b, name) for b in batches])
    return ReadBatch(cat('raw_signal'), off('sig_off'), cat('sequence'), off('seq_off'), cat('map_base'),
                     cat('map_sig'), off('map_off'))


def concat_alignments(bas, contig=None, shift=None):
    """Per-part BaseAlignmentBatch objects end to end; ``contig``: per part its contig index (-> the batch carries
    ``contig``); ``shift``: per part a function (ref_idx, reverse per pair) -> ref_idx (a lift to other coordinates)."""
    from nadavca_amd.readbatch import BaseAlignmentBatch
    ref = []
    for p, b in enumerate(bas):
        r = b.ref_idx
        if shift is not None:
            r = shift[p](r, np.repeat(b.reverse, np.diff(b.off)))
        ref.append(r)
    off = np.concatenate([[0]] + [np.diff(b.off) for b in bas]).cumsum().astype(np.int64)
    c = None if contig is None else np.concatenate([np.full(b.reverse.size, ci, np.int32) for ci, b in zip(contig, bas)])
    return BaseAlignmentBatch(np.concatenate([b.read_idx for b in bas]), np.concatenate(ref), off,
                              np.concatenate([b.reverse for b in bas]), contig=c)


def two_contig_samples(model5):
    """The input of the site tests' two-contig cases: per sample (unmodified; 0.3 of the CG sites modified) 150 reads
    of a 2 000-base contig and 100 of a 1 200-base one in one ReadBatch, and ONE ``SeedAligner`` over the
    ``ReferenceSet`` of the two.  -> ([ReadBatch A, ReadBatch B], the contigs' codes, their names, the aligner)"""
    from nadavca_amd import ReferenceSet, SeedAligner, synthetic
    shapes = ((150, 41, 2000), (100, 42, 1200))                  # reads per sample, genome seed, bases
    samples, contigs = [], None
    for fraction, read_seed in ((0.0, 111), (0.3, 211)):
        parts = [synthetic.make_modified_read_batch(n, model5, seed=seed, modified_fraction=fraction, genome_length=g,
                                                    length=200, spread=20, read_seed=read_seed + seed)
                 for n, seed, g in shapes]
        contigs = [p[2] for p in parts]
        samples.append(concat_batches([p[0] for p in parts]))
    names = ['chrA', 'chrB']
    return samples, contigs, names, SeedAligner(ReferenceSet.from_arrays(names, contigs))


class ContigFixture:
    def __init__(self, model):
        from nadavca_amd import synthetic
        from nadavca_amd.refset import ReferenceSet
        self.parts = []          # (ReadBatch, SyntheticBatchAligner, genome codes) per contig with reads
        for seed, g in zip(SEEDS, LENGTHS):
            kw = dict(length=400, spread=0) if g == 400 else {}
            self.parts.append(synthetic.make_read_batch(READS_PER_CONTIG, model, seed=seed, genome_length=g, **kw))
        tiny = np.random.default_rng(34).integers(0, 4, 9).astype(np.int32)
        self.contigs = [p[2] for p in self.parts] + [tiny, np.zeros(0, np.int32)]
        self.refset = ReferenceSet.from_arrays(NAMES, self.contigs)
        self.rb = concat_batches([p[0] for p in self.parts])
        self.contig = np.repeat(np.arange(3, dtype=np.int32), READS_PER_CONTIG)     # truth, per read
        self.local = [p[1].get_base_alignments(p[0]) for p in self.parts]           # truth pairs, contig-local
        self.read_base = np.arange(3) * READS_PER_CONTIG                            # first read of each part

    def local_alignments(self):
        """The truth as one BaseAlignmentBatch with ``contig``."""
        return concat_alignments(self.local, contig=range(3))

    def global_alignments(self):
        """The truth lifted to the concatenation's oriented coordinates (no ``contig``)."""
        off, G = self.refset.offsets, self.refset.total
        shift = [lambda r, rev, c=c: r + np.where(rev, G - off[c + 1], off[c]) for c in range(3)]
        return concat_alignments(self.local, shift=shift)
