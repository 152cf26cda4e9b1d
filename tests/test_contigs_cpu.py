"""Multi-contig references without a GPU: ``refset.ReferenceSet`` and its coordinates, the seed index that leaves out
k-mers across a join, the contig rule of ``SeedAligner`` (seedalign.py, step 1) restated in numpy, and
``readbatch.signal_alignments`` over a ReferenceSet against the per-contig calls."""
import numpy as np
import pytest

from contig_fixture import ContigFixture, NAMES, READS_PER_CONTIG
from test_seed_align_cpu import _batch


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


@pytest.fixture(scope='module')
def fx(model):
    return ContigFixture(model)


def test_reference_set_round_trip_and_locate(tmp_path):
    import torch
    from nadavca_amd.refset import ReferenceSet
    fa = tmp_path / 'three.fa'
    fa.write_text('>one first record\nACGTTG\nCA\n>empty\n>two\nGGA\n')
    rs = ReferenceSet.from_fasta(str(fa))
    assert rs.names == ['one first record', 'empty', 'two']
    assert rs.offsets.dtype == np.int64 and rs.offsets.tolist() == [0, 8, 8, 11]
    assert rs.codes.dtype == np.int32 and rs.codes.tolist() == [0, 1, 2, 3, 3, 2, 1, 0, 2, 2, 0]
    assert rs.n_contigs == 3 and rs.total == 11 and rs.contig_codes(2).tolist() == [2, 2, 0]
    again = ReferenceSet.from_arrays(rs.names, [rs.contig_codes(c) for c in range(3)])
    assert again.offsets.tolist() == rs.offsets.tolist() and np.array_equal(again.codes, rs.codes)
    # every position, the boundaries among them: the zero-length contig owns none
    x = np.arange(11)
    c, local = rs.locate(x)
    assert c.tolist() == [0] * 8 + [2] * 3 and local.tolist() == list(range(8)) + [0, 1, 2]
    ct, lt = rs.locate(torch.from_numpy(x))
    assert ct.tolist() == c.tolist() and lt.tolist() == local.tolist()
    # end positions map through x - 1: the end 8 belongs to contig 0 (local end 8), the end 11 to contig 2
    ends = np.array([1, 8, 9, 11])
    c, local = rs.locate(ends - 1)
    assert c.tolist() == [0, 0, 2, 2] and (local + 1).tolist() == [1, 8, 1, 3]
    assert [int(v) for v in rs.locate_range(8, 11)] == [2, 0, 3]
    c, local = rs.locate(np.int64(7))
    assert (int(c), int(local)) == (0, 7)


def test_reference_set_refuses_duplicates_and_too_many_bases():
    from nadavca_amd.refset import ReferenceSet
    with pytest.raises(ValueError, match='duplicate'):
        ReferenceSet.from_arrays(['a', 'b', 'a'], [[0, 1], [2], [3]])
    # the limit is checked on the offsets alone: nothing of that size is allocated
    with pytest.raises(ValueError, match='2\\^30'):
        ReferenceSet(['a', 'b'], [0, 1 << 29, (1 << 30) + 1], np.zeros(0, np.int32))
    ReferenceSet(['a'], [0, 3], [0, 1, 2])
    for bad in ([0, 3, 2], [1, 3, 4], [0, 3]):
        with pytest.raises(ValueError):
            ReferenceSet(['a', 'b'], bad, [0, 1, 2, 3])
    with pytest.raises(ValueError):
        ReferenceSet(['a'], [0, 3], [0, 1])


def test_index_leaves_out_kmers_across_a_join(fx):
    from nadavca_amd.seedalign import SeedAligner
    a, b = fx.contigs[0], fx.contigs[1]
    rb = _batch([np.concatenate([a[-20:], b[:20]])])
    strand, diag, votes = SeedAligner(fx.refset.codes, device='cpu', k=14).seed(rb)
    assert (int(strand[0]), int(diag[0]), int(votes[0])) == (0, 9980, 27)
    strand, diag, votes = SeedAligner(fx.refset, device='cpu', k=14).seed(rb)
    assert (int(strand[0]), int(diag[0]), int(votes[0])) == (0, 9980, 14)   # the 13 k-mers across the join are gone
    # the same on the other strand
    rc = _batch([3 - np.concatenate([a[-20:], b[:20]])[::-1]])
    G = fx.refset.total
    strand, diag, votes = SeedAligner(fx.refset, device='cpu', k=14).seed(rc)
    assert (int(strand[0]), int(diag[0]), int(votes[0])) == (1, G - 10020, 14)
    # contigs shorter than k index nothing, though their concatenation is longer than k
    tiny = SeedAligner(type(fx.refset).from_arrays(['t', 'e', 'u'], [fx.contigs[3], fx.contigs[4], fx.contigs[3]]),
                       device='cpu', k=10)
    assert all(keys.numel() == 0 for keys, _ in tiny._index)
    assert all(keys.numel() == 9 for keys, _ in SeedAligner(tiny.reference_num, device='cpu', k=10)._index)


def numpy_contig_rule(refset, seq_off, strand, diag):
    """The contig rule of seedalign.py's step 1, plain numpy: -> (contig, lo, hi) per read."""
    off, G = refset.offsets, refset.total
    out = []
    for j in range(len(strand)):
        if strand[j] < 0:
            out.append((-1, 0, G))
            continue
        m = int(seq_off[j + 1] - seq_off[j])
        x = min(max(int(diag[j]) + (m - 1) // 2, 0), G - 1)
        ranges = [(G - off[c + 1], G - off[c]) if strand[j] == 1 else (off[c], off[c + 1])
                  for c in range(refset.n_contigs)]
        hit = [c for c, (lo, hi) in enumerate(ranges) if lo <= x < hi]
        assert len(hit) == 1
        out.append((hit[0], int(ranges[hit[0]][0]), int(ranges[hit[0]][1])))
    return np.array(out)


def test_contig_rule_finds_every_reads_contig(fx):
    from nadavca_amd.seedalign import SeedAligner
    al = SeedAligner(fx.refset, device='cpu')
    strand, diag, votes = al.seed(fx.rb)
    contig, lo, hi = (t.numpy() for t in al.contig_of(fx.rb, strand, diag))
    strand, diag = strand.numpy(), diag.numpy()
    assert (strand >= 0).all() and (strand == 1).sum() == 72
    assert contig.dtype == np.int32 and np.array_equal(contig, fx.contig)
    exp = numpy_contig_rule(fx.refset, fx.rb.seq_off, strand, diag)
    assert np.array_equal(np.stack([contig, lo, hi], 1), exp)
    # both strands occur in every contig
    for c in range(3):
        assert set(strand[fx.contig == c].tolist()) == {0, 1}
    # a read without a strand has no contig
    rb = _batch([np.zeros(5, np.int32), fx.contigs[1][100:160]])
    strand, diag, _ = al.seed(rb)
    contig, lo, hi = (t.numpy() for t in al.contig_of(rb, strand, diag))
    assert contig.tolist() == [-1, 1] and (lo[0], hi[0]) == (0, fx.refset.total)
    assert (lo[1], hi[1]) == (fx.refset.offsets[1], fx.refset.offsets[2])


SA_EQUAL = ('anchors', 'win_len', 'slice_start', 'reverse', 'read_seq_start', 'read_seq_end', 'reference',
            'context_before', 'context_after')
SA_OFFSETS = ('anc_off', 'ref_off', 'cb_off', 'ca_off')


def test_signal_alignments_over_a_reference_set_equal_the_per_contig_calls(fx, model):
    from nadavca_amd.readbatch import contig_local_range, signal_alignments
    k, central = model[0], model[1]
    multi_t = signal_alignments(fx.rb, fx.local_alignments(), 30, fx.refset, k, central)
    multi = multi_t.host()
    each = [signal_alignments(rb, ba, 30, genome, k, central).host()
            for (rb, _, genome), ba in zip(fx.parts, fx.local)]
    cat = lambda f: np.concatenate([getattr(e, f) for e in each])
    for f in SA_EQUAL:
        assert np.array_equal(getattr(multi, f), cat(f)), f
    for f in SA_OFFSETS:
        assert np.array_equal(np.diff(getattr(multi, f)), np.concatenate([np.diff(getattr(e, f)) for e in each])), f
    assert np.array_equal(multi.live, np.concatenate([e.live + b for e, b in zip(each, fx.read_base)]))
    sig_base = fx.rb.sig_off[fx.read_base]
    assert np.array_equal(multi.win_start, np.concatenate([e.win_start + b for e, b in zip(each, sig_base)]))
    assert multi.contig.dtype == np.int32 and np.array_equal(multi.contig, fx.contig[multi.live])
    assert multi.live.size == fx.rb.n and multi.reverse.any() and not multi.reverse.all()
    # the global ranges, located, are the per-contig ranges
    c, start = fx.refset.locate(multi.ref_start)
    c_end, end = fx.refset.locate(multi.ref_end - 1)
    assert np.array_equal(c, multi.contig) and np.array_equal(c_end, multi.contig)
    assert np.array_equal(start, cat('ref_start')) and np.array_equal(end + 1, cat('ref_end'))
    ls, le = contig_local_range(multi_t, fx.refset)
    assert np.array_equal(ls.numpy(), cat('ref_start')) and np.array_equal(le.numpy(), cat('ref_end'))
    # the 400-base contig's reads reach both of its joins: their pairs cover it end to end, their anchors (the
    # simulation trims 3 bases and thins the rest) start and end within a few bases of them
    flush = multi.contig == 2
    assert all(b.ref_idx[b.off[:-1]].max() == 0 and b.ref_idx[b.off[1:] - 1].min() == 399 for b in fx.local[2:])
    assert (multi.ref_start[flush] <= fx.refset.offsets[2] + 12).all()
    assert (multi.ref_end[flush] >= fx.refset.offsets[3] - 12).all()
    # the truth lifted to global coordinates, without contigs, gives the same stage
    lifted = signal_alignments(fx.rb, fx.global_alignments(), 30, fx.refset, k, central).host()
    for f in type(multi).FIELDS:
        assert np.array_equal(getattr(lifted, f), getattr(multi, f)), f


def test_signal_alignments_refuse_contigs_they_cannot_place(fx, model):
    from nadavca_amd.readbatch import BaseAlignmentBatch, signal_alignments
    k, central = model[0], model[1]
    ba = fx.local_alignments()
    with pytest.raises(ValueError, match='ReferenceSet'):
        signal_alignments(fx.rb, ba, 30, fx.refset.codes, k, central)
    for wrong in (-1, len(NAMES)):
        contig = ba.contig.copy()
        contig[5] = wrong
        with pytest.raises(ValueError, match='contig'):
            signal_alignments(fx.rb, BaseAlignmentBatch(ba.read_idx, ba.ref_idx, ba.off, ba.reverse, contig),
                              30, fx.refset, k, central)
    # a read without pairs may carry any index (SeedHits gives -1 to an unaligned read)
    keep = np.arange(ba.read_idx.size) >= ba.off[1]      # read 0 loses its pairs
    off = np.concatenate([[0], np.cumsum(np.where(np.arange(fx.rb.n) == 0, 0, np.diff(ba.off)))])
    contig = ba.contig.copy()
    contig[0] = -1
    cut = BaseAlignmentBatch(ba.read_idx[keep], ba.ref_idx[keep], off, ba.reverse, contig)
    assert signal_alignments(fx.rb, cut, 30, fx.refset, k, central).live.tolist() == list(range(1, fx.rb.n))
    # pairs that leave their contig (a read of contig 0 said to lie in the 400-base one)
    contig = ba.contig.copy()
    contig[1] = 2
    with pytest.raises(ValueError, match='outside its contig'):
        signal_alignments(fx.rb, BaseAlignmentBatch(ba.read_idx, ba.ref_idx, ba.off, ba.reverse, contig), 30,
                          fx.refset, k, central)
    with pytest.raises(ValueError):
        BaseAlignmentBatch(ba.read_idx, ba.ref_idx, ba.off, ba.reverse, ba.contig[:-1])


def test_one_contig_behaves_as_the_plain_array(fx, model):
    from nadavca_amd.readbatch import BaseAlignmentBatch, signal_alignments
    from nadavca_amd.refset import ReferenceSet
    from nadavca_amd.seedalign import SeedAligner
    rb, syn, genome = fx.parts[1]
    one = ReferenceSet.from_arrays(['only'], [genome])
    plain, single = SeedAligner(genome, device='cpu'), SeedAligner(one, device='cpu')
    assert plain.reference_set is None and single.reference_set is one
    assert np.array_equal(plain.reference_num, single.reference_num)
    for a, b in zip(plain.seed(rb), single.seed(rb)):
        assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy())
    strand, diag, _ = single.seed(rb)
    contig, lo, hi = single.contig_of(rb, strand, diag)
    assert (contig == 0).all() and (lo == 0).all() and (hi == genome.size).all()
    k, central = model[0], model[1]
    ba = syn.get_base_alignments(rb)
    with_contig = BaseAlignmentBatch(ba.read_idx, ba.ref_idx, ba.off, ba.reverse, np.zeros(rb.n, np.int32))
    a = signal_alignments(rb, ba, 30, genome, k, central).host()
    b = signal_alignments(rb, with_contig, 30, one, k, central).host()
    for f in type(a).FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert ba.contig is None and (a.contig == 0).all()


def test_seed_hits_carry_contigs_only_from_a_reference_set():
    from nadavca_amd.refset import ReferenceSet
    from nadavca_amd.seedalign import SeedHits
    z = np.zeros(2, np.int64)
    args = (np.array([0, -1], np.int32), z, z, np.array([40, 0], np.int32), np.zeros((2, 2), np.int32),
            np.array([True, False]), np.array([0, 1, 1]), np.array([3], np.int32), np.array([7]))
    hits = SeedHits(*args)
    assert hits.contig.tolist() == [0, -1] and hits.base_alignments().contig is None
    rs = ReferenceSet.from_arrays(['a', 'b'], [[0, 1], [2, 3]])
    hits = SeedHits(*args, contig=np.array([1, -1], np.int32), reference_set=rs)
    assert hits.base_alignments().contig.tolist() == [1, -1]


def test_a_fasta_of_several_records_goes_in_as_a_reference_set(tmp_path, fx):
    from nadavca_amd.refset import ReferenceSet
    from nadavca_amd.seedalign import SeedAligner
    letters = np.array(list('ACGT'))
    fa = tmp_path / 'contigs.fa'
    fa.write_text(''.join('>%s\n%s\n' % (name, ''.join(letters[codes])) for name, codes in zip(NAMES, fx.contigs)))
    rs = ReferenceSet.from_fasta(fa)
    assert rs.names == NAMES and np.array_equal(rs.offsets, fx.refset.offsets) and np.array_equal(rs.codes,
                                                                                                    fx.refset.codes)
    al = SeedAligner(rs, device='cpu')
    strand, diag, _ = al.seed(fx.rb)
    assert np.array_equal(al.contig_of(fx.rb, strand, diag)[0].numpy(), fx.contig)
    with pytest.raises(ValueError, match='from_fasta'):      # the path itself stands for one record
        SeedAligner(str(fa), device='cpu')
