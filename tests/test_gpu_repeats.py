"""``count_repeats_batch`` end to end on the simulated batch of tests/repeats_ref.py (one CAG locus, alleles of 10 and
25 copies, 40 reads each, both strands, every fifth read cut off inside the repeat): against the workflow in numpy,
the quality conditions, the windows ``repeat_items`` makes, and the batches that give empty tables."""
import numpy as np
import pytest

import repeats_ref as P
import signal_map_ref as R

pytestmark = pytest.mark.gpu

# What the CPU restatement gives on this batch (tests/test_repeats_cpu.py): the margins on the alleles' medians
MEDIAN_10, MEDIAN_25 = 10.0, 25.5
# ... and the share of the 64 windowed items whose count equals the whole-read call's there: 64 of 64
WINDOW_SHARE = 1.0


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.fixture(scope='module')
def model(km):
    return (km.k, km.central_position, km.alphabet_size, km.mean, km.sigma)


@pytest.fixture(scope='module')
def simulated(model):
    return P.simulated_batch(model)


@pytest.fixture(scope='module')
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp('hosts')
    return R.build_host(d), P.build_host(d)


@pytest.fixture(scope='module')
def counted(simulated, km):
    from nadavca_amd import count_repeats_batch
    return count_repeats_batch(simulated[0], simulated[1], kmer_model=km)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def assert_equals_restatement(got, ref):
    for name in got.FIELDS:
        a, b = getattr(got, name), ref[name]
        assert a.shape == b.shape, name
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), name


def test_count_repeats_batch_equals_its_stages_in_numpy(simulated, counted, hosts, model):
    rb, loci = simulated[0], simulated[1]
    assert_equals_restatement(counted, P.cpu_count_repeats(hosts[0], hosts[1], rb, loci, model))
    assert counted.n == rb.n and counted.c0.tolist() == [3]


def test_quality(simulated, counted):
    """The four conditions of the CPU test on the device's result: every uncut read REP_OK on its strand and nearer
    its own allele; the cut reads' worse flank below the median uncut read's; ``alleles()`` two classes whose medians
    lie within the restatement's own deviation (0 and 0.5) plus one copy of 10 and 25.  Measured on the restatement:
    counts 9-12 (median 10) and 23-28 (median 25.5)."""
    truth = simulated[2]
    q = P.quality(counted, truth)
    print({k: v for k, v in q.items() if k != 'cut_worse'}, np.sort(q['cut_worse']).round(2))
    assert q['spanning_uncut'] == 64 and q['wrong_strand'] == 0 and q['wrong_allele'] == 0
    assert (q['cut_worse'] < q['median_worse']).all()
    alleles = counted.alleles()[0]
    assert len(alleles) == 2
    assert abs(alleles[0][0] - 10) <= abs(MEDIAN_10 - 10) + 1 and abs(alleles[1][0] - 25) <= abs(MEDIAN_25 - 25) + 1


def test_min_flank_score_marks_the_cut_reads(simulated, counted, km):
    from nadavca_amd import count_repeats_batch
    truth = simulated[2]
    floor = P.quality(counted, truth)['median_worse']
    marked = count_repeats_batch(simulated[0], simulated[1], kmer_model=km, min_flank_score=floor)
    assert not marked.spanning[truth['cut']].any() and marked.spanning[~truth['cut']].sum() >= 32
    assert np.array_equal(marked.count, counted.count) and np.array_equal(bits(marked.score), bits(counted.score))


def test_windows_from_base_alignments(simulated, counted, hosts, model, km):
    """``items=repeat_items(...)`` from the constructed alignments of the batch: the result equals the numpy workflow
    on the same items, and the counts equal the whole-read call's on at least the share the restatement reaches,
    64 of 64."""
    from nadavca_amd import count_repeats_batch, repeat_items
    rb, loci, truth, specs, reference = simulated
    full, aligner = P.aligned_batch(rb, truth, specs, reference)
    items = repeat_items(full, aligner, loci)
    assert np.array_equal(items.read, np.nonzero(~truth['cut'])[0])
    got = count_repeats_batch(full, loci, kmer_model=km, items=items)
    assert_equals_restatement(got, P.cpu_count_repeats(hosts[0], hosts[1], rb, loci, model, items=items))
    assert got.spanning.all() and np.isnan(got.margin).all()
    same = got.count == counted.count[items.read]
    print('windowed counts equal to the whole-read counts: %d of %d' % (same.sum(), same.size))
    assert same.mean() >= WINDOW_SHARE


def test_empty_tables(simulated, km):
    from nadavca_amd import RepeatItems, count_repeats_batch
    from nadavca_amd.readbatch import ReadBatch
    rb, loci = simulated[0], simulated[1]
    none = np.zeros(0, np.int32)
    empty = ReadBatch.from_signals(np.zeros(0, np.int16), np.zeros(1, np.int64), none, np.zeros(1, np.int64))
    for res in (count_repeats_batch(empty, loci, kmer_model=km), count_repeats_batch(rb, [], kmer_model=km),
                count_repeats_batch(rb, loci, kmer_model=km, items=RepeatItems(*[np.zeros(0, np.int64)] * 5))):
        assert res.n == 0 and all(getattr(res, f).shape == (0,) for f in res.FIELDS)
        assert res.alleles() == [[] for _ in res.loci] and [t['reads'] for t in res.locus_table()] == [0] * len(res.loci)
    # reads without samples, and reads too short to hold events: every pair REP_NO_EVENTS, nothing spanning
    silent = ReadBatch.from_signals(np.zeros(0, np.int16), np.zeros(4, np.int64), none, np.zeros(4, np.int64))
    short = ReadBatch.from_signals(rb.raw_signal[:90], np.array([0, 40, 90]), none, np.zeros(3, np.int64))
    for batch in (silent, short):
        res = count_repeats_batch(batch, loci, kmer_model=km)
        assert res.n == batch.n and (res.status == P.REP_NO_EVENTS).all() and (res.count == -1).all()
        assert not res.spanning.any() and np.isnan(res.score).all() and np.isnan(res.margin).all()
        assert res.locus_table()[0]['reads'] == 0 and res.alleles() == [[]]
