"""The repeat counter without a GPU: the CPU restatement of nvk_repeat_count_dev (tests/host_shims/repeats_host.cpp,
which carries loops, first event and marks in the cell as the kernel does) against a plain Python DP that traces back;
a hand-made path; ``repeat_chain`` and ``RepeatLocus``; the workflow in numpy on the simulated batch; ``repeat_items``
on constructed alignments; the allele split."""
import numpy as np
import pytest

import repeats_ref as P
import signal_map_ref as R


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return P.build_host(tmp_path_factory.mktemp('repeats_host'))


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


@pytest.fixture(scope='module')
def simulated(host, model, tmp_path_factory):
    """-> (ReadBatch, loci, truth, specs, reference, the numpy workflow's result)"""
    sim = P.simulated_batch(model)
    map_host = R.build_host(tmp_path_factory.mktemp('map_host'))
    return sim + (P.cpu_count_repeats(map_host, host, sim[0], sim[1], model), map_host)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.fixture(scope='module')
def traced(host):
    """per constructed case: (name, case, the shim's (hit, score), the traceback DP's (hit, score, ties))"""
    return [(name, case, P.run_host(host, case), P.python_case(case)) for name, case in P.kernel_cases()]


def test_carrying_equals_tracing(traced):
    """Every i32 equal and every f64 bit for bit, on every item of the constructed cases"""
    for name, case, (hit, score), (want_hit, want_score, _) in traced:
        bad = np.nonzero((hit != want_hit).any(1) | (bits(score) != bits(want_score)).any(1))[0]
        assert bad.size == 0, (name, bad[:5].tolist(), hit[bad[:2]].tolist(), want_hit[bad[:2]].tolist())


def test_cases_cover_what_they_claim(traced):
    name, case, (hit, score), _ = traced[0]
    N = np.diff(case['st_off'])
    assert sorted(set(N.tolist())) == P.KERNEL_STATES
    par = case['chain_par']
    assert set((par[:, 0] - par[:, 1] + 1).tolist()) == set(P.KERNEL_UNITS)
    E, chain = case['items'][:, 2] - case['items'][:, 1], case['items'][:, 0]
    for n in P.KERNEL_STATES:
        assert {0, 1, (n - 1) // 2, 64, 65} <= set(E[N[chain] == n].tolist()), n
    assert (E == 300).sum() >= 2
    # status_in, no events, no path; a finite result in every instantiation, with and without trips round the loop
    assert hit[5].tolist() == [7, int(E[5]), -1, -1, -1, -1, -1, 0] and np.isneginf(score[5]).all()
    assert (hit[E == 0, 0] == P.REP_NO_EVENTS).all() and (hit[E == 0, 2:7] == -1).all()
    short = (E > 0) & (E < 1 + N[chain] // 2) & (case['status_in'] == 0)
    assert short.any() and (hit[short, 0] == P.REP_NO_PATH).all() and np.isneginf(score[short]).all()
    ok = hit[:, 0] == P.REP_OK
    for lo, hi in ((3, 64), (65, 128), (129, 256)):
        here = ok & (N[chain] >= lo) & (N[chain] <= hi)
        assert (hit[here, 4] > 0).any() and (hit[here, 4] == 0).any(), (lo, hi)
    assert np.isfinite(score[ok]).all() and (hit[ok, 5] >= 0).all() and (hit[ok, 6] >= hit[ok, 5]).all()
    # two windows of one read's events
    a, b, c = case['items'][-3:]
    assert a[0] == b[0] == c[0] and (b[1], b[2]) == (a[1] + 3, a[2]) and (c[1], c[2]) == (a[1], a[2] - 5)


def test_grid_cases_do_tie(traced):
    """Each pair of candidates that are adjacent in the order open, step, loop, stay, skip ties for the largest
    somewhere in the grid case (open and step never meet: state 0 has no step)"""
    name, case, _, (_, _, ties) = traced[1]
    assert name == 'grid'
    for pair in P.TIE_PAIRS:
        assert ties[pair] > 0, (pair, ties)


def test_hand_made_path(host):
    case, (first, last, loops, i1, i2) = P.hand_case()
    hit, score = P.run_host(host, case)
    assert loops == 4
    assert hit[0].tolist() == [P.REP_OK, case['level'].size, first, last, loops, i1, i2, 0]
    want_hit, want_score, _ = P.python_case(case)
    assert np.array_equal(hit, want_hit) and np.array_equal(bits(score), bits(want_score))
    # the end value pays the trim on both sides
    assert score[0, 0] == score[0, 1] + float(P.HAND_TAIL) * case['trim']


# ---- repeat_chain ------------------------------------------------------------------------------------------------
def test_repeat_chain(model):
    from nadavca_amd.repeats import RepeatLocus, repeat_chain
    km = P.TableModel(model)
    rng = np.random.default_rng(3)
    for unit, c0_want in (('CA', 4), ('CAG', 3), ('CAGGTT', 2), ('CAGGTTA', 2)):
        left, right = rng.integers(0, 4, 30), rng.integers(0, 4, 25)
        locus = RepeatLocus('x', left, unit, right)
        ids, lp_from, lp_to, m1, m2, c0 = repeat_chain(locus, km)
        u, k = len(unit), 6
        assert c0 == c0_want and (lp_from, lp_to, m1, m2) == (30 + u - 1, 30, 30, 30 + c0 * u - k + 1)
        T = np.concatenate([left, np.tile(locus.unit, c0), right])
        assert ids.size == T.size - k + 1 and 0 <= lp_to < lp_from < m2 <= ids.size - 1
        for j in (0, lp_to, m2, ids.size - 1):
            assert ids[j] == sum(int(T[j + t]) * 4 ** (k - 1 - t) for t in range(k))
        # the back edge lands where a step would: the states that lie inside the repeat recur one unit on
        assert m2 - u >= lp_from + 1 - u + 1 and np.array_equal(ids[lp_to:m2 - u], ids[lp_to + u:m2])
        assert ids[lp_from + 1] == ids[lp_to] and ids[m2] != ids[m2 - u]
        assert len(set(ids[lp_to:lp_from + 1].tolist())) == u
        # the reverse chain is the chain of the reverse complement
        rc = RepeatLocus('rc', 3 - right[::-1], 3 - locus.unit[::-1], 3 - left[::-1])
        for got, want in zip(repeat_chain(locus, km, reverse=True), repeat_chain(rc, km)):
            assert np.array_equal(got, want)
        assert repeat_chain(locus, km, reverse=True)[2] == 25


def test_refusals(model):
    from nadavca_amd.repeats import RepeatLocus, repeat_chain
    km = P.TableModel(model)
    flank = 'ACGTACGTAC'
    for unit in ('A', '', 'CACA', 'GG', 'CAGCAG'):
        with pytest.raises(ValueError):
            RepeatLocus('x', flank, unit, flank)
    with pytest.raises(ValueError):
        RepeatLocus('x', 'ACGN', 'CA', flank)
    for left, right in (('ACGTA', flank), (flank, 'ACGTA')):
        with pytest.raises(ValueError, match='at least k'):
            repeat_chain(RepeatLocus('x', left, 'CAG', right), km)
    with pytest.raises(ValueError, match='256'):
        repeat_chain(RepeatLocus('x', 'ACGT' * 32, 'CAG', 'ACGT' * 32), km)
    assert repeat_chain(RepeatLocus('x', 'ACGT' * 31, 'CAG', 'ACGT' * 31 + 'A'), km)[0].size == 253
    five = P.TableModel((6, 2, 5, np.zeros(5 ** 6), np.ones(5 ** 6)))
    with pytest.raises(ValueError, match='letters'):
        repeat_chain(RepeatLocus('x', flank, 'CAG', flank), five)
    # from_reference: the range must be whole copies of the unit, the flanks inside the sequence
    ref = np.concatenate([np.zeros(40), np.tile([1, 0, 2], 10), np.ones(40)]).astype(np.int32)
    locus = RepeatLocus.from_reference(ref, 40, 70, 'CAG', flank=30)
    assert (locus.start, locus.end, locus.contig, locus.ref_length) == (40, 70, 0, 110)
    assert locus.left.size == 30 and np.array_equal(locus.right, np.ones(30))
    for start, end, unit, fl in ((40, 71, 'CAG', 30), (41, 71, 'CAG', 30), (40, 70, 'CAT', 30), (40, 70, 'CAG', 41),
                                 (70, 40, 'CAG', 30)):
        with pytest.raises(ValueError):
            RepeatLocus.from_reference(ref, start, end, unit, flank=fl)
    from nadavca_amd.refset import ReferenceSet
    rs = ReferenceSet.from_arrays(['a', 'b'], [np.zeros(50, np.int32), ref])
    assert np.array_equal(RepeatLocus.from_reference(rs, 40, 70, 'CAG', contig=1).left, locus.left)
    with pytest.raises(ValueError):
        RepeatLocus.from_reference(rs, 40, 70, 'CAG', contig=0)


# ---- the workflow in numpy ----------------------------------------------------------------------------------------
# What the restatement gives on the simulated batch (seed 5, the first tried): its own deviations are the margins below
MEDIAN_10, MEDIAN_25 = 10.0, 25.5


def test_workflow_quality(simulated):
    """One CAG locus, flanks of 30, alleles of 10 and 25 copies, 40 reads each, both strands, every fifth read cut off
    inside the repeat (seed 5, the first tried).  The restatement: all 64 uncut reads are REP_OK on the right strand
    (the other strand at least 356 nats behind); counts for n = 10: median 10, range 9-12; for n = 25: median 25.5,
    range 23-28; every count nearer its own allele; the worse flank of the cut reads scores -8.35 .. -3.14 per event,
    that of the uncut reads -3.02 at worst, median -1.73; ``alleles()`` gives (10.0, 25.5) with or without the cut
    reads.  The medians may deviate by what they do here plus one copy: 1 and 1.5."""
    rb, loci, truth, _, _, res, _ = simulated
    q = P.quality(res, truth)
    print({k: v for k, v in q.items() if k != 'cut_worse'}, np.sort(q['cut_worse']).round(2))
    assert (res['status'] == P.REP_OK).all() and truth['cut'].sum() == 16
    assert q['spanning_uncut'] == 64 and q['wrong_strand'] == 0 and q['wrong_allele'] == 0
    assert (q['cut_worse'] < q['median_worse']).all()
    assert q[10][0] == MEDIAN_10 and q[25][0] == MEDIAN_25


def test_library_stage_six_equals_the_restatement(simulated):
    """``pair_results`` (numpy, what count_repeats_batch ends with) on the shim's outputs: every field of the per-pair
    loop of the restatement, the scores bit for bit; ``alleles``, ``locus_table``, ``write_tsv``"""
    from nadavca_amd.repeats import pair_results
    rb, loci, truth, _, _, res, _ = simulated
    n = rb.n
    for flank in (None, float(np.median(np.fmin(res['left_score'], res['right_score'])[~truth['cut']]))):
        got = pair_results(loci, res['c0'], np.arange(n), np.zeros(n, np.int64), None, res['hit'], res['path_score'],
                           res['case']['items'][:, 1], simulated_ev_start(simulated), res['case']['trim'], flank)
        for name in got.FIELDS:
            a, b = getattr(got, name), res[name]
            if name == 'spanning' and flank is not None:
                continue
            same = np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
            assert same, name
    # with the median uncut read's worse flank as the floor, no cut read is spanning
    assert not got.spanning[truth['cut']].any() and got.spanning[~truth['cut']].sum() >= 32
    alleles = got.alleles()[0]
    assert len(alleles) == 2 and abs(alleles[0][0] - 10) <= abs(MEDIAN_10 - 10) + 1 \
        and abs(alleles[1][0] - 25) <= abs(MEDIAN_25 - 25) + 1
    assert alleles[0][1] + alleles[1][1] == int(got.spanning.sum())
    table = got.locus_table()[0]
    assert table['name'] == 'CAG' and table['reads'] == n and table['spanning'] == int(got.spanning.sum())
    assert sum(table['histogram'].values()) == table['spanning']
    assert len(got.alleles(max_alleles=1)[0]) == 1
    with pytest.raises(ValueError):
        got.alleles(max_alleles=3)


def simulated_ev_start(simulated):
    import decode_ref as D
    from nadavca_amd import synthetic
    rb, map_host = simulated[0], simulated[6]
    return D.cpu_events(map_host, rb.raw_signal, rb.sig_off, synthetic.load_model_arrays())[2]


def test_write_tsv(simulated, tmp_path):
    from nadavca_amd.repeats import pair_results
    rb, loci, truth, _, _, res, _ = simulated
    got = pair_results(loci, res['c0'], np.arange(rb.n), np.zeros(rb.n, np.int64), None, res['hit'], res['path_score'],
                       res['case']['items'][:, 1], simulated_ev_start(simulated), res['case']['trim'], None)
    path = tmp_path / 'counts.tsv'
    assert got.write_tsv(str(path)) == rb.n
    lines = path.read_text().splitlines()
    assert len(lines) == rb.n + 1 and lines[0].split('\t')[:5] == ['read', 'locus', 'strand', 'status', 'count']
    first = lines[1].split('\t')
    assert first[:3] == ['read_0', 'CAG', '+'] and int(first[4]) == got.count[0]


def test_split_counts():
    from nadavca_amd.repeats import split_counts
    assert split_counts([]) == []
    assert split_counts([7, 7, 7]) == [(7.0, 3)]
    assert split_counts([10, 11, 10, 12, 11]) == [(11.0, 5)]            # no cut gains a factor 8
    assert split_counts([10, 25, 11, 26, 10, 24, 9]) == [(10.0, 4), (25.0, 3)]
    assert split_counts([10, 25, 11, 26, 10, 24, 9], min_gain=float('inf')) == [(11.0, 7)]
    assert split_counts([3, 40]) == [(3.0, 1), (40.0, 1)]


def test_nothing_to_count_needs_no_device(simulated, model):
    """An empty batch, no loci, no items and reads without samples return before the first device call"""
    from nadavca_amd import RepeatItems, count_repeats_batch
    from nadavca_amd.readbatch import ReadBatch
    rb, loci, km = simulated[0], simulated[1], P.TableModel(model)
    none = np.zeros(0, np.int32)
    empty = ReadBatch.from_signals(np.zeros(0, np.int16), np.zeros(1, np.int64), none, np.zeros(1, np.int64))
    for res in (count_repeats_batch(empty, loci, kmer_model=km), count_repeats_batch(rb, [], kmer_model=km),
                count_repeats_batch(rb, loci, kmer_model=km, items=RepeatItems(*[np.zeros(0, np.int64)] * 5))):
        assert res.n == 0 and all(getattr(res, f).shape == (0,) for f in res.FIELDS)
    silent = ReadBatch.from_signals(np.zeros(0, np.int16), np.zeros(4, np.int64), none, np.zeros(4, np.int64))
    res = count_repeats_batch(silent, loci, kmer_model=km)
    assert res.n == 3 and (res.status == P.REP_NO_EVENTS).all() and (res.count == -1).all() and not res.spanning.any()
    assert np.isnan(res.margin).all() and res.alleles() == [[]]
    for bad in (dict(min_events=0), dict(trim_cost=0.5), dict(p_stay=1.0),
                dict(items=RepeatItems([rb.n], [0], [False], [0], [10])),
                dict(items=RepeatItems([0], [0], [False], [0], [10 ** 9]))):
        with pytest.raises(ValueError):
            count_repeats_batch(rb, loci, kmer_model=km, **bad)


# ---- repeat_items -------------------------------------------------------------------------------------------------
def constructed_alignments():
    """Five reads of 3 000 samples against two contigs (400 and 500 bases); the locus is [200, 230) of contig 1 with
    flanks of 30.  Rows: every fifth base, at sample 10 b.  0: forward over 100..400; 1: reverse over 100..400; 2:
    forward over 100..250 (ends inside the right flank); 3: as 0 without rows before base 100; 4: as 0 on contig 0."""
    from nadavca_amd.readbatch import BaseAlignmentBatch, ReadBatch, SyntheticBatchAligner
    from nadavca_amd.refset import ReferenceSet
    from nadavca_amd.repeats import RepeatLocus
    rng = np.random.default_rng(9)
    c1 = rng.integers(0, 4, 500).astype(np.int32)
    c1[200:230] = np.tile([1, 0, 2], 10)
    rs = ReferenceSet.from_arrays(['c0', 'c1'], [rng.integers(0, 4, 400).astype(np.int32), c1])
    locus = RepeatLocus.from_reference(rs, 200, 230, 'CAG', flank=30, contig=1)
    lengths = [300, 300, 150, 300, 300]
    read_idx = [np.arange(L) for L in lengths]
    ref_idx = [100 + np.arange(300), 500 - 1 - (399 - np.arange(300)), 100 + np.arange(150), 100 + np.arange(300),
               100 + np.arange(300)]
    rows = [np.arange(0, L, 5) for L in lengths]
    rows[3] = rows[3][rows[3] >= 100]
    off = lambda xs: P.offsets([len(x) for x in xs])
    rb = ReadBatch(np.zeros(15000, np.int16), P.offsets([3000] * 5), np.zeros(sum(lengths), np.int32), off(read_idx),
                   np.concatenate(rows), 10 * np.concatenate(rows), off(rows))
    ba = BaseAlignmentBatch(np.concatenate(read_idx), np.concatenate(ref_idx), off(read_idx),
                            [False, True, False, False, False], contig=[1, 1, 1, 1, 0])
    return rb, SyntheticBatchAligner(rs.codes, ba), locus


def test_repeat_items_on_constructed_alignments():
    from nadavca_amd.repeats import RepeatLocus, repeat_items
    rb, aligner, locus = constructed_alignments()
    it = repeat_items(rb, aligner, [locus], pad=50)
    assert it.read.tolist() == [0, 1] and it.locus.tolist() == [0, 0] and it.reverse.tolist() == [False, True]
    # 0: the anchors at bases 70 (position 170) and 160 (260); 1: at bases 230 (position 169) and 135 (264)
    assert it.sig_lo.tolist() == [650, 1300] and it.sig_hi.tolist() == [1650, 2350]
    wide = repeat_items(rb, aligner, [locus], pad=1000)
    assert wide.sig_lo.tolist() == [0, 350] and wide.sig_hi.tolist() == [2600, 3000]
    # a second locus on the other contig: read 4 alone spans it
    other = RepeatLocus('other', locus.left, 'CAG', locus.right, start=200, end=230, contig=0, ref_length=400)
    both = repeat_items(rb, aligner, [locus, other])
    assert both.read.tolist() == [0, 1, 4] and both.locus.tolist() == [0, 0, 1]
    with pytest.raises(ValueError, match='from_reference'):
        repeat_items(rb, aligner, [RepeatLocus('bare', locus.left, 'CAG', locus.right)])


def test_items_on_the_simulated_batch(simulated, host, model):
    """``repeat_items`` from the constructed alignments of the simulated batch keeps the 64 uncut reads, each on its
    strand; counted in those windows, 64 of 64 have the whole-read count (the share the GPU test holds the device to)"""
    from nadavca_amd.repeats import repeat_items
    rb, loci, truth, specs, reference, res, map_host = simulated
    full, aligner = P.aligned_batch(rb, truth, specs, reference)
    it = repeat_items(full, aligner, loci)
    assert np.array_equal(it.read, np.nonzero(~truth['cut'])[0]) and np.array_equal(it.reverse, truth['reverse'][it.read])
    assert (it.sig_lo > 0).all() and (it.sig_hi < np.diff(rb.sig_off)[it.read]).all()
    win = P.cpu_count_repeats(map_host, host, rb, loci, model, items=it)
    assert (win['status'] == P.REP_OK).all() and np.isnan(win['margin']).all()
    assert np.array_equal(win['strand'], truth['reverse'][it.read].astype(int))
    assert (win['n_events'] < res['n_events'][it.read]).all()
    assert np.array_equal(win['count'], res['count'][it.read])
