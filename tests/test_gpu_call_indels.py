"""``call_indels_batch`` on the GPU.  A 1 500-base genome gets six planted one-base edits (three deletions, three
insertions, two of them inside homopolymer runs, where left-alignment decides the site's position); 150 reads of about
200 bases are simulated from the MUTATED genome on both strands and aligned to the ORIGINAL with ``SeedAligner``, with
the packaged 6-mer table.

Parity through the pipeline: for every planted site, every read row that scored it is recomputed with the CPU oracle
on the read's own window (signal, reference part, contexts and anchors copied from the alignment stage to the host;
``to_read_frame`` and ``apply_edit`` make the edited part; the expectation is the oracle's no-substitution total on it
minus that on the part itself), with the tolerance of tests/test_gpu_hypotheses.py, 1e-9 relative + 1e-9 absolute.  A
row is compared when the operator's mapped band is the band the oracle computes for the edited part (always, unless a
deleted base carries an anchor that shaped the band; such rows are counted and must be few).  The workflow runs with
bandwidth 40 instead of the packaged 150, which keeps the oracle's share of this test to a few seconds.

Every planted site must be in the table at its left-aligned position with at least 8 reads and a positive summed
ratio.  Whether it is also the best candidate nearby, and how many unplanted sites sum above the weakest planted one,
is printed, not asserted.

The deleted base in a run sits in ``AGGGT``.  The first version of this test deleted one of five A's (``CAAAAAG``):
its rows agreed with the oracle and summed to -29.7 nats over 20 reads.  That is the model, not the kernel: on the CPU
oracle alone (8 simulated reads per design, packaged table) a deletion from a run of 4 or 5 equal bases sums to -7.6 ..
-18.8 nats with 0 or 1 reads above 0 — the k-mers of such a run are nearly the same level and the longer reference has
more paths — while one from a run of 3 sums to +10 .. +56.  So the site was moved to a run of 3, as the k-mer table
allows; an insertion into a run of 4 (``TCCCCA``, here) sums to +25 with 8 of 8 above 0 and stayed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-9
GENOME, N_READS, SEED = 1500, 150, 11


def _left_aligned(genome, x, d, letter):
    while x > 0 and (genome[x - 1] == genome[x + d - 1] if d else genome[x - 1] == letter):
        x -= 1
    return x


def _setup():
    from nadavca_amd import synthetic
    rng = np.random.default_rng(SEED)
    genome = rng.integers(0, 4, GENOME).astype(np.int32)
    # two homopolymer runs with other letters on both sides
    genome[399:404] = [0, 2, 2, 2, 3]
    genome[999:1005] = [3, 1, 1, 1, 1, 0]
    other = lambda x: int((genome[x - 1] + 1 + (genome[x] == (genome[x - 1] + 1) % 4)) % 4)   # neither neighbour
    planted = [(200, 1, -1), (401, 1, -1), (650, 1, -1), (850, 0, other(850)), (1002, 0, 1), (1250, 0, other(1250))]
    mutated = synthetic.apply_edits(genome, [(x, d, [s] if s >= 0 else []) for x, d, s in planted])
    assert mutated.size == GENOME
    sites = [(_left_aligned(genome, x, d, s), d, s) for x, d, s in planted]
    assert sites[1][0] == 400 and sites[4][0] == 1000 and len(set(sites)) == 6
    model = synthetic.load_model_arrays()
    rb, _, _ = synthetic.make_error_read_batch(N_READS, mutated, seed=SEED, length=200, spread=20, model=model)
    return genome, sites, rb, model


@pytest.fixture(scope='module')
def world():
    from nadavca_amd import call_indels_batch, defaults, dtw, synthetic, SeedAligner
    from nadavca_amd.batchflow import load_config
    genome, sites, rb, model = _setup()
    km = dtw.KmerModel(*model)
    config = dict(load_config(defaults.CONFIG_FILE), bandwidth=40)
    aligner = SeedAligner(genome)
    ib = call_indels_batch(rb, aligner, km, config=config, keep_rows='all')
    return dict(genome=genome, sites=sites, rb=rb, model=model, km=km, config=config, aligner=aligner, ib=ib)


def _find(ib, contig, x, d, s):
    hit = np.nonzero((ib.contig == contig) & (ib.position == x) & (ib.del_len == d) & (ib.ins_letter == s))[0]
    assert hit.size <= 1
    return int(hit[0]) if hit.size else None


def _band(anchors, N, R, bw):
    bs, be = np.zeros(R + 1, dtype=np.int64), np.full(R + 1, N, dtype=np.int64)
    for sig, at in anchors:
        bs[at], be[at] = max(0, sig - bw), min(N, sig + bw)
    return np.maximum.accumulate(bs), np.minimum.accumulate(be[::-1])[::-1]


def test_planted_sites_parity_and_recall(world, oracle_port):
    from nadavca_amd import defaults
    from nadavca_amd.batchflow import align_batch
    from nadavca_amd.call_indels import apply_edit, mapped_bands, to_read_frame
    from nadavca_amd.readbatch import contig_local_range
    ib, config, km = world['ib'], world['config'], world['km']
    mo = oracle_port.KmerModel(*world['model'])
    stage = align_batch(world['rb'], config, km, defaults.RENORM_ROUNDS, world['aligner']).stage
    db, sa = stage.dbatch, stage.sa
    host = lambda t: t.cpu().numpy()
    start, end = (host(x) for x in contig_local_range(sa, stage.reference))
    live, rev = host(sa.live), host(sa.reverse)
    assert np.array_equal(live, ib.live) and set(rev.tolist()) == {False, True}
    flat = {name: host(getattr(db, name)) for name in ('signal', 'sig_off', 'reference', 'ref_off', 'context_before',
                                                       'cb_off', 'context_after', 'ca_off', 'anchors', 'anc_off')}
    part = lambda j, data, off: flat[data][flat[off][j]:flat[off][j + 1]]
    bw, mel, w = config['bandwidth'], config['min_event_length'], config['model_wobbling']

    def oracle_total(j, ref, anchors):
        ll = np.asarray(oracle_port.estimate_log_likelihoods(
            part(j, 'signal', 'sig_off'), ref.astype(np.int32), part(j, 'context_before', 'cb_off'),
            part(j, 'context_after', 'ca_off'), anchors.astype(np.int32), bw, mel, mo, w))
        return ll[0, ref[0]]
    compared = skipped = 0
    worst = 0.0
    for x, d, s in world['sites']:
        t = _find(ib, 0, x, d, s)
        assert t is not None, (x, d, s)
        rows = np.nonzero(ib.row_site == t)[0]
        assert rows.size == ib.reads[t]
        # the table's columns are the rows' sums (the device sums in numpy's pairwise order)
        assert ib.support[t] == int((ib.row_llr[rows] > 0).sum())
        assert np.isclose(ib.llr[t], ib.row_llr[rows].sum(), rtol=1e-12, atol=1e-12)
        strands = set()
        for r in rows.tolist():
            j = int(np.nonzero(live == ib.row_read[r])[0][0])
            assert ib.row_strand[r] == rev[j] and ib.status[j] == 0
            strands.add(bool(rev[j]))
            ref = part(j, 'reference', 'ref_off')
            anchors = flat['anchors'].reshape(-1, 2)[flat['anc_off'][j]:flat['anc_off'][j + 1]]
            R, N = len(ref), len(part(j, 'signal', 'sig_off'))
            assert R == end[j] - start[j]
            p, d2, s2 = (int(v) for v in to_read_frame(x, d, s, start[j], end[j], rev[j]))
            letters = [s2] if s2 >= 0 else []
            ref2, anchors2, _ = apply_edit(ref, anchors, p, d2, letters)
            bs, be = _band(anchors, N, R, bw)
            mapped, recomputed = mapped_bands(bs, be, R, p, d2, len(letters)), _band(anchors2, N, len(ref2), bw)
            if not all(np.array_equal(a, b) for a, b in zip(mapped, recomputed)):
                skipped += 1
                continue
            exp = oracle_total(j, ref2, anchors2) - oracle_total(j, ref, anchors)
            got = ib.row_llr[r]
            assert np.isfinite(got) and np.isfinite(exp)
            worst = max(worst, abs(got - exp))
            assert np.isclose(got, exp, rtol=RTOL, atol=ATOL), (x, d, s, int(ib.row_read[r]), got, exp)
            compared += 1
        assert strands == {False, True}, (x, d, s)
        # every planted site is found: at least 8 reads, and together they prefer the edit
        print('planted (%d, del %d, ins %d): %d reads, %d with llr > 0, summed llr %.2f'
              % (x, d, s, ib.reads[t], ib.support[t], ib.llr[t]))
        assert ib.reads[t] >= 8 and ib.llr[t] > 0, (x, d, s, int(ib.reads[t]), float(ib.llr[t]))
    print('rows compared with the oracle %d, largest |llr - expected| %.3e; rows whose band the oracle cannot restate '
          '%d' % (compared, worst, skipped))
    assert compared >= 48 and skipped <= compared // 4

    # reported, not asserted: is the planted edit the best candidate within k - 1 positions, and how many unplanted
    # sites sum above the weakest planted one
    k = world['model'][0]
    planted = [_find(ib, 0, *site) for site in world['sites']]
    best = sum(1 for t in planted
               if ib.llr[t] >= ib.llr[(ib.contig == 0) & (np.abs(ib.position - ib.position[t]) <= k - 1)].max())
    weakest = min(ib.llr[t] for t in planted)
    above = int((ib.llr > weakest).sum()) - sum(1 for t in planted if ib.llr[t] > weakest)
    print('planted edit is the best candidate within %d positions at %d of 6 sites; %d of %d unplanted sites sum above '
          'the weakest planted one (%.2f); %d sites sum above 0; candidates per read %.1f'
          % (k - 1, best, above, len(ib) - 6, weakest, int((ib.llr > 0).sum()), ib.candidates.mean()))


def test_keep_rows_determinism_and_threshold(world):
    from nadavca_amd import call_indels_batch
    ib = world['ib']
    run = lambda **kw: call_indels_batch(world['rb'], world['aligner'], world['km'], config=world['config'], **kw)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    table = lambda b: (b.contig, b.position, b.del_len, b.ins_letter, b.reads, b.support, bits(b.llr))
    assert len(ib) > 1000 and ib.row_site.size == ib.reads.sum() == ib.candidates[ib.status == 0].sum()
    assert (np.diff(ib.row_site) >= 0).all() and ib.contig_names is None and (ib.contig == 0).all()
    key = ((ib.contig.astype(np.int64) * GENOME + ib.position) * 2 + ib.del_len) * 5 + ib.ins_letter + 1
    assert (np.diff(key) > 0).all()                                       # sorted, every site once
    assert ib.threshold == 0.0 and np.array_equal(ib.called, np.nonzero(ib.llr > 0)[0])
    # two runs: the same bits, rows included
    again = run(keep_rows='all')
    for a, b in zip(table(ib) + (ib.row_site, ib.row_read, ib.row_strand, bits(ib.row_llr), bits(ib.total)),
                    table(again) + (again.row_site, again.row_read, again.row_strand, bits(again.row_llr),
                                    bits(again.total))):
        assert np.array_equal(a, b)
    # the default keeps the rows of the called sites, None keeps none; the table does not depend on it
    threshold = float(np.sort(ib.llr)[-20])
    called = run(threshold=threshold)
    assert called.threshold == threshold and called.called.size == 19
    assert all(np.array_equal(a, b) for a, b in zip(table(called), table(ib)))
    keep = np.isin(ib.row_site, called.called)
    assert keep.sum() == ib.reads[called.called].sum() > 0
    for a, b in ((called.row_site, ib.row_site[keep]), (called.row_read, ib.row_read[keep]),
                 (called.row_strand, ib.row_strand[keep]), (bits(called.row_llr), bits(ib.row_llr[keep]))):
        assert np.array_equal(a, b)
    none = run(keep_rows=None)
    assert none.row_site.size == none.row_llr.size == 0 and all(np.array_equal(a, b)
                                                                for a, b in zip(table(none), table(ib)))
    # longer deletions and a wider trim: more kinds of site, fewer positions
    wide = run(max_del=3, trim=20, keep_rows=None)
    assert set(wide.del_len.tolist()) == {0, 1, 2, 3} and wide.candidates.sum() > 0
    import io
    out = io.StringIO()
    called.write_tsv(out)
    lines = out.getvalue().splitlines()
    assert len(lines) == 20 and lines[0].split('\t') == ['contig', 'position', 'del_len', 'ins', 'reads', 'support',
                                                         'llr']


def test_reference_set_reports_contig_local_positions(world):
    """The same reads behind a 700-base contig without reads: contig 1, the planted sites at the same contig-local
    positions with the same columns."""
    from nadavca_amd import call_indels_batch, ReferenceSet, SeedAligner
    ib = world['ib']
    other = np.random.default_rng(SEED + 1).integers(0, 4, 700).astype(np.int32)
    refset = ReferenceSet.from_arrays(['chrA', 'chrB'], [other, world['genome']])
    ib2 = call_indels_batch(world['rb'], SeedAligner(refset), world['km'], config=world['config'], keep_rows=None)
    assert ib2.contig_names == ['chrA', 'chrB'] and (ib2.contig == 1).all()
    assert 0 <= ib2.position.min() and ib2.position.max() < GENOME
    for x, d, s in world['sites']:
        t = _find(ib2, 1, x, d, s)
        assert t is not None and ib2.reads[t] >= 8 and ib2.llr[t] > 0
        t0 = _find(ib, 0, x, d, s)
        assert ib2.reads[t] == ib.reads[t0] and ib2.support[t] == ib.support[t0]
        assert np.isclose(ib2.llr[t], ib.llr[t0], rtol=RTOL, atol=ATOL)


def test_empty_batches(world):
    from nadavca_amd import call_indels_batch
    from nadavca_amd.readbatch import BaseAlignmentBatch, SyntheticBatchAligner
    rb = world['rb']
    nothing = BaseAlignmentBatch(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(rb.n + 1, np.int64),
                                 np.zeros(rb.n, bool))
    none = SyntheticBatchAligner(world['genome'], nothing)
    ib = call_indels_batch(rb, none, world['km'], config=world['config'])
    assert len(ib) == 0 and ib.live.size == 0 and ib.called.size == 0 and ib.llr.dtype == np.float64
    # a trim that leaves no position
    ib = call_indels_batch(rb, world['aligner'], world['km'], config=world['config'], trim=500)
    assert len(ib) == 0 and ib.live.size == world['ib'].live.size and (ib.candidates == 0).all()
    assert np.isfinite(ib.total[ib.status == 0]).all()
