"""``call_mods_batch`` on the GPU: every row against ``ll[p, 4] - ll[p, ref[p]]`` of the existing full-matrix operator
on the same alignment stage (tolerance and -inf rule of tests/test_gpu_ell.py: 1e-9 relative + 1e-9 absolute, no NaN),
with the sites found by a plain numpy loop; every row's coordinate against the genome itself; and the sign of the
ratio against the simulated truth, per strand."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-9
N_READS = 1200


def _model5(seed=5, sd=0.6):
    """The packaged 6-mer table extended to 5 letters: an M k-mer = its C k-mer's level + N(0, sd^2)."""
    from nadavca_amd import synthetic, kmer_train
    k, central, _, mean, sigma = synthetic.load_model_arrays()
    mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
    has_m = np.zeros(5 ** k, dtype=bool)
    for m in range(k):
        has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
    mean5 = mean5 + np.where(has_m, np.random.default_rng(seed).normal(0.0, sd, 5 ** k), 0.0)
    return k, central, 5, mean5, sigma5


@pytest.fixture(scope='module')
def model5():
    return _model5()


@pytest.fixture(scope='module')
def km5(model5):
    from nadavca_amd import dtw
    return dtw.KmerModel(*model5)


def _expected_rows(stage, align_status, ll, pattern, mod_offset, k):
    """Plain loop over the host copy of the stage: -> rows (read, contig, position, strand, llr, crowded)."""
    from nadavca_amd.readbatch import contig_local_range
    sa = stage.sa
    start, end = (x.cpu().numpy() for x in contig_local_range(sa, stage.reference))
    ref = stage.dbatch.reference.cpu().numpy()
    off = stage.dbatch.ref_off.cpu().numpy()
    live, rev, contig = sa.live.cpu().numpy(), sa.reverse.cpu().numpy(), sa.contig.cpu().numpy()
    m = len(pattern)
    rows = []
    for j in range(len(live)):
        if align_status[j] != 0:
            continue
        part = ref[off[j]:off[j + 1]]
        ps = [q + mod_offset for q in range(len(part) - m + 1) if all(part[q + t] == pattern[t] for t in range(m))]
        for p in ps:
            f = end[j] - 1 - p if rev[j] else start[j] + p
            crowded = any(p2 != p and abs(p2 - p) <= k - 1 for p2 in ps)
            rows.append((int(live[j]), int(contig[j]), int(f), int(rev[j]),
                         ll[off[j] + p, 4] - ll[off[j] + p, part[p]], crowded))
    return rows


def _compare(mb, rows):
    assert len(mb) == len(rows)
    exp = np.array([r[4] for r in rows], dtype=float)
    assert mb.read.tolist() == [r[0] for r in rows]
    assert mb.contig.tolist() == [r[1] for r in rows]
    assert mb.position.tolist() == [r[2] for r in rows]
    assert mb.strand.tolist() == [r[3] for r in rows]
    assert mb.crowded.tolist() == [r[5] for r in rows]
    assert not np.isnan(mb.llr).any() and not np.isnan(exp).any()
    assert np.array_equal(np.isinf(mb.llr), np.isinf(exp))
    fin = np.isfinite(exp)
    err = float(np.max(np.abs(mb.llr[fin] - exp[fin]))) if fin.any() else 0.0
    print('rows %d, largest |llr - expected| %.3e' % (len(rows), err))
    assert np.allclose(mb.llr[fin], exp[fin], rtol=RTOL, atol=ATOL), err


def _full_matrix_on_stage(rb, aligner, km, config):
    """The alignment stage of the workflow and the existing full-matrix operator on it."""
    from nadavca_amd import defaults
    from nadavca_amd.batchflow import align_batch
    from nadavca_amd.device import estimate_log_likelihoods_dev
    res = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
    ll, st = estimate_log_likelihoods_dev(res.stage.dbatch, config['bandwidth'], config['min_event_length'], km,
                                          config['model_wobbling'])
    st = st.cpu().numpy()
    align_status = res.status.cpu().numpy()
    assert (st[align_status == 0] == 0).all()
    return res.stage, align_status, ll.cpu().numpy()


def test_call_mods_rows_against_full_matrix(model5, km5):
    from nadavca_amd import call_mods_batch, defaults, synthetic
    from nadavca_amd.batchflow import load_config
    config = load_config(defaults.CONFIG_FILE)
    rb, aligner, genome, truth = synthetic.make_modified_read_batch(N_READS, model5, seed=21)
    mb = call_mods_batch(rb, aligner, km5)
    stage, align_status, ll = _full_matrix_on_stage(rb, aligner, km5, config)
    rows = _expected_rows(stage, align_status, ll, [1, 2], 0, model5[0])
    assert len(rows) > 20 * N_READS * 0.8
    _compare(mb, rows)
    assert set(mb.strand.tolist()) == {0, 1} and mb.contig_names is None and (mb.contig == 0).all()
    assert np.array_equal(mb.live, stage.sa.live.cpu().numpy()) and mb.status.shape == mb.live.shape
    assert np.isfinite(mb.total[mb.status == 0]).all()

    # structural, exact: every row is the C of a CG on its strand of the genome
    G = genome.size
    for p, s in zip(mb.position.tolist(), mb.strand.tolist()):
        if s == 0:
            assert genome[p] == 1 and genome[p + 1] == 2
        else:
            assert genome[p] == 2 and genome[p - 1] == 1      # 3 - G = C on the reverse strand, 3 - C = G after it
    assert 0 <= mb.position.min() and mb.position.max() < G

    # sign and strand sanity, a condition and not a measurement: chance level per strand
    for s, mask in ((0, truth['forward']), (1, truth['reverse'])):
        sel = (mb.strand == s) & ~mb.crowded
        is_mod = mask[mb.position[sel]]
        llr = mb.llr[sel]
        share_mod, share_unmod = float(np.mean(llr[is_mod] > 0)), float(np.mean(llr[~is_mod] < 0))
        print('strand %d: %d modified rows, llr > 0 on %.3f; %d unmodified rows, llr < 0 on %.3f'
              % (s, is_mod.sum(), share_mod, (~is_mod).sum(), share_unmod))
        assert is_mod.sum() > 1000 and (~is_mod).sum() > 1000
        assert share_mod > 0.5 and share_unmod > 0.5

    # another pattern and offset: GC with the C substituted
    mb2 = call_mods_batch(rb, aligner, km5, pattern='GC', mod_offset=1)
    rows2 = _expected_rows(stage, align_status, ll, [2, 1], 1, model5[0])
    _compare(mb2, rows2)
    for p, s in zip(mb2.position.tolist(), mb2.strand.tolist()):
        assert (genome[p] == 1 and genome[p - 1] == 2) if s == 0 else (genome[p] == 2 and genome[p + 1] == 1)

    # the site table adds up
    tab = mb.site_table()
    assert tab['reads'].sum() == len(mb)
    assert len(set(zip(tab['contig'].tolist(), tab['position'].tolist(), tab['strand'].tolist()))) == len(tab['reads'])


def test_call_mods_contigs_with_seed_aligner(model5, km5):
    """Reads of three contigs through ``SeedAligner`` over a ``ReferenceSet``: contig-local positions."""
    from contig_fixture import concat_batches
    from nadavca_amd import call_mods_batch, defaults, synthetic, SeedAligner, ReferenceSet
    from nadavca_amd.batchflow import load_config
    config = load_config(defaults.CONFIG_FILE)
    parts = [synthetic.make_modified_read_batch(n, model5, seed=seed, genome_length=g)
             for n, seed, g in ((400, 41, 10000), (400, 42, 4000), (240, 43, 1500))]
    names = ['chrA', 'chrB', 'chrC']
    contigs = [p[2] for p in parts]
    refset = ReferenceSet.from_arrays(names, contigs)
    rb = concat_batches([p[0] for p in parts])
    aligner = SeedAligner(refset)
    mb = call_mods_batch(rb, aligner, km5)
    stage, align_status, ll = _full_matrix_on_stage(rb, aligner, km5, config)
    rows = _expected_rows(stage, align_status, ll, [1, 2], 0, model5[0])
    assert len(rows) > 10000
    _compare(mb, rows)
    assert mb.contig_names == names and set(mb.contig.tolist()) == {0, 1, 2}
    first = np.cumsum([0, 400, 400])
    for r, c, p, s in zip(mb.read.tolist(), mb.contig.tolist(), mb.position.tolist(), mb.strand.tolist()):
        g = contigs[c]
        assert c == np.searchsorted(first, r, side='right') - 1           # the read's true contig
        assert (g[p] == 1 and g[p + 1] == 2) if s == 0 else (g[p] == 2 and g[p - 1] == 1)
    for c, part in enumerate(parts):
        truth = part[3]
        for s, mask in ((0, truth['forward']), (1, truth['reverse'])):
            sel = (mb.contig == c) & (mb.strand == s) & ~mb.crowded
            is_mod = mask[mb.position[sel]]
            assert np.mean(mb.llr[sel][is_mod] > 0) > 0.5 and np.mean(mb.llr[sel][~is_mod] < 0) > 0.5


def test_call_mods_refusals_and_empty_batches(model5, km5):
    from nadavca_amd import call_mods_batch, dtw, synthetic
    from nadavca_amd.readbatch import BaseAlignmentBatch, SyntheticBatchAligner
    rb, aligner, genome, truth = synthetic.make_modified_read_batch(32, model5, seed=22, genome_length=3000)
    km4 = dtw.KmerModel(*synthetic.load_model_arrays())
    with pytest.raises(ValueError, match='no modified base'):
        call_mods_batch(rb, aligner, km4)
    with pytest.raises(ValueError, match='no modified base'):
        call_mods_batch(rb, aligner, km5, mod_code=5)
    with pytest.raises(ValueError, match='mod_offset'):
        call_mods_batch(rb, aligner, km5, mod_offset=2)
    # no aligned read
    none = SyntheticBatchAligner(genome, BaseAlignmentBatch(np.zeros(0, np.int32), np.zeros(0, np.int64),
                                                            np.zeros(rb.n + 1, np.int64), np.zeros(rb.n, bool)))
    mb = call_mods_batch(rb, none, km5)
    assert len(mb) == 0 and mb.live.size == 0 and mb.status.size == 0 and mb.llr.dtype == np.float64
    # a pattern without an occurrence (a letter outside ACGT matches nothing; 14 bases of one letter do not occur)
    for pattern in ('CN', 'A' * 14):
        mb = call_mods_batch(rb, aligner, km5, pattern=pattern)
        assert len(mb) == 0 and mb.live.size == rb.n and (mb.status == 0).all() and np.isfinite(mb.total).all()
        assert mb.site_table()['reads'].size == 0
    assert len(call_mods_batch(rb, aligner, km5)) > 0
