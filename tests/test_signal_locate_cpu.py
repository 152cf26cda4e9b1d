"""The rules of ``signal_locate_batch`` without a GPU: the C++ restatement of nvk_signal_locate_dev against a plain
Python DP (bit for bit, tie order included), the block reduction and the chain rule on hand-made tables (the numpy
restatements of tests/locate_ref.py and the torch code of nadavca_amd/locate.py, on CPU tensors), and the whole
workflow in numpy on the 300 leader-padded reads of the signal_map quality batch."""
import numpy as np
import pytest

import locate_ref as L
import signal_map_ref as R


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return L.build_host(tmp_path_factory.mktemp('locate_host'))


@pytest.fixture(scope='module')
def map_host(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp('map_host'))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize('name,case', L.small_cases(), ids=[c[0] for c in L.small_cases()])
def test_shim_equals_the_plain_python_dp(host, name, case):
    score, hit = host.locate(case['level'], case['q_off'], case['mu'], case['ac'], case['mc'], case['col_off'],
                             *case['costs'])
    q_off, col_off = case['q_off'], case['col_off']
    assert score.shape == (q_off.size - 1, L.n_blocks_of(col_off))
    for q in range(q_off.size - 1):
        want_s, want_h = [], []
        for t in range(col_off.size - 1):
            cols = slice(col_off[t], col_off[t + 1])
            s, h = L.python_locate(case['level'][q_off[q]:q_off[q + 1]], case['mu'][cols], case['ac'][cols],
                                   case['mc'][cols], *case['costs'])
            want_s += s
            want_h += h
        assert np.array_equal(bits(score[q]), bits(want_s)), (name, q)
        assert np.array_equal(hit[q], np.array(want_h, dtype=np.int32).reshape(-1, 4)), (name, q)


def test_grid_cases_do_tie():
    """The grid cases are there for the tie order: in most of them some cell has two equal best candidates."""
    tied = 0
    cases = [c for n, c in L.small_cases() if n.startswith('grid')]
    for case in cases:
        lev, mu = case['level'][:case['q_off'][1]], case['mu'][:case['col_off'][1]]
        l_stay, l_step, l_skip, trim = case['costs']
        S = np.full((lev.size, mu.size), -np.inf)
        found = False
        for i in range(lev.size):
            for j in range(mu.size):
                c = [i * trim, (S[i - 1, j - 1] if i and j else -np.inf) + l_step, (S[i - 1, j] if i else -np.inf) + l_stay,
                     (S[i - 1, j - 2] if i and j > 1 else -np.inf) + l_skip]
                found |= sorted(c)[-1] == sorted(c)[-2]
                S[i, j] = max(c) - 0.5 * (lev[i] - mu[j]) ** 2
        tied += found
    assert tied >= len(cases) // 2


def both_reduce(score, hit, n_events, col_off):
    """reduce_blocks of the numpy restatement and of the package (torch on the CPU): they must agree -> the numpy one"""
    import torch
    from nadavca_amd import locate
    tables = L.block_tables(col_off)
    ref = L.reduce_blocks(score, hit, n_events, *tables)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    got = locate.reduce_blocks(t(score), t(hit), t(np.asarray(n_events, np.int64)),
                               *locate.block_tables(t(np.asarray(col_off, np.int64))))
    assert all(np.array_equal(a, b) for a, b in zip(tables, (x.numpy() for x in locate.block_tables(t(col_off)))))
    for a, b in zip(ref, got):
        b = b.numpy()
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
    return ref


def test_block_reduction_and_exclusion_zone():
    # two targets: 1000 columns (blocks 0..3) and 300 (blocks 4, 5)
    col_off = np.array([0, 1000, 1300], np.int64)
    hit = np.zeros((5, 6, 4), np.int32)
    hit[:, :, 0] = np.array([100, 300, 600, 900, 50, 280])     # each block's end column
    hit[3, 1, 0] = 511                                          # (query 3 ends on its block's last column)
    score = np.array([
        [-50.0, -10.0, -12.0, -40.0, -30.0, -45.0],   # best 1 (end 300), Q = 10: [280, 320] touches block 1 alone
        [-50.0, -10.0, -12.0, -40.0, -30.0, -45.0],   # Q = 100: [100, 500] touches blocks 0 and 1, not 2 (from 512)
        [-50.0, -10.0, -12.0, -40.0, -30.0, -45.0],   # Q = 128: [44, 556] touches blocks 0, 1 and 2
        [-11.0, -10.0, -50.0, -10.0, -10.5, -45.0],   # blocks 1 and 3 tie: the smaller one is the best, the other second
        [-50.0, -60.0, -70.0, -80.0, -20.0, -45.0]])  # best on the second target's first block
    n_events = np.array([10, 100, 128, 20, 40], np.int64)
    blk, best, second, margin, top = both_reduce(score, hit, n_events, col_off)
    assert blk.tolist() == [1, 1, 1, 1, 4]
    assert second.tolist() == [-12.0, -12.0, -30.0, -10.0, -45.0]
    # query 3: end 511, Q = 20 -> [471, 551] touches blocks 1 and 2 of its target; block 3 (equal score) is second
    assert margin.tolist() == [(-10.0 + 12.0) / 10, (-10.0 + 12.0) / 100, (-10.0 + 30.0) / 128, 0.0, (-20.0 + 45.0) / 40]
    assert top[:, 0].tolist() == [300, 300, 300, 511, 50]
    # query 4: best block 4 ends at 50, Q = 40: [-30, 130] touches block 4 alone; block 5 (columns 256..299) is not
    # excluded, so an equal score there is the second and the margin is 0
    score[4, 5] = -20.0
    assert both_reduce(score, hit, n_events, col_off)[3][4] == 0.0
    hit[4, 4, 0] = 200                                 # [120, 280] touches block 5 as well
    assert both_reduce(score, hit, n_events, col_off)[3][4] == (-20.0 + 50.0) / 40
    # a single block: no second, the margin is +inf
    one = both_reduce(np.array([[-3.0]]), np.zeros((1, 1, 4), np.int32), np.array([5]), np.array([0, 200], np.int64))
    assert one[2][0] == -np.inf and one[3][0] == np.inf


def both_chain(rows, chunk_off, min_margin=0.2):
    """``rows``: per chunk (target, start, end, first event, last event, margin) -> (status, anchor, joined) of the
    numpy restatement, checked against the package's torch code"""
    import torch
    from nadavca_amd import locate
    rows = np.array(rows, dtype=np.float64).reshape(-1, 6)
    ints = [rows[:, k].astype(np.int64) for k in range(5)]
    chunk_off = np.asarray(chunk_off, np.int64)
    ref = L.chain_chunks(chunk_off, *ints, rows[:, 5], min_margin)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    got = locate.chain_chunks(t(chunk_off), *[t(x) for x in ints], t(rows[:, 5].copy()), min_margin)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b.numpy())
    return ref


def test_chain_rule():
    # (target, start, end, first event, last event, margin); chunks of 100 events each: chunk c holds events 100 c ..
    status, anchor, joined = both_chain([(2, 500, 580, 3, 97, 0.9)], [0, 1])
    assert status.tolist() == [0] and anchor.tolist() == [0] and joined.tolist() == [True]
    status, _, _ = both_chain([(2, 500, 580, 3, 97, 0.19)], [0, 1])
    assert status.tolist() == [L.LOC_AMBIGUOUS]
    # read 0: three chunks in a row, the anchor (largest margin, the FIRST of equal ones) in the middle
    # read 1: no chunks
    # read 2: the second chunk is on another target; the third joins: gap 84 <= between 100 + 16
    # read 3: the second chunk lies beyond the bound (gap 25 > between 8 + 16); the third is then judged against the
    #         last JOINED chunk, the anchor: gap 103 <= between 104 + 16
    # read 4: a low-margin chunk in the middle is bridged: gap 95 <= between (2 + 100 + 1) + 16
    rows = [(0, 100, 190, 0, 99, 0.5), (0, 191, 280, 100, 199, 0.8), (0, 281, 370, 200, 299, 0.8),
            (1, 40, 120, 0, 99, 0.7), (3, 121, 200, 100, 199, 0.6), (1, 205, 290, 200, 297, 0.3),
            (4, 1000, 1080, 0, 95, 0.9), (4, 1106, 1200, 104, 199, 0.9), (4, 1184, 1300, 200, 299, 0.9),
            (5, 10, 90, 0, 97, 0.6), (5, 600, 700, 100, 199, 0.1), (5, 186, 270, 201, 299, 0.6)]
    status, anchor, joined = both_chain(rows, [0, 3, 3, 6, 9, 12])
    assert status.tolist() == [0, L.LOC_NO_EVENTS, 0, 0, 0]
    assert anchor.tolist() == [1, -1, 3, 6, 9]
    assert joined.tolist() == [True, True, True, True, False, True, True, False, True, True, False, True]


def test_chain_bounds():
    # one column beyond the bound and the chunk stays out: the walk goes on from the anchor and takes the third chunk,
    # which overlaps the second by 17 columns and so stays out once the second is in
    for beyond, want in ((1, False), (0, True)):
        rows = [(4, 1000, 1080, 0, 95, 0.9), (4, 1081 + 8 + 16 + beyond, 1200, 104, 199, 0.9),
                (4, 1184, 1300, 200, 299, 0.9)]
        assert both_chain(rows, [0, 3])[2].tolist() == [True, want, not want]
    # an overlap of more than 16 columns does not join; of 16 it does; walking to the left mirrors it
    for overlap, want in ((17, False), (16, True)):
        rows = [(0, 300, 400, 0, 99, 0.5), (0, 401 - overlap, 480, 100, 199, 0.9)]
        assert both_chain(rows, [0, 2])[2].tolist() == [want, True]          # anchor: the second chunk
        rows = [(0, 300, 400, 0, 99, 0.9), (0, 401 - overlap, 480, 100, 199, 0.5)]
        assert both_chain(rows, [0, 2])[2].tolist() == [True, want]


@pytest.fixture(scope='module')
def located(host, map_host):
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    _, aligner, _, (raw, sig_off, lead) = R.quality_batch(model)
    res = L.cpu_signal_locate(map_host, host, raw, sig_off, [aligner.reference_num], model)
    return res, R.quality_places(model)


def test_cpu_signal_locate_places_the_leader_padded_reads(located):
    """Measured: 300 of 300 located, all on the right strand; window start against the truth -15 / +22 bases, end
    -22 / +15 (5th / 95th percentile); start and end each within 32 bases for 0.9867 of the reads; 4.46 chunks per
    read.  The bounds are the issue's: 0.98 located, 0.90 within 32 bases."""
    res, (g0, length, reverse) = located
    ok = res['status'] == L.LOC_OK
    d_start, d_end = (res['ref_start'] - g0)[ok], (res['ref_end'] - (g0 + length))[ok]
    near = (np.abs(d_start) <= 32) & (np.abs(d_end) <= 32)
    pct = lambda x: tuple(np.percentile(x, [5, 95]).tolist())
    print('located %d of %d, right strand %d, start %+.0f / %+.0f, end %+.0f / %+.0f (5th / 95th percentile, bases), '
          'both within 32: %.4f, start within 32: %.4f, end within 32: %.4f, chunks per read %.2f'
          % ((ok.sum(), ok.size, (res['reverse'] == reverse)[ok].sum()) + pct(d_start) + pct(d_end)
             + (near.mean(), (np.abs(d_start) <= 32).mean(), (np.abs(d_end) <= 32).mean(), res['n_chunks'].mean())))
    assert (res['reverse'] == reverse)[ok].all() and (res['contig'][ok] == 0).all()
    assert ok.mean() >= 0.98
    assert (np.abs(d_start) <= 32).mean() >= 0.90 and (np.abs(d_end) <= 32).mean() >= 0.90


def test_located_windows_map(located, map_host):
    """cpu_signal_map on the located windows.  Measured: 300 of 300 reads mapped, 0.9867 of the windows' bases mapped,
    0.9697 of those within 20 samples of the simulator's starts, 0.0273 further off than 40 (0.9973 / 0.00008 with the
    true sequences: the deficit is the windows' ends).  The floors are those of the GPU chain test."""
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    res, _ = located
    _, aligner, true_starts, (raw, sig_off, lead) = R.quality_batch(model)
    codes, col_off = L.target_codes([aligner.reference_num])
    seqs = [codes[col_off[int(rv)] + s:col_off[int(rv)] + s + n] for rv, s, n in
            zip(res['reverse'], res['win_start'], res['win_len'])]
    seq_off = R.offsets([s.size for s in seqs])
    sm = R.cpu_signal_map(map_host, raw, sig_off, np.concatenate(seqs), seq_off, model)
    share, near, far = L.window_quality(sm, res, R.quality_places(model), true_starts, lead)
    print('reads mapped %d of %d; bases mapped %.4f, within 20 samples %.4f, beyond 40 %.4f'
          % ((sm['status'] == 0).sum(), sm['status'].size, share, near, far))
    assert (sm['status'] == 0).mean() >= 0.97 and near >= 0.93 and far <= 0.05
