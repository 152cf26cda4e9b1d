"""``signal_map_batch`` without a GPU: the CPU restatements the kernels are held to (tests/host_shims/events_host.cpp,
eventalign_host.cpp; tests/test_gpu_signal_map_kernels.py does the holding) against plain Python —

* the event detector against a per-sample restatement of the border rules on constructed signals;
* the banded alignment against a full-matrix DP with the same moves, ties, free ends and lost rule, on reads small
  enough that the band covers the matrix, and on one long read whose band moves both ways;
* the band's moves: the rule for two -inf ends, a band that moves both ways, a read with 100 bases of signal cut out;
* the quality of the banded restatement on 300 simulated reads against the simulator's true starts, with and without
  unrelated samples around every read;
* the C-ABI entries declared, bound and exported, and the ReadBatch round trip."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import signal_map_ref as R
from nadavca_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIM, SKIP = math.log(0.01), math.log(1e-10)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp('signal_map'))


@pytest.fixture(scope='module')
def model():
    return synthetic.load_model_arrays()


@pytest.fixture(scope='module')
def quality(host, model):
    """The 300-read batch mapped by the restatement, plain and with leaders and trailers (computed once)."""
    rb, _, true_starts, (raw2, sig_off2, lead) = R.quality_batch(model)
    plain = R.cpu_signal_map(host, rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off, model)
    padded = R.cpu_signal_map(host, raw2, sig_off2, rb.sequence, rb.seq_off, model)
    return rb, true_starts, lead, plain, padded


@pytest.mark.parametrize('case', R.detector_cases(), ids=lambda c: c[0])
def test_detector_equals_plain_python(host, case):
    _, signal, sig_off, w, threshold, var_floor = case
    got = host.flags(signal, sig_off, w, threshold, var_floor)
    want = [f for r in range(sig_off.size - 1)
            for f in R.python_flags(signal[sig_off[r]:sig_off[r + 1]], w, threshold, var_floor)]
    assert got.tolist() == want
    # sample 0 of every read is a border, so no event crosses two reads
    assert all(got[sig_off[r]] == 1 for r in range(sig_off.size - 1) if sig_off[r + 1] > sig_off[r])
    ev_pos = np.nonzero(got)[0]
    start, length, level = host.levels(signal, sig_off, ev_pos)
    ends = np.append(ev_pos[1:], signal.size)
    owner = np.searchsorted(sig_off, ev_pos, side='right') - 1
    assert start.tolist() == (ev_pos - sig_off[owner]).tolist() and length.tolist() == (ends - ev_pos).tolist()
    for e in range(ev_pos.size):
        total = 0.0
        for v in signal[ev_pos[e]:ends[e]]:
            total += float(v)
        assert level[e] == total / float(ends[e] - ev_pos[e])


def test_detector_cases_do_what_they_are_for(host):
    cases = {c[0]: c for c in R.detector_cases()}
    flags = lambda name: host.flags(*cases[name][1:])
    assert flags('shorter than 2w').tolist() == [1, 0, 0]
    assert flags('constant').tolist() == [1] + [0] * 39
    # 0 0 0 1 2 2 2 ...: s(3) == s(4), the border stands at 3 alone
    f = flags('equal adjacent statistics')
    assert f[3] == 1 and f[4] == 0
    for at in (R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE):
        f = flags('border at %d' % at)
        assert f[at] == 1 and f[at - 1] == 0 and f[at + 1] == 0


def brute(case, trim=TRIM, skip=SKIP):
    return R.brute_force_align(case['level'].tolist(), case['mu'].tolist(), case['ac'].tolist(), case['mc'].tolist(),
                               case['l_stay'], case['l_step'], trim, skip)


@pytest.mark.parametrize('band', [64, 128])
def test_alignment_equals_the_full_matrix(host, band):
    named = R.small_align_cases()
    seen = set()
    for grid in (False, True):
        cases = [c for name, c in named if name.startswith('grid') == grid]
        names = [name for name, _ in named if name.startswith('grid') == grid]
        trim, skip = R.GRID_COSTS if grid else (TRIM, SKIP)
        hit, score, be = host.align(band=band, trim_cost=trim, skip_cost=skip, **R.pack_align_cases(cases))
        off = R.offsets([c['mu'].size for c in cases])
        for r, (name, c) in enumerate(zip(names, cases)):
            status, first, last, total, base_event = brute(c, trim, skip)
            assert hit[r].tolist() == [status, c['level'].size, first, last], name
            assert be[off[r]:off[r + 1]].tolist() == base_event, name
            assert score[r] == total, name
            if 'lost' in name:
                assert status == R.MAP_LOST
            elif not grid:
                assert status == R.MAP_OK, name
            seen.add(status)
    assert seen == {R.MAP_OK, R.MAP_LOST}


def test_skips_are_forced_and_ends_are_free(host):
    cases = dict(R.small_align_cases())
    one = lambda name: host.align(band=64, trim_cost=TRIM, skip_cost=SKIP, **R.pack_align_cases([cases[name]]))
    hit, _, be = one('E < K: one skip forced')
    assert hit[0, 0] == 0 and (be < 0).sum() == 1
    hit, _, be = one('E < K: two skips forced')
    assert hit[0, 0] == 0 and (be < 0).sum() == 2
    hit, _, be = one('leader and trailer')
    n = cases['leader and trailer']['level'].size
    assert hit[0, 0] == 0 and hit[0, 2] == 9 and hit[0, 3] == n - 9 and be[0] == 9
    hit, _, be = one('K = 1')
    assert hit[0].tolist() == [0, 5, 1, 3] and be.tolist() == [1]


def test_band_alternates_while_both_ends_are_minus_infinity(host):
    c = dict(R.small_align_cases())['K < k']
    for band in (64, 128):
        *_, corner = host.align(band=band, trim_cost=TRIM, skip_cost=SKIP, corners=True, **R.pack_align_cases([c]))
        H = band // 2
        assert corner[0].tolist() == [H - 1, -1 - H] and corner[1].tolist() == [H, -1 - H]
        for b in range(2, corner.shape[0]):
            step = (corner[b] - corner[b - 1]).tolist()
            assert step == ([0, 1] if b % 2 else [1, 0]), b   # right on odd bands, down on even ones


def test_band_moves_both_ways_and_keeps_the_best_path(host, model):
    """One read of 150 bases, about 310 events: past the first ``band`` bands the corner is steered by the scores;
    it moves right and down in runs, and the path it keeps is the full matrix's."""
    rb, *_ = R.quality_batch(model, 1)
    stride = int(rb.seq_off[1]) - 50
    res = R.cpu_signal_map(host, rb.raw_signal, rb.sig_off, rb.sequence[:stride], [0, stride], model)
    c = dict(level=res['scaled'], mu=res['mu'], ac=res['ac'], mc=res['mc'], l_stay=float(res['l_stay'][0]),
             l_step=float(res['l_step'][0]))
    hit, score, be, corner = host.align(band=128, trim_cost=TRIM, skip_cost=SKIP, corners=True,
                                        **R.pack_align_cases([c]))
    moves = np.diff(corner, axis=0)
    assert (moves.sum(axis=1) == 1).all() and (moves >= 0).all()
    right = moves[:, 1]
    runs = np.diff(np.flatnonzero(np.diff(right) != 0))
    assert right.sum() > 50 and (1 - right).sum() > 50 and runs.max() >= 3      # not an alternation any more
    status, first, last, total, base_event = brute(c)
    assert hit[0].tolist() == [status, c['level'].size, first, last] and status == 0
    assert be.tolist() == base_event and score[0] == total
    assert hit[0, 3] < c['level'].size - 40   # the signal of the last 50 bases stays outside: a free end


@pytest.mark.parametrize('band', [64, 128])
@pytest.mark.parametrize('cut_from', [30, 100, 180])
def test_cut_out_signal_is_lost(host, model, band, cut_from):
    raw, seq, whole = R.cut_read(model, cut_from=cut_from)
    res = R.cpu_signal_map(host, raw, [0, raw.size], seq, [0, seq.size], model, band=band)
    assert res['status'].tolist() == [R.MAP_LOST]
    assert res['map_off'].tolist() == [0, 0] and (res['base_event'] == -1).all()
    assert np.isinf(res['path_score'][0]) and res['first_event'][0] == -1 and res['last_event'][0] == -1
    res = R.cpu_signal_map(host, whole, [0, whole.size], seq, [0, seq.size], model, band=band)
    assert res['status'].tolist() == [R.MAP_OK]


def check_caps(res, seq_off, true_starts, lead=None):
    assert (res['status'] == 0).all()
    mapped, near, far = R.quality(res, seq_off, true_starts, lead)
    print('mapped %.4f, within 20 samples %.4f, beyond 40 samples %.5f' % (mapped, near, far))
    assert mapped >= 0.98
    assert near >= 0.98
    assert far <= 0.002


def test_quality_on_300_reads(quality):
    """Measured with the defaults (window 2, threshold 5, var_floor 0.02, band 128, sigma_scale 0.5): 0.9910 of the
    bases mapped, 0.9976 of those within 20 samples of the true start, 0.00013 beyond 40."""
    rb, true_starts, _, plain, _ = quality
    assert 1.5 < plain['ev_off'][-1] / rb.seq_off[-1] < 2.6    # events per base
    check_caps(plain, rb.seq_off, true_starts)


def test_quality_with_leaders_and_trailers(quality):
    """The same reads with 150-300 unrelated samples before and after each, scored on the original bases.  Measured:
    0.9911 mapped, 0.9973 within 20 samples, 0.00008 beyond 40."""
    rb, true_starts, lead, _, padded = quality
    check_caps(padded, rb.seq_off, true_starts, lead)
    # the leaders' events are trimmed, not aligned
    first_sample = padded['ev_start'][padded['ev_off'][:-1] + padded['first_event']]
    assert np.mean(np.abs(first_sample - lead) <= 20) > 0.95


def test_tables_are_ascending_and_one_row_per_mapped_base(quality):
    rb, _, _, plain, _ = quality
    for r in range(rb.n):
        lo, hi = plain['map_off'][r], plain['map_off'][r + 1]
        b, s = plain['map_base'][lo:hi], plain['map_sig'][lo:hi]
        assert (np.diff(b) > 0).all() and (np.diff(s) > 0).all()
        assert b.min() >= 0 and b.max() < rb.seq_off[r + 1] - rb.seq_off[r]
        assert s.min() >= 0 and s.max() < rb.sig_off[r + 1] - rb.sig_off[r]


def test_entries_declared_bound_and_exported():
    import nadavca_amd
    from nadavca_amd import _lib, device, signal_map
    header = open(os.path.join(ROOT, 'include', 'nadavca_hip.h')).read()
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail('the library is not built: %s' % _lib.LIB_PATH)
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in (('nvk_event_flags_dev', 9), ('nvk_event_levels_dev', 10), ('nvk_event_align_dev', 19)):
        m = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert m, '%s is not declared' % name
        params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == n_args
        for p, a in zip(params, args):
            want = C.c_void_p if '*' in p else C.c_int64 if p.startswith('int64_t') else \
                C.c_double if p.startswith('double') else C.c_int
            assert a is want, (name, p)
        assert hasattr(lib, name)
    for word, value in (('NVK_MAP_OK', _lib.MAP_OK), ('NVK_MAP_NO_EVENTS', _lib.MAP_NO_EVENTS),
                        ('NVK_MAP_LOST', _lib.MAP_LOST)):
        assert re.search(r'%s = %d\b' % (word, value), header)
    assert callable(device.event_flags_dev) and callable(device.event_levels_dev) and callable(device.event_align_dev)
    assert nadavca_amd.signal_map_batch is signal_map.signal_map_batch
    assert nadavca_amd.SignalMapBatch is signal_map.SignalMapBatch
    makefile = open(os.path.join(ROOT, 'nadavca_amd', 'csrc', 'Makefile')).read()
    assert 'kernels_events.hip' in makefile and 'kernels_eventalign.hip' in makefile


def test_from_signals_and_read_batch_round_trip(quality):
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.signal_map import SignalMapBatch
    rb, _, _, plain, _ = quality
    bare = ReadBatch.from_signals(rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off)
    assert bare.n == rb.n and bare.map_base.size == 0 and bare.map_sig.size == 0
    assert bare.map_off.tolist() == [0] * (rb.n + 1)
    assert bare.raw_signal.dtype == rb.raw_signal.dtype and np.array_equal(bare.raw_signal, rb.raw_signal)
    assert np.array_equal(bare.sequence, rb.sequence) and np.array_equal(bare.seq_off, rb.seq_off)
    with pytest.raises(ValueError):
        ReadBatch.from_signals(rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off[:-1])
    sm = SignalMapBatch(plain['status'], plain['n_events'], plain['path_score'], plain['shift'], plain['scale'],
                        plain['first_event'], plain['last_event'], plain['map_base'], plain['map_sig'],
                        plain['map_off'])
    out = sm.read_batch(bare)
    assert out is not bare and out.n == rb.n and sm.n_mapped == rb.n
    assert out.map_base.dtype == np.int32 and out.map_sig.dtype == np.int32 and out.map_off.dtype == np.int64
    assert np.array_equal(out.map_base, plain['map_base']) and np.array_equal(out.map_sig, plain['map_sig'])
    assert np.array_equal(out.map_off, plain['map_off']) and np.array_equal(out.raw_signal, rb.raw_signal)
    with pytest.raises(ValueError):
        sm.read_batch(ReadBatch.from_signals(rb.raw_signal[:10], [0, 10], rb.sequence[:4], [0, 4]))
