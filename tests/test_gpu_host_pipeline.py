"""The pipelined host-pointer path (csrc/pipeline.hip) where it cuts a call into chunks and uses a lane again: every
chunked call must give, bit for bit, what ONE device-pointer call over the whole batch gives (nadavca_amd/device.py:
that call never touches pipeline.hip), and a sample of reads must equal the CPU oracle.  Chunking changes every read's
neighbours and the slot that serves it, so the comparison also sees state that leaks from one read into the next in
the persistent waves' LDS rings or row store.

The batch is tests/pipeline_cases.py: 1300 reads, 5 498 437 samples, two tiny reads in front, four refused reads in
four chunks.  The knobs NADAVCA_E2E_LANES / _CHUNKS / _GROWTH / _MIN_READS are set before a fresh context is made (the
lane count is read at a context's first host-pointer call); the ``schedules`` fixture gets the chunks of every setting
from the host build of csrc/pipe_plan.h and fails if a setting no longer chunks as the tests assume.

Lines of csrc/pipeline.hip each test guards:
  test_refine_chunked_equals_one_piece
      lane_submit: the rebased pack and the copies out of the caller's arrays at h.*_off[a]; j.out_events
      = out_events + 2 * ref_off[a], j.out_status = out_status + a, j.out_ties = out_ties + a; a chunk whose context
      and anchor arrays are all empty (growth 10: read 0 alone).  run_pipelined: lane_collect before lane_submit on a
      busy lane (5 chunks on 1, 2 and 3 lanes), the sums of lane_collect in last_batch_stats, the tie counts and
      ctx->ties_host behind last_tie_flags.
  test_log_likelihoods_chunked_equal_one_piece
      lane_submit: j.out_ll = out_ll + alphabet * ref_off[a] with alphabet 4 and 5; lane_run / lane_collect: the
      JOB_ELL branches (llb = total_ref * alphabet * 8).
  test_one_context_serves_growing_and_shrinking_calls, test_workspace_limit_set_before_and_after_the_lanes_exist
      nvk_grow of a lane's staging between calls and chunks, out_a holding events and then log-likelihoods, L.alphabet
      and L.model following the call's model; pipe_get: L.ctx->ws_limit = ctx->ws_limit; nvk_pipe_set_ws_limit.
  test_an_error_inside_a_lane_is_reported_and_leaves_no_lane_busy
      lane_run: j->err; lane_collect: L.busy = false on a failed job; run_pipelined: first_err / err_txt kept through
      the drain of every lane.
  test_stream_on_two_lanes_out_of_order_and_across_a_batch_call
      nvk_refine_alignment_submit on a busy lane -> collect_ticketed stores a verdict; nvk_refine_alignment_wait from
      the verdict table, out of order, twice, and for a ticket never given; run_pipelined delivering batches in flight
      before it resets the call's statistics."""
import ctypes as C

import numpy as np
import pytest

import pipeline_cases as pc
from pipe_plan_shim import build_shim, shim_schedule

pytestmark = pytest.mark.gpu

BW, MEL = pc.BANDWIDTH, pc.MEL
RTOL = ATOL = 1e-9
# (lanes, chunks, growth x 100) -> the chunks the fixture expects of pipe_plan.h for this batch
SETTINGS = {
    (2, 5, 200): pc.GROWTH2_CHUNKS,
    (1, 3, 100): [(0, 431), (431, 850), (850, 1300)],
    (3, 5, 1000): [(0, 1), (1, 2), (2, 13), (13, 126), (126, 1300)],
}
STATS = ('band_cells', 'wave_steps', 'reads_redone_exact', 'reads_tie_ambiguous', 'reads_tie_exact', 'reads_tie_near',
         'reads_tie_ulp')


@pytest.fixture(scope='module')
def dtw():
    from nadavca_amd import dtw as d
    return d


@pytest.fixture(scope='module')
def data(dtw):
    """per model: its arrays, the doctored reads and their flat batch"""
    from nadavca_amd import synthetic
    out = {}
    for key, model in (('6mer', synthetic.load_model_arrays()),
                       ('alphabet5', synthetic.synth_model_arrays(k=4, central=1, alphabet=5))):
        cases = pc.make_cases(model)
        flat = pc.flat_of(dtw, cases)
        assert flat.n == pc.N_READS and int(flat.sig_off[-1]) == pc.N_SAMPLES >= 5 << 20
        out[key] = dict(model=model, cases=cases, flat=flat)
    assert np.array_equal(out['6mer']['flat'].sig_off, out['alphabet5']['flat'].sig_off)
    return out


@pytest.fixture(scope='module')
def schedules(data, tmp_path_factory):
    """(lanes, chunks, growth x 100) -> [(lo, hi), ...] from the host build of csrc/pipe_plan.h"""
    lib = build_shim(tmp_path_factory.mktemp('pipe_plan'))
    sig_off = data['6mer']['flat'].sig_off
    got = {s: shim_schedule(lib, sig_off, s[1], s[2] / 100.0, 1) for s in SETTINGS}
    assert got == SETTINGS
    assert shim_schedule(lib, sig_off, 3, 2.0, 1024) == [(0, pc.N_READS)]     # the defaults leave it in one piece
    g2 = got[(2, 5, 200)]
    chunk_of = lambda i: [c for c, (lo, hi) in enumerate(g2) if lo <= i < hi][0]
    assert sorted(chunk_of(i) for i in pc.STATUS) == [1, 2, 3, 4]             # four refused reads, four chunks
    assert pc.BAD_CODE == g2[1][0] and pc.SWAPPED == g2[2][1] - 1 and pc.NO_PATH == g2[3][1] - 1
    assert got[(3, 5, 1000)][:2] == [(0, 1), (1, 2)] and pc.TINY == (0, 1)    # a tiny read alone
    for i in pc.TINY:
        c = data['6mer']['cases'][i]
        assert len(c['reference']) == 20 and not len(c['context_before']) and not len(c['context_after']) \
            and not len(c['approximate_alignment'])
    return got


class Reference:
    """The device-pointer calls on the whole batch, each computed once, on a context of their own."""

    def __init__(self, dtw, data):
        import torch
        from nadavca_amd import _lib
        from nadavca_amd.device import DeviceBatch
        self.dtw, self.data = dtw, data
        self.ctx = _lib.Context(0)
        self.dev = torch.device('cuda', 0)
        self.models = {k: dtw.KmerModel(*d['model'], context=self.ctx) for k, d in data.items()}
        self.batches = {k: DeviceBatch(d['flat'], self.dev) for k, d in data.items()}
        self.cache = {}

    def refine(self, key, transitions):
        from nadavca_amd.device import refine_alignment_dev
        k = ('refine', key, bool(transitions))
        if k not in self.cache:
            ev, st = refine_alignment_dev(self.batches[key], BW, MEL, self.models[key], transitions)
            self.cache[k] = dict(events=ev.cpu().numpy(), status=st.cpu().numpy(),
                                 ties=self.ctx.last_tie_flags(pc.N_READS), stats=self.ctx.last_batch_stats())
        return self.cache[k]

    def ell(self, key, wobbling):
        from nadavca_amd.device import estimate_log_likelihoods_dev
        k = ('ell', key, bool(wobbling))
        if k not in self.cache:
            ll, st = estimate_log_likelihoods_dev(self.batches[key], BW, MEL, self.models[key], wobbling)
            self.cache[k] = dict(ll=ll.cpu().numpy(), status=st.cpu().numpy())
        return self.cache[k]


@pytest.fixture(scope='module')
def reference(dtw, data):
    return Reference(dtw, data)


_oracle_cache = {}


def _oracle(oracle, what, data, key, i, flag):
    """the CPU oracle's events / log-likelihoods of read i (each computed once)"""
    k = (what, key, i, bool(flag))
    if k not in _oracle_cache:
        mk = ('model', key)
        if mk not in _oracle_cache:
            _oracle_cache[mk] = oracle.KmerModel(*data[key]['model'])
        c = data[key]['cases'][i]
        fn = oracle.refine_alignment if what == 'refine' else oracle.estimate_log_likelihoods
        _oracle_cache[k] = np.asarray(fn(c['signal'], c['reference'], c['context_before'], c['context_after'],
                                         c['approximate_alignment'], BW, MEL, _oracle_cache[mk], flag))
    return _oracle_cache[k]


# A lane sizes its spill workspace for its share of 60 % of the free HBM (csrc/api.hip: nvk_spill_cap): tens of GB
# per fresh context, seconds to allocate and free.  The fresh contexts here are capped at 4 GiB a lane; results do not
# depend on the cap (fewer reads are resident, each wave serves more reads in turn).  The refine test at (2, 5, 200)
# runs without a cap.
WS_LIMIT = 4 << 30


def _fresh(dtw, monkeypatch, setting, models, data, ws_limit=WS_LIMIT):
    """-> (context, {key: KmerModel}) with the knobs of ``setting`` = (lanes, chunks, growth x 100) in force"""
    from nadavca_amd import _lib
    lanes, chunks, growth = setting
    monkeypatch.setenv('NADAVCA_E2E_LANES', str(lanes))
    monkeypatch.setenv('NADAVCA_E2E_CHUNKS', str(chunks))
    monkeypatch.setenv('NADAVCA_E2E_GROWTH', str(growth))
    monkeypatch.setenv('NADAVCA_E2E_MIN_READS', '1')
    ctx = _lib.Context(0)
    if ws_limit:
        ctx.set_workspace_limit(ws_limit)
    return ctx, {k: dtw.KmerModel(*data[k]['model'], context=ctx) for k in models}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_refine(ctx, got, want, n=pc.N_READS):
    events, status = got
    assert np.array_equal(status, want['status'])
    assert np.array_equal(events, want['events'])
    assert np.array_equal(ctx.last_tie_flags(n), want['ties'])
    stats = ctx.last_batch_stats()
    assert {k: stats[k] for k in STATS} == {k: want['stats'][k] for k in STATS}


def _check_doctored(status):
    for i, st in pc.STATUS.items():
        assert int(status[i]) == st, i
        assert int(status[i - 1]) == 0 and int(status[i + 1]) == 0, i
    assert int(np.count_nonzero(status)) == len(pc.STATUS)


@pytest.mark.parametrize('transitions', [True, False], ids=['trans', 'plain'])
@pytest.mark.parametrize('setting', list(SETTINGS), ids=['lanes%d_chunks%d_growth%d' % s for s in SETTINGS])
def test_refine_chunked_equals_one_piece(dtw, data, schedules, reference, oracle_port, monkeypatch, setting,
                                         transitions):
    want = reference.refine('6mer', transitions)
    ctx, models = _fresh(dtw, monkeypatch, setting, ['6mer'], data,
                         ws_limit=0 if setting == (2, 5, 200) else WS_LIMIT)
    flat = data['6mer']['flat']
    events, status = dtw.refine_alignment_flat(flat, BW, MEL, models['6mer'], transitions, on_error='status')
    _check_refine(ctx, (events, status), want)
    _check_doctored(status)
    # the oracle on every 60th served read and on the neighbours of the refused ones
    sample = [i for i in range(0, pc.N_READS, 60) if status[i] == 0]
    assert len(sample) >= 20 and 0 in sample
    for i in sample + [j for i in pc.STATUS for j in (i - 1, i + 1)]:
        exp = _oracle(oracle_port, 'refine', data, '6mer', i, transitions)
        got = events[flat.ref_off[i]:flat.ref_off[i + 1]]
        assert got.shape == exp.shape and np.array_equal(got, exp), i
    assert len(_oracle(oracle_port, 'refine', data, '6mer', pc.NO_PATH, transitions)) == 0


@pytest.mark.parametrize('setting', [(2, 5, 200), (3, 5, 1000)], ids=['lanes2_chunks5_growth200',
                                                                      'lanes3_chunks5_growth1000'])
@pytest.mark.parametrize('key,wobbling', [('6mer', True), ('alphabet5', False)], ids=['6mer_wobbling', 'alphabet5'])
def test_log_likelihoods_chunked_equal_one_piece(dtw, data, schedules, reference, oracle_port, monkeypatch, setting,
                                                 key, wobbling):
    want = reference.ell(key, wobbling)
    ctx, models = _fresh(dtw, monkeypatch, setting, [key], data)
    flat = data[key]['flat']
    ll, status = dtw.estimate_log_likelihoods_flat(flat, BW, MEL, models[key], wobbling, on_error='status')
    assert ll.shape == (int(flat.ref_off[-1]), data[key]['model'][2]) == want['ll'].shape
    assert np.array_equal(status, want['status'])
    _check_doctored(status)
    differ = np.nonzero((_bits(ll) != _bits(want['ll'])).any(axis=1))[0]
    assert differ.size == 0, 'rows %s of %d differ from the one-piece call' % (differ[:5], len(ll))
    # the oracle on the first served read of at most 150 bases in each of chunks 1 to 4 of the growth-2 schedule
    R = np.diff(flat.ref_off)
    sample = [next(i for i in range(lo, hi) if status[i] == 0 and R[i] <= 150) for lo, hi in pc.GROWTH2_CHUNKS[1:]]
    for i in sample:
        exp = _oracle(oracle_port, 'ell', data, key, i, wobbling)
        got = ll[flat.ref_off[i]:flat.ref_off[i + 1]]
        assert got.shape == exp.shape
        assert np.array_equal(np.isneginf(got), np.isneginf(exp)) and not np.any(np.isnan(got))
        fin = np.isfinite(exp)
        assert np.allclose(got[fin], exp[fin], rtol=RTOL, atol=ATOL), float(np.max(np.abs(got[fin] - exp[fin])))


def _slice_of(want, flat, lo, hi, field):
    per = flat.ref_off if field in ('events', 'll') else np.arange(flat.n + 1)
    return want[field][per[lo]:per[hi]]


def test_one_context_serves_growing_and_shrinking_calls(dtw, data, schedules, reference, monkeypatch):
    ctx, models = _fresh(dtw, monkeypatch, (2, 5, 200), ['6mer', 'alphabet5'], data)
    want_r, want_l = reference.refine('6mer', True), reference.ell('alphabet5', False)
    f6, f5 = data['6mer']['flat'], data['alphabet5']['flat']
    # a 40-read refine: small staging, out_a holds events
    events, status = dtw.refine_alignment_flat(pc.flat_of(dtw, data['6mer']['cases'], 0, 40), BW, MEL, models['6mer'],
                                               True, on_error='status')
    assert np.array_equal(events, _slice_of(want_r, f6, 0, 40, 'events'))
    assert np.array_equal(status, _slice_of(want_r, f6, 0, 40, 'status'))
    assert np.array_equal(ctx.last_tie_flags(40), _slice_of(want_r, f6, 0, 40, 'ties'))
    # the full log-likelihood call, five columns: every staging buffer grows, out_a holds doubles
    ll, status = dtw.estimate_log_likelihoods_flat(f5, BW, MEL, models['alphabet5'], False, on_error='status')
    assert np.array_equal(_bits(ll), _bits(want_l['ll'])) and np.array_equal(status, want_l['status'])
    # 40 reads again, the bad code among them: the staging is larger than the call
    ll, status = dtw.estimate_log_likelihoods_flat(pc.flat_of(dtw, data['alphabet5']['cases'], 20, 60), BW, MEL,
                                                   models['alphabet5'], False, on_error='status')
    assert np.array_equal(_bits(ll), _bits(_slice_of(want_l, f5, 20, 60, 'll')))
    assert np.array_equal(status, _slice_of(want_l, f5, 20, 60, 'status')) and status[pc.BAD_CODE - 20] == -1
    # the full refine: out_a holds events again, the other model
    got = dtw.refine_alignment_flat(f6, BW, MEL, models['6mer'], True, on_error='status')
    _check_refine(ctx, got, want_r)


def test_workspace_limit_set_before_and_after_the_lanes_exist(dtw, data, schedules, reference, monkeypatch):
    want = reference.refine('6mer', True)
    flat = data['6mer']['flat']
    # before the context's first host-pointer call: the lanes inherit it when they are made
    ctx, models = _fresh(dtw, monkeypatch, (2, 5, 200), ['6mer'], data, ws_limit=0)
    ctx.set_workspace_limit(32 << 20)
    _check_refine(ctx, dtw.refine_alignment_flat(flat, BW, MEL, models['6mer'], True, on_error='status'), want)
    # after it: nvk_pipe_set_ws_limit hands it to the lanes that exist
    ctx2, models2 = _fresh(dtw, monkeypatch, (2, 5, 200), ['6mer'], data, ws_limit=0)
    small = pc.flat_of(dtw, data['6mer']['cases'], 0, 40)
    dtw.refine_alignment_flat(small, BW, MEL, models2['6mer'], True, on_error='status')
    ctx2.set_workspace_limit(32 << 20)
    _check_refine(ctx2, dtw.refine_alignment_flat(flat, BW, MEL, models2['6mer'], True, on_error='status'), want)


def test_an_error_inside_a_lane_is_reported_and_leaves_no_lane_busy(dtw, data, schedules, reference, monkeypatch):
    from nadavca_amd import synthetic, _lib
    ctx, models = _fresh(dtw, monkeypatch, (2, 5, 200), ['6mer'], data)
    # a table the log-likelihood kernel is not compiled for (k + 2 lanes per hypothesis, 16 at most); the signals
    # are those of the big batch, the base codes folded into its two letters
    wide_model = dtw.KmerModel(*synthetic.synth_model_arrays(3, k=15, central=7, alphabet=2), context=ctx)
    f = data['6mer']['flat']
    folded = dtw.FlatBatch.from_arrays(f.signal, f.sig_off, f.reference % 2, f.ref_off, f.context_before % 2, f.cb_off,
                                       f.context_after % 2, f.ca_off, f.anchors, f.anc_off)
    with pytest.raises(_lib.NadavcaHipError, match='k-mer size 15'):
        dtw.estimate_log_likelihoods_flat(folded, BW, MEL, wide_model, True, on_error='status')
    got = dtw.refine_alignment_flat(f, BW, MEL, models['6mer'], True, on_error='status')
    _check_refine(ctx, got, reference.refine('6mer', True))


def test_stream_on_two_lanes_out_of_order_and_across_a_batch_call(dtw, data, schedules, monkeypatch):
    from nadavca_amd import _lib
    lib = _lib.load()
    ctx, models = _fresh(dtw, monkeypatch, (2, 5, 200), ['6mer'], data)
    m = models['6mer']
    cases = data['6mer']['cases']
    # 80, 20, 120, 60 and 100 reads (the first holds the tiny reads and the bad code), and a sixth for the batch call
    bounds = [(0, 80), (80, 100), (100, 220), (220, 280), (300, 400), (600, 640)]
    assert bounds[0][0] <= pc.BAD_CODE < bounds[0][1] and bounds[5][0] <= pc.NO_PATH < bounds[5][1]
    flats = [pc.flat_of(dtw, cases, lo, hi) for lo, hi in bounds]
    want = []
    for f in flats:
        ev, st = dtw.refine_alignment_flat(f, BW, MEL, m, True, on_error='status')
        want.append((ev, st, ctx.last_tie_flags(f.n), ctx.last_batch_stats()))
    assert want[0][1][pc.BAD_CODE] == -1 and np.count_nonzero(want[0][1]) == 1
    rs = dtw.RefineStream(m, BW, MEL, True)
    got = {}
    t = [rs.submit(flats[0]), rs.submit(flats[1])]
    t.append(rs.submit(flats[2]))            # lane 0 is busy with ticket 0: collected here, its verdict kept
    assert t == [0, 1, 2]
    for i in (2, 0, 1):
        got[i] = rs.wait(t[i])
    t += [rs.submit(flats[3]), rs.submit(flats[4])]
    ev, st = dtw.refine_alignment_flat(flats[5], BW, MEL, m, True, on_error='status')   # delivers tickets 3 and 4
    stats = ctx.last_batch_stats()
    assert np.array_equal(ev, want[5][0]) and np.array_equal(st, want[5][1])
    assert np.array_equal(ctx.last_tie_flags(flats[5].n), want[5][2])
    assert {k: stats[k] for k in STATS} == {k: want[5][3][k] for k in STATS}
    for i in (4, 3):
        got[i] = rs.wait(t[i])
    for i in range(5):
        for a, b in zip(got[i], want[i][:3]):
            assert np.array_equal(a, b), i
    assert np.array_equal(ctx.last_tie_flags(flats[5].n), want[5][2])      # a submit or a wait is not a batch call
    for ticket, text in ((t[0], b'ticket 0 was already waited for'), (t[4], b'ticket 4 was already waited for'),
                         (99, b'no such ticket'), (-1, b'no such ticket')):
        assert lib.nvk_refine_alignment_wait(m.handle, C.c_int64(ticket)) == _lib.NVK_ERR_INVALID
        assert text in lib.nvk_last_error()
