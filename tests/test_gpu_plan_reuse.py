"""refine_alignment plans a resident batch once: a DeviceBatch carries a token (include/nadavca_hip.h: plan once, sweep
again), and a call whose token, settings and addresses equal the plan its context holds launches no planner and asks
nothing of the device before its sweeps (csrc/api.hip, csrc/plan_key.h).

Every batch is compared read by read with the CPU oracle.  Where a call that reused stands beside one that planned, the
two are compared byte for byte: events, status, nvk_last_tie_flags, last_batch_stats, last_launches and
last_read_skews.  The key comparison alone is tests/test_plan_key_cpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_cases
import variant_cases
from conftest import ROOT
from fuzz_cases import make_fuzz_batch, reads_of

pytestmark = pytest.mark.gpu

READ_OK, READ_NO_PATH, READ_BAD_BAND = 0, 1, -2
SHARP = (11, 4230)   # the batch of tests/test_gpu_plan_fastpath.py whose sharp-model read goes to the exact kernel
BW, MEL = 30, 2      # the settings of the plan_cases shapes
EMPTY = np.zeros((0, 2), dtype=np.int32)


@pytest.fixture(scope='module')
def dtw():
    from nadavca_amd import dtw as d
    return d


def _no_path_read():
    """Fewer samples than two per base: no path at min event length 2, for the reference as well."""
    rng = np.random.default_rng(20261101)
    return dict(signal=rng.normal(0, 1, 30), reference=rng.integers(0, 4, 20).astype(np.int32),
                context_before=np.zeros(0, np.int32), context_after=np.zeros(0, np.int32),
                approximate_alignment=np.array([[0, 0], [29, 19]], dtype=np.int32))


def _reads(names):
    """plan_cases reads by the names of their one-read cases, then a read with a bad band (two anchors out of order) and
    a read with no path."""
    by_name = {c['name']: c for c in plan_cases.build_cases()}
    return [by_name[n]['reads'][0] for n in names] + [by_name['anchors_out_of_order']['reads'][0], _no_path_read()]


MIXED_TRANS = ('trans_R32', 'trans_R33', 'trans_R1025')   # (R + 1 above PLAN_BCAP: planned in global scratch)
MIXED_PLAIN = ('plain_R63', 'plain_R64', 'plain_R1024')
SMALL = ('trans_R32', 'trans_R33', 'trans_R129')

_want = {}


def _oracle(oracle, model, cases, bw, mel, tr, tag):
    """The oracle's events per read ([] for the read with the bad band, which the reference refuses), once per tag."""
    if tag not in _want:
        mo = oracle.KmerModel(*model)
        out = []
        for c in cases:
            bs, be = oracle.bands(c['approximate_alignment'], len(c['reference']), len(c['signal']), bw)
            out.append(None if np.any(be < bs) else
                       oracle.refine_alignment(c['signal'], c['reference'], c['context_before'], c['context_after'],
                                               c['approximate_alignment'], bw, mel, mo, tr))
        _want[tag] = out
    return _want[tag]


def _device_batch(dtw, cases, device=0):
    import torch
    from nadavca_amd.device import DeviceBatch
    flat = dtw.FlatBatch(reads_of(cases))
    return DeviceBatch(flat, torch.device('cuda', device)), flat


def _call(db, km, bw, mel, tr):
    """One refine_alignment_dev call with fresh output tensors -> everything a caller can see of it."""
    from nadavca_amd.device import refine_alignment_dev
    ctx = km.context
    ctx.timing_enable(True)
    ctx.timing_reset()
    ev, st = refine_alignment_dev(db, bw, mel, km, tr)
    plan_launches = ctx.timing_read()['plan'][1]
    ctx.timing_enable(False)
    c, cw = ctx.last_read_skews(db.n)
    return dict(events=ev.cpu().numpy(), status=st.cpu().numpy(), flags=ctx.last_tie_flags(db.n),
                stats=ctx.last_batch_stats(), launches=ctx.last_launches(), c=c, cw=cw,
                reused=ctx.last_plan_reused(), plan_launches=plan_launches)


def _planned(r):
    return not r['reused'] and r['plan_launches'] > 0


def _reused(r):
    return r['reused'] and r['plan_launches'] == 0


def _same_call(a, b):
    """Byte for byte what two calls left, whichever of them planned."""
    return (a['events'].tobytes() == b['events'].tobytes() and a['status'].tobytes() == b['status'].tobytes()
            and a['flags'].tobytes() == b['flags'].tobytes() and a['stats'] == b['stats']
            and a['launches'] == b['launches'] and a['c'].tobytes() == b['c'].tobytes()
            and a['cw'].tobytes() == b['cw'].tobytes())


def _equals_oracle(r, flat, want, rely=None):
    for j, w in enumerate(want):
        if rely is not None and j not in rely:
            continue
        st = int(r['status'][j])
        if w is None:
            if st != READ_BAD_BAND:
                return False
            continue
        if st != (READ_OK if len(w) else READ_NO_PATH):
            return False
        got = r['events'][flat.ref_off[j]:flat.ref_off[j + 1]] if st == READ_OK else EMPTY
        if len(w) and not np.array_equal(got, w):
            return False
    return True


def _base_model(dtw, ctx):
    return dtw.KmerModel(*plan_cases.model_arrays(plan_cases.BASE), context=ctx)


def _three_times(dtw, oracle, names, tr, tag):
    from nadavca_amd import _lib
    ctx = _lib.Context(0)
    km = _base_model(dtw, ctx)
    cases = _reads(names)
    want = _oracle(oracle, plan_cases.model_arrays(plan_cases.BASE), cases, BW, MEL, tr, tag)
    db, flat = _device_batch(dtw, cases)
    runs = [_call(db, km, BW, MEL, tr) for _ in range(3)]
    assert _planned(runs[0]) and _reused(runs[1]) and _reused(runs[2]), [(r['reused'], r['plan_launches']) for r in runs]
    assert sorted(int(s) for s in runs[0]['status']) == [READ_BAD_BAND, 0, 0, 0, READ_NO_PATH]
    for r in runs:
        assert _equals_oracle(r, flat, want)
        assert _same_call(r, runs[0])


def test_mixed_batch_three_times(dtw, oracle_port):
    """Reads of T <= 64, just above, and one planned in global scratch, a read with a bad band and a read with no path:
    the second and third call reuse, launch no planner, and leave what the first left, which the oracle has."""
    _three_times(dtw, oracle_port, MIXED_TRANS, True, 'mixed_trans')


def test_mixed_batch_three_times_plain_rows(dtw, oracle_port):
    _three_times(dtw, oracle_port, MIXED_PLAIN, False, 'mixed_plain')


def test_signal_changed_in_place(dtw, oracle_port):
    """Between two calls every read's signal is rescaled in place (a x + b, another pair per read), as the renorm loop
    does: the second call reuses the plan, equals the oracle on the new signal and a fresh DeviceBatch of it."""
    import torch
    from nadavca_amd import _lib
    ctx = _lib.Context(0)
    km = _base_model(dtw, ctx)
    model = plan_cases.model_arrays(plan_cases.BASE)
    cases = _reads(SMALL)
    db, flat = _device_batch(dtw, cases)
    first = _call(db, km, BW, MEL, True)
    assert _planned(first) and _equals_oracle(first, flat, _oracle(oracle_port, model, cases, BW, MEL, True, 'small'))
    rng = np.random.default_rng(20261102)
    a, b = rng.uniform(0.9, 1.1, flat.n), rng.uniform(-0.2, 0.2, flat.n)
    per_sample = lambda v: torch.from_numpy(np.repeat(v, np.diff(flat.sig_off))).to(db.device)
    db.signal.mul_(per_sample(a)).add_(per_sample(b))
    new_signal = db.signal.cpu().numpy()
    rescaled = [dict(c, signal=new_signal[flat.sig_off[j]:flat.sig_off[j + 1]].copy()) for j, c in enumerate(cases)]
    second = _call(db, km, BW, MEL, True)
    assert _reused(second)
    assert _equals_oracle(second, flat, _oracle(oracle_port, model, rescaled, BW, MEL, True, 'small_rescaled'))
    assert second['events'].tobytes() != first['events'].tobytes()   # (the rescaled signal does move events)
    fresh_db, fresh_flat = _device_batch(dtw, rescaled)
    assert np.array_equal(fresh_db.signal.cpu().numpy(), new_signal)
    fresh = _call(fresh_db, km, BW, MEL, True)
    assert _planned(fresh) and _same_call(fresh, second)


def test_retry_on_a_reused_plan(dtw, oracle_port):
    """The sharp-model batch twice: the fast kernel hands a read on, the row table is made for the exact kernel; the
    second call reuses the plan (and the table), redoes the same reads and equals the oracle."""
    from nadavca_amd import _lib
    fb = make_fuzz_batch(*SHARP)
    ctx = _lib.Context(0)
    km = dtw.KmerModel(*fb['model'], context=ctx)
    want = _oracle(oracle_port, fb['model'], fb['cases'], fb['bw'], fb['mel'], fb['tr'], 'sharp')
    db, flat = _device_batch(dtw, fb['cases'])
    first, second = (_call(db, km, fb['bw'], fb['mel'], fb['tr']) for _ in range(2))
    assert _planned(first) and _reused(second)
    assert first['stats']['reads_redone_exact'] >= 1
    assert second['stats']['reads_redone_exact'] == first['stats']['reads_redone_exact']
    assert _equals_oracle(first, flat, want) and _equals_oracle(second, flat, want)
    assert _same_call(first, second)
    assert [l['op'] for l in second['launches']].count('exact') >= 1


def test_every_invalidation(dtw, oracle_port):
    """Whatever overwrites the held plan, or asks for another one, makes the next call plan again — and that call and
    the reused one after it are still what the first call left."""
    from nadavca_amd import _lib
    from nadavca_amd.device import estimate_log_likelihoods_dev
    ctx = _lib.Context(0)
    km = _base_model(dtw, ctx)
    model = plan_cases.model_arrays(plan_cases.BASE)
    cases = _reads(SMALL)
    want = _oracle(oracle_port, model, cases, BW, MEL, True, 'small')
    # a first batch small enough that the next one grows the workspaces
    tiny_db, tiny_flat = _device_batch(dtw, cases[:1])
    tiny = _call(tiny_db, km, BW, MEL, True)
    assert _planned(tiny) and _equals_oracle(tiny, tiny_flat, want[:1])
    db, flat = _device_batch(dtw, cases)
    ref = _call(db, km, BW, MEL, True)
    assert _planned(ref) and _equals_oracle(ref, flat, want)

    def plans_again_then_reuses(what):
        again, then = _call(db, km, BW, MEL, True), _call(db, km, BW, MEL, True)
        assert _planned(again), what
        assert _reused(then), what
        assert _same_call(again, ref) and _same_call(then, ref), what

    assert _reused(_call(db, km, BW, MEL, True))
    # another DeviceBatch of the same shape with different reads (the same reads in another order), aligned in between
    other_cases = cases[::-1]
    other_db, other_flat = _device_batch(dtw, other_cases)
    assert (other_db.n, other_db.total_signal, other_db.total_ref, other_db.total_anchors) == \
        (db.n, db.total_signal, db.total_ref, db.total_anchors)
    other = _call(other_db, km, BW, MEL, True)
    assert _planned(other) and _equals_oracle(other, other_flat, want[::-1])
    plans_again_then_reuses('another batch in between')
    estimate_log_likelihoods_dev(db, BW, MEL, km, True)
    plans_again_then_reuses('estimate_log_likelihoods in between')
    # another bandwidth, min event length, row layout or model: planned, correct, and the plan held is then that one's
    k2 = plan_cases.model_arrays(plan_cases.K2)
    km2 = dtw.KmerModel(*k2, context=ctx)
    for what, (m_arrays, m, bw, mel, tr) in (('bandwidth', (model, km, BW + 1, MEL, True)),
                                             ('min_event_length', (model, km, BW, MEL + 1, True)),
                                             ('transitions', (model, km, BW, MEL, False)),
                                             ('model', (k2, km2, BW, MEL, True))):
        changed = _call(db, m, bw, mel, tr)
        assert _planned(changed), what
        assert _equals_oracle(changed, flat, _oracle(oracle_port, m_arrays, cases, bw, mel, tr, 'small_' + what)), what
        assert _reused(_call(db, m, bw, mel, tr)), what
        plans_again_then_reuses(what)
    token = db.plan_token
    db.geometry_changed()
    assert db.plan_token not in (0, token)
    plans_again_then_reuses('geometry_changed')
    db.anchors = db.anchors.clone()   # a geometry field replaced: a new token by itself
    plans_again_then_reuses('a geometry tensor replaced')


def test_same_shape_at_the_same_addresses(dtw, oracle_port):
    """A batch is aligned and deleted; the allocator hands the next batch of the same shape the same addresses.  Its
    totals and pointers equal the held key's, its contents do not: it is not served the first one's plan."""
    import torch
    from nadavca_amd import _lib
    ctx = _lib.Context(0)
    km = _base_model(dtw, ctx)
    model = plan_cases.model_arrays(plan_cases.BASE)
    cases = _reads(SMALL)
    want = _oracle(oracle_port, model, cases, BW, MEL, True, 'small')
    db, flat = _device_batch(dtw, cases)
    first = _call(db, km, BW, MEL, True)
    assert _planned(first) and _equals_oracle(first, flat, want)
    addresses = [p.value for p in db.pointers()]
    del db, first
    torch.cuda.synchronize()
    db2, flat2 = _device_batch(dtw, cases[::-1])
    assert [p.value for p in db2.pointers()] == addresses   # (what this test is about; torch's caching allocator)
    second = _call(db2, km, BW, MEL, True)
    assert _planned(second) and _equals_oracle(second, flat2, want[::-1])


def test_the_entry_point_without_a_token_never_reuses(dtw, oracle_port):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    ctx = _lib.Context(0)
    km = _base_model(dtw, ctx)
    cases = _reads(SMALL)
    want = _oracle(oracle_port, plan_cases.model_arrays(plan_cases.BASE), cases, BW, MEL, True, 'small')
    db, flat = _device_batch(dtw, cases)
    assert _planned(_call(db, km, BW, MEL, True))   # (a plan is held now)
    for _ in range(2):
        ev = torch.zeros((db.total_ref, 2), dtype=torch.int32, device=db.device)
        st = torch.zeros(db.n, dtype=torch.int32, device=db.device)
        _lib.check(lib.nvk_refine_alignment_batch_dev(
            km.handle, db.n, db.total_signal, db.total_ref, db.total_anchors, *db.pointers(), BW, MEL, 1,
            C.c_void_p(ev.data_ptr()), C.c_void_p(st.data_ptr())), 'nvk_refine_alignment_batch_dev')
        assert not ctx.last_plan_reused()
        assert _equals_oracle(dict(events=ev.cpu().numpy(), status=st.cpu().numpy()), flat, want)
    assert _planned(_call(db, km, BW, MEL, True))   # (... and the call without a token left none)


def test_team_path(dtw, oracle_port):
    """A wide-band read swept by a team of four waves, with its narrow company: twice, the second time reused."""
    from nadavca_amd import _lib
    case = next(c for c in variant_cases.team_cases() if c['name'] == 'team_mel2_trans_p16')
    ctx = _lib.Context(0)
    km = dtw.KmerModel(*case['model'], context=ctx)
    bw, mel, tr = case['bandwidth'], case['mel'], case['transitions']
    want = _oracle(oracle_port, case['model'], case['reads'], bw, mel, tr, case['name'])
    db, flat = _device_batch(dtw, case['reads'])
    first, second = _call(db, km, bw, mel, tr), _call(db, km, bw, mel, tr)
    assert _planned(first) and _reused(second) and _same_call(first, second)
    assert sorted(l['waves'] for l in second['launches'] if l['op'] == 'sweep') == [1, 4]
    assert second['stats']['reads_redone_exact'] == 0
    rely = set(case['rely']) | {len(case['reads']) - 1}
    assert _equals_oracle(first, flat, want, rely) and _equals_oracle(second, flat, want, rely)


def test_chunked_spill(dtw, oracle_port):
    """A workspace limit that cuts the batch's sweeps into several chunks, twice: the reused call cuts the same chunks
    from the step counts the pinned block still holds."""
    from nadavca_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_workspace_limit(256 << 10)
    km = _base_model(dtw, ctx)
    cases = _reads(SMALL)
    want = _oracle(oracle_port, plan_cases.model_arrays(plan_cases.BASE), cases, BW, MEL, True, 'small')
    db, flat = _device_batch(dtw, cases)
    first, second = _call(db, km, BW, MEL, True), _call(db, km, BW, MEL, True)
    assert _planned(first) and _reused(second) and _same_call(first, second)
    assert [l['chunks'] for l in second['launches'] if l['op'] == 'sweep'][0] >= 2
    assert _equals_oracle(first, flat, want) and _equals_oracle(second, flat, want)


# ------------------------------------------------------------------------------------------------------------------
# child processes: what an environment variable decides
# ------------------------------------------------------------------------------------------------------------------
def _loop_batch(dtw):
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    batch = synthetic.make_batch(6, model, seed=20261103, R=120, R_spread=10, bandwidth=60)
    return model, batch.cases


def _renorm_loop(dtw, path=None):
    """refine_renorm_loop_dev with three rounds (align, fit, align, fit) on a context of its own -> (arrays, the
    planner's timed launches, whether the last alignment reused); with ``path``, the arrays go into an .npz."""
    from nadavca_amd import _lib
    from nadavca_amd.device import refine_renorm_loop_dev
    model, cases = _loop_batch(dtw)
    ctx = _lib.Context(0)
    km = dtw.KmerModel(*model, context=ctx)
    db, _ = _device_batch(dtw, cases)
    ctx.timing_enable(True)
    ctx.timing_reset()
    events, status, fits = refine_renorm_loop_dev(db, 60, 2, km, True, 3)
    plan_launches = ctx.timing_read()['plan'][1]
    ctx.timing_enable(False)
    out = dict(events=events.cpu().numpy(), status=status.cpu().numpy(), signal=db.signal.cpu().numpy())
    for i, f in enumerate(fits):
        out['fit%d' % i] = f.cpu().numpy()
    if path:
        np.savez(path, **out)
    return out, plan_launches, ctx.last_plan_reused()


def _child_renorm_loop(path):
    from nadavca_amd import dtw
    out, plan_launches, reused = _renorm_loop(dtw, path)
    assert not reused
    print('PLAN-LAUNCHES %d' % plan_launches)


def _child_exact_switch(path):
    """NADAVCA_ALIGN_KERNEL is read at every call: default, =1, =1 again, default again on one batch."""
    from nadavca_amd import dtw, _lib
    ctx = _lib.Context(0)
    km = _base_model(dtw, ctx)
    db, flat = _device_batch(dtw, _reads(SMALL))
    out = {}
    for i, force in enumerate((None, '1', '1', None, None)):
        if force is None:
            os.environ.pop('NADAVCA_ALIGN_KERNEL', None)
        else:
            os.environ['NADAVCA_ALIGN_KERNEL'] = force
        r = _call(db, km, BW, MEL, True)
        out['events%d' % i], out['status%d' % i] = r['events'], r['status']
        out['reused%d' % i] = np.array([int(r['reused']), int(r['plan_launches'])])
        out['ops%d' % i] = np.array([l['op'] for l in r['launches']])
    np.savez(path, **out)


def _child(function, path, **env):
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")\n'
            'import test_gpu_plan_reuse as t\n'
            't.%s(%r)\n'
            'print("CHILD-OK")\n' % (ROOT, ROOT, function, path))
    p = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and 'CHILD-OK' in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_the_exact_kernel_switch_plans_again(dtw, oracle_port, tmp_path):
    """A plan made without the row table does not serve NADAVCA_ALIGN_KERNEL=1 and the other way round; within a mode
    the plan is reused.  In a child process, which sets the variable between its calls."""
    path = str(tmp_path / 'exact.npz')
    _child('_child_exact_switch', path)
    got = np.load(path)
    cases = _reads(SMALL)
    flat = dtw.FlatBatch(reads_of(cases))
    want = _oracle(oracle_port, plan_cases.model_arrays(plan_cases.BASE), cases, BW, MEL, True, 'small')
    assert [int(got['reused%d' % i][0]) for i in range(5)] == [0, 0, 1, 0, 1]
    assert [int(got['reused%d' % i][1]) > 0 for i in range(5)] == [True, True, False, True, False]
    for i in range(5):
        assert _equals_oracle(dict(events=got['events%d' % i], status=got['status%d' % i]), flat, want), i
        assert got['events%d' % i].tobytes() == got['events0'].tobytes()
        assert ('exact' in got['ops%d' % i] and 'sweep' not in got['ops%d' % i]) == (i in (1, 2)), i


def test_the_renorm_loop_plans_once(dtw, tmp_path):
    """refine_renorm_loop_dev with three rounds aligns twice, with the signal re-fitted in place in between: it plans
    once (the planner's and the order kernels' timed launches, one each) and reuses once.  Its events, status, fits and
    final signal are byte for byte those of a child process that runs it with NADAVCA_PLAN_REUSE=0."""
    out, plan_launches, reused = _renorm_loop(dtw)
    assert reused and plan_launches == 2
    assert (out['status'] == 0).all() and len(out) == 5   # (two fits)
    path = str(tmp_path / 'loop.npz')
    stdout = _child('_child_renorm_loop', path, NADAVCA_PLAN_REUSE='0')
    assert 'PLAN-LAUNCHES 4' in stdout
    off = np.load(path)
    assert sorted(off.files) == sorted(out)
    for name, a in out.items():
        assert a.dtype == off[name].dtype and a.tobytes() == off[name].tobytes(), name
