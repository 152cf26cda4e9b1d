"""refine_alignment around its sweeps: the planner writes the RowParam table only for the exact kernel, the launch
order is counted in LDS, and the host sets up the sweeps while the planner runs (csrc/kernels_plan.hip, csrc/api.hip).

* a read the fast kernel hands to the exact kernel is served although its batch was planned without the table, also
  after another batch has left other rows in the workspace, and also when it is planned in global scratch;
* NADAVCA_ALIGN_KERNEL=1, which plans with the table, gives what the default path gives;
* the sizes at which the planner changes path, alone and mixed;
* the order kernels at their block edges (256 reads per block), reads without a plan among them.

Everything is compared with the CPU oracle, read by read."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_cases
from conftest import ROOT
from fuzz_cases import make_fuzz_batch, reads_of

pytestmark = pytest.mark.gpu

READ_BAD_BAND = -2
SHARP = (11, 4230)   # tests/dev/fuzz_parity.py seed, iteration: the batch of test_gpu_edge_cases whose sharp-model read
                     # is handed to the exact kernel
# tests/plan_cases.py: T = 2 R <= 64, just above, T = PLAN_VT, and R + 1 above PLAN_BCAP (planned in global scratch)
SHAPES = ('trans_R32', 'trans_R33', 'trans_R1024', 'trans_R1025', 'plain_R63', 'plain_R64', 'plain_R1024')


@pytest.fixture(scope='module')
def dtw():
    from nadavca_amd import dtw as d
    return d


def _oracle_events(oracle, mo, c, bw, mel, tr):
    return oracle.refine_alignment(c['signal'], c['reference'], c['context_before'], c['context_after'],
                                   c['approximate_alignment'], bw, mel, mo, tr)


def _dev_run(dtw, ctx_model, cases, bw, mel, tr):
    """One nvk_refine_alignment_batch_dev call on the model's own context -> (events per read, status,
    reads_redone_exact).  (The host-pointer entry points hand a batch to lanes with contexts of their own.)"""
    import torch
    from nadavca_amd.device import DeviceBatch, refine_alignment_dev
    flat = dtw.FlatBatch(reads_of(cases))
    db = DeviceBatch(flat, torch.device('cuda', ctx_model.context.device))
    ev, st = refine_alignment_dev(db, bw, mel, ctx_model, tr)
    ev, st = ev.cpu().numpy(), st.cpu().numpy()
    redone = int(ctx_model.context.last_batch_stats()['reads_redone_exact'])
    none = np.zeros((0, 2), dtype=np.int32)   # (no path in the band: the reference returns no events either)
    return [ev[flat.ref_off[j]:flat.ref_off[j + 1]] if st[j] == 0 else none for j in range(flat.n)], st, redone


def _sharp_batch():
    fb = make_fuzz_batch(*SHARP)
    return fb, dict(bw=fb['bw'], mel=fb['mel'], tr=fb['tr'])


@pytest.fixture(scope='module')
def sharp(oracle_port):
    """The sharp-model batch, a long read and two short ones drawn with its model and settings, and the oracle's
    events of all of them (computed once)."""
    from nadavca_amd import synthetic
    fb, kw = _sharp_batch()
    mo = oracle_port.KmerModel(*fb['model'])
    mel = fb['mel']
    extra = [synthetic.make_dp_case(np.random.default_rng([20261019, i]), fb['model'], R=R, bandwidth=fb['bw'],
                                    dwell=(max(mel, 1), max(mel, 1) + 3), noise=0.35, jitter=4, trim=3)
             for i, R in enumerate((plan_cases.PLAN_BCAP + 6, 20, 70))]
    cases = fb['cases'] + extra
    want = [_oracle_events(oracle_port, mo, c, kw['bw'], kw['mel'], kw['tr']) for c in cases]
    return dict(fb=fb, kw=kw, cases=cases, want=want, n_fuzz=len(fb['cases']))


def _same(got, want):
    return len(got) == len(want) and all((len(g) == 0 and len(w) == 0) or np.array_equal(g, w)
                                         for g, w in zip(got, want))


def test_retry_after_a_plan_without_the_row_table(dtw, oracle_port, sharp):
    """The fast kernel hands the sharp-model read on; its batch was planned without the table, which is made then.
    A batch of other reads and more rows that needs no retry follows on the same context — a table left by the first
    batch would now belong to other reads — and then the first batch again."""
    from nadavca_amd import synthetic, _lib
    ctx = _lib.Context(0)
    fb, kw, n = sharp['fb'], sharp['kw'], sharp['n_fuzz']
    ms = dtw.KmerModel(*fb['model'], context=ctx)
    model = synthetic.load_model_arrays()
    mg, mo = dtw.KmerModel(*model, context=ctx), oracle_port.KmerModel(*model)
    other = synthetic.make_batch(12, model, seed=20261020, R=150, R_spread=30, bandwidth=40).cases
    assert sum(len(c['reference']) for c in other) > sum(len(c['reference']) for c in fb['cases'])
    other_want = [_oracle_events(oracle_port, mo, c, 40, 2, True) for c in other]
    for rnd in range(2):
        got, st, redone = _dev_run(dtw, ms, sharp['cases'][:n], kw['bw'], kw['mel'], kw['tr'])
        print('round %d: reads_redone_exact %d of %d' % (rnd, redone, n))
        assert redone >= 1
        assert _same(got, sharp['want'][:n]), rnd
        if rnd == 0:
            got, st, redone = _dev_run(dtw, mg, other, 40, 2, True)
            assert redone == 0 and not st.any()
            assert _same(got, other_want)


def test_retry_in_a_batch_with_a_read_planned_in_global_scratch(dtw, sharp):
    """The sharp-model reads beside a read of more than PLAN_BCAP band rows (its bands planned in global scratch; its
    rows, like a short read's, written only on request) and two short ones, twice on one context: the pass that
    makes the table for the exact kernel goes over a batch that holds both kinds of read.  (The long read itself is
    not the one that retries: neither plan_cases nor fuzz_cases makes a read of that length that does, and searching
    seeds for one costs an oracle run of a 1000-base read each.  The exact kernel reads a long read's rows in
    test_the_exact_kernel_equals_the_default_path.)"""
    from nadavca_amd import _lib
    ctx = _lib.Context(0)
    fb, kw = sharp['fb'], sharp['kw']
    ms = dtw.KmerModel(*fb['model'], context=ctx)
    assert len(sharp['cases'][sharp['n_fuzz']]['reference']) + 1 > plan_cases.PLAN_BCAP
    for rnd in range(2):
        got, st, redone = _dev_run(dtw, ms, sharp['cases'], kw['bw'], kw['mel'], kw['tr'])
        print('round %d: reads_redone_exact %d of %d' % (rnd, redone, len(sharp['cases'])))
        assert redone >= 1
        assert _same(got, sharp['want']), rnd


@pytest.fixture(scope='module')
def shape_cases():
    by_name = {c['name']: c for c in plan_cases.build_cases()}
    cases = [by_name[n] for n in SHAPES]
    # a read of more than PLAN_BCAP band rows with short ones, once per row layout
    for tr, names in ((True, ('trans_R1', 'trans_R1025', 'trans_R33', 'trans_R129')),
                      (False, ('plain_R63', 'plain_R1024', 'plain_R252'))):
        reads = [by_name[n]['reads'][0] for n in names]
        cases.append(dict(name='long_with_short_%s' % ('trans' if tr else 'plain'), model=plan_cases.BASE,
                          bandwidth=30, mel=2, transitions=tr, reads=reads, bad=()))
    assert max(len(r['reference']) for c in cases for r in c['reads']) + 1 > plan_cases.PLAN_BCAP
    return cases


_shape_want = {}


def _shape_oracle(oracle, mo, case):
    if case['name'] not in _shape_want:
        _shape_want[case['name']] = [_oracle_events(oracle, mo, c, case['bandwidth'], case['mel'], case['transitions'])
                                     for c in case['reads']]
    return _shape_want[case['name']]


def _run_shapes(dtw, cases):
    """-> {case name: (events per read, status)} through the host-pointer entry point, one model for all."""
    mg = dtw.KmerModel(*plan_cases.model_arrays(plan_cases.BASE))
    out = {}
    for case in cases:
        ev, st, _ = plan_cases.run_case(dtw, case, mg)
        out[case['name']] = (ev, st)
    return out


def test_the_sizes_at_which_the_planner_changes_path(dtw, oracle_port, shape_cases):
    """T <= 64 (no offsets pass), just above, T = PLAN_VT, a read above PLAN_BCAP (global scratch), and batches that
    mix such a read with short ones: planned without the row table, every read as the oracle has it."""
    mo = oracle_port.KmerModel(*plan_cases.model_arrays(plan_cases.BASE))
    got = _run_shapes(dtw, shape_cases)
    for case in shape_cases:
        ev, st = got[case['name']]
        assert not np.asarray(st).any(), case['name']
        assert _same(ev, _shape_oracle(oracle_port, mo, case)), case['name']


def _child_dump(path):
    """(child process of test_the_exact_kernel_equals_the_default_path) the shape cases and the sharp-model batch
    -> an .npz of every read's events and status."""
    from nadavca_amd import dtw
    out = {}
    by_name = {c['name']: c for c in plan_cases.build_cases()}
    cases = [by_name[n] for n in SHAPES]
    for name, (ev, st) in _run_shapes(dtw, cases).items():
        for i, e in enumerate(ev):
            out['%s/%d' % (name, i)] = e
        out['%s/status' % name] = np.asarray(st)
    fb, kw = _sharp_batch()
    ev, st = dtw.refine_alignment_batch(reads_of(fb['cases']), kw['bw'], kw['mel'], dtw.KmerModel(*fb['model']),
                                        kw['tr'], on_error='status', return_status=True)
    for i, e in enumerate(ev):
        out['sharp/%d' % i] = e
    out['sharp/status'] = np.asarray(st)
    np.savez(path, **out)


def test_the_exact_kernel_equals_the_default_path(dtw, oracle_port, shape_cases, sharp, tmp_path):
    """NADAVCA_ALIGN_KERNEL=1 plans with the row table and sends every read to the exact kernel; the variable is read
    at call time, so the batches run in a fresh child process that has it set from the start.  Its events and
    statuses equal the default path's (and so the oracle's: the tests above)."""
    path = str(tmp_path / 'exact.npz')
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")\n'
            'import test_gpu_plan_fastpath as t\n'
            't._child_dump(%r)\n'
            'print("EXACT-PATH-OK")\n' % (ROOT, ROOT, path))
    env = dict(os.environ, NADAVCA_ALIGN_KERNEL='1')
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and 'EXACT-PATH-OK' in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    exact = np.load(path)
    singles = [c for c in shape_cases if c['name'] in SHAPES]
    default = _run_shapes(dtw, singles)
    for case in singles:
        ev, st = default[case['name']]
        assert np.array_equal(exact['%s/status' % case['name']], st), case['name']
        for i, e in enumerate(ev):
            assert np.array_equal(exact['%s/%d' % (case['name'], i)], e), (case['name'], i)
    fb, kw = sharp['fb'], sharp['kw']
    ev, st = dtw.refine_alignment_batch(reads_of(fb['cases']), kw['bw'], kw['mel'], dtw.KmerModel(*fb['model']),
                                        kw['tr'], on_error='status', return_status=True)
    assert np.array_equal(exact['sharp/status'], st)
    for i, e in enumerate(ev):
        assert np.array_equal(exact['sharp/%d' % i], e), ('sharp', i)


# ------------------------------------------------------------------------------------------------------------------
# the order kernels
# ------------------------------------------------------------------------------------------------------------------
ORDER_BW, ORDER_MEL = 10, 2


@pytest.fixture(scope='module')
def tiny_pool(dtw, oracle_port):
    """48 tiny reads (12-40 bases, two to nine samples per base: step counts from ~40 to ~350, so many buckets of the
    launch order fill), two of them with an empty band, each aligned ALONE once: (cases, events, status, model)."""
    from nadavca_amd import synthetic
    model = synthetic.synth_model_arrays(20261021, k=4, central=1)
    mg, mo = dtw.KmerModel(*model), oracle_port.KmerModel(*model)
    cases = []
    for i in range(48):
        rng = np.random.default_rng([20261021, i])
        lo = int(rng.integers(2, 7))
        cases.append(synthetic.make_dp_case(rng, model, R=int(rng.integers(12, 41)), bandwidth=ORDER_BW,
                                            dwell=(lo, lo + 3), jitter=2, trim=3))
    for i in (5, 29):   # two anchors far apart with their samples exchanged: the prefix maximum passes the suffix minimum
        anc = cases[i]['approximate_alignment'].copy()
        a, b = 1, len(anc) - 2
        assert int(anc[b][0]) - int(anc[a][0]) > 2 * ORDER_BW + 2
        anc[a, 0], anc[b, 0] = int(anc[b][0]), int(anc[a][0])
        cases[i] = dict(cases[i], approximate_alignment=anc)
        bs, be = oracle_port.bands(anc, len(cases[i]['reference']), len(cases[i]['signal']), ORDER_BW)
        assert np.any(be < bs)
    events, status = [], []
    for i, c in enumerate(cases):
        ev, st = dtw.refine_alignment_batch(reads_of([c]), ORDER_BW, ORDER_MEL, mg, True, on_error='status',
                                            return_status=True)
        events.append(ev[0])
        status.append(int(st[0]))
        if i in (5, 29):
            assert status[-1] == READ_BAD_BAND and len(ev[0]) == 0
        else:
            assert status[-1] == 0
            assert np.array_equal(ev[0], _oracle_events(oracle_port, mo, c, ORDER_BW, ORDER_MEL, True)), i
    assert len({len(c['signal']) // 16 for c in cases}) >= 8   # step counts spread over many buckets
    return cases, events, status, mg


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1025])
def test_order_kernels_at_their_block_edges(dtw, tiny_pool, n):
    """Batches of 1, 255, 256, 257 and 1025 tiny reads of mixed lengths — a block of the order kernels takes 256 —
    with reads that have no plan (an empty band) among them: the launch order must be a permutation with the step
    counts at their positions, or a read is swept twice, not at all, or in a spill slot of the wrong size.  Every
    read's events and status equal those of the same read aligned alone (which equal the oracle's: tiny_pool)."""
    cases, events, status, mg = tiny_pool
    pick = np.random.default_rng([20261022, n]).integers(0, len(cases), n)
    if n > 1:
        pick[n // 2], pick[n - 1] = 5, 29   # reads without a plan, one of them in the last, partial block
    ev, st = dtw.refine_alignment_batch(reads_of([cases[i] for i in pick]), ORDER_BW, ORDER_MEL, mg, True,
                                        on_error='status', return_status=True)
    assert [int(s) for s in st] == [status[i] for i in pick]
    for j, i in enumerate(pick):
        assert ev[j].shape == events[i].shape and np.array_equal(ev[j], events[i]), (j, int(i))
