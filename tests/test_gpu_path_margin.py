"""The forward sweep's path comparison forms gt_tol's margin only where a tie is near (csrc/path_step.h; the arithmetic
itself: tests/test_path_step_cpu.py).  Here the sweeps run on 64 reads chosen so that every tie class occurs:

* 63 reads of 40-80 bases under a bandwidth of 20-30, min event length 0, 2 and 4, with and without transition rows
  (six batches of 10 or 11 reads);
* 16 of them on a homopolymer-rich reference with their signals quantised to ADC steps of 1/12 — equal samples make
  equal densities and path scores tie exactly or almost (tests/test_gpu_parity_full.py has the shape at full size);
* one read wide enough for a team of four waves, the smallest of tests/variant_cases.py (270 bases, bandwidth 280,
  min event length 2, no transition rows), in a batch of its own.

Events and statuses equal the exact kernel's (NADAVCA_ALIGN_KERNEL=1, read by the library at every call) on every read,
no read is handed on to it, and the per-read tie flags equal tests/golden/path_margin_ties.json, recorded by
tools/record_path_margin_ties.py with the library of the commit BEFORE the margin left the usual path (as
plan_totals.json was for the planner).  SEED was chosen there as the first of 0, 1, .. whose 64 reads hold each of
NVK_TIE_EXACT, NVK_TIE_ULP, NVK_TIE_NEAR and a read without any of them; the test fails if the fixture does not."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'path_margin_ties.json')
SEED = 10
TIE_EXACT, TIE_NEAR, TIE_ULP = 1, 2, 4   # include/nadavca_hip.h
N_READS = 64


def build_batches(seed=SEED):
    """-> [dict(name, model, bw, mel, tr, cases)]: the seven batches."""
    import variant_cases
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    out = []
    for b, (mel, tr) in enumerate((m, t) for t in (False, True) for m in (0, 2, 4)):
        rng = np.random.default_rng([20261020, seed, b])
        bw = int(rng.integers(20, 31))
        n, n_runs = (11, 3) if b < 3 else (10, 3 if b == 3 else 2)     # 63 reads, 16 of them run-rich and quantised
        cases = []
        for i in range(n):
            c = synthetic.make_dp_case(rng, model, R=int(rng.integers(40, 81)), bandwidth=bw, dwell=(max(mel, 1), 9),
                                       jitter=6, anchor_density=float(rng.uniform(0.1, 0.9)), with_context=bool(i % 3),
                                       bases=synthetic.homopolymer_rich if i < n_runs else None)
            if i < n_runs:
                c['signal'] = np.round(c['signal'] * 12.0) / 12.0
            cases.append(c)
        out.append(dict(name='mel%d_%s_bw%d' % (mel, 'trans' if tr else 'plain', bw), model=model, bw=bw, mel=mel, tr=tr,
                        cases=cases))
    mel, tr, period = 2, False, 8
    bw, specs = variant_cases.TEAM_SPECS[(mel, tr, period)]
    team = variant_cases._team_batch('team_mel2_plain_p8', (1, mel, int(tr), period), mel, tr, period, bw, specs)
    out.append(dict(name='team_mel2_plain_bw%d' % bw, model=team['model'], bw=bw, mel=mel, tr=tr, cases=team['reads'][:1]))
    assert sum(len(b['cases']) for b in out) == N_READS
    return out


def run_batches(batches, exact=False):
    """-> {name: (events per read, statuses, tie flags, reads handed to the exact kernel, team skew per read)}.
    exact: the whole batch by the exact kernel."""
    import torch
    from fuzz_cases import reads_of
    from nadavca_amd import dtw, _lib
    from nadavca_amd.device import DeviceBatch, refine_alignment_dev
    ctx = _lib.default_context()
    had = os.environ.get('NADAVCA_ALIGN_KERNEL')
    os.environ.pop('NADAVCA_ALIGN_KERNEL', None)
    if exact:
        os.environ['NADAVCA_ALIGN_KERNEL'] = '1'
    try:
        out, models = {}, {}
        for b in batches:
            key = id(b['model'])
            if key not in models:
                models[key] = dtw.KmerModel(*b['model'], context=ctx)
            n = len(b['cases'])
            db = DeviceBatch(dtw.FlatBatch(reads_of(b['cases'])), torch.device('cuda', ctx.device))
            ev, st = refine_alignment_dev(db, b['bw'], b['mel'], models[key], b['tr'])
            flags, redone = ctx.last_tie_flags(n).copy(), ctx.last_batch_stats()['reads_redone_exact']
            cw = None if exact else np.asarray(ctx.last_read_skews(n)[1]).copy()
            ev, st, off = ev.cpu().numpy(), st.cpu().numpy(), db.ref_off.cpu().numpy()
            # (a read without a path has no events: whatever its slice holds is not compared)
            out[b['name']] = ([ev[off[i]:off[i + 1]] if st[i] == 0 else ev[:0] for i in range(n)], st, flags, redone, cw)
        return out
    finally:
        os.environ.pop('NADAVCA_ALIGN_KERNEL', None)
        if had is not None:
            os.environ['NADAVCA_ALIGN_KERNEL'] = had


def flags_of(results, batches):
    return {b['name']: [int(x) for x in results[b['name']][2]] for b in batches}


def classes_held(flags):
    """(reads with the exact bit, the ulp bit, the near bit, none of the three) over all batches"""
    f = np.array([x for v in flags.values() for x in v])
    return tuple(int(((f & bit) != 0).sum()) for bit in (TIE_EXACT, TIE_ULP, TIE_NEAR)) + (int(((f & 7) == 0).sum()),)


@pytest.fixture(scope='module')
def batches():
    return build_batches()


@pytest.fixture(scope='module')
def swept(batches):
    return run_batches(batches)


def test_the_fixture_holds_every_tie_class(batches):
    want = json.load(open(FIXTURE))
    assert want['seed'] == SEED and sorted(want['ties']) == sorted(b['name'] for b in batches)
    assert all(len(want['ties'][b['name']]) == len(b['cases']) for b in batches)
    held = classes_held(want['ties'])
    print('fixture: reads with the exact / ulp / near bit, and without any: %d / %d / %d / %d' % held)
    assert min(held) >= 1, held


@pytest.mark.gpu
def test_events_and_statuses_equal_the_exact_kernel(batches, swept):
    exact = run_batches(batches, exact=True)
    for b in batches:
        ev, st, _, redone, cw = swept[b['name']]
        xev, xst = exact[b['name']][:2]
        assert np.all((cw != 0) == (b is batches[-1])), (b['name'], cw)   # one wave per read, but for the team read
        assert redone == 0, (b['name'], redone)     # the sweeps themselves are compared, not the kernel they fall back on
        assert np.array_equal(st, xst), (b['name'], st, xst)
        for i, (e, x) in enumerate(zip(ev, xev)):
            assert e.shape == x.shape and np.array_equal(e, x), (b['name'], i)
    assert sum(int((swept[b['name']][1] == 0).sum()) for b in batches) > N_READS // 2   # (most reads have a path)


@pytest.mark.gpu
def test_tie_flags_equal_the_recorded_ones(batches, swept):
    want = json.load(open(FIXTURE))['ties']
    got = flags_of(swept, batches)
    print('reads with the exact / ulp / near bit, and without any: %d / %d / %d / %d' % classes_held(got))
    for b in batches:
        assert got[b['name']] == want[b['name']], b['name']
