"""The row switch of the one-wave sweeps (csrc/kernels_align3.hip) at the shapes where serving it as a scalar event of
the oldest open row can go wrong: the step tests the oldest open row's sample index against its band end, the block
serves ``while the oldest row is past its end``, takes the record of the next row with an unconditional load (index
clamped, the record made inert where the lane gets no row) and derives "an emitting lane switched", "first row" and
"last row" from the scalar row counter.

Batches built as tests/test_gpu_sweep_trips.py builds its own (tests/switch_order_cases.py has the reads):

* reads of 63, 64, 65 and 129 rows (with transition rows 62, 64, 66, 130): no lane with a second row, the first with
  a second row, a lane with a third — with and without transition rows at min event length 0, 2 and 4;
* band ends clipped to the signal's end on the last rows and band starts clipped to 0 on the first: several rows
  leave on the same step at the end of either sweep;
* reads of 64 < rows < 128, in which the last switches hand their lanes "no row";
* two reads per batch, in both orders, swept by one persistent wave per launch (``set_slots(1)``): the wave starts its
  second read with the first one's switch state.

Every case is asserted to have the shape it is named for.  Events and statuses equal the exact kernel's
(NADAVCA_ALIGN_KERNEL=1) on every read and the CPU oracle's on every read without a tie flag; no read is handed to the
exact kernel — which is also what the sweeps' own guard of the switch order reports (a lane found past its row's end at
a rescale step) — and the launch report names the one-wave kernel."""
import os

import numpy as np
import pytest

import switch_order_cases as soc


def run_batches(batches, model, exact=False):
    """-> {name: dict(ev, st, flags, stats, launches, cw)}.  exact: the whole batch by the exact kernel."""
    import torch
    from nadavca_amd import dtw, _lib
    from nadavca_amd.device import DeviceBatch, refine_alignment_dev
    ctx = _lib.default_context()
    had = os.environ.get('NADAVCA_ALIGN_KERNEL')
    os.environ.pop('NADAVCA_ALIGN_KERNEL', None)
    if exact:
        os.environ['NADAVCA_ALIGN_KERNEL'] = '1'
    try:
        out = {}
        km = dtw.KmerModel(*model, context=ctx)
        for b in batches:
            n = len(b['cases'])
            ctx.set_slots(1 if n > 1 else 0)   # one persistent wave per launch: it sweeps the reads one after the other
            db =DeviceBatch(dtw.FlatBatch(soc_reads(b['cases'])), torch.device('cuda', ctx.device))
            ev, st = refine_alignment_dev(db, b['bw'], b['mel'], km, b['tr'])
            out[b['name']] = dict(flags=ctx.last_tie_flags(n).copy(), stats=ctx.last_batch_stats(),
                                  launches=ctx.last_launches(), cw=ctx.last_read_skews(n)[1].copy(),
                                  ev=ev.cpu().numpy().reshape(-1), st=st.cpu().numpy())
        return out
    finally:
        ctx.set_slots(0)
        os.environ.pop('NADAVCA_ALIGN_KERNEL', None)
        if had is not None:
            os.environ['NADAVCA_ALIGN_KERNEL'] = had


def soc_reads(cases):
    return [(c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'])
            for c in cases]


def events_of(b, ev):
    """-> the reads' event slices: two integers per base, reads one behind the other."""
    out, at = [], 0
    for c in b['cases']:
        n = 2 * len(c['reference'])
        out.append(ev[at:at + n])
        at += n
    assert at == ev.size, (b['name'], at, ev.size)
    return out


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


@pytest.fixture(scope='module')
def batches(model):
    return soc.build_cases(model)


@pytest.fixture(scope='module')
def swept(batches, model):
    return run_batches(batches, model)


def test_the_cases_have_the_shapes_they_are_named_for(batches):
    names = [b['name'] for b in batches]
    assert len(set(names)) == len(names) == 24 + 4 + 4
    for tr in (False, True):
        for mel in (0, 2, 4):
            rows = sorted(b['rows'][0] for b in batches[:24] if b['tr'] == tr and b['mel'] == mel)
            assert rows == ([62, 64, 66, 130] if tr else [63, 64, 65, 129]), (tr, mel, rows)
    for b in batches:
        assert [soc.rows_of(b['tr'], len(c['reference'])) for c in b['cases']] == b['rows'], b['name']
        for c in b['cases']:
            p = soc.plan_geometry(c, b['bw'], b['mel'], b['tr'])
            assert p['c'] <= soc.C_CAP and p['cw'] == 0, (b['name'], p['c'])     # one wave per read
        if 'clipped_ends' in b['name']:   # at least three consecutive rows at either end
            p = soc.plan_geometry(b['cases'][0], b['bw'], b['mel'], b['tr'])
            assert (p['BE'][-3:] == p['N']).all() and (p['BS'][:3] == 0).all(), b['name']
            assert b['rows'][0] > 64
        if 'two_reads' in b['name']:      # every lane's last switch finds no row; the second read starts on a used wave
            assert len(b['cases']) == 2 and all(64 < r < 128 for r in b['rows']), (b['name'], b['rows'])
    assert sum('clipped_ends' in n for n in names) == 4 and sum('two_reads' in n for n in names) == 4


@pytest.mark.gpu
def test_no_read_is_redone_and_the_one_wave_kernel_ran(batches, swept):
    from variant_cases import base_period
    for b in batches:
        got = swept[b['name']]
        print('%s: wave_steps %d, redone %d, launches %s' % (b['name'], got['stats']['wave_steps'],
                                                             got['stats']['reads_redone_exact'],
                                                             [(x['op'], x['waves'], x['period']) for x in got['launches']]))
    for b in batches:
        got = swept[b['name']]
        assert got['stats']['reads_redone_exact'] == 0, b['name']
        want = [('sweep', 1, b['mel'], int(b['tr']), base_period(b['tr']))]
        assert [(x['op'], x['waves'], x['mel'], x['transitions'], x['period']) for x in got['launches']] == want, \
            (b['name'], got['launches'])
        assert (np.asarray(got['cw']) == 0).all(), (b['name'], got['cw'])


@pytest.mark.gpu
def test_events_and_statuses_equal_the_exact_kernel(batches, swept, model):
    exact = run_batches(batches, model, exact=True)
    with_path = 0
    for b in batches:
        got, want = swept[b['name']], exact[b['name']]
        assert want['launches'] and all(x['op'] == 'exact' for x in want['launches']), (b['name'], want['launches'])
        assert np.array_equal(got['st'], want['st']), (b['name'], got['st'], want['st'])
        for k, (e_got, e_want) in enumerate(zip(events_of(b, got['ev']), events_of(b, want['ev']))):
            if got['st'][k] == 0:   # (a read without a path has no events: whatever its slice holds is not compared)
                assert np.array_equal(e_got, e_want), (b['name'], k)
                with_path += 1
    assert with_path > sum(len(b['cases']) for b in batches) // 2   # (most reads have a path)


@pytest.mark.gpu
def test_events_and_statuses_equal_the_oracle(batches, swept, model, oracle_port):
    from nadavca_amd import _lib
    mo = oracle_port.KmerModel(*model)
    compared = total = 0
    for b in batches:
        got = swept[b['name']]
        for k, (c, ev) in enumerate(zip(b['cases'], events_of(b, got['ev']))):
            total += 1
            if int(got['flags'][k]) != 0:   # a tie on record: the reference's own rounding may decide (parity contract)
                continue
            exp = np.asarray(oracle_port.refine_alignment(c['signal'], c['reference'], c['context_before'],
                                                          c['context_after'], c['approximate_alignment'], b['bw'],
                                                          b['mel'], mo, b['tr'])).reshape(-1, 2)
            assert int(got['st'][k]) == (_lib.READ_OK if len(exp) else _lib.READ_NO_PATH), (b['name'], k, got['st'])
            if len(exp):
                assert np.array_equal(ev.reshape(-1, 2), exp), (b['name'], k)
            compared += 1
    print('reads compared with the oracle: %d of %d' % (compared, total))
    assert compared > total // 2
