"""The sweeps at the shapes where the forward sweep's prefetch ring and the rescale step can go wrong
(csrc/kernels_align3.hip): the ring's first four loads are issued before the step loop and every later one eight
steps ahead of its use, a trip is 16 steps, the padded step count a multiple of 32, and the scale moves by the wave's
maximum (wave_max_i, csrc/wave.h) every 8 steps, every 16 with transition rows — lanes without a row take part in
it with a sentinel.

One read per batch, so that a batch's ``wave_steps`` is that read's padded step count:

* step counts of exactly 32, 64 and 96 — one, two and three pairs of trips — with and without transition rows at min
  event length 0, 2 and 4 (18 reads of 2-25 bases, every one of fewer than 64 rows: lanes without a row);
* a read of 65 rows (64 bases without transition rows): one lane takes a second row;
* the smallest team read of tests/variant_cases.py (270 bases under bandwidth 280, min event length 2, no transition
  rows), swept by four waves.

The reads are made as tests/test_gpu_path_margin.py makes its own (synthetic.make_dp_case, fuzz_cases.reads_of); R,
bandwidth, dwell and seed of each were chosen for its step count, which the test asserts — a case that no longer has
the shape it is named for fails instead of hiding.  Events and statuses equal the exact kernel's
(NADAVCA_ALIGN_KERNEL=1) on every read and the CPU oracle's on every read without a tie flag, no read is handed to
the exact kernel, and the launch report names the one-wave or the team kernel."""
import os

import numpy as np
import pytest

SEED = 20261021

# name -> (transition rows, min event length, R, bandwidth, dwell lo, dwell hi, seed, padded step count)
STEP_CASES = {
    'plain_mel0_steps32': (False, 0, 11, 4, 1, 2, 1, 32),
    'plain_mel0_steps64': (False, 0, 21, 4, 1, 2, 0, 64),
    'plain_mel0_steps96': (False, 0, 25, 14, 1, 2, 0, 96),
    'plain_mel2_steps32': (False, 2, 7, 4, 2, 3, 0, 32),
    'plain_mel2_steps64': (False, 2, 17, 4, 2, 3, 0, 64),
    'plain_mel2_steps96': (False, 2, 25, 8, 2, 3, 1, 96),
    'plain_mel4_steps32': (False, 4, 3, 4, 4, 5, 0, 32),
    'plain_mel4_steps64': (False, 4, 7, 4, 4, 5, 0, 64),
    'plain_mel4_steps96': (False, 4, 12, 4, 4, 5, 1, 96),
    'trans_mel0_steps32': (True, 0, 8, 4, 1, 2, 1, 32),
    'trans_mel0_steps64': (True, 0, 16, 4, 1, 2, 0, 64),
    'trans_mel0_steps96': (True, 0, 25, 4, 1, 2, 0, 96),
    'trans_mel2_steps32': (True, 2, 6, 4, 2, 3, 0, 32),
    'trans_mel2_steps64': (True, 2, 13, 4, 2, 3, 0, 64),
    'trans_mel2_steps96': (True, 2, 21, 4, 2, 3, 0, 96),
    'trans_mel4_steps32': (True, 4, 2, 8, 4, 5, 0, 32),
    'trans_mel4_steps64': (True, 4, 5, 8, 4, 5, 1, 64),
    'trans_mel4_steps96': (True, 4, 8, 8, 4, 5, 0, 96),
    'plain_mel2_rows65_steps320': (False, 2, 64, 8, 2, 5, 1, 320),
}
TEAM_NAME, TEAM_STEPS = 'team_mel2_plain_steps1504', 1504
N_BATCHES = len(STEP_CASES) + 1


def rows_of(tr, R):
    return 2 * R if tr else R + 1


def make_read(model, tr, mel, R, bw, dlo, dhi, seed):
    from nadavca_amd import synthetic
    rng = np.random.default_rng([SEED, mel, int(tr), R, bw, dlo, dhi, seed])
    return synthetic.make_dp_case(rng, model, R=R, bandwidth=bw, dwell=(dlo, dhi), jitter=2, anchor_density=0.6,
                                  with_context=bool(seed % 2), trim=min(3, R // 3))


def build_batches():
    """-> [dict(name, model, bw, mel, tr, cases, steps, waves)]: one read each."""
    import variant_cases
    from nadavca_amd import synthetic
    model = synthetic.load_model_arrays()
    out = []
    for name, (tr, mel, R, bw, dlo, dhi, seed, steps) in STEP_CASES.items():
        out.append(dict(name=name, model=model, bw=bw, mel=mel, tr=tr, steps=steps, waves=1,
                        cases=[make_read(model, tr, mel, R, bw, dlo, dhi, seed)]))
    mel, tr, period = 2, False, 8
    bw, specs = variant_cases.TEAM_SPECS[(mel, tr, period)]
    team = variant_cases._team_batch('team_mel2_plain_p8', (1, mel, int(tr), period), mel, tr, period, bw, specs)
    out.append(dict(name=TEAM_NAME, model=team['model'], bw=bw, mel=mel, tr=tr, steps=TEAM_STEPS, waves=4,
                    cases=team['reads'][:1]))
    return out


def run_batches(batches, exact=False):
    """-> {name: dict(ev, st, flags, stats, launches, cw)}.  exact: the whole batch by the exact kernel."""
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
            db = DeviceBatch(dtw.FlatBatch(reads_of(b['cases'])), torch.device('cuda', ctx.device))
            ev, st = refine_alignment_dev(db, b['bw'], b['mel'], models[key], b['tr'])
            out[b['name']] = dict(flags=ctx.last_tie_flags(1).copy(), stats=ctx.last_batch_stats(),
                                  launches=ctx.last_launches(), cw=int(ctx.last_read_skews(1)[1][0]),
                                  ev=ev.cpu().numpy(), st=st.cpu().numpy())
        return out
    finally:
        os.environ.pop('NADAVCA_ALIGN_KERNEL', None)
        if had is not None:
            os.environ['NADAVCA_ALIGN_KERNEL'] = had


@pytest.fixture(scope='module')
def batches():
    return build_batches()


@pytest.fixture(scope='module')
def swept(batches):
    return run_batches(batches)


def test_the_cases_cover_the_shapes(batches):
    assert len(batches) == N_BATCHES and all(len(b['cases']) == 1 for b in batches)
    for tr in (False, True):
        for mel in (0, 2, 4):
            assert sorted(b['steps'] for b in batches[:18] if b['tr'] == tr and b['mel'] == mel) == [32, 64, 96]
    rows = [rows_of(b['tr'], len(b['cases'][0]['reference'])) for b in batches]
    assert max(rows[:18]) < 64 and rows[18] == 65 and rows[19] > 256, rows


@pytest.mark.gpu
def test_step_counts_and_kernels_are_the_ones_named(batches, swept):
    from variant_cases import base_period
    for b in batches:
        got = swept[b['name']]
        print('%s: wave_steps %d, launches %s, team skew %d' % (b['name'], got['stats']['wave_steps'],
                                                                [(x['op'], x['waves'], x['period']) for x in got['launches']],
                                                                got['cw']))
    for b in batches:
        got = swept[b['name']]
        assert got['stats']['wave_steps'] == b['steps'], (b['name'], got['stats']['wave_steps'])
        assert got['stats']['reads_redone_exact'] == 0, b['name']
        # one launch class: the one-wave pair at its base period, or the team's
        want = [('sweep', b['waves'], b['mel'], int(b['tr']), base_period(b['tr']))]
        assert [(x['op'], x['waves'], x['mel'], x['transitions'], x['period']) for x in got['launches']] == want, \
            (b['name'], got['launches'])
        assert (got['cw'] != 0) == (b['waves'] == 4), (b['name'], got['cw'])


@pytest.mark.gpu
def test_events_and_statuses_equal_the_exact_kernel(batches, swept):
    exact = run_batches(batches, exact=True)
    for b in batches:
        got, want = swept[b['name']], exact[b['name']]
        assert want['launches'] and all(x['op'] == 'exact' for x in want['launches']), (b['name'], want['launches'])
        assert got['stats']['reads_redone_exact'] == 0, b['name']
        assert np.array_equal(got['st'], want['st']), (b['name'], got['st'], want['st'])
        if got['st'][0] == 0:   # (a read without a path has no events: whatever its slice holds is not compared)
            assert got['ev'].shape == want['ev'].shape and np.array_equal(got['ev'], want['ev']), b['name']
    assert sum(int(swept[b['name']]['st'][0] == 0) for b in batches) > N_BATCHES // 2   # (most reads have a path)


@pytest.mark.gpu
def test_events_and_statuses_equal_the_oracle(batches, swept, oracle_port):
    from nadavca_amd import _lib
    models, compared = {}, 0
    for b in batches:
        got = swept[b['name']]
        if int(got['flags'][0]) != 0:   # a tie on record: the reference's own rounding may decide (parity contract)
            continue
        key = id(b['model'])
        if key not in models:
            models[key] = oracle_port.KmerModel(*b['model'])
        c = b['cases'][0]
        exp = np.asarray(oracle_port.refine_alignment(c['signal'], c['reference'], c['context_before'],
                                                      c['context_after'], c['approximate_alignment'], b['bw'],
                                                      b['mel'], models[key], b['tr'])).reshape(-1, 2)
        assert int(got['st'][0]) == (_lib.READ_OK if len(exp) else _lib.READ_NO_PATH), (b['name'], got['st'])
        if len(exp):   # (a read without a path has no events: whatever its slice holds is not compared)
            ev = got['ev'].reshape(-1, 2)
            assert ev.shape == exp.shape and np.array_equal(ev, exp), b['name']
        compared += 1
    print('reads compared with the oracle: %d of %d' % (compared, N_BATCHES))
    assert compared > N_BATCHES // 2
