"""The align planner at every size where it changes path (tests/plan_cases.py): events and statuses equal the CPU
oracle's, and the planner's totals — band cells, wave steps under the per-row offsets, reads handed to the exact
kernel, tie flags — equal tests/golden/plan_totals.json, which tools/record_plan_totals.py recorded on the GPU before
the planner moved its intermediates into LDS.  A planner that emits valid but longer offsets fails on wave_steps, one
that emits invalid offsets fails the oracle comparison."""
import json
import os

import numpy as np
import pytest

import plan_cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = plan_cases.build_cases()
with open(os.path.join(GOLDEN, 'plan_totals.json')) as _f:
    TOTALS = json.load(_f)
_expected = {}   # id(read dict) -> the oracle's events: the mixed batches hold the reads of the single cases again


@pytest.fixture(scope='module')
def dtw():
    from nadavca_amd import dtw as d
    return d


@pytest.fixture(scope='module')
def models(dtw, oracle_port):
    cache = {}

    def get(key):
        if key not in cache:
            arrays = plan_cases.model_arrays(key)
            cache[key] = (dtw.KmerModel(*arrays), oracle_port.KmerModel(*arrays))
        return cache[key]
    return get


def _oracle(oracle, mo, case, i):
    """-> (status, events) the oracle gives read i of the case."""
    c = case['reads'][i]
    if i in case['bad']:
        return -1, None   # NVK_READ_BAD_INPUT: the reference indexes its table out of range there
    R, N = len(c['reference']), len(c['signal'])
    bs, be = oracle.bands(c['approximate_alignment'], R, N, case['bandwidth'])
    if np.any(be < bs):
        return -2, None   # NVK_READ_BAD_BAND: the reference sizes a row with a negative width
    key = (id(c), case['bandwidth'], case['mel'], case['transitions'])
    if key not in _expected:
        _expected[key] = oracle.refine_alignment(c['signal'], c['reference'], c['context_before'],
                                                 c['context_after'], c['approximate_alignment'], case['bandwidth'],
                                                 case['mel'], mo, case['transitions'])
    ev = _expected[key]
    return (0 if len(ev) else 1), ev


def test_every_case_is_recorded():
    assert sorted(TOTALS) == sorted(c['name'] for c in CASES)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_plan_shape(dtw, oracle_port, models, case):
    mg, mo = models(case['model'])
    events, status, totals = plan_cases.run_case(dtw, case, mg)
    for i in range(len(case['reads'])):
        st, ev = _oracle(oracle_port, mo, case, i)
        assert int(status[i]) == st, (case['name'], i)
        if st == 0:
            assert events[i].shape == ev.shape and np.array_equal(events[i], ev), (case['name'], i)
        else:
            assert len(events[i]) == 0, (case['name'], i)
    assert totals == TOTALS[case['name']], case['name']


def _skew_lower_bound(oracle, case):
    """A lower bound of the wavefront skew the planner finds for a one-read case, from the oracle's bands alone: a
    lane's next row lies 64 rows on, and it must have left its row (whose span holds the band) before."""
    c = case['reads'][0]
    R, N = len(c['reference']), len(c['signal'])
    bs, be = oracle.bands(c['approximate_alignment'], R, N, case['bandwidth'])
    T = 2 * R if case['transitions'] else R + 1
    band = (lambda r: (r + 1) // 2) if case['transitions'] else (lambda r: r)
    need = 1
    for r in range(64, T):
        d = int(be[band(r - 64)]) - int(bs[band(r)]) + 1
        if d >= 0:
            need = max(need, d // 64 + 1)
    return need


def _planner_skews(dtw, models, case):
    """(c, cw) the planner gave the one read of a case: a device-pointer call, then the library's own record of the
    batch planned last (Context.last_read_skews)."""
    import torch
    from nadavca_amd.device import DeviceBatch, refine_alignment_dev
    mg, _ = models(case['model'])
    c = case['reads'][0]
    batch = dtw.FlatBatch([(c['signal'], c['reference'], c['context_before'], c['context_after'],
                            c['approximate_alignment'])])
    refine_alignment_dev(DeviceBatch(batch, torch.device('cuda', mg.context.device)), case['bandwidth'], case['mel'],
                         mg, case['transitions'])
    skew, team_skew = mg.context.last_read_skews(1)
    return int(skew[0]), int(team_skew[0])


def test_the_team_cases_are_team_reads(dtw, oracle_port, models):
    """Skew above ALIGN1_C_CAP = 3 (csrc/nvk_internal.h) is what hands a read to a team of waves."""
    by_name = {c['name']: c for c in CASES}
    for t in ('trans', 'plain'):
        assert _skew_lower_bound(oracle_port, by_name['team_R300_%s' % t]) > 3
        assert _skew_lower_bound(oracle_port, by_name['team_R1100_%s' % t]) > 3
        assert _skew_lower_bound(oracle_port, by_name['mel2_%s_R129' % t]) <= 3
        # ... and the planner says so itself: a team skew for the team reads, none for the other
        for name, team in (('team_R300_%s' % t, True), ('team_R1100_%s' % t, True), ('mel2_%s_R129' % t, False)):
            c, cw = _planner_skews(dtw, models, by_name[name])
            assert c >= _skew_lower_bound(oracle_port, by_name[name])
            assert (c > 3 and cw >= 1) if team else (c <= 3 and cw == 0), (name, c, cw)


def test_the_cases_reach_what_they_are_for():
    """The special cases are what their names say (were a builder change to defuse one, the totals would still match a
    re-recorded file)."""
    by_name = {c['name']: c for c in CASES}
    assert TOTALS['anchors_out_of_order']['wave_steps'] == 0          # refused: no steps planned
    assert all(TOTALS['plateau_%s' % t]['tie_flags'][0] & 8 for t in ('trans', 'plain'))
    assert not TOTALS['trans_R129']['tie_flags'][0] & 8
    assert len(by_name['bad_codes']['reads']) == 3 and by_name['bad_codes']['bad'] == (0, 1)
    mixed = [c for c in CASES if c['name'].startswith('mixed_')]
    assert any(len(c['reads']) > 10 for c in mixed)
    # every read has company in some batch: each setting with a read has a mixed batch
    assert {(c['model'], c['bandwidth'], c['mel'], c['transitions']) for c in CASES} == \
        {(c['model'], c['bandwidth'], c['mel'], c['transitions']) for c in mixed}
