"""What tests/variant_cases.py promises, as far as the CPU oracle can tell: the names, the completeness of the
log-likelihood cases, a path in the oracle for every read a case relies on, and — from the oracle's bands — that the
team reads are team reads whose skew lies where the case's name says.  The bounds here are lower bounds from the
reference's bands, not a restatement of the planner: which kernel a case really ran is asserted on the GPU through the
launch report (tests/test_gpu_variant_census.py)."""
import itertools

import numpy as np
import pytest

import variant_cases as vc

ALIGN = vc.align_cases()
EXACT = vc.exact_cases()
ELL = vc.ell_cases()


@pytest.fixture(scope='module')
def models(oracle_port):
    cache = {}

    def get(arrays):
        if id(arrays) not in cache:
            cache[id(arrays)] = oracle_port.KmerModel(*arrays)
        return cache[id(arrays)]
    return get


def test_names_are_unique_and_say_what_the_case_is_for():
    names = [c['name'] for c in ALIGN + EXACT + ELL + [vc.ell_too_wide_case()]]
    assert len(set(names)) == len(names)
    for c in ALIGN:
        if c['name'].startswith(('wave_', 'team_')):
            # the name is the variant: its min event length, row layout and, for a team, its period
            assert 'mel%d_%s' % (c['mel'], 'trans' if c['transitions'] else 'plain') in c['name']
            waves = 4 if c['name'].startswith('team_') else 1
            mine = [v for v in c['sweeps'] if v[2] == waves]
            assert len(mine) == 1 and (waves == 1 or c['name'].endswith('_p%d' % mine[0][3]))


def test_every_log_likelihood_kernel_has_a_case():
    """ell_dispatch's kernel tables hold min event length 0-4 x {8, 16} lanes x the four kinds (csrc/kernels_ell.hip)."""
    have = {(c['mel'], c['lanes'], c['kind']) for c in ELL}
    assert have == set(itertools.product(range(5), (8, 16), vc.ELL_KINDS)) and len(ELL) == 40
    for c in ELL:
        k = c['model'][0]
        assert (k + 2 > 8) == (c['lanes'] == 16)        # launch_ell: wide_groups
        assert all(3 <= len(r['reference']) <= 90 for r in c['reads'])


def test_every_exact_kernel_has_a_case():
    assert {c['mel'] for c in EXACT} == set(range(5)) and all(c['exact'] for c in EXACT)


def test_the_sweep_cases_claim_every_period_of_every_min_event_length():
    """(Which combinations are BUILT is asked of the library on the GPU; this is the table the cases were made for.)"""
    claimed = {v for c in ALIGN for v in c['sweeps']}
    want = {(mel, tr, 1, vc.base_period(tr)) for mel in range(5) for tr in (False, True)}
    want |= {(mel, False, 4, p) for mel in range(5) for p in (8, 16, 32)}
    want |= {(mel, True, 4, p) for mel in range(5) for p in (16, 32)}
    assert claimed == want and len(want) == 35


@pytest.mark.parametrize('case', ALIGN + EXACT, ids=[c['name'] for c in ALIGN + EXACT])
def test_relied_on_reads_have_a_path(oracle_port, models, case):
    mo = models(case['model'])
    ok = []
    for i in case['rely']:
        r = case['reads'][i]
        ev = oracle_port.refine_alignment(r['signal'], r['reference'], r['context_before'], r['context_after'],
                                          r['approximate_alignment'], case['bandwidth'], case['mel'], mo,
                                          case['transitions'])
        ok.append(len(ev) > 0)
    if case.get('rely_any'):
        assert any(ok)
    else:
        assert all(ok)


@pytest.mark.parametrize('case', [c for c in ALIGN if c['team']], ids=[c['name'] for c in ALIGN if c['team']])
def test_team_reads_lie_where_the_name_says(oracle_port, case):
    """A one-wave lower bound above ALIGN1_C_CAP makes the read a team read; the 256-row lower bound + min event length
    lies in the interval of the case's period (an edge case: at most at its sum; a read above the LDS fit: above)."""
    for i, (lo, hi) in case['team'].items():
        r = case['reads'][i]
        one = vc.skew_lower_bound(oracle_port, r, case['bandwidth'], case['transitions'], 64)
        assert one > vc.ALIGN1_C_CAP, (case['name'], i, one)
        team = vc.skew_lower_bound(oracle_port, r, case['bandwidth'], case['transitions'], vc.TEAM_ROWS)
        assert lo <= team + case['mel'] <= hi, (case['name'], i, team)
    # the company read is no team read
    for i, r in enumerate(case['reads']):
        if i not in case['team']:
            assert vc.skew_lower_bound(oracle_port, r, case['bandwidth'], case['transitions'], 64) <= vc.ALIGN1_C_CAP


def test_the_lds_fit_table_is_launch_align3s_arithmetic():
    """TEAM_C_FIT restated: 1 KB exponent table, four signal rings, (c + mel + 1) slots of 256 lanes x 20 B and the
    exchange words within 160 KB."""
    def lds(c, mel):
        sr = 256
        while sr < 64 * c + 64:
            sr *= 2
        return 128 * 8 + 4 * sr * 8 + (c + mel + 1) * 256 * 20 + 20 + 16 + 12 * 4
    for mel, fit in vc.TEAM_C_FIT.items():
        assert lds(fit, mel) <= 160 * 1024 < lds(fit + 1, mel)


def test_hypothesis_lists_hold_the_rows_they_are_for():
    for lanes in (8, 16):
        _, k, central = vc.ELL_LANES[lanes]
        alphabet = 4
        r = vc.ell_reads(2, lanes)[6]
        ref = np.asarray(r['reference'])
        rows = sorted({vc.joint_rows(h, ref, k, central) for h in vc.joint_list(ref, k, central, alphabet, lanes)})
        assert vc.JOINT_ROWS in rows and 0 in rows
        assert vc.joint_rows(vc.joint_one_row_more(ref, k, central, alphabet), ref, k, central) == vc.JOINT_ROWS + 1
        erows = sorted({vc.edit_rows(len(ref), k, central, p, d, len(s))
                        for p, d, s in vc.edit_list(ref, r['approximate_alignment'], k, central, alphabet, lanes)})
        assert vc.JOINT_ROWS in erows
        p, d, s = vc.edit_one_row_more(ref, k, central, alphabet)
        assert vc.edit_rows(len(ref), k, central, p, d, len(s)) == vc.JOINT_ROWS + 1
        if lanes == 8:   # either side of rows + 2 <= 8: the front and the back of the item list
            assert 6 in rows and 7 in rows and 6 in erows and 7 in erows
