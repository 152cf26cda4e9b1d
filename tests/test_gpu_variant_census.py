"""Census of the built kernel variants: every kernel pair select_sweeps has (csrc/kernels_align3.hip), every
align_kernel<MEL> (csrc/kernels_align.hip) and every ell_kernel<M, lanes, kind> of ell_dispatch's tables (csrc/kernels_ell.hip) is
launched by a named smallest case of tests/variant_cases.py and compared with the CPU oracle there.

Which variant a batch ran is what the library's launch report says (include/nadavca_hip.h: nvk_last_launches,
nvk_last_read_skews); which variants are built is what nvk_built_sweep_variants says, asked of select_sweeps itself.

* Completeness: the variants reported over all cases equal the built ones — a built variant without a case fails
  test_every_built_*, a case that no longer reaches its variant fails its own test.
* refine_alignment, per case: the report names the variant, every read goes through the parity contract of
  include/nadavca_hip.h (equal to the oracle, or a loose tie bit and a difference fuzz_cases.classify_difference
  explains — the rules of test_gpu_parity_full._fuzz_contract, no cap on the differing share), and the reads the
  case relies on have a path in the oracle, carry neither NVK_TIE_NEAR nor NVK_TIE_ULP and equal the oracle exactly,
  so that no variant counts as compared through no-path reads or accepted differences.
* log-likelihoods, per case: rtol = atol = 1e-9 against the oracle, the same -inf pattern, no NaN; listed
  hypotheses bit-equal to the full matrix of the same variant.

The oracle runs once per read and setting (_expected); a case runs once per process (_runs), so the completeness
tests cost nothing after the per-case tests and run every case when they are selected alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import variant_cases as vc
from conftest import ROOT

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-9
TIE_EXACT, TIE_NEAR, TIE_ULP, TIE_PLATEAU = 1, 2, 4, 8   # include/nadavca_hip.h
TIE_LOOSE = TIE_NEAR | TIE_ULP
READ_OK, READ_NO_PATH, READ_BAD_INPUT, READ_TOO_WIDE = 0, 1, -1, -3
LDS_LIMIT = 160 * 1024

ALIGN = vc.align_cases()
ELL = vc.ell_cases()
_runs = {}       # case name -> what _run_align / _run_ell found
_expected = {}   # the oracle's answers
_models = {}


def _model(oracle, arrays):
    """-> (GPU model on the default context, oracle model) of a table, made once."""
    from nadavca_amd import dtw, _lib
    if id(arrays) not in _models:
        _models[id(arrays)] = (dtw.KmerModel(*arrays, context=_lib.default_context()), oracle.KmerModel(*arrays), arrays)
    return _models[id(arrays)][:2]


def _device_batch(reads, ctx):
    import torch
    from nadavca_amd import dtw
    from nadavca_amd.device import DeviceBatch
    return DeviceBatch(dtw.FlatBatch(vc.reads_of(reads)), torch.device('cuda', ctx.device))


# ---------------------------------------------------------------------------------------------------------------------
# refine_alignment
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_events(oracle, mo, case, i):
    r = case['reads'][i]
    key = ('refine', id(r), case['bandwidth'], case['mel'], case['transitions'])
    if key not in _expected:   # (the entry holds the read, so that its id is not given to another one)
        _expected[key] = (r, oracle.refine_alignment(r['signal'], r['reference'], r['context_before'],
                                                     r['context_after'], r['approximate_alignment'], case['bandwidth'],
                                                     case['mel'], mo, case['transitions']))
    return _expected[key][1]


def _run_align(oracle, case):
    """One device-pointer refine_alignment call of the case, the launch report it left, and the parity contract on
    every read.  -> dict(launches, sweeps, c, cw, status, flags, stats, clean): ``clean[i]``: read i has a path in the
    oracle, no loose tie bit and the oracle's events exactly."""
    if case['name'] in _runs:
        return _runs[case['name']]
    from fuzz_cases import classify_difference, SCORED
    from nadavca_amd.device import refine_alignment_dev
    mg, mo = _model(oracle, case['model'])
    ctx = mg.context
    n = len(case['reads'])
    db = _device_batch(case['reads'], ctx)
    ev, st = refine_alignment_dev(db, case['bandwidth'], case['mel'], mg, case['transitions'])
    launches = ctx.last_launches()
    c, cw = ctx.last_read_skews(n)
    flags = ctx.last_tie_flags(n)
    stats = ctx.last_batch_stats()
    ev, st = ev.cpu().numpy(), st.cpu().numpy()
    off = db.ref_off.cpu().numpy()
    k, central, alphabet = case['model'][:3]
    clean = []
    for i, r in enumerate(case['reads']):
        if i in case.get('above', ()):
            # beyond the LDS fit: handed to the exact kernel, whose one-wave rings it does not fit either
            assert int(st[i]) == READ_TOO_WIDE, (case['name'], i, int(st[i]))
            clean.append(False)
            continue
        exp = np.asarray(_oracle_events(oracle, mo, case, i)).reshape(-1, 2)
        assert int(st[i]) == (READ_OK if len(exp) else READ_NO_PATH), (case['name'], i, int(st[i]))
        got = ev[off[i]:off[i + 1]] if st[i] == READ_OK else np.zeros((0, 2), dtype=np.int32)
        same = got.shape == exp.shape and np.array_equal(got, exp)
        if not same:
            assert flags[i] & TIE_LOOSE, ('a read without a tie bit differs', case['name'], i)
            why = classify_difference(got, exp, r, case['model'], k, central, alphabet, case['bandwidth'], case['mel'],
                                      case['transitions'])
            assert why != 'UNEXPLAINED', ('unexplained difference', case['name'], i, SCORED[-1])
            if why == 'flat-plateau':
                assert flags[i] & TIE_PLATEAU, ('flat-plateau difference without the plateau mark', case['name'], i)
        clean.append(bool(len(exp) and same and not flags[i] & TIE_LOOSE))
    sweeps = sorted((x['mel'], bool(x['transitions']), x['waves'], x['period']) for x in launches if x['op'] == 'sweep')
    _runs[case['name']] = dict(launches=launches, sweeps=sweeps, c=c, cw=cw, status=st, flags=flags, stats=stats,
                               clean=clean)
    print('%s: %s; skews c %s cw %s; tie flags %s; clean %s'
          % (case['name'], [(x['op'], x['mel'], x['transitions'], x['waves'], x['period'], x['kind'], x['c'], x['H'],
                             x['SR'], x['lds_bytes'], x['reads'], x['chunks']) for x in launches],
             c.tolist(), cw.tolist(), flags.tolist(), clean))
    return _runs[case['name']]


def _clean_reads_of(case, run, variant):
    """The clean reads of the case that the launch class of ``variant`` swept."""
    team = variant[2] > 1
    cap = max([x['c'] for x in run['launches'] if x['op'] == 'sweep' and (x['waves'] > 1) == team] + [0])
    if case.get('retry'):
        return []   # (which of its reads the exact kernel redid, the report does not say)
    return [i for i, ok in enumerate(run['clean'])
            if ok and i not in case.get('handed', ())
            and ((run['cw'][i] > 0 and run['cw'][i] <= cap) if team else run['cw'][i] == 0)]


@pytest.mark.parametrize('case', ALIGN, ids=[c['name'] for c in ALIGN])
def test_align_case(oracle_port, case):
    run = _run_align(oracle_port, case)
    n = len(case['reads'])
    # the report names the variants the case is for, and only sweeps (and the retry behind them)
    assert run['sweeps'] == case['sweeps'], (case['name'], run['launches'])
    for x in run['launches']:
        assert x['lds_bytes'] <= LDS_LIMIT and x['chunks'] >= 1
        if x['op'] == 'sweep':
            assert x['H'] == max(x['c'] + x['mel'], 1) + (1 if x['waves'] > 1 else 0)
            assert x['period'] == vc.period_of(x['c'], x['mel'], bool(x['transitions']))
            assert x['SR'] >= 64 * x['c'] + 64
        else:
            assert x['op'] == 'exact' and x['kind'] == 'retry' and x['mel'] == case['mel']
    by_waves = {x['waves']: x for x in run['launches'] if x['op'] == 'sweep'}
    assert sum(x['reads'] for x in by_waves.values()) == n
    # the planner's skews: a team read has a one-wave skew above the cap and the team skew the case was made for
    for i in range(n):
        if i in case['team']:
            assert run['c'][i] > vc.ALIGN1_C_CAP and run['cw'][i] > 0, (case['name'], i)
        elif case['team']:
            assert run['c'][i] <= vc.ALIGN1_C_CAP and run['cw'][i] == 0, (case['name'], i)
    for i, want in case.get('cw', {}).items():
        assert run['cw'][i] == want, (case['name'], i, int(run['cw'][i]))
    if case['team']:
        assert by_waves[4]['reads'] == len(case['team']) and by_waves[1]['reads'] == n - len(case['team'])
        # the team launch is sized by the batch's widest team skew, cut to what fits the LDS
        assert by_waves[4]['c'] == case['c_launch'] <= vc.TEAM_C_FIT[case['mel']]
    # the reads the case relies on were compared, not excused
    rely = [run['clean'][i] for i in case['rely']]
    assert (any(rely) if case.get('rely_any') else all(rely)), (case['name'], rely, run['flags'].tolist())
    for v in case['sweeps']:
        if v[2] == (4 if case['team'] else 1) and case['rely']:
            assert _clean_reads_of(case, run, v), (case['name'], v)
    # what the sweeps handed on to the exact kernel: the reads above the LDS fit, the reads the case says so of, no other
    # — a relied-on read was swept by the variant the case is named for
    handed = len(case.get('above', ())) + len(case.get('handed', ()))
    if case.get('retry'):
        assert run['stats']['reads_redone_exact'] > 0
    else:
        assert run['stats']['reads_redone_exact'] == handed, (case['name'], run['stats'])
    assert any(x['op'] == 'exact' for x in run['launches']) == (run['stats']['reads_redone_exact'] > 0)
    if 'cut' in case:
        # the read at the fit is swept, the read above it is cut off: the launch has the fit's rings, not the batch's
        team = by_waves[4]
        assert team['c'] == case['cut'] == vc.TEAM_C_FIT[case['mel']] < max(run['cw'])
        assert run['cw'][0] == team['c'] and run['clean'][0]


def test_the_period_doubles_exactly_at_the_edges(oracle_port):
    """Team skew + min event length 7 | 8 and 15 | 16: the same reads, the bandwidth a sample apart."""
    by_name = {c['name']: c for c in ALIGN}
    seen = set()
    for name, (tr, mel, specs, bw_lo, bw_hi) in vc.EDGE_SPECS.items():
        cw = max(sp[3] for sp in specs)
        lo, hi = by_name['%s_sum%d' % (name, cw + mel)], by_name['%s_sum%d' % (name, cw + mel + 1)]
        assert hi['bandwidth'] - lo['bandwidth'] == 1
        assert all(np.array_equal(x['signal'], y['signal']) for x, y in zip(lo['reads'], hi['reads']))
        a, b = _run_align(oracle_port, lo), _run_align(oracle_port, hi)
        (ca, pa), (cb, pb) = [[(x['c'], x['period']) for x in r['launches'] if x['op'] == 'sweep' and x['waves'] == 4][0]
                              for r in (a, b)]
        assert (ca, cb) == (cw, cw + 1) and pb == 2 * pa, (name, ca, cb, pa, pb)
        assert (int(max(a['cw'])), int(max(b['cw']))) == (cw, cw + 1)
        seen.add((cw + mel, pa))
    assert seen >= {(7, 8), (15, 16)}


def test_every_built_sweep_variant_was_swept_and_compared(oracle_port):
    """Every pair select_sweeps has was reported by some case, and for every one some case holds a read that the
    sweeps kept (nothing handed on beyond what the case names), without a loose tie bit, equal to the oracle."""
    from nadavca_amd import _lib
    built = set(_lib.built_sweep_variants())
    ran, compared = set(), set()
    for case in ALIGN:
        run = _run_align(oracle_port, case)
        for v in run['sweeps']:
            ran.add(v)
            # a variant counts through the case named for it alone (wave_* / team_*), so that taking that case away
            # shows here even where an edge or cut case happens to run the same kernel
            if case['name'].startswith(('wave_', 'team_')) and _clean_reads_of(case, run, v):
                compared.add(v)
    assert ran == built, ('built, no case: %s; ran, not built: %s' % (sorted(built - ran), sorted(ran - built)))
    assert compared == built, sorted(built - compared)


def test_the_special_cases_are_there():
    """What no completeness count shows: a read the sweeps hand on, and the LDS cut with and without transition rows
    (the edges have test_the_period_doubles_exactly_at_the_edges)."""
    assert any(c.get('retry') for c in ALIGN)
    assert {c['transitions'] for c in ALIGN if 'cut' in c} == {True, False}


# ----- the exact kernel: NADAVCA_ALIGN_KERNEL=1 is read at call time, so its cases run in a child process ----------
def _exact_child():
    """Run in the child: the exact cases through _run_align; prints one line with their reports."""
    from oracle.oracle import Oracle
    oracle = Oracle('port')
    out = {}
    for case in vc.exact_cases():
        run = _run_align(oracle, case)
        rely = [run['clean'][i] for i in case['rely']]
        assert (any(rely) if case.get('rely_any') else all(rely)), (case['name'], rely)
        out[case['name']] = [[x['op'], x['kind'], x['mel'], x['reads']] for x in run['launches']]
    print('EXACT-CENSUS ' + json.dumps(out))


def _exact_runs():
    if 'exact' not in _runs:
        code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")\n'
                'import test_gpu_variant_census as t\n'
                't._exact_child()\n' % (ROOT, ROOT))
        env = dict(os.environ, NADAVCA_ALIGN_KERNEL='1')
        p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
        print(p.stdout[-3000:])
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('EXACT-CENSUS ')]
        assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-2000:]
        _runs['exact'] = json.loads(lines[-1][len('EXACT-CENSUS '):])
    return _runs['exact']


def test_every_exact_kernel_was_run_and_compared():
    """align_kernel<0..4>: every case reports exact launches of its min event length only, serving every read, and
    (in the child) passes the contract with the reads it relies on equal to the oracle."""
    runs = _exact_runs()
    cases = {c['name']: c for c in vc.exact_cases()}
    assert set(runs) == set(cases)
    seen = set()
    for name, launches in runs.items():
        assert launches and all(op == 'exact' and kind == 'all' and mel == cases[name]['mel']
                                for op, kind, mel, _ in launches), (name, launches)
        assert sum(reads for _, _, _, reads in launches) == len(cases[name]['reads'])
        if name.startswith('exact_team_'):
            assert len(launches) == 2    # the narrow and the wide class
        seen.add((cases[name]['mel'], len(launches)))
    # every kernel with its narrow class alone and with both classes
    assert seen == {(mel, n) for mel in range(5) for n in (1, 2)}


# ---------------------------------------------------------------------------------------------------------------------
# estimate_log_likelihoods and the listed / joint / edit hypotheses
# ---------------------------------------------------------------------------------------------------------------------
def _close(got, exp, what):
    got, exp = np.asarray(got, dtype=float), np.asarray(exp, dtype=float)
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isneginf(got), np.isneginf(exp)), what
    assert not np.any(np.isnan(got)), what
    fin = np.isfinite(exp)
    err = float(np.max(np.abs(got[fin] - exp[fin]))) if fin.any() else 0.0
    assert np.allclose(got[fin], exp[fin], rtol=RTOL, atol=ATOL), (what, err)
    return err


def _oracle_ll(oracle, mo, r, bw, mel, w, ref=None, anchors=None):
    ref = r['reference'] if ref is None else np.ascontiguousarray(ref, dtype=np.int32)
    anchors = r['approximate_alignment'] if anchors is None else np.ascontiguousarray(anchors, dtype=np.int32)
    key = ('ell', id(r), bw, mel, w, ref.tobytes(), anchors.tobytes())
    if key not in _expected:
        _expected[key] = (r, np.asarray(oracle.estimate_log_likelihoods(r['signal'], ref, r['context_before'],
                                                                        r['context_after'], anchors, bw, mel, mo, w)))
    return _expected[key][1]


def _full_matrix(case, mg, reads, w):
    """The full matrix on the device path -> (per-read matrices, status, launch report, skews)."""
    from nadavca_amd.device import estimate_log_likelihoods_dev
    ctx = mg.context
    db = _device_batch(reads, ctx)
    ll, st = estimate_log_likelihoods_dev(db, case['bandwidth'], case['mel'], mg, w)
    launches = ctx.last_launches()
    c, _ = ctx.last_read_skews(len(reads))
    ll, st, off = ll.cpu().numpy(), st.cpu().numpy(), db.ref_off.cpu().numpy()
    return [ll[off[i]:off[i + 1]] for i in range(len(reads))], st, launches, c


def _all_substitutions(ref, alphabet):
    p = np.repeat(np.arange(ref.size), alphabet)
    b = np.tile(np.arange(alphabet), ref.size)
    return np.stack([p, b], 1)[b != ref[p]]


def _run_ell(oracle, case):
    if case['name'] in _runs:
        return _runs[case['name']]
    from nadavca_amd import dtw
    from nadavca_amd.call_indels import apply_edit
    mg, mo = _model(oracle, case['model'])
    ctx = mg.context
    k, central, alphabet = case['model'][:3]
    bw, mel, kind, reads = case['bandwidth'], case['mel'], case['kind'], case['reads']
    n = len(reads)
    tup = vc.reads_of(reads)
    worst, count, reports = 0.0, 0, []
    for w in (False, True):
        plain = [_oracle_ll(oracle, mo, r, bw, mel, w) for r in reads]
        totals = np.array([plain[j][0, r['reference'][0]] for j, r in enumerate(reads)])
        if kind in ('full', 'listed'):
            full, st, launches, c = _full_matrix(case, mg, reads, w)
            assert not st.any(), st
        if kind == 'full':
            for j in range(n):
                worst = max(worst, _close(full[j], plain[j], (case['name'], w, j)))
                count += full[j].size
        elif kind == 'listed':
            lists = [_all_substitutions(np.asarray(r['reference']), alphabet) for r in reads]
            lists[0] = lists[0][::-1]      # any order, duplicates, none
            lists[1] = np.concatenate([lists[1], lists[1][:5]])
            lists[3] = lists[3][:0]
            total, got, st = dtw.estimate_hypotheses_batch(tup, lists, bw, mel, mg, w, on_error='status',
                                                           return_status=True)
            launches = ctx.last_launches()
            c, _ = ctx.last_read_skews(n)
            assert not st.any(), st
            for j, rows in enumerate(lists):
                exp = np.ascontiguousarray(full[j][rows[:, 0], rows[:, 1]])
                assert np.array_equal(got[j].view(np.int64), exp.view(np.int64)), (case['name'], w, j)
                assert np.float64(total[j]).view(np.int64) == np.float64(full[j][0, reads[j]['reference'][0]]).view(np.int64)
                worst = max(worst, _close(got[j], plain[j][rows[:, 0], rows[:, 1]], (case['name'], w, j)))
                count += len(rows)
            _close(total, totals, (case['name'], w, 'total'))
        else:
            # the listed reads, and the last of them once more with a hypothesis of one row too many
            refs = [np.asarray(r['reference']) for r in reads]
            if kind == 'joint':
                lists = [vc.joint_list(refs[j], k, central, alphabet, case['lanes']) if j in case['hyp_reads'] else []
                         for j in range(n)]
                bad = lists[case['wide_read']] + [vc.joint_one_row_more(refs[case['wide_read']], k, central, alphabet)]
                run = dtw.estimate_joint_hypotheses_batch
            else:
                lists = [vc.edit_list(refs[j], reads[j]['approximate_alignment'], k, central, alphabet, case['lanes'])
                         if j in case['hyp_reads'] else [] for j in range(n)]
                bad = lists[case['wide_read']] + [vc.edit_one_row_more(refs[case['wide_read']], k, central, alphabet)]
                run = dtw.estimate_edit_hypotheses_batch
            total, got, st = run(tup + [tup[case['wide_read']]], lists + [bad], bw, mel, mg, w, on_error='status',
                                 return_status=True)
            launches = ctx.last_launches()
            c, _ = ctx.last_read_skews(n + 1)
            c = c[:n]
            assert st.tolist() == [READ_OK] * n + [READ_BAD_INPUT], st
            assert np.isnan(total[n]) and np.all(np.isnan(got[n]))
            for j, hs in enumerate(lists):
                exp = []
                for h in hs:
                    if kind == 'joint':
                        ref2 = refs[j].copy()
                        ref2[h[:-1, 0]] = h[:-1, 1]
                        exp.append(_oracle_ll(oracle, mo, reads[j], bw, mel, w, ref=ref2)[h[-1, 0], h[-1, 1]])
                    else:
                        ref2, anchors2, was_clean = apply_edit(reads[j]['reference'], reads[j]['approximate_alignment'], *h)
                        assert was_clean
                        exp.append(_oracle_ll(oracle, mo, reads[j], bw, mel, w, ref=ref2, anchors=anchors2)[0, ref2[0]])
                assert got[j].shape == (len(hs),)
                if hs:
                    worst = max(worst, _close(got[j], np.array(exp, dtype=float), (case['name'], w, j)))
                count += len(hs)
            _close(total[:n], totals, (case['name'], w, 'total'))
            assert count > 0
        assert len(launches) == 1 and launches[0]['op'] == 'ell', launches
        x = launches[0]
        assert x['lds_bytes'] <= LDS_LIMIT and x['H'] == max(x['c'] + 1, 2) and x['SR'] >= 64 * x['c'] + 128
        assert x['c'] == int(max(c)) and x['transitions'] == int(w)
        # both hand-overs of the sweeps: a read of skew 1 and one of skew >= 2 (sweep_fast<MEL, true / false>)
        assert int(c[case['wide_read']]) >= 2 and int(min(c)) == 1, c.tolist()
        reports.append((x['mel'], x['waves'], x['kind']))
    assert len(set(reports)) == 1
    _runs[case['name']] = dict(variant=reports[0], worst=worst, count=count, launch=x, skews=c.tolist())
    print('%s: ell_kernel<%d, %d, %s>, c_max %d, H %d, SR %d, %d B of LDS; skews %s; %d values, largest |difference| %.3e'
          % (case['name'], x['mel'], x['waves'], x['kind'], x['c'], x['H'], x['SR'], x['lds_bytes'], c.tolist(), count,
             worst))
    return _runs[case['name']]


@pytest.mark.parametrize('case', ELL, ids=[c['name'] for c in ELL])
def test_ell_case(oracle_port, case):
    run = _run_ell(oracle_port, case)
    assert run['variant'] == (case['mel'], case['lanes'], case['kind'])


def test_every_built_log_likelihood_kernel_was_run_and_compared(oracle_port):
    """ell_dispatch's tables hold the full product (csrc/kernels_ell.hip), 40 kernels."""
    ran = {_run_ell(oracle_port, case)['variant'] for case in ELL}
    assert ran == {(mel, lanes, kind) for mel in range(5) for lanes in (8, 16) for kind in vc.ELL_KINDS}
    assert len(ran) == 40


def test_a_read_above_the_log_likelihood_rings_is_refused_alone(oracle_port):
    """Skew above launch_ell's c_max: NVK_READ_TOO_WIDE for that read, the launch sized by the LDS fit, the other
    reads as the oracle has them."""
    case = vc.ell_too_wide_case()
    mg, mo = _model(oracle_port, case['model'])
    for w in (False, True):
        full, st, launches, c = _full_matrix(case, mg, case['reads'], w)
        wide = case['too_wide']
        assert st.tolist() == [READ_TOO_WIDE if j == wide else READ_OK for j in range(len(case['reads']))]
        assert len(launches) == 1 and launches[0]['c'] == vc.ELL_C_MAX < int(c[wide])
        assert launches[0]['lds_bytes'] <= LDS_LIMIT
        for j, r in enumerate(case['reads']):
            if j != wide:
                _close(full[j], _oracle_ll(oracle_port, mo, r, case['bandwidth'], case['mel'], w), (w, j))
