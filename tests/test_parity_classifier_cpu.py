"""The gate of the parity contract, tested on the CPU: fuzz_cases.classify_difference accepts a read that differs
from the reference only where its path is an arg-max of the reference's path objective to within
d * NVK_TIE_ULPS ulps of the reference's log score (include/nadavca_hip.h, PARITY CONTRACT).

The stand-in engine is the reference's own answer with one boundary moved: such mutants are what a kernel that
misplaces a boundary would return.  Two read sets: ``random`` — make_fuzz_batch(20261004, it), it < 60 (few-level
k-mer models, where equal adjacent levels are common) — and ``packaged`` — 60 reads of make_run_batch on the
packaged 6-mer model, homopolymer-rich bases, half of them quantised to 1/12.

Every expected verdict is computed here from LongDoubleReferee.path_score alone, not taken from the classifier."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fuzz_cases
from fuzz_cases import NVK_TIE_ULPS, classify_difference, flat_row, make_fuzz_batch, make_run_batch, same_level_bases

SEED = 20261004
THREADS = max(1, min(16, os.cpu_count() or 1))   # the oracle's ctypes calls release the GIL


def _map(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


class _Read:
    """One read with everything the tests share: the double reference's rows, the long-double reference's, the
    better of their two scores and the path that reaches it."""

    def __init__(self, fb, case, oracle, mo, ld):
        from oracle.oracle import LongDoubleReferee
        self.fb, self.case, self.ld = fb, case, ld
        c = case
        self.args = (c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'],
                     fb['bw'], fb['mel'], fb['tr'])
        self.R = len(c['reference'])
        self.exp = oracle.refine_alignment(*self.args[:7], mo, fb['tr'])
        self.hp = ld.refine_alignment(*self.args)
        self.ok = self.exp.shape == (self.R, 2) and self.hp.shape == (self.R, 2)
        if not self.ok:
            return
        self.s_ref, self.s_ld = ld.path_scores(*self.args, [self.exp, self.hp])
        assert self.s_ref is not None and self.s_ld is not None   # the reference's own paths are valid paths
        better = self.exp if self.s_ref[0] >= self.s_ld[0] else self.hp
        self.best, self.max_abs = max(self.s_ref, self.s_ld, key=lambda x: x[0]) if self.s_ref[0] != self.s_ld[0] \
            else self.s_ref
        self.p_best = LongDoubleReferee.events_to_path(better, self.R, fb['tr'])
        k, central, alphabet = fb['model'][:3]
        self.same_level = same_level_bases(c, fb['model'], k, central, alphabet)

    def verdict(self, ev):
        """-> (valid, within the margin, deficit / margin) of rows ``ev`` by the definition of the contract."""
        from oracle.oracle import LongDoubleReferee
        s = self.ld.path_score(*self.args, ev)
        if s is None:
            return False, False, None
        d = int((LongDoubleReferee.events_to_path(ev, self.R, self.fb['tr']) != self.p_best).sum())
        margin = d * NVK_TIE_ULPS * np.longdouble(2.0) ** -52 * self.max_abs
        deficit = self.best - s[0]
        return True, bool(deficit <= margin), (float(deficit / margin) if margin > 0 else None)

    def classify(self, ev):
        fb = self.fb
        k, central, alphabet = fb['model'][:3]
        return classify_difference(ev, self.exp, self.case, fb['model'], k, central, alphabet, fb['bw'], fb['mel'],
                                   fb['tr'], referee=self.ld)

    def moved(self, j, delta):
        """The reference's rows with the boundary between bases j - 1 and j moved by ``delta`` samples."""
        ev = self.exp.copy()
        ev[j - 1, 1] += delta
        ev[j, 0] += delta
        return ev

    def old_criterion(self, ev):
        """What the classifier accepted as 'flat-plateau' before it scored paths."""
        rows = np.nonzero((ev != self.exp).any(axis=1))[0]
        return len(rows) > 0 and all(flat_row(ev, self.exp, self.same_level, j) for j in rows)


@pytest.fixture(scope='module')
def read_sets(oracle_port):
    from oracle.oracle import LongDoubleReferee
    sets = {'random': [], 'packaged': []}
    for name, batches in (('random', (make_fuzz_batch(SEED, it) for it in range(60))),
                          ('packaged', (make_run_batch(SEED, it, n_reads=6, all_runs=True) for it in range(10)))):
        for fb in batches:
            mo = oracle_port.KmerModel(*fb['model'])
            ld = LongDoubleReferee(*fb['model'])
            sets[name] += [r for r in _map(lambda c: _Read(fb, c, oracle_port, mo, ld), fb['cases']) if r.ok]
    return sets


@pytest.fixture(scope='module')
def equal_level_mutants(read_sets):
    """Per read set, one record per mutant: the reference's rows with one boundary between two EQUAL-level bases
    (the middle one of the read's) moved by -2, -1, +1 or +2 samples -> (old criterion, valid, within the margin,
    deficit / margin, the classifier's verdict)."""
    out = {}
    for name, reads in read_sets.items():
        mutants = []
        for r in reads:
            js = np.nonzero(r.same_level)[0]
            if len(js):
                mutants += [(r, r.moved(int(js[len(js) // 2]), delta)) for delta in (-2, -1, 1, 2)]
        out[name] = _map(lambda m: (m[0].old_criterion(m[1]),) + m[0].verdict(m[1]) + (m[0].classify(m[1]),), mutants)
    return out


@pytest.mark.parametrize('name,floor', [('random', 0.8), ('packaged', 0.9)])
def test_equal_level_mutants_are_scored_not_waved_through(equal_level_mutants, name, floor):
    """One boundary between two bases of EQUAL k-mer level moved by 1 or 2 samples.  Every such mutant meets the
    condition that alone made a difference a 'flat-plateau' before paths were scored; now the verdict is
    'flat-plateau' exactly where the mutant is a valid path within the margin, 'UNEXPLAINED' otherwise.
    Rejected here: 0.93 of 400 mutants on the random-model set, 228 of 228 on the packaged-model set (floors
    against vacuity: 0.8 and 0.9)."""
    n = rejected = 0
    worst = 0.0
    for old, valid, within, ratio, why in equal_level_mutants[name]:
        assert old                          # the hole being closed: all of these used to pass
        assert why == ('flat-plateau' if valid and within else 'UNEXPLAINED'), (why, valid, within, ratio)
        n += 1
        rejected += why == 'UNEXPLAINED'
        if valid and within and ratio is not None:
            worst = max(worst, ratio)
    print('%s: %d equal-level mutants, %d rejected (%.3f); largest deficit/margin among the accepted: %.3g'
          % (name, n, rejected, rejected / max(n, 1), worst))
    assert n >= 150
    assert rejected >= floor * n, (rejected, n)


def test_true_plateaus_are_still_accepted(equal_level_mutants):
    """Positive control: the equal-level mutants whose deficit is within the margin — boundaries that really sit
    on a flat stretch of the posterior — are accepted as 'flat-plateau', and there are such mutants
    (27 of 628 here)."""
    n = 0
    for name in ('random', 'packaged'):
        for old, valid, within, ratio, why in equal_level_mutants[name]:
            if valid and within:
                assert why == 'flat-plateau'
                n += 1
    print('%d true plateaus accepted' % n)
    assert n >= 10


def test_any_boundary_mutants_are_rejected(read_sets):
    """One path row of the reference's answer, any row, moved by 1 or 2 samples (four mutants per read): at least
    0.99 of the mutants are rejected (1 368 of 1 368 here), and one that is accepted is within the margin."""
    rng = np.random.default_rng([SEED, 1])
    mutants = []
    for name in ('random', 'packaged'):
        for r in read_sets[name]:
            for _ in range(4):
                ev = r.exp.copy()
                delta = int(rng.choice([-2, -1, 1, 2]))
                if r.fb['tr']:
                    ev.reshape(-1)[int(rng.integers(0, 2 * r.R))] += delta
                else:
                    j = int(rng.integers(0, r.R + 1))   # boundary j: the end of base j - 1 and the start of base j
                    if j > 0:
                        ev[j - 1, 1] += delta
                    if j < r.R:
                        ev[j, 0] += delta
                mutants.append((r, ev))
    n = rejected = 0
    for (valid, within, ratio), why in _map(lambda m: (m[0].verdict(m[1]), m[0].classify(m[1])), mutants):
        n += 1
        if why == 'UNEXPLAINED':
            rejected += 1
        else:
            assert valid and within, (why, ratio)
    print('%d any-boundary mutants, %d rejected' % (n, rejected))
    assert n >= 1200 and rejected >= 0.99 * n, (rejected, n)


def test_long_double_rows_are_accepted_and_the_reference_stays_inside_the_gate(read_sets):
    """Positive control: where the long-double reference's rows differ from the double reference's, they are
    accepted (no label needs a flat row: the referee sides with them on every row).  And the reference alone
    stays inside the gate it sets: on those reads the deficit of the double path against the better of the two
    is within ONE margin (d = 1; at most 0.006 of it on the 15 such reads here)."""
    n = 0
    worst = 0.0
    for name in ('random', 'packaged'):
        for r in read_sets[name]:
            if np.array_equal(r.exp, r.hp):
                continue
            n += 1
            why = r.classify(r.hp)
            assert why in ('reference-rounding', 'flat-plateau'), why
            one = NVK_TIE_ULPS * np.longdouble(2.0) ** -52 * r.max_abs
            deficit = r.best - r.s_ref[0]
            assert deficit <= one, (float(deficit), float(one))
            worst = max(worst, float(deficit / one))
    print('%d reads where double and long double differ; largest deficit of the double path: %.3g of one margin'
          % (n, worst))
    assert n >= 5


def test_malformed_rows_are_unexplained(read_sets):
    """Rows that are no path of the search: wrong shape, rows that do not join up without transition rows, a
    boundary outside its band, an event shorter than min_event_length."""
    plain = next(r for r in read_sets['random'] if not r.fb['tr'] and r.R >= 8 and r.fb['mel'] >= 2)
    trans = next(r for r in read_sets['random'] if r.fb['tr'] and r.R >= 8 and r.fb['mel'] >= 2)
    for r in (plain, trans):
        assert r.classify(r.exp[:-1]) == 'UNEXPLAINED'
        assert r.classify(np.concatenate([r.exp, r.exp[-1:]])) == 'UNEXPLAINED'
        ev = r.exp.copy()                       # event 3 made shorter than the minimum event length
        ev[3, 1] = ev[3, 0] + r.fb['mel'] - 1
        ev[4, 0] = ev[3, 1]
        assert r.verdict(ev)[0] is False
        assert r.classify(ev) == 'UNEXPLAINED'
        ev = r.exp.copy()                       # the last boundary beyond the end of the signal
        ev[-1, 1] = len(r.case['signal']) + 1
        assert r.classify(ev) == 'UNEXPLAINED'
        ev = r.exp.copy()                       # the first boundary left of the band
        ev[0, 0] = -1
        assert r.classify(ev) == 'UNEXPLAINED'
    ev = plain.exp.copy()                       # a gap between two events where there are no transition rows
    ev[4, 0] += 1
    assert plain.classify(ev) == 'UNEXPLAINED'
    assert fuzz_cases.SCORED[-1]['valid'] is False
