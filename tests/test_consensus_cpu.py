"""tests/consensus_ref.py against the reference: the long-double restatement of the consensus sums and the posterior
reproduces every chunk of tests/golden/consensus_cases.npz (the reference's own estimate_probabilities on constructed
log-likelihoods; oracle/make_golden_consensus.py) within the chain bound the module derives.  No GPU."""
import numpy as np
import pytest

import consensus_ref as CR


@pytest.fixture(scope='module')
def cases():
    return CR.load_cases()


def test_the_golden_holds_the_cases_it_is_there_for(cases):
    assert {c.k for c in cases} == {1, 2, 3, 6}
    assert {c.snp_prior for c in cases} == {1e-6, 0.001, 0.01}
    assert {c.nel for c in cases} == {1.0, 3.0, 10.0}
    for c in cases:
        assert len(c.genome.item()) <= 300 and set(c.reverse) == {0, 1}
        lengths = c.reads[:, 1] - c.reads[:, 0]
        assert lengths.min() == 1 and lengths.max() <= 40
        groups = [e - s for s, e in CR.group_ranges(c.ranges)]
        assert {1, c.k, 2 * c.k - 1, 2 * c.k} - {0} <= set(groups)
        assert {c.k - 1, 2 * c.k - 2} - {0} <= set(groups)
        assert set(c.kinds) == {0, 1, 2, 3}
        # touching chunks stayed apart, and some chunk holds several reads
        assert any(a[1] == b[0] for a, b in zip(c.cons_ranges[:-1], c.cons_ranges[1:]))
        assert c.cons_coverage.max() >= 3
    values = np.concatenate([c.cons_values for c in cases])
    assert (values == 0).any()                                    # some exp were exactly 0
    assert (np.sort(values, axis=1)[:, -2] > 1e-3).mean() > 0.2   # a second base often matters
    assert (values.argmax(axis=1) != np.concatenate(
        [np.concatenate([c.codes[s:e] for s, e in c.cons_ranges]) for c in cases])).mean() > 0.05  # others win


def test_positivity_condition_holds_for_every_case(cases):
    for c in cases:
        assert CR.priors_positive(c.snp_prior, c.k, 4)
        for w in range(1, 2 * c.k):
            snp_h, non_h = CR.corrected_priors(w - 1, c.snp_prior, 4)
            assert snp_h > 0 and non_h > 0


def test_group_ranges_gives_the_golden_chunk_intervals(cases):
    from nadavca_amd.estimator import ProbabilityEstimator
    for c in cases:
        want = [tuple(r) for r in c.cons_ranges.tolist()]
        assert ProbabilityEstimator.group_ranges(c.ranges) == want
        assert CR.group_ranges(c.ranges) == want


def test_restatement_reproduces_the_golden_consensus(cases):
    worst = 0.0
    for c in cases:
        groups, cov, post, seg_off = CR.expected_consensus(c)
        assert groups == [tuple(r) for r in c.cons_ranges.tolist()]
        assert np.array_equal(np.concatenate([cov[s:e] for s, e in groups]), c.cons_coverage)
        assert np.isfinite(post.want.astype(np.float64)).all()
        worst = max(worst, CR.ratio(c.cons_values, post.want, CR.tolerance(post)))
    print('reference float64 against the restatement, consensus chunks: error / bound at most %.3f' % worst)
    assert worst <= 1.0


def test_restatement_reproduces_the_golden_independent_chunks(cases):
    worst = 0.0
    for c in cases:
        assert np.array_equal(c.ind_ranges, c.reads[:, :2])
        post = CR.expected_independent(c)
        worst = max(worst, CR.ratio(c.ind_values, post.want, CR.tolerance(post)))
    print('reference float64 against the restatement, independent chunks: error / bound at most %.3f' % worst)
    assert worst <= 1.0


def test_the_window_and_the_priors_matter_in_the_golden(cases):
    """What the older fixture could not show: leaving the context out, or the window one wider, moves the golden's
    values by far more than any bound here."""
    for c in cases:
        if c.k == 1:
            continue
        groups, cov, post, seg_off = CR.expected_consensus(c)
        pos = np.concatenate([np.arange(s, e) for s, e in groups])
        acc, _, _ = CR.accumulate(c.ll, c.reference, c.ref_off, c.chunk_start, c.reverse, None, c.nel, len(c.codes))
        for other_k in (1, c.k + 1):
            other = CR.posterior(acc[pos], c.codes[pos], seg_off, other_k, c.snp_prior)
            assert CR.ratio(other.want, post.want, CR.tolerance(post)) > 1e6
