"""TEST INFRASTRUCTURE ONLY (build container only) — regenerate tests/golden/consensus_cases.npz.

Runs the reference's OWN ``ProbabilityEstimator.estimate_probabilities`` (imported in place by oracle/pyref.py) on
constructed log-likelihood matrices, so that everything after the DP — normalise, strand flip, sort, group, per-position
sum, coverage, corrected priors, posterior — is reference code on inputs chosen to make the context window, the
priors and the chunk borders matter.  Substitutions are at the edges only:

  * an aligner whose ``get_signal_alignment`` returns the read's prepared reference range and strand,
  * ``nadavca.dtw.estimate_log_likelihoods`` returning the prepared matrix of the read in hand (it also checks that
    the reference part it is handed is the one tests/consensus_ref.py derives from the stored genome),
  * a k-mer model object answering ``get_k()`` / ``get_central_position()``,
  * ``tweak_signal_normalization`` off.

Stored per case c<i>_: genome, k, snp_prior, nel, reads (n, 3: start, end, reverse), ll (sum R, 4: the reads' rows end
to end, in read order), kinds (n,: index into KINDS), and the reference's results: cons_ranges (chunks, 2), cons_values
and cons_coverage (the chunks end to end) of ``estimate_probabilities(genome, reads)``, ind_ranges (n, 2) and ind_values
(sum R, 4) of ``estimate_probabilities(genome, [read])[0]`` per read.  Usage:  python3 oracle/make_golden_consensus.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'consensus_cases.npz')
LIMIT = os.path.join(ROOT, 'tests', 'golden', 'estimator.npz')
ALPHA = 4
KS = (1, 2, 3, 6)
PRIORS = (1e-6, 0.001, 0.01)
NELS = (1, 3, 10)
KINDS = ('normal', 'refwins', 'tied', 'spread')
KIND_CYCLE = (0, 0, 1, 0, 2, 0, 3)
SEED = 20260


def priors_positive(snp_prior, k, alpha=ALPHA):
    """Both corrected priors are positive for every window of up to 2k - 1 positions:
    p1/p2 > (context_positions - 1) * (alphabet - 1) keeps the SNP hypotheses' prior positive, one more position's
    worth keeps the reference hypothesis' prior positive too."""
    c = alpha - 1
    ratio = (1 - snp_prior) / (snp_prior / c)
    ctx = 2 * k - 2
    return ratio > (ctx - 1) * c and ratio > ctx * c


def layout(k):
    """Chunk intervals: alone (lengths 1, k-1, k, 2k-2, 2k-1, 2k), touching, overlapping in a chain, nested
    -> (intervals, genome length)"""
    spans, c = [], 2
    for length in sorted({1, k - 1, k, 2 * k - 2, 2 * k - 1, 2 * k} - {0}):
        spans.append((c, c + length))
        c += length + 2
    for length in (5, k, 1):  # touching: must not merge
        spans.append((c, c + length))
        c += length
    c += 3
    spans += [(c, c + 20), (c + 10, c + 40), (c + 35, c + 50), (c + 49, c + 60)]  # overlapping
    c += 63
    spans += [(c, c + 40), (c + 5, c + 12), (c + 5, c + 6), (c + 5, c + 12), (c + 20, c + 40), (c + 39, c + 40),
              (c, c + 1)]  # nested, one interval twice, ends shared with the container
    c += 40
    spans.append((c, c + 7))  # touches the nest's end
    c += 7
    return spans, c + 3


def read_rows(rng, kind, refpart, nel):
    """The DP's output for one read as the generator makes it up: (R, 4) rows against ``refpart``, the read's
    strand-corrected reference codes"""
    R = len(refpart)
    ll = rng.normal(-30.0, 12.0, (R, ALPHA))
    at = np.arange(R)
    if kind == 'refwins':
        ll = rng.normal(-200.0, 12.0, (R, ALPHA))
        ll[at, refpart] = rng.normal(-5.0, 1.0, R)
    elif kind == 'tied':
        for p in range(R):
            if rng.integers(0, 2):
                ll[p, :] = np.round(ll[p, 0])  # all four equal
            else:
                others = [b for b in range(ALPHA) if b != refpart[p]]
                ll[p, others[1]] = ll[p, others[0]]  # two non-reference bases equal
    elif kind == 'spread':
        for p in range(0, R, 3):
            others = [b for b in range(ALPHA) if b != refpart[p]]
            ll[p, others[int(rng.integers(0, 3))]] = -30.0 - 2000.0 * nel  # -2000 after the division: exp is 0
    return ll


class _Apx:
    def __init__(self, start, end, reverse):
        self.reference_range = (start, end)
        self.reverse_complement = bool(reverse)
        self.signal_range = (0, 0)
        self.read_sequence_range = (0, 0)
        self.alignment = None


class _Read:
    normalized_signal = np.zeros(0)
    sequence = ''

    def __init__(self, apx, ll, refpart):
        self.apx, self.ll, self.refpart = apx, ll, refpart


class _Aligner:
    current = None

    def get_signal_alignment(self, read, bandwidth):
        self.current = read
        return read.apx


class _Model:
    def __init__(self, k):
        self.k = k

    def get_k(self):
        return self.k

    def get_central_position(self):
        return (self.k - 1) // 2


def main():
    pyref.load()
    import nadavca.dtw as rdtw
    import nadavca.estimator as rest
    from nadavca.alphabet import alphabet

    assert len(alphabet) == ALPHA
    aligner = _Aligner()

    def prepared(signal, reference, **kw):
        read = aligner.current
        assert np.array_equal(np.asarray(reference), read.refpart)
        return read.ll.copy()

    rdtw.estimate_log_likelihoods = prepared

    rng = np.random.default_rng(SEED)
    blob, zeros, n_case = {}, 0, 0
    for ki, k in enumerate(KS):
        for pi, snp_prior in enumerate(PRIORS):
            nel = NELS[(ki + pi) % 3]
            assert priors_positive(snp_prior, k)
            spans, glen = layout(k)
            codes = rng.integers(0, ALPHA, glen)
            genome = [alphabet[c] for c in codes]
            order = rng.permutation(len(spans))
            kinds = np.array([KIND_CYCLE[i % len(KIND_CYCLE)] for i in range(len(spans))])
            rng.shuffle(kinds)
            reverse = rng.integers(0, 2, len(spans))
            reverse[:2] = (0, 1)
            reads, rows = [], []
            for j, idx in enumerate(order):
                s, e = spans[idx]
                refpart = codes[s:e] if not reverse[j] else (ALPHA - 1 - codes[s:e])[::-1]
                ll = read_rows(rng, KINDS[kinds[j]], refpart, nel)
                reads.append(_Read(_Apx(s, e, reverse[j]), ll, refpart))
                rows.append((s, e, int(reverse[j])))
            config = dict(bandwidth=10, snp_prior_probability=snp_prior, min_event_length=2, model_wobbling=True,
                          model_transitions=True, tweak_signal_normalization=False, normalization_event_length=nel)
            est = rest.ProbabilityEstimator(_Model(k), aligner, config)
            chunks = est.estimate_probabilities(genome, reads)
            ind = [est.estimate_probabilities(genome, [r])[0] for r in reads]
            pre = 'c%d_' % n_case
            blob[pre + 'genome'] = np.array(''.join(genome))
            blob[pre + 'k'] = np.int64(k)
            blob[pre + 'snp_prior'] = np.float64(snp_prior)
            blob[pre + 'nel'] = np.float64(nel)
            blob[pre + 'reads'] = np.array(rows, dtype=np.int64)
            blob[pre + 'kinds'] = kinds.astype(np.int64)
            blob[pre + 'll'] = np.concatenate([r.ll for r in reads]).astype(np.float64)
            blob[pre + 'cons_ranges'] = np.array([(c.start, c.end) for c in chunks], dtype=np.int64)
            blob[pre + 'cons_values'] = np.concatenate([np.asarray(c.values, dtype=np.float64) for c in chunks])
            blob[pre + 'cons_coverage'] = np.concatenate([np.asarray(c.coverage, dtype=np.int64) for c in chunks])
            blob[pre + 'ind_ranges'] = np.array([(c.start, c.end) for c in ind], dtype=np.int64)
            blob[pre + 'ind_values'] = np.concatenate([np.asarray(c.values, dtype=np.float64) for c in ind])
            assert np.isfinite(blob[pre + 'cons_values']).all() and np.isfinite(blob[pre + 'ind_values']).all()
            assert set(reverse) == {0, 1} and set(kinds) == set(range(len(KINDS)))
            zeros += int((blob[pre + 'cons_values'] == 0).sum()) + int((blob[pre + 'ind_values'] == 0).sum())
            n_case += 1
    assert zeros > 0  # some exp were exactly 0
    blob['n_cases'] = np.int64(n_case)
    blob['kind_names'] = np.array(KINDS)
    np.savez_compressed(OUT, **blob)
    size = os.path.getsize(OUT)
    assert size <= os.path.getsize(LIMIT), size
    print('consensus_cases.npz %d KiB; %d cases; %d exact zeros' % (size // 1024, n_case, zeros))


if __name__ == '__main__':
    main()
