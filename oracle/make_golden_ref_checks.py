"""TEST INFRASTRUCTURE ONLY — regenerate tests/golden/ref_checks.npz.

The outputs of the reference's own DP (oracle/_ref/libnadavca_ref.so, built by ``make -C oracle ref``) for
the two checks that used to need oracle/_ref at test time, so that they run wherever the suite runs:

  r<i>_*           tests/test_oracle_golden.py: six random cases (synthetic.make_dp_case, default_rng([55, i]),
                   4-mer model of synth_model_arrays(3)) — inputs, refine_alignment and
                   estimate_log_likelihoods with the flag on / off (``_f1`` / ``_f0``)
  cfg2_sha1_t1/t0  tests/test_gpu_parity_full.py: sha1 of the int32 (R, 2) event rows of each of the first 500
                   reads of bench.py's cfg2_align batch (seed 1000), transitions on / off

Usage (where oracle/_ref is built): python3 oracle/make_golden_ref_checks.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle  # noqa: E402
from nadavca_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ref_checks.npz')
N_RANDOM = 6
N_CFG2 = 500


def random_cases():
    """-> (model arrays, [(case, bandwidth, min_event_length)]) of the bit-identity check."""
    model = synthetic.synth_model_arrays(3, k=4, central=1)
    cases = []
    for i in range(N_RANDOM):
        rng = np.random.default_rng([55, i])
        c = synthetic.make_dp_case(rng, model, R=40 + 5 * i, bandwidth=20 + i, dwell=(2, 7), jitter=4)
        cases.append((c, 20 + i, [2, 1, 3, 0, 2, 2][i]))
    return model, cases


def events_sha1(ev):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(np.asarray(ev).reshape(-1, 2),
                                                           dtype=np.int32).tobytes()).digest(), dtype=np.uint8)


def main():
    ref = Oracle('reference')
    blob = {}
    model, cases = random_cases()
    mr = ref.KmerModel(*model)
    for i, (c, bw, mel) in enumerate(cases):
        for key in ('signal', 'reference', 'context_before', 'context_after', 'approximate_alignment'):
            blob['r%d_%s' % (i, key)] = c[key]
        a = (c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'],
             bw, mel, mr)
        for flag in (1, 0):
            blob['r%d_refine_f%d' % (i, flag)] = ref.refine_alignment(*a, bool(flag)).astype(np.int32)
            blob['r%d_ell_f%d' % (i, flag)] = ref.estimate_log_likelihoods(*a, bool(flag))
    cmodel = synthetic.load_model_arrays()
    mc = ref.KmerModel(*cmodel)
    wl = dict(synthetic.WORKLOADS['cfg2_align'])
    wl.pop('n_reads')
    batch = synthetic.make_batch(N_CFG2, cmodel, seed=1000, **wl)
    for tr in (1, 0):
        blob['cfg2_sha1_t%d' % tr] = np.stack([
            events_sha1(ref.refine_alignment(c['signal'], c['reference'], c['context_before'], c['context_after'],
                                             c['approximate_alignment'], wl['bandwidth'], 2, mc, bool(tr)))
            for c in batch.cases])
    np.savez_compressed(OUT, **blob)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
