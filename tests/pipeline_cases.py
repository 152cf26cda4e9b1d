"""The batch of tests/test_gpu_host_pipeline.py: the smallest batch the pipelined host-pointer path (csrc/pipeline.hip)
still cuts five ways — 1300 reads of 20 to 780 bases, 5 498 437 samples (at least 5 x 2^20: five chunks of 8 MiB) —
with two tiny reads in front and four reads doctored so that the library refuses them, each in another chunk of the
growth-2 schedule.  No doctoring changes a signal, so the chunk schedule is that of the plain batch."""
import numpy as np

from nadavca_amd import synthetic

N_READS = 1300
N_SAMPLES = 5498437
BANDWIDTH = 150
MEL = 2
# the schedule of (chunks 5, growth 2.0, min reads 1) the doctored reads are placed by; the GPU test's fixture checks it
GROWTH2_CHUNKS = [(0, 40), (40, 121), (121, 287), (287, 619), (619, 1300)]
TINY = (0, 1)          # 20 bases, no contexts, no anchors: the band is the whole matrix
BAD_CODE = 40          # first read of chunk 1: a base code = alphabet size   -> READ_BAD_INPUT (-1)
SWAPPED = 286          # last read of chunk 2: two anchors exchanged          -> READ_BAD_BAND (-2)
NO_PATH = 618          # last read of chunk 3: fewer than 2 R samples         -> READ_NO_PATH (1)
TOO_WIDE = 900         # chunk 4: 381 bases, 4223 samples, anchors removed    -> READ_TOO_WIDE (-3)
STATUS = {BAD_CODE: -1, SWAPPED: -2, NO_PATH: 1, TOO_WIDE: -3}


def make_cases(model):
    """-> the list of make_dp_case dicts, doctored, for a model tuple of ``synthetic.load_model_arrays``."""
    alphabet = model[2]
    cases = list(synthetic.make_batch(N_READS, model, seed=5, R=400, R_spread=380, bandwidth=BANDWIDTH).cases)
    none = np.zeros(0, dtype=np.int32)
    for i in TINY:
        cases[i] = dict(cases[i], reference=cases[i]['reference'][:20].copy(), context_before=none,
                        context_after=none, approximate_alignment=np.zeros((0, 2), dtype=np.int32))
    ref = cases[BAD_CODE]['reference'].copy()
    ref[len(ref) // 2] = alphabet
    cases[BAD_CODE] = dict(cases[BAD_CODE], reference=ref)
    # two anchors far apart with their samples exchanged: the prefix maximum passes the suffix minimum
    anc = cases[SWAPPED]['approximate_alignment'].copy()
    i, j = 3, len(anc) - 4
    assert int(anc[j][0]) - int(anc[i][0]) > 2 * BANDWIDTH + 2
    anc[i, 0], anc[j, 0] = int(anc[j][0]), int(anc[i][0])
    cases[SWAPPED] = dict(cases[SWAPPED], approximate_alignment=anc)
    # more bases than half the samples: every base needs MEL samples, no path
    c = cases[NO_PATH]
    longer = len(c['signal']) // 2 + 20
    extra = np.random.default_rng([5, NO_PATH, 1]).integers(0, alphabet, longer - len(c['reference']))
    cases[NO_PATH] = dict(c, reference=np.concatenate([c['reference'], extra]).astype(np.int32))
    cases[TOO_WIDE] = dict(cases[TOO_WIDE], approximate_alignment=np.zeros((0, 2), dtype=np.int32))
    return cases


def flat_of(dtw, cases, lo=0, hi=None):
    """reads [lo, hi) as a dtw.FlatBatch (the flat arrays rebuilt from the doctored reads)"""
    return dtw.FlatBatch([(c['signal'], c['reference'], c['context_before'], c['context_after'],
                           c['approximate_alignment']) for c in cases[lo:hi]])
