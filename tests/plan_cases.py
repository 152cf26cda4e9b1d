"""Seeded reads at the sizes where the align planner (csrc/kernels_plan.hip) changes path, shared by
tests/test_gpu_plan_shapes.py and tools/record_plan_totals.py.

A case is one refine_alignment batch: ``dict(name, model, bandwidth, mel, transitions, reads, bad)`` with ``reads`` a
list of make_dp_case dicts and ``bad`` the indices of the reads that carry a base code outside the alphabet.  Every
shape is a batch of ONE read, so the planner totals recorded for it are per read; the ``mixed_*`` cases at the end hold
every read of one (model, bandwidth, min event length, transitions) setting once more as one batch."""
import numpy as np

from nadavca_amd import synthetic

# (seed, k, central) of synthetic.synth_model_arrays
BASE = (11, 5, 2)
K2 = (12, 2, 0)
K10 = (13, 10, 4)
PLATEAU = ('plateau',) + BASE

# band rows (R + 1) up to which plan_kernel keeps a read's bands in LDS (PLAN_BCAP, kernels_plan.hip)
PLAN_BCAP = 1024

_models = {}


def model_arrays(key):
    """-> (k, central, alphabet, mean, sigma) of a model key."""
    if key not in _models:
        if key[0] == 'plateau':
            # the base table with the levels of bases 20 and 21 of the plateau read made equal
            k, central, alphabet, mean, sigma = synthetic.synth_model_arrays(*key[1:])
            c = _plateau_read()
            ext = np.concatenate([c['context_before'], c['reference'], c['context_after']])
            ids = synthetic.kmer_ids(ext, len(c['context_before']), len(c['reference']), k, central, alphabet)
            mean = mean.copy()
            mean[ids[21]] = mean[ids[20]]
            _models[key] = (k, central, alphabet, mean, sigma)
        else:
            _models[key] = synthetic.synth_model_arrays(*key)
    return _models[key]


def _read(seed, R, bandwidth, model=BASE, dwell=(2, 4), **kw):
    rng = np.random.default_rng([20240, *seed])
    kw.setdefault('jitter', 4)
    kw.setdefault('trim', min(3, R // 3))
    kw.setdefault('anchor_density', 0.6)
    return synthetic.make_dp_case(rng, model_arrays(model), R=R, bandwidth=bandwidth, dwell=dwell, **kw)


def _plateau_read():
    return _read((5, 0), 70, 30, dwell=(3, 4))


def _case(name, reads, bandwidth=30, mel=2, transitions=True, model=BASE, bad=()):
    return dict(name=name, model=model, bandwidth=bandwidth, mel=mel, transitions=transitions, reads=list(reads),
                bad=tuple(bad))


def _anchor_cases():
    bw = 30
    c = _read((7, 0), 60, bw, dwell=(3, 4))
    anc = c['approximate_alignment']
    out = [_case('anchors_none', [dict(c, approximate_alignment=np.zeros((0, 2), dtype=np.int32))], bw)]
    # the same row twice: the later anchor wins (dtw.cpp:11-15), also when it comes out of order and on row R
    dup = np.array([[int(anc[3][0]) + 5, int(anc[3][1])]], dtype=np.int32)
    last = np.array([[len(c['signal']) - 2, 60]], dtype=np.int32)
    out.append(_case('anchors_duplicated', [dict(c, approximate_alignment=np.concatenate(
        [anc[:6], dup, anc[6:][::-1], last]).astype(np.int32))], bw))
    # bands clipped at both ends of the slice: the slice loses half a bandwidth on either side
    cut = bw // 2
    sig = c['signal'][cut:len(c['signal']) - cut]
    clipped = anc.copy()
    clipped[:, 0] = np.clip(clipped[:, 0] - cut, 0, len(sig) - 1)
    out.append(_case('anchors_clipped', [dict(c, signal=np.ascontiguousarray(sig), approximate_alignment=clipped)],
                     bw))
    # two anchors far apart with their samples exchanged: the prefix maximum passes the suffix minimum
    swapped = anc.copy()
    i, j = 3, len(anc) - 4
    assert int(anc[j][0]) - int(anc[i][0]) > 2 * bw + 2
    swapped[i, 0], swapped[j, 0] = anc[j][0], anc[i][0]
    out.append(_case('anchors_out_of_order', [dict(c, approximate_alignment=swapped)], bw))
    return out


def _bad_code_case():
    good = _read((8, 0), 40, 30, dwell=(3, 4))
    other = _read((8, 1), 50, 30, dwell=(3, 4))
    ref = other['reference'].copy()
    ref[17] = 4
    third = _read((8, 2), 45, 30, dwell=(3, 4))
    ca = third['context_after'].copy()
    ca[0] = -1
    return _case('bad_codes', [dict(other, reference=ref), dict(third, context_after=ca), good], 30, bad=(0, 1))


def build_cases():
    cases = []
    # transition rows, T = 2 R: the smallest reads, no / first offset pass (T > 64), the block stride, T = VT and one
    # past it (uniform offsets), and R + 1 below / at / above PLAN_BCAP (R = 1024 is both)
    # R = 126 / 127: T = 252 / 254, the rows a block writes per round of its last phase (63 per wave, lane 0 only
    # hands the row above over) and the first read that needs a second round
    for R in (1, 2, 32, 33, 126, 127, 128, 129, PLAN_BCAP - 2, PLAN_BCAP - 1, 1024, 1025):
        cases.append(_case('trans_R%d' % R, [_read((1, R), R, 30)], 30))
    # no transition rows, T = R + 1
    # (R = 62 / 63: T = 63 / 64, one wave's rows of a round and one more; R = 251 / 252: T = 252 / 253, a block's)
    for R in (62, 63, 64, 251, 252, 255, 256, PLAN_BCAP - 2, PLAN_BCAP - 1, PLAN_BCAP):
        cases.append(_case('plain_R%d' % R, [_read((2, R), R, 30)], 30, transitions=False))
    for mel in range(5):
        for tr in (True, False):
            lo = max(mel, 2)
            cases.append(_case('mel%d_%s_R129' % (mel, 'trans' if tr else 'plain'),
                               [_read((3, mel), 129, 30, dwell=(lo, lo + 2))], 30, mel=mel, transitions=tr))
    cases += _anchor_cases()
    cases.append(_bad_code_case())
    # a band this wide for its row spacing is swept by a team of waves (skew above ALIGN1_C_CAP)
    for tr in (True, False):
        cases.append(_case('team_R300_%s' % ('trans' if tr else 'plain'),
                           [_read((4, 0), 300, 200, dwell=(2, 3), jitter=10)], 200, transitions=tr))
    # ... and a team read of more than PLAN_BCAP band rows.  (Without transition rows the read of seed (4, 1) carries
    # NVK_TIE_ULP beside its plateau mark and differs from the oracle in two rows, which the tie contract of
    # include/nadavca_hip.h allows and test_plan_shape does not; the read of seed (4, 2) has no tie.)
    for tr, seed in ((True, (4, 1)), (False, (4, 2))):
        cases.append(_case('team_R1100_%s' % ('trans' if tr else 'plain'),
                           [_read(seed, 1100, 200, dwell=(2, 3), jitter=10)], 200, transitions=tr))
    # the other min event lengths above PLAN_BCAP band rows: T = 1031 without transition rows, and T = PLAN_VT with
    # them, the last size whose per-row offsets come from the fixed point
    for mel in (0, 1, 3, 4):
        lo = max(mel, 2)
        cases.append(_case('mel%d_plain_R1030' % mel, [_read((3, mel, 1030), 1030, 30, dwell=(lo, lo + 2))], 30,
                           mel=mel, transitions=False))
        cases.append(_case('mel%d_trans_R1024' % mel, [_read((3, mel, 1024), 1024, 30, dwell=(lo, lo + 2))], 30,
                           mel=mel, transitions=True))
    # adjacent bases with the same level: the plateau mark of last_tie_flags
    for tr in (True, False):
        cases.append(_case('plateau_%s' % ('trans' if tr else 'plain'),
                           [_plateau_read()], 30, transitions=tr, model=PLATEAU))
    # other window sizes, the contexts shorter than the window needs (the missing bases read as 0)
    c2 = _read((6, 2), 90, 30, model=K2, dwell=(3, 4))
    cases.append(_case('k2', [dict(c2, context_after=c2['context_after'][:0])], 30, model=K2))
    c10 = _read((6, 10), 90, 30, model=K10, dwell=(3, 4))
    cases.append(_case('k10', [dict(c10, context_before=c10['context_before'][2:],
                                    context_after=c10['context_after'][:1])], 30, model=K10))
    # company for the reads of the other settings: a second read (another length, so another path through the
    # planner's loops) beside the team read, at every min event length, and for each of the other tables
    for tr in (True, False):
        t = 'trans' if tr else 'plain'
        cases.append(_case('team_company_%s' % t, [_read((9, 0), 90, 200, dwell=(2, 3), jitter=10)], 200,
                           transitions=tr))
        cases.append(_case('plateau_company_%s' % t, [_read((9, 1), 140, 30, model=BASE, dwell=(3, 4))], 30,
                           transitions=tr, model=PLATEAU))
        for mel in (0, 1, 3, 4):
            lo = max(mel, 2)
            cases.append(_case('mel%d_company_%s' % (mel, t), [_read((9, 2, mel), 70, 30, dwell=(lo, lo + 2))], 30,
                               mel=mel, transitions=tr))
    cases.append(_case('k2_company', [_read((9, 3), 150, 30, model=K2, dwell=(3, 4))], 30, model=K2))
    cases.append(_case('k10_company', [_read((9, 4), 150, 30, model=K10, dwell=(3, 4))], 30, model=K10))
    # ... and every read of one setting once more as one batch
    groups = {}
    for c in cases:
        key = (c['model'], c['bandwidth'], c['mel'], c['transitions'])
        groups.setdefault(key, []).append(c)
    for key, members in groups.items():
        reads, bad = [], []
        for c in members:
            bad += [len(reads) + i for i in c['bad']]
            reads += c['reads']
        if len(reads) > 1:
            model, bw, mel, tr = key
            name = 'mixed_%s_bw%d_mel%d_%s' % ('-'.join(str(x) for x in model), bw, mel, 'trans' if tr else 'plain')
            cases.append(_case(name, reads, bw, mel, tr, model, bad))
    assert len({c['name'] for c in cases}) == len(cases)
    return cases


def run_case(dtw, case, kmer_model):
    """One refine_alignment batch on the GPU -> (events per read, status, planner totals and tie flags as the golden
    file holds them).  ``kmer_model``: a dtw.KmerModel of ``model_arrays(case['model'])``."""
    reads = [(c['signal'], c['reference'], c['context_before'], c['context_after'], c['approximate_alignment'])
             for c in case['reads']]
    events, status = dtw.refine_alignment_batch(reads, case['bandwidth'], case['mel'], kmer_model,
                                                case['transitions'], on_error='status', return_status=True)
    stats = kmer_model.context.last_batch_stats()
    flags = kmer_model.context.last_tie_flags(len(reads))
    totals = dict(band_cells=int(stats['band_cells']), wave_steps=int(stats['wave_steps']),
                  reads_redone_exact=int(stats['reads_redone_exact']), tie_flags=[int(f) for f in flags])
    return events, np.asarray(status), totals
