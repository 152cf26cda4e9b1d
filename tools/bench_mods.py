"""call_mods_batch on N synthetic reads with modified bases (pattern CG by default; the packaged 6-mer table extended
to 5 letters, an M k-mer = its C k-mer's level + N(0, 0.6^2)): the workflow end to end, then on one alignment stage the
listed-hypotheses call alone and, for comparison, the full-matrix estimate_log_likelihoods_dev with the same table —
what scoring the same sites took before the listed call existed.  Wall time, time in the library's kernels
(ctx.timing_read) and reads/s; then the share of truly modified / unmodified sites with llr > 0 / < 0.
``--joint``: also ``call_mods_batch(joint=True)`` end to end, the joint-hypotheses call alone on the same stage (every
non-empty subset of every cluster of sites), and the shares of the joint ratio beside those of the single one on the
same rows.  `python tools/bench_mods.py [N] [pattern] [--joint]`."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nadavca_amd import synthetic, defaults, kmer_train, dtw, call_mods_batch  # noqa: E402
from nadavca_amd.batchflow import align_batch, load_config  # noqa: E402
from nadavca_amd.call_mods import find_sites, cluster_sites, joint_lists  # noqa: E402
from nadavca_amd.detect_meth import pattern_codes  # noqa: E402
from nadavca_amd.device import (estimate_hypotheses_dev, estimate_joint_hypotheses_dev,  # noqa: E402
                                estimate_log_likelihoods_dev)
from nadavca_amd.readbatch import contig_local_range  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
n_reads = int(args[0]) if args else 2000
pattern = args[1] if len(args) > 1 else 'CG'
joint = '--joint' in sys.argv[1:]

k, central, _, mean, sigma = synthetic.load_model_arrays()
mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
has_m = np.zeros(5 ** k, dtype=bool)
for m in range(k):
    has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
mean5 = mean5 + np.where(has_m, np.random.default_rng(5).normal(0.0, 0.6, 5 ** k), 0.0)
model5 = (k, central, 5, mean5, sigma5)
km = dtw.KmerModel(*model5)
config = load_config(defaults.CONFIG_FILE)
t0 = time.perf_counter()
rb, aligner, genome, truth = synthetic.make_modified_read_batch(n_reads, model5, seed=7, pattern=pattern)
print('built %d reads (%.0f samples, %.0f bases each on average) in %.1f s' % (
    n_reads, rb.sig_off[-1] / n_reads, rb.seq_off[-1] / n_reads, time.perf_counter() - t0))
ctx = km.context


def timed(name, fn):
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t = time.perf_counter()
    out = fn()
    ctx.synchronize()
    dt = time.perf_counter() - t
    ctx.timing_enable(False)
    timing = ctx.timing_read()
    kern = sum(ms for ms, _ in timing.values())
    print('%-44s %9.1f ms wall, %7.1f ms in kernels (ell_hyp %.2f ms), %9.0f reads/s' % (
        name, dt * 1e3, kern, timing['ell_hyp'][0], n_reads / dt))
    return out


# warm-up: workspaces, first touch, the model's tables
warm = synthetic.make_modified_read_batch(64, model5, seed=8, pattern=pattern)
call_mods_batch(warm[0], warm[1], km, pattern=pattern)
if joint:
    call_mods_batch(warm[0], warm[1], km, pattern=pattern, joint=True)

for rep in range(2):
    mb = timed('call_mods_batch (end to end)', lambda: call_mods_batch(rb, aligner, km, pattern=pattern))
    if joint:
        mj = timed('call_mods_batch (joint=True, end to end)',
                   lambda: call_mods_batch(rb, aligner, km, pattern=pattern, joint=True))
res = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
stage = res.stage
start, end = contig_local_range(stage.sa, stage.reference)
site_off, owner, pos, forward, crowded = find_sites(
    stage.dbatch.reference, stage.dbatch.ref_off, start, end, stage.sa.reverse, pattern_codes(pattern), 0, k,
    keep=res.status == 0, total_ref=stage.dbatch.total_ref)
base = pos * 0 + 4
hyp_args = (stage.dbatch, config['bandwidth'], config['min_event_length'], km, config['model_wobbling'])
print('%d sites in %d aligned reads (%.1f per read)' % (int(pos.numel()), stage.n_live, int(pos.numel()) / stage.n_live))
for rep in range(3):
    timed('estimate_hypotheses_dev (listed sites)', lambda: estimate_hypotheses_dev(*hyp_args, site_off, pos, base))
    timed('estimate_log_likelihoods_dev (full, 5 letters)', lambda: estimate_log_likelihoods_dev(*hyp_args))
if joint:
    cluster, first, size, cut = cluster_sites(owner, pos, k, 4)
    hyp_off, sub_off, sub_pos, sub_base, _, _ = joint_lists(owner, pos, stage.n_live, first, size, 4)
    print('%d clusters of more than one site hold %.3f of the sites; %d joint hypotheses (%.1f per read: %.1f of one '
          'substitution, %.1f of several), %.3f of the sites stay crowded'
          % (int((size > 1).sum()), float((size[cluster] > 1).double().mean()), int(sub_off.numel()) - 1,
             (int(sub_off.numel()) - 1) / stage.n_live, int(((sub_off[1:] - sub_off[:-1]) == 1).sum()) / stage.n_live,
             int(((sub_off[1:] - sub_off[:-1]) > 1).sum()) / stage.n_live, float(cut.double().mean())))
    for rep in range(3):
        timed('estimate_joint_hypotheses_dev (all subsets)',
              lambda: estimate_joint_hypotheses_dev(*hyp_args, hyp_off, sub_off, sub_pos, sub_base))

for s, name in ((0, 'forward'), (1, 'reverse')):
    for label, sel in (('all rows', mb.strand == s), ('not crowded', (mb.strand == s) & ~mb.crowded)):
        is_mod = truth[name][mb.position[sel]]
        llr = mb.llr[sel]
        print('%-8s %-12s %7d modified sites: llr > 0 on %.3f (mean %+.1f); %7d unmodified: llr < 0 on %.3f (mean %+.1f)'
              % (name, label, is_mod.sum(), np.mean(llr[is_mod] > 0), llr[is_mod].mean(), (~is_mod).sum(),
                 np.mean(llr[~is_mod] < 0), llr[~is_mod].mean()))
print('crowded rows: %.3f of %d' % (mb.crowded.mean(), len(mb)))
if joint:
    is_mod = np.where(mj.strand == 0, truth['forward'][mj.position], truth['reverse'][mj.position])
    for label, sel in (('all rows', np.ones(len(mj), dtype=bool)), ('clustered rows', mj.cluster > 1),
                       ('rows not crowded (joint)', ~mj.crowded)):
        for name, llr in (('joint ', mj.llr), ('single', mj.llr_single)):
            print('%-24s %s: %7d modified sites: llr > 0 on %.3f; %7d unmodified: llr < 0 on %.3f; wrong sign on %d'
                  % (label, name, (sel & is_mod).sum(), np.mean(llr[sel & is_mod] > 0), (sel & ~is_mod).sum(),
                     np.mean(llr[sel & ~is_mod] < 0),
                     int(np.sum(np.where(is_mod[sel], llr[sel] <= 0, llr[sel] >= 0)))))
    print('crowded rows with joint=True: %.3f of %d' % (mj.crowded.mean(), len(mj)))
