"""call_indels_batch on N synthetic reads (packaged 6-mer table, reads of about 400 bases against one random genome):
the workflow end to end, then on one alignment stage the edit-hypotheses call alone and, beside it, the full-matrix
estimate_log_likelihoods_dev — every substitution of every base, what the engine could score before.  Wall time, time
in the library's kernels (ctx.timing_read; ell_hyp is the likelihood kernel itself) and reads/s; then the candidates
per read by kind and the rows each kind re-runs.  `python tools/bench_indels.py [N] [max_del]`."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nadavca_amd import synthetic, defaults, dtw, call_indels_batch  # noqa: E402
from nadavca_amd.batchflow import align_batch, load_config  # noqa: E402
from nadavca_amd.call_indels import enumerate_candidates  # noqa: E402
from nadavca_amd.device import estimate_edit_hypotheses_dev, estimate_log_likelihoods_dev  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
max_del = int(sys.argv[2]) if len(sys.argv) > 2 else 1
trim = 5

model = synthetic.load_model_arrays()
k, central, alphabet = model[:3]
km = dtw.KmerModel(*model)
config = load_config(defaults.CONFIG_FILE)
t0 = time.perf_counter()
rb, aligner, genome = synthetic.make_read_batch(n_reads, model, seed=7)
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
    print('%-46s %9.1f ms wall, %7.1f ms in kernels (ell_hyp %.2f ms), %9.0f reads/s' % (
        name, dt * 1e3, kern, timing['ell_hyp'][0], n_reads / dt))
    return out


# warm-up: workspaces, first touch, the model's tables
warm = synthetic.make_read_batch(64, model, seed=8)
call_indels_batch(warm[0], warm[1], km, max_del=max_del, trim=trim)

for rep in range(2):
    ib = timed('call_indels_batch (end to end)',
               lambda: call_indels_batch(rb, aligner, km, max_del=max_del, trim=trim, keep_rows=None))
res = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
stage = res.stage
hyp_off, owner, local, edit_pos, edit_del, letter, ins_off, ins_base = enumerate_candidates(
    stage.dbatch.reference, stage.dbatch.ref_off, stage.sa.reverse, res.status == 0, max_del, trim,
    stage.dbatch.total_ref)
hyp_args = (stage.dbatch, config['bandwidth'], config['min_event_length'], km, config['model_wobbling'])
n_hyp, n_live, total_ref = int(owner.numel()), stage.n_live, stage.dbatch.total_ref
for rep in range(3):
    timed('estimate_edit_hypotheses_dev (candidates)',
          lambda: estimate_edit_hypotheses_dev(*hyp_args, hyp_off, edit_pos, edit_del, ins_off, ins_base))
    timed('estimate_log_likelihoods_dev (full matrix)', lambda: estimate_log_likelihoods_dev(*hyp_args))
n_del, n_ins = int((edit_del > 0).sum()), int((letter >= 0).sum())
print('%d candidates in %d aligned reads of %.1f bases: %.1f per read (%.1f deletions, %.1f insertions), %.2f per base '
      'against (4 + max_del) = %d before left-alignment; the full matrix holds %d hypotheses per read'
      % (n_hyp, n_live, total_ref / n_live, n_hyp / n_live, n_del / n_live, n_ins / n_live, n_hyp / total_ref,
         4 + max_del, (alphabet - 1) * total_ref // n_live))
print('rows re-run per hypothesis: substitution %d, one-base deletion %d, one-base insertion %d; rows per read: '
      'candidates %.0f, full matrix %.0f'
      % (k, k - 1, k, (n_del * (k - 1) + n_ins * k) / n_live, (alphabet - 1) * k * total_ref / n_live))
print('sites %d, with a summed llr above 0: %d (reads without any edit: every one of them is a false call at '
      'threshold 0)' % (len(ib), ib.called.size))
