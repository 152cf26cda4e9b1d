"""One round of estimate_mod_model on N synthetic reads (synthetic.make_modified_read_batch: int16 raw data, half of
the CG sites of each strand modified, drawn from the packaged table extended with M levels = C levels + N(0, 0.6^2);
the start is the table with M = C), split into its parts: the alignment (the device half of align_signal_batch), the
E-step (call_mods.score_sites with joint clusters; the time of its `ell_hyp` kernels inside it), the rows kernel (count
and fill), the stable sort and the gather (torch), and the reduce kernel.  Rows per read, and the bandwidth of the rows
kernel against the bytes it must move: 8 B per sample of an event that has rows, 8 B of events per such base, 40 B per
row out, and per base the 8 B count out and the 8 B offset in.  call_mods_batch on the same batch stands beside it, and
the whole estimate_mod_model(rounds=1).  `python tools/bench_mod_train.py [N] [repeats]`."""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nadavca_amd import call_mods_batch, defaults, dtw, estimate_mod_model, kmer_train, synthetic  # noqa: E402
from nadavca_amd.batchflow import align_batch, load_config  # noqa: E402
from nadavca_amd.call_mods import score_sites  # noqa: E402
from nadavca_amd.device import mod_kmer_reduce_dev, mod_kmer_rows_dev  # noqa: E402

import torch  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
n_reads = int(args[0]) if args else 10000
repeats = int(args[1]) if len(args) > 1 else 3
k, central, _, mean, sigma = synthetic.load_model_arrays()
mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
has_m = np.zeros(5 ** k, dtype=bool)
for m in range(k):
    has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
truth = (k, central, 5, mean5 + np.where(has_m, np.random.default_rng(5).normal(0.0, 0.6, 5 ** k), 0.0), sigma5)
t0 = time.perf_counter()
rb, aligner, _, _ = synthetic.make_modified_read_batch(n_reads, truth, seed=7)
print('built %d reads (%.0f samples each on average) in %.1f s' % (n_reads, rb.sig_off[-1] / n_reads,
                                                                   time.perf_counter() - t0))
km = dtw.KmerModel(k, central, 5, mean5, sigma5)
ctx = km.context
config = load_config(defaults.CONFIG_FILE)
fraction = 0.5


def timed(fn):
    ctx.synchronize()
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def kernel_ms(fn, name):
    ctx.timing_reset()
    ctx.timing_enable(True)
    out, wall = timed(fn)
    ctx.timing_enable(False)
    return out, wall, ctx.timing_read()[name]


align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)   # warm-up: workspaces, first touch
for r in range(repeats):
    res, t_align = timed(lambda: align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner))
    dbatch = res.stage.dbatch
    sc, t_e, (ell_ms, ell_n) = kernel_ms(lambda: score_sites(res, config, km, [1, 2], 0, 4, True, 4, fraction),
                                         'ell_hyp')

    def gammas():
        pos = sc.pos[sc.ok].contiguous()
        site_off = torch.zeros(res.stage.n_live + 1, dtype=torch.int64, device=pos.device)
        torch.cumsum(torch.bincount(sc.owner[sc.ok], minlength=res.stage.n_live), 0, out=site_off[1:])
        return site_off, pos, torch.sigmoid(sc.llr[sc.ok] + math.log(fraction / (1.0 - fraction)))

    (site_off, pos, gamma), t_gamma = timed(gammas)
    level = torch.from_numpy(km.mean).to(dbatch.device)
    (key, val, row_off, skipped), t_rows, (rows_ms, rows_n) = kernel_ms(
        lambda: mod_kmer_rows_dev(dbatch, ctx, res.events, res.status, k, central, 5, 5, site_off, pos, gamma, 4,
                                  level), 'kmer')

    def sort_gather():
        skey, order = torch.sort(key, stable=True)
        sval = val[order]
        n_neg = (skey < 0).sum().reshape(1)
        ukey, counts = torch.unique_consecutive(skey[skey >= 0], return_counts=True)
        return sval, torch.cat([n_neg, n_neg + torch.cumsum(counts, 0)]), ukey

    (sval, run_off, ukey), t_sort = timed(sort_gather)
    (sums, count), t_reduce, (reduce_ms, reduce_n) = kernel_ms(lambda: mod_kmer_reduce_dev(ctx, sval, run_off), 'kmer')
    n_rows = int(key.numel())
    widths = row_off[1:] - row_off[:-1]
    first = row_off[:-1][widths > 0]
    samples = int(val[first, 1].sum())
    bytes_moved = 8 * samples + 8 * int(first.numel()) + 40 * n_rows + 16 * dbatch.total_ref
    print('round %d: align %.1f ms | E-step %.1f ms (ell_hyp kernels %.1f ms, %d launches; gamma %.2f ms) | rows '
          'kernel %.3f ms (%d launches, %.2f ms wall with the cumulative sum) | sort and gather %.2f ms | reduce kernel '
          '%.3f ms (%.2f ms wall)' % (r, t_align, t_e, ell_ms, ell_n, t_gamma, rows_ms, rows_n, t_rows, t_sort,
                                      reduce_ms, t_reduce))
    print('         %d sites, %d rows (%.1f per read), %d runs, longest %d rows, %d windows skipped; rows kernel '
          '%.1f MB, %.1f GB/s' % (int(pos.numel()), n_rows, n_rows / max(n_reads, 1), int(ukey.numel()),
                                  int(count.max()) if int(count.numel()) else 0, skipped, bytes_moved / 1e6,
                                  bytes_moved / (rows_ms * 1e-3) / 1e9 if rows_ms > 0 else 0.0))
_, t_call = timed(lambda: call_mods_batch(rb, aligner, km, joint=True, max_joint=4, site_prior=fraction))
est, t_est = timed(lambda: estimate_mod_model(rb, aligner, km, rounds=1))
print('call_mods_batch(joint=True) on the same batch: %.1f ms; estimate_mod_model(rounds=1): %.1f ms, %d k-mers '
      'updated, fraction %.3f' % (t_call, t_est, est.history[0]['kmers_updated'], est.fraction))
