"""The per-site mixture tests on the two samples of tools/bench_site_ranks.py (N synthetic reads each over one genome;
sample A unmodified, sample B with 0.3 of its CG sites modified): site_mixture_tests_batch (resident) and
compare_site_mixtures on two rows=True batches end to end, beside two site_levels_batch calls and beside
site_rank_tests_batch; then on the rows of both samples the back half in parts: the sorts, the site list (torch, HIP
events), the mixture kernel, and the rank-test kernel on the same rows as the yardstick.  Wall time and the time in the
library's kernels (ctx.timing_read; `site` holds the rows kernels, the moments kernel, the rank-test kernel and the
mixture kernel), then sites, rows, EM steps and ns per site.
`python tools/bench_site_mixtures.py [N] [genome_length]`."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import (compare_site_mixtures, defaults, dtw, kmer_train, site_levels_batch,  # noqa: E402
                         site_mixture_tests_batch, site_rank_tests_batch, synthetic)
from nadavca_amd.batchflow import load_config  # noqa: E402
from nadavca_amd.device import (common_sites, site_mixture_tests_dev, site_rank_tests_dev,  # noqa: E402
                                sort_site_rows)
from nadavca_amd.site_tests import sample_rows  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
TRIM, MIN_COVERAGE, ITERATIONS, MIN_SD_RATIO, EXACT_CELLS = 5, 5, 32, 0.1, 16384

model = synthetic.load_model_arrays()
k, central, _, mean, sigma = model
mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
has_m = np.zeros(5 ** k, dtype=bool)
for j in range(k):
    has_m |= (np.arange(5 ** k) // 5 ** j) % 5 == 4
model5 = (k, central, 5, mean5 + np.where(has_m, np.random.default_rng(5).normal(0.0, 0.6, 5 ** k), 0.0), sigma5)
km = dtw.KmerModel(*model)
ctx = km.context
config = load_config(defaults.CONFIG_FILE)
t0 = time.perf_counter()
(rb_a, al_a, genome, _), (rb_b, al_b, _, truth) = (
    synthetic.make_modified_read_batch(n_reads, model5, seed=7, modified_fraction=fraction, genome_length=G,
                                       read_seed=read_seed) for fraction, read_seed in ((0.0, 107), (0.3, 207)))
print('built 2 x %d reads (%.0f samples, %.0f bases each on average) over %d bases, %d modified sites, in %.1f s' % (
    n_reads, rb_a.sig_off[-1] / n_reads, rb_a.seq_off[-1] / n_reads, G,
    int(truth['forward'].sum() + truth['reverse'].sum()), time.perf_counter() - t0))


def timed(name, fn, unit, what):
    """-> (fn's result, wall ms, ms in the `site` kernels, ms between two HIP events)."""
    ctx.synchronize()
    torch.cuda.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    ctx.synchronize()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    ctx.timing_enable(False)
    timing = ctx.timing_read()
    kern = sum(ms for ms, _ in timing.values())
    print('%-52s %9.2f ms wall, %8.3f ms between events, %8.3f ms in kernels (site %.3f), %11.0f %s/s' % (
        name, dt * 1e3, e0.elapsed_time(e1), kern, timing['site'][0], unit / dt, what))
    return out, dt * 1e3, timing['site'][0], e0.elapsed_time(e1)


warm = synthetic.make_modified_read_batch(64, model5, seed=8, genome_length=G)
site_mixture_tests_batch(warm[0], warm[0], warm[1], km, config)
site_rank_tests_batch(warm[0], warm[0], warm[1], km, config)

reads = 2 * n_reads
for rep in range(2):
    _, t_levels, _, _ = timed('2 x site_levels_batch (for comparison)',
                              lambda: (site_levels_batch(rb_a, al_a, km, config), site_levels_batch(rb_b, al_b, km,
                                                                                                     config)),
                              reads, 'reads')
    _, t_ranks, _, _ = timed('site_rank_tests_batch (for comparison)',
                             lambda: site_rank_tests_batch(rb_a, rb_b, (al_a, al_b), km, config, trim=TRIM), reads,
                             'reads')
    res, t_resident, _, _ = timed('site_mixture_tests_batch (end to end)',
                                  lambda: site_mixture_tests_batch(rb_a, rb_b, (al_a, al_b), km, config, trim=TRIM),
                                  reads, 'reads')
    (a, b), t_rows, _, _ = timed('2 x site_levels_batch(rows=True)',
                                 lambda: (site_levels_batch(rb_a, al_a, km, config, rows=True),
                                          site_levels_batch(rb_b, al_b, km, config, rows=True)), reads, 'reads')
    res2, t_compare, _, _ = timed('compare_site_mixtures of the two (upload, kernel, host)',
                                  lambda: compare_site_mixtures(a, b), reads, 'reads')
print('site_mixture_tests_batch / 2 x site_levels_batch: %.2f x; / site_rank_tests_batch: %.2f x; host-table form / 2 x '
      'site_levels_batch: %.2f x' % (t_resident / t_levels, t_resident / t_ranks, (t_rows + t_compare) / t_levels))
assert len(res) == len(res2) and np.array_equal(res.p, res2.p, equal_nan=True)
print('%d sites tested, median coverage %d / %d, largest %d / %d; %d fitted, %d with p <= 1e-3; median delta_rate of '
      'those %.3f' % (len(res), np.median(res.n_a), np.median(res.n_b), res.n_a.max(), res.n_b.max(),
                      int(res.fitted.sum()), int((res.p <= 1e-3).sum()),
                      np.median(res.delta_rate[res.p <= 1e-3]) if (res.p <= 1e-3).any() else float('nan')))
del a, b

j = 0       # column 'level'
(key_a, val_a, _), (key_b, val_b, _) = (sample_rows(rb, al, km, config, defaults.RENORM_ROUNDS, TRIM, j)
                                        for rb, al in ((rb_a, al_a), (rb_b, al_b)))
rows = int(key_a.numel() + key_b.numel())
for rep in range(3):
    (sa, sb), _, _, t_sort = timed('  drop + two stable sorts per sample (torch)',
                                   lambda: (sort_site_rows(key_a, val_a), sort_site_rows(key_b, val_b)), rows, 'rows')
    (site_key, _), _, _, t_list = timed('  site list (torch)', lambda: common_sites(sa[0], sb[0], MIN_COVERAGE), rows,
                                        'rows')
    out, _, t_kernel, _ = timed('  site_mixture_tests_dev (sorts, list and kernel)',
                                lambda: site_mixture_tests_dev(ctx, key_a, val_a, key_b, val_b, MIN_COVERAGE,
                                                               ITERATIONS, MIN_SD_RATIO), rows, 'rows')
    _, _, t_rank_kernel, _ = timed('  site_rank_tests_dev (sorts, list and kernel)',
                                   lambda: site_rank_tests_dev(ctx, key_a, val_a, key_b, val_b, MIN_COVERAGE,
                                                               EXACT_CELLS), rows, 'rows')
n_sites = int(site_key.numel())
counted = int(sa[0].numel() + sb[0].numel())
counts = out[1].cpu().numpy()
steps = int(counts[:, 3:].sum())
row_steps = int(((counts[:, 0] + counts[:, 1]) * counts[:, 3:].sum(axis=1)).sum())
print('%d rows, %d counted, %d sites tested, %d fitted' % (rows, counted, n_sites, int(counts[:, 2].sum())))
print('sorts: %.3f ms; site list: %.3f ms' % (t_sort, t_list))
print('mixture kernel: %.3f ms (rank-test kernel on the same rows: %.3f ms, %.1f x): %.1f ns per site, %d EM steps '
      '(%.2f ns per step of a site), %d row-steps (one exp each): %.2f per ns' % (
          t_kernel, t_rank_kernel, t_kernel / t_rank_kernel if t_rank_kernel > 0 else 0.0,
          t_kernel * 1e6 / max(n_sites, 1), steps, t_kernel * 1e6 / max(steps, 1), row_steps,
          row_steps / (t_kernel * 1e6) if t_kernel > 0 else 0.0))
