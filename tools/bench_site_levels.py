"""site_levels_batch on N synthetic reads (synthetic.make_read_batch: int16 raw data, the packaged 6-mer table, reads of
about 400 bases): the workflow end to end beside align_signal_batch on the same batch, then on one alignment stage its
back half in parts — the rows kernel beside pass 1 of the k-mer statistics (kmer_event_kernel: the same samples read
once, one of the two sums), the stable sort and gather (torch, HIP events), the moments kernel.  Wall time and the time
in the library's kernels (ctx.timing_read; `site` is the new kernels), then the bytes the two kernels must move and the
bandwidth they reach.  `python tools/bench_site_levels.py [N] [genome_length]`."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import align_signal_batch, defaults, dtw, site_levels_batch, synthetic  # noqa: E402
from nadavca_amd.batchflow import align_batch, load_config  # noqa: E402
from nadavca_amd.device import (expected_levels_dev, kmer_event_stats_dev, site_level_rows_dev,  # noqa: E402
                                site_moments_dev)

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
TRIM = 5

model = synthetic.load_model_arrays()
k, central, alphabet = model[:3]
km = dtw.KmerModel(*model)
ctx = km.context
config = load_config(defaults.CONFIG_FILE)
t0 = time.perf_counter()
rb, aligner, genome = synthetic.make_read_batch(n_reads, model, seed=7, genome_length=G)
print('built %d reads (%.0f samples, %.0f bases each on average) over %d bases in %.1f s' % (
    n_reads, rb.sig_off[-1] / n_reads, rb.seq_off[-1] / n_reads, G, time.perf_counter() - t0))


def timed(name, fn, unit=n_reads, what='reads'):
    """-> (fn's result, wall ms, ms in the `site` kernels, ms in the `kmer` kernels, ms between two HIP events)."""
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
    print('%-46s %9.2f ms wall, %8.3f ms between events, %8.3f ms in kernels (site %.3f, kmer %.3f), %11.0f %s/s' % (
        name, dt * 1e3, e0.elapsed_time(e1), kern, timing['site'][0], timing['kmer'][0], unit / dt, what))
    return out, dt * 1e3, timing['site'][0], timing['kmer'][0], e0.elapsed_time(e1)


warm = synthetic.make_read_batch(64, model, seed=8, genome_length=G)
site_levels_batch(warm[0], warm[1], km, config)

for rep in range(2):
    _, t_align, _, _, _ = timed('align_signal_batch (end to end)',
                                lambda: align_signal_batch(None, rb, config=config, kmer_model=km, aligner=aligner))
    res, t_site, _, _, _ = timed('site_levels_batch (end to end)', lambda: site_levels_batch(rb, aligner, km, config))
    timed('site_levels_batch(rows=True) (end to end)', lambda: site_levels_batch(rb, aligner, km, config, rows=True))
print('site_levels_batch / align_signal_batch: %.2f x; %d sites with coverage, mean coverage %.1f, max %d' % (
    t_site / t_align, len(res), float(res.count.mean()), int(res.count.max())))

al = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
sa, dbatch, events, status = al.stage.sa, al.stage.dbatch, al.events, al.status
expected = expected_levels_dev(dbatch, km, with_contexts=True)
start, rev = sa.ref_start.contiguous(), sa.reverse.to(torch.int32)
bases = dbatch.total_ref
for rep in range(3):
    _, _, _, t_kmer, _ = timed('  kmer_event_stats_dev pass 1 (for comparison)',
                               lambda: kmer_event_stats_dev(dbatch, ctx, events, status, k, central, alphabet, TRIM),
                               bases, 'bases')
    (key, val), _, t_rows, _, _ = timed('  site_level_rows_dev',
                                        lambda: site_level_rows_dev(ctx, dbatch, events, expected, start, rev, status,
                                                                    TRIM, G), bases, 'bases')
    (skey, sval), _, _, _, t_sort = timed('  stable sort + gather (torch)',
                                          lambda: (lambda s: (s[0], val[s[1]]))(torch.sort(key, stable=True)),
                                          bases, 'bases')
    (count, mean, m2), _, t_mom, _, _ = timed('  site_moments_dev', lambda: site_moments_dev(ctx, skey, sval, 2 * G),
                                              bases, 'bases')
counted = key >= 0
samples = int(val[counted, 2].sum())
n_counted = int(counted.sum())
rows_bytes = 8 * samples + (8 + 8 + 40) * bases
mom_bytes = 40 * n_counted + (8 + 64) * 2 * G
print('%d bases, %d counted events, %d samples in them' % (bases, n_counted, samples))
print('rows kernel: %.3f ms for %.1f MB (8 B per sample once; events 8 B, expected 8 B in and 40 B out per base): '
      '%.0f GB/s; %.2f x kmer_event_kernel pass 1 (%.3f ms)' % (
          t_rows, rows_bytes / 1e6, rows_bytes / (t_rows * 1e-3) / 1e9 if t_rows > 0 else 0.0,
          t_rows / t_kmer if t_kmer > 0 else 0.0, t_kmer))
print('sort + gather: %.3f ms' % t_sort)
print('moments kernel: %.3f ms for %.1f MB (40 B per counted row in, 72 B per key out, %d keys): %.0f GB/s' % (
    t_mom, mom_bytes / 1e6, 2 * G, mom_bytes / (t_mom * 1e-3) / 1e9 if t_mom > 0 else 0.0))
