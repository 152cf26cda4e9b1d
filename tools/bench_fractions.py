"""estimate_allele_fractions_batch on N synthetic reads of a 50 / 50 mixture of two haplotypes (packaged 6-mer table,
reads of about 400 bases, one substitution per 500 bases on the second haplotype): the workflow end to end beside
estimate_snps_batch on the same batch, then on one stage the back half alone and its parts apart — the rows kernel,
the stable sort and gather (torch), the solve kernel.  Wall time, time in the library's kernels (ctx.timing_read;
`allele` is the two new kernels) and reads/s; then the rows per second of the two kernels and what the planted sites
score.  `python tools/bench_fractions.py [N] [genome_length] [event_length]`."""
import copy
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import synthetic, defaults, dtw, estimate_allele_fractions_batch, estimate_snps_batch  # noqa: E402
from nadavca_amd.allele_fractions import allele_fractions_of_rows  # noqa: E402
from nadavca_amd.batchflow import device_stage, likelihood_rows, load_config  # noqa: E402
from nadavca_amd.device import allele_rows_dev, allele_solve_dev  # noqa: E402
from nadavca_amd.readbatch import SyntheticBatchAligner  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
event_length = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0

model = synthetic.load_model_arrays()
km = dtw.KmerModel(*model)
config = load_config(defaults.CONFIG_FILE)
ctx = km.context
rng = np.random.default_rng(5)
ref = rng.integers(0, 4, G).astype(np.int32)
planted = np.sort(rng.choice(np.arange(50, G - 50), max(1, G // 500), replace=False))
hap = ref.copy()
hap[planted] = (ref[planted] + rng.integers(1, 4, planted.size)) % 4
t0 = time.perf_counter()
rb, truth, info = synthetic.make_mixed_read_batch(n_reads, [ref, hap], [0.5, 0.5], seed=7, model=model,
                                                  anchor_density=0.75, jitter=20)
aligner = SyntheticBatchAligner(ref, truth)
print('built %d reads (%.0f samples, %.0f bases each on average) over %d bases, %d planted substitutions, in %.1f s' % (
    n_reads, rb.sig_off[-1] / n_reads, rb.seq_off[-1] / n_reads, G, planted.size, time.perf_counter() - t0))


def timed(name, fn, unit=n_reads, what='reads'):
    ctx.synchronize()
    torch.cuda.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t = time.perf_counter()
    out = fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    ctx.timing_enable(False)
    timing = ctx.timing_read()
    kern = sum(ms for ms, _ in timing.values())
    print('%-44s %9.2f ms wall, %8.2f ms in kernels (allele %.3f ms), %11.0f %s/s' % (
        name, dt * 1e3, kern, timing['allele'][0], unit / dt, what))
    return out


warm = synthetic.make_mixed_read_batch(64, [ref, hap], [0.5, 0.5], seed=8, model=model)
estimate_allele_fractions_batch(ref, warm[0], config=config, kmer_model=km, aligner=SyntheticBatchAligner(ref, warm[1]))

for rep in range(2):
    timed('estimate_snps_batch (end to end)',
          lambda: estimate_snps_batch(ref, copy.deepcopy(rb), config=config, kmer_model=km, aligner=aligner))
    res = timed('estimate_allele_fractions_batch (end to end)',
                lambda: estimate_allele_fractions_batch(ref, copy.deepcopy(rb), config=config, kmer_model=km,
                                                        aligner=aligner, event_length=event_length))

stage = device_stage(copy.deepcopy(rb), ref, config, km, aligner, 'pooled')
ll, status, _ = likelihood_rows(stage, config, km)
sa, dbatch = stage.sa, stage.dbatch
start, rev = sa.ref_start.contiguous(), sa.reverse.to(torch.int32)
codes = torch.from_numpy(ref).to(ll.device)
rows = dbatch.total_ref
for rep in range(3):
    timed('back half (rows, sort, solve, selection, copy)',
          lambda: allele_fractions_of_rows(stage, ll, status, ref, None, km, event_length))
    key, val = timed('  allele_rows_dev', lambda: allele_rows_dev(ctx, dbatch, ll, start, rev, status, event_length, G),
                     rows, 'rows')
    skey, sval = timed('  stable sort + gather (torch)',
                       lambda: (lambda s: (s[0], val[s[1]]))(torch.sort(key, stable=True)), rows, 'rows')
    out = timed('  allele_solve_dev', lambda: allele_solve_dev(ctx, skey, sval, codes), rows, 'rows')
cov = out[4]
print('%d rows over %d positions: coverage mean %.1f, max %d; the rows kernel moves %d B per row, the solve reads '
      '%d B per row' % (rows, G, float(cov.double().mean()), int(cov.max()), 16 * 4 + 8, 8 * 4 + 8))

at = {(int(p), int(b)): t for t, (p, b) in enumerate(zip(res.position, res.alt_base))}
hit = np.array([at.get((int(p), int(hap[p])), -1) for p in planted])
found = hit[hit >= 0]
far = np.abs(res.position[:, None] - planted[None, :]).min(axis=1) > model[0] - 1 if planted.size < 5000 else None
print('planted (site, base) pairs with fraction > 0: %d of %d; their fraction: median %.3f, 5 %% .. 95 %% %.3f .. %.3f; '
      'their lrt: min %.1f, median %.1f' % (
          found.size, planted.size, np.median(res.fraction[found]), np.quantile(res.fraction[found], 0.05),
          np.quantile(res.fraction[found], 0.95), res.lrt[found].min(), np.median(res.lrt[found])))
if far is not None:
    print('rows more than k - 1 from every planted site: %d with fraction > 0, largest lrt %.1f, 99.9 %% quantile %.1f'
          % (int(far.sum()), res.lrt[far].max(), np.quantile(res.lrt[far], 0.999)))
