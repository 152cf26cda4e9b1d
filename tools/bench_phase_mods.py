"""phase_mods_batch on N synthetic reads of two haplotypes (packaged 6-mer table and its 5-letter extension, reads of
about 400 bases, a substitution about every 300 bases on each haplotype, the CG occurrences at least 12 bases from
every substitution dealt into "modified on haplotype 1 only / on 2 only / on both / on neither"): the whole call beside
phase_reads_batch and call_mods_batch alone on the same batch, then the tail apart on the two batches of one run —
``phase_mods_of_rows`` (grouping, sort, operator, host columns), its torch part (sort and phase sets) and the operator
alone.  Wall time, time in the library's kernels (ctx.timing_read; `allele` holds the allele, phase and mod-site
kernels) and reads/s; then the contrast per class.
The phased sites are the planted substitutions, passed as known variants (``sites=``).
`python tools/bench_phase_mods.py [N] [genome_length]`."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import (synthetic, defaults, dtw, kmer_train, call_mods_batch, phase_mods_batch,  # noqa: E402
                         phase_reads_batch)
from nadavca_amd.batchflow import load_config  # noqa: E402
from nadavca_amd.device import mod_site_solve_dev  # noqa: E402
from nadavca_amd.phase_mods import SET_MASKS, phase_mods_of_rows, site_phase_sets, site_ranges  # noqa: E402
from nadavca_amd.readbatch import SyntheticBatchAligner  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
CLIP = 30.0

model = synthetic.load_model_arrays()
k, central, _, mean, sigma = model
mean5, sigma5 = kmer_train.extend_kmer_model(k, central, mean, sigma)
has_m = np.zeros(5 ** k, dtype=bool)
for m in range(k):
    has_m |= (np.arange(5 ** k) // 5 ** m) % 5 == 4
model5 = (k, central, 5, mean5 + np.where(has_m, np.random.default_rng(5).normal(0.0, 0.6, 5 ** k), 0.0), sigma5)
km, km5 = dtw.KmerModel(*model), dtw.KmerModel(*model5)
config = load_config(defaults.CONFIG_FILE)
ctx = km.context
rng = np.random.default_rng(5)
ref = rng.integers(0, 4, G).astype(np.int32)
planted = np.arange(100, G - 100, 150) + rng.integers(-20, 21, len(range(100, G - 100, 150)))
owner = 1 + np.arange(planted.size) % 2
haps = [ref.copy(), ref.copy()]
alts = (ref[planted] + rng.integers(1, 4, planted.size)) % 4
for h in (0, 1):
    haps[h][planted[owner == h + 1]] = alts[owner == h + 1]
cg = np.nonzero((ref[:-1] == 1) & (ref[1:] == 2))[0]
gap = np.abs(cg[:, None, None] + np.array([0, 1])[None, :, None] - planted[None, None, :]).min(axis=(1, 2))
far = cg[gap >= 12]
cls = {int(x): j % 4 for j, x in enumerate(far)}
on = lambda *classes: [x for x in far.tolist() if cls[x] in classes]
modified = [[], on(0, 2), on(1, 2)]
known = (planted.astype(np.int64), alts.astype(np.int64))
t0 = time.perf_counter()
rb, truth, info = synthetic.make_phased_modified_read_batch(n_reads, [ref] + haps, [0.0, 0.5, 0.5], modified, model5,
                                                            seed=7, anchor_density=0.75, jitter=20)
aligner = SyntheticBatchAligner(ref, truth)
print('built %d reads (%.0f samples, %.0f bases each on average) over %d bases, %d planted substitutions, %d CGs in '
      'classes, in %.1f s' % (n_reads, rb.sig_off[-1] / n_reads, rb.seq_off[-1] / n_reads, G, planted.size, far.size,
                              time.perf_counter() - t0))


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
    print('%-46s %9.2f ms wall, %8.2f ms in kernels (allele %.3f ms), %11.0f %s/s' % (
        name, dt * 1e3, kern, timing['allele'][0], unit / dt, what))
    return out


warm = synthetic.make_phased_modified_read_batch(64, [ref] + haps, [0.0, 0.5, 0.5], modified, model5, seed=8)
phase_mods_batch(ref, warm[0], SyntheticBatchAligner(ref, warm[1]), km, km5, config=config, sites=known)

for rep in range(2):
    phase = timed('phase_reads_batch (end to end)',
                  lambda: phase_reads_batch(ref, rb, config=config, kmer_model=km, aligner=aligner,
                                            sites=known))
    mods = timed('call_mods_batch joint (end to end)',
                 lambda: call_mods_batch(rb, aligner, km5, config=config, joint=True))
    res = timed('phase_mods_batch (end to end)',
                lambda: phase_mods_batch(ref, rb, aligner, km, km5, config=config, sites=known,
                                         clip=CLIP))

dev = torch.device('cuda', ctx.device)
solve = lambda *a: mod_site_solve_dev(ctx, *a)
n_rows = len(res.mods)
for rep in range(3):
    timed('tail: phase_mods_of_rows', lambda: phase_mods_of_rows(res.mods, res.phase, solve, k, CLIP, 4, dev), n_rows,
          'rows')
    order, lo, hi, site_of = timed('  rows to the device, stable sort, ranges', lambda: site_ranges(res.mods, dev),
                                   n_rows, 'rows')
    site_ps, group = timed('  phase sets and groups',
                           lambda: site_phase_sets(order, site_of, int(lo.numel()), res.mods, res.phase, dev), n_rows,
                           'rows')
    val = torch.from_numpy(res.mods.llr).to(dev)[order].contiguous()
    timed('  mod_site_solve_dev (4 sets)', lambda: mod_site_solve_dev(ctx, lo, hi, val, group, SET_MASKS, CLIP), n_rows,
          'rows')
    timed('  mod_site_solve_dev (1 set, no groups)', lambda: mod_site_solve_dev(ctx, lo, hi, val, None, (1,), CLIP),
          n_rows, 'rows')
print('%d sites with %d rows (%.1f per site) of %d reads; %d phased sites' % (
    len(res), n_rows, n_rows / max(len(res), 1), n_reads, len(res.phase)))

# the contrast per class
site_cls = np.array([cls.get(int(p) - int(s), -1) for p, s in zip(res.position, res.strand)])
gate = ~np.isnan(res.asm_lrt)
tagged = res.phase.haplotype > 0
print('reads tagged: %d of %d; sites with both haplotypes at min_tagged: %d of %d; near a variant: %d' % (
    int(tagged.sum()), n_reads, int(gate.sum()), len(res), int(res.near_variant.sum())))
for c, name in enumerate(('haplotype 1 only', 'haplotype 2 only', 'both', 'neither')):
    m = gate & (site_cls == c)
    if m.any():
        print('%-17s %6d sites: asm_lrt median %8.2f, p <= 0.001 on %.4f, |delta| median %.3f' % (
            name, int(m.sum()), float(np.median(res.asm_lrt[m])), float((res.p[m] <= 1e-3).mean()),
            float(np.median(np.abs(res.delta[m])))))
