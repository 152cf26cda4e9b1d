"""phase_reads_batch on N synthetic reads of two haplotypes (packaged 6-mer table, reads of about 400 bases, a
substitution about every 300 bases on each haplotype, the two alternating, reads drawn 50 / 50): the workflow end to end
beside estimate_allele_fractions_batch on the same batch, then on one stage the back half alone and the phasing's parts
apart — the links kernel, the tag kernel, the votes kernel, the whole loop of ``device.phase_sites_dev``.  Wall time,
time in the library's kernels (ctx.timing_read; `allele` holds the allele and the phase kernels) and reads/s; then the
share of correctly phased adjacent pairs of sites and of correctly tagged reads.  With `--span W` (2 .. 8) the workflow
and the loop run with ``span=W``, and the span-links launch is timed beside the old links launch, the forest
(``device.phase_forest``, wall time) beside ``phase_blocks``, the tag kernel of either kind.
`python tools/bench_phase.py [N] [genome_length] [threshold] [--span W]`."""
import copy
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import synthetic, defaults, dtw, estimate_allele_fractions_batch, phase_reads_batch  # noqa: E402
from nadavca_amd.batchflow import device_stage, likelihood_rows, load_config  # noqa: E402
from nadavca_amd.device import (allele_sorted_rows_dev, phase_blocks, phase_forest, phase_links_dev,  # noqa: E402
                                phase_sites_dev, phase_span_links_dev, phase_tag_blocks_dev, phase_tag_dev,
                                phase_votes_dev)
from nadavca_amd.phase import phase_of_rows  # noqa: E402
from nadavca_amd.readbatch import SyntheticBatchAligner  # noqa: E402

argv = list(sys.argv[1:])
SPAN = 1
if '--span' in argv:
    at = argv.index('--span')
    SPAN = int(argv[at + 1])
    del argv[at:at + 2]
n_reads = int(argv[0]) if len(argv) > 0 else 10000
G = int(argv[1]) if len(argv) > 1 else 100000
threshold = float(argv[2]) if len(argv) > 2 else 200.0
CLIP, MIN_SHARED, MIN_LINK, ROUNDS = 30.0, 3, 2.0, 2

model = synthetic.load_model_arrays()
km = dtw.KmerModel(*model)
config = load_config(defaults.CONFIG_FILE)
ctx = km.context
rng = np.random.default_rng(5)
ref = rng.integers(0, 4, G).astype(np.int32)
# a site every 150 bases (+- 20), alternating between the haplotypes: 300 apart on each
planted = np.arange(100, G - 100, 150) + rng.integers(-20, 21, len(range(100, G - 100, 150)))
owner = 1 + np.arange(planted.size) % 2
haps = [ref.copy(), ref.copy()]
alts = (ref[planted] + rng.integers(1, 4, planted.size)) % 4
for h in (0, 1):
    haps[h][planted[owner == h + 1]] = alts[owner == h + 1]
t0 = time.perf_counter()
rb, truth, info = synthetic.make_mixed_read_batch(n_reads, [ref] + haps, [0.0, 0.5, 0.5], seed=7, model=model,
                                                  anchor_density=0.75, jitter=20)
aligner = SyntheticBatchAligner(ref, truth)
print('built %d reads (%.0f samples, %.0f bases each on average) over %d bases, %d planted sites, in %.1f s' % (
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
    print('%-46s %9.2f ms wall, %8.2f ms in kernels (allele %.3f ms), %11.0f %s/s' % (
        name, dt * 1e3, kern, timing['allele'][0], unit / dt, what))
    return out


warm = synthetic.make_mixed_read_batch(64, [ref] + haps, [0.0, 0.5, 0.5], seed=8, model=model)
phase_reads_batch(ref, warm[0], config=config, kmer_model=km, aligner=SyntheticBatchAligner(ref, warm[1]),
                  threshold=threshold, span=SPAN)

for rep in range(2):
    timed('estimate_allele_fractions_batch (end to end)',
          lambda: estimate_allele_fractions_batch(ref, copy.deepcopy(rb), config=config, kmer_model=km,
                                                  aligner=aligner))
    res = timed('phase_reads_batch (end to end, span %d)' % SPAN,
                lambda: phase_reads_batch(ref, copy.deepcopy(rb), config=config, kmer_model=km, aligner=aligner,
                                          threshold=threshold, clip=CLIP, min_shared=MIN_SHARED, min_link=MIN_LINK,
                                          rounds=ROUNDS, span=SPAN))

stage = device_stage(copy.deepcopy(rb), ref, config, km, aligner, 'pooled')
ll, status, _ = likelihood_rows(stage, config, km)
sa, dbatch = stage.sa, stage.dbatch
start, rev = sa.ref_start.contiguous(), sa.reverse.to(torch.int32)
key, val, skey, order = allele_sorted_rows_dev(ctx, dbatch, ll, start, rev, status, 1.0, G)
sval = val[order]
dev = ll.device
up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
site_pos, site_alt = up(res.position, np.int64), up(res.alt_base, np.int32)
S = len(res)
chain = torch.ones(S, dtype=torch.int32, device=dev)
chain[:1] = 0
row_read = (torch.searchsorted(dbatch.ref_off, order, right=True) - 1).contiguous()
lo, hi = torch.searchsorted(skey, site_pos).contiguous(), torch.searchsorted(skey, site_pos, right=True).contiguous()
site_rows = int((hi - lo).sum())
site_first = torch.zeros(S, dtype=torch.int64, device=dev)
for rep in range(3):
    timed('back half (rows, sort, solve, sites, loop, copy)',
          lambda: phase_of_rows(stage, ll, status, ref, None, km, rb.n, threshold, None, 0.25, 8, 1.0, CLIP,
                                MIN_SHARED, MIN_LINK, ROUNDS, SPAN))
    timed('  phase_sites_dev (links, %d x (tag, votes))' % (ROUNDS + 1),
          lambda: phase_sites_dev(ctx, dbatch.ref_off, start, rev, key, val, skey, sval, order, site_pos, site_alt,
                                  chain, CLIP, MIN_SHARED, MIN_LINK, ROUNDS, span=SPAN), S, 'sites')
    link, shared = timed('    phase_links_dev', lambda: phase_links_dev(ctx, lo, hi, site_alt, chain, row_read, sval,
                                                                        CLIP), site_rows, 'rows')
    block, sigma = timed('    phase_blocks (torch)', lambda: phase_blocks(link, shared, chain, MIN_SHARED, MIN_LINK),
                         S, 'sites')
    tag = timed('    phase_tag_dev', lambda: phase_tag_dev(ctx, dbatch.ref_off, start, rev, key, val, site_pos, site_alt,
                                                           block, sigma, CLIP))
    if SPAN > 1:
        span_link, span_shared = timed('    phase_span_links_dev (span %d)' % SPAN,
                                       lambda: phase_span_links_dev(ctx, lo, hi, site_alt, site_first, row_read, sval,
                                                                    CLIP, SPAN), site_rows, 'rows')
        _, block, sigma = timed('    phase_forest (torch, span %d)' % SPAN,
                                lambda: phase_forest(span_link, span_shared, site_first, MIN_SHARED, MIN_LINK), S,
                                'sites')
        block, sigma = block.contiguous(), sigma.contiguous()
        tag = timed('    phase_tag_blocks_dev', lambda: phase_tag_blocks_dev(ctx, dbatch.ref_off, start, rev, key, val,
                                                                             site_pos, site_alt, block, sigma, CLIP))
    timed('    phase_votes_dev', lambda: phase_votes_dev(ctx, lo, hi, site_alt, block, sigma, row_read, sval, tag[0],
                                                         tag[1], CLIP), site_rows, 'rows')
print('%d sites with %d rows (%.1f per site) among %d rows of %d reads' % (S, site_rows, site_rows / max(S, 1),
                                                                           dbatch.total_ref, n_reads))

# quality against the truth
at = {int(p): t for t, p in enumerate(planted)}
known = np.array([at.get(int(p), -1) for p in res.position])
right_alt = (known >= 0) & (res.alt_base == alts[np.maximum(known, 0)])
print('sites: %d selected, %d of the %d planted (position, base) pairs among them, %d blocks, flips per round %r' % (
    S, int(right_alt.sum()), planted.size, res.n_blocks, res.flips_per_round))
site_owner = np.where(right_alt, owner[np.maximum(known, 0)], 0)
# (with --span a block need not be an interval; adjacent sites of one block are judged all the same)
pair = (res.block[1:] == res.block[:-1]) & (site_owner[1:] > 0) & (site_owner[:-1] > 0)
same_truth = site_owner[1:] == site_owner[:-1]
same_called = res.phase[1:] == res.phase[:-1]
print('adjacent pairs of sites inside one block: %d, correctly phased: %d (%.4f)' % (
    int(pair.sum()), int((pair & (same_truth == same_called)).sum()),
    float((pair & (same_truth == same_called)).sum()) / max(int(pair.sum()), 1)))
tagged = res.haplotype > 0
first_site = np.searchsorted(res.position, np.maximum(res.read_phase_set, 0))
first_owner = site_owner[np.minimum(first_site, max(S - 1, 0))] if S else np.zeros(rb.n, dtype=np.int64)
judged = tagged & (first_owner > 0)
called = np.where(res.haplotype == 1, first_owner, 3 - first_owner)
print('reads: %d tagged of %d, correctly tagged: %d of %d (%.4f)' % (
    int(tagged.sum()), rb.n, int((called[judged] == info['haplotype'][judged]).sum()), int(judged.sum()),
    float((called[judged] == info['haplotype'][judged]).sum()) / max(int(judged.sum()), 1)))
