"""count_repeats_batch on N simulated reads over one tandem-repeat locus (150 random bases, (CAG)n, 150 random bases,
both strands, the simulated signal of ``synthetic.make_read_spec``; n drawn from ``--copies``), counted against
``--loci`` loci (the first is the reads' own, the others random flanks and units: every read is scored against every
locus on both strands): its stages timed apart by HIP events — upload, normalisation, event detection, the rescale
onto the table's means, the items, the operator (``nvk_repeat_count_dev``) and the host's stage 6 — the operator's own
launch time and items per second, the counts it finds, and beside them the front end of ``decode_batch`` (the same
four stages before its operator) on the same batch.  With ``--layers n`` the call with ``layers=n`` is timed too, in
the same session: its stage (``nvk_repeat_likelihoods_dev`` on every pair's chosen item), the operator's own launch
time and cell updates per second (cells = events x layers x states), the whole call beside the plain one, and what
``genotypes()`` makes of it.  After a warm-up; the figures are the median of ``--reps`` runs.
`python tools/bench_repeats.py [N] [--copies a,b] [--loci m] [--reps R] [--layers n]`."""
import argparse
import inspect
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import RepeatLocus, count_repeats_batch, decode, decode_batch, defaults, synthetic  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.readbatch import ReadBatch  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('n_reads', nargs='?', type=int, default=10000)
parser.add_argument('--copies', default='10,25', help='the alleles, copies of the unit; reads take them in turn')
parser.add_argument('--loci', type=int, default=1)
parser.add_argument('--reps', type=int, default=3)
parser.add_argument('--layers', type=int, default=0, help='also time the call with layers=n (0: not)')
opts = parser.parse_args()
alleles = [int(x) for x in opts.copies.split(',')]

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
ctx = km.context
dev = torch.device('cuda', ctx.device)
model = synthetic.load_model_arrays()
rng = np.random.default_rng(11)
SIDE, FLANK, UNIT = 150, 30, np.array([1, 0, 2])
left, right = rng.integers(0, 4, SIDE), rng.integers(0, 4, SIDE)
genomes = [np.concatenate([left, np.tile(UNIT, n), right]).astype(np.int32) for n in alleles]
loci = [RepeatLocus.from_reference(genomes[0], SIDE, SIDE + 3 * alleles[0], UNIT, flank=FLANK, name='CAG')]
for m in range(1, opts.loci):
    unit = rng.integers(0, 4, 3)
    while len(set(unit.tolist())) < 2:
        unit = rng.integers(0, 4, 3)
    loci.append(RepeatLocus('other_%d' % m, rng.integers(0, 4, FLANK), unit, rng.integers(0, 4, FLANK)))
raws, copies = [], []
for i in range(opts.n_reads):
    a = (i // 2) % len(alleles)
    s = synthetic.make_read_spec(np.random.default_rng([11, i]), genomes[a], model, i, length=genomes[a].size, spread=0)
    raws.append(np.rint(s['raw_signal']).astype(np.int16))
    copies.append(alleles[a])
copies = np.array(copies)
bare = ReadBatch.from_signals(np.concatenate(raws), np.concatenate([[0], np.cumsum([x.size for x in raws])]),
                              np.zeros(0, np.int32), np.zeros(len(raws) + 1, np.int64))
STAGES = ('upload', 'normalise', 'events', 'rescale', 'items', 'count', 'results')
STAGES_LIK = STAGES[:-1] + ('likelihoods', 'results')
FRONT = ('upload', 'normalise', 'events', 'rescale', 'decode')


def staged(stages, run):
    """``run(timer)`` with a HIP event after each stage -> (its result, ms per stage)"""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
    torch.cuda.synchronize(dev)
    marks[0].record()
    at = iter(marks[1:])
    out = run(lambda name: next(at).record())
    torch.cuda.synchronize(dev)
    return out, [a.elapsed_time(b) for a, b in zip(marks, marks[1:])]


count = lambda timer: count_repeats_batch(bare, loci, kmer_model=km, timer=timer)
count_lik = lambda timer: count_repeats_batch(bare, loci, kmer_model=km, timer=timer, layers=opts.layers)
defaults_of = inspect.signature(decode_batch).parameters
front_args = tuple(defaults_of[name].default for name in ('p_stay', 'p_skip', 'sigma_scale', 'min_events', 'window',
                                                          'threshold', 'var_floor'))
front = lambda timer: decode.decode_stages(bare, km, *front_args, timer=timer)

staged(STAGES, count)   # warm-up: workspaces, the allocator's blocks, first launches
staged(FRONT, front)
if opts.layers:
    staged(STAGES_LIK, count_lik)
rows, kernel, front_rows, lik_rows, lik_kernel = [], [], [], [], []
for _ in range(opts.reps):
    res, ms = staged(STAGES, count)
    rows.append(ms)
    kernel.append(res.kernel_ms)
    front_rows.append(staged(FRONT, front)[1])
    if opts.layers:
        with_lik, ms = staged(STAGES_LIK, count_lik)
        lik_rows.append(ms)
        lik_kernel.append(with_lik.lik_ms)
med, kernel_ms = np.median(np.array(rows), axis=0), float(np.median(kernel))
front_ms = np.median(np.array(front_rows), axis=0)
n_items = 2 * opts.n_reads * len(loci)
own = res.locus == 0
n_states = loci[0].left.size + 3 * int(res.c0[0]) + loci[0].right.size - km.get_k() + 1   # every locus: the same shape
print('%d reads, %.0f events and %.0f samples each on average; %d locus/loci, %d items; chain of %d states'
      % (opts.n_reads, res.n_events[own].mean(), bare.sig_off[-1] / opts.n_reads, len(loci), n_items,
         n_states))
for name, text in zip(STAGES, ('upload (raw signal, offsets)', 'normalise (nvk_normalize_groups_dev)',
                               'events (flags, prefix sums, levels)', 'rescale onto the table\'s means, chain tables',
                               'items (torch)', 'operator call (checks, launch, wait)',
                               'results to the host, stage 6 in numpy')):
    print('%-46s %9.2f ms' % (text, med[STAGES.index(name)]))
print('%-46s %9.2f ms  (%.2f M items/s, %.1f G cell updates/s)'
      % ('operator, its launches alone (HIP events)', kernel_ms, n_items / kernel_ms / 1e3,
         float(res.n_events[own].sum()) * 2 * len(loci) * n_states / kernel_ms / 1e6))
print('%-46s %9.2f ms  (%.1f k reads/s)' % ('count_repeats_batch, the whole call', med.sum(),
                                            opts.n_reads / med.sum()))
print('%-46s %9.2f ms  (upload %.2f, normalise %.2f, events %.2f, rescale %.2f)'
      % ('decode_batch\'s front end, the same batch', front_ms[:4].sum(), *front_ms[:4]))
ok = own & res.spanning
print('strand right for %d of %d reads; counts per allele (median, min-max): %s' % (
    int((res.strand[own] == (np.arange(opts.n_reads) % 2))[res.status[own] == 0].sum()), opts.n_reads,
    ', '.join('%d: %.1f, %d-%d' % (n, np.median(res.count[ok & (copies[res.read] == n)]),
                                    res.count[ok & (copies[res.read] == n)].min(),
                                    res.count[ok & (copies[res.read] == n)].max()) for n in alleles)))
print('alleles():', res.alleles()[0])
if opts.layers:
    lik_med, lik_ms = np.median(np.array(lik_rows), axis=0), float(np.median(lik_kernel))
    cells = float(with_lik.n_events[with_lik.status == 0].sum()) * opts.layers * n_states
    print('--- layers=%d: one item per pair, %d items' % (opts.layers, with_lik.n))
    print('%-46s %9.2f ms' % ('likelihoods stage (items, call, to the host)', lik_med[STAGES_LIK.index('likelihoods')]))
    print('%-46s %9.2f ms  (%.1f G cell updates/s)' % ('operator, its launches alone (HIP events)', lik_ms,
                                                       cells / lik_ms / 1e6))
    print('%-46s %9.2f ms  (%.1f k reads/s; the plain call: %.2f ms)'
          % ('count_repeats_batch(layers=%d), the whole call' % opts.layers, lik_med.sum(),
             opts.n_reads / lik_med.sum(), med.sum()))
    lik_own = with_lik.locus == 0
    print('count_map equals count on %d of %d pairs of the reads\' own locus; %d clipped'
          % (int((with_lik.count_map == with_lik.count)[lik_own].sum()), int(lik_own.sum()),
             int(with_lik.clipped[lik_own].sum())))
    print('genotypes():', {k: v for k, v in with_lik.genotypes()[0].items() if k != 'table'})
