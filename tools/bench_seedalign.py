"""SeedAligner on N bench-shaped reads (cfg2_align: 400 +- 40 bases on a 10 000-base reference, both strands, the
simulated signal of ``synthetic.make_read_batch``): ``SeedAligner.align`` with the seeding (torch) and the extension
kernel (``nvk_seed_extend_dev``) timed apart, and ``align_signal_batch`` with ``SeedAligner`` against the same call with
``SyntheticBatchAligner``.  HIP events after a warm-up; the figures are the median of ``--reps`` runs.
``--contigs C`` cuts the same genome into C equal contigs (a ``ReferenceSet``: the bounded entry of the kernel, the
contig rule, k-mers across the joins left out) for the same reads; reads that cross a join then align to one side.
`python tools/bench_seedalign.py [N] [--reps R] [--contigs C]`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import synthetic, defaults, _lib  # noqa: E402
from nadavca_amd.align_signal import align_signal_batch  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.seedalign import SeedAligner  # noqa: E402

import argparse  # noqa: E402
parser = argparse.ArgumentParser()
parser.add_argument('n_reads', nargs='?', type=int, default=10000)
parser.add_argument('--reps', type=int, default=5)
parser.add_argument('--contigs', type=int, default=0)
opts = parser.parse_args()
n_reads, reps = opts.n_reads, opts.reps

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
ctx = km.context
rb, syn, genome = synthetic.make_read_batch(n_reads, synthetic.load_model_arrays(), seed=7)
dev = torch.device('cuda', ctx.device)
reference = genome
if opts.contigs:
    from nadavca_amd.refset import ReferenceSet  # noqa: E402
    cuts = np.linspace(0, genome.size, opts.contigs + 1).astype(np.int64)
    reference = ReferenceSet(['contig%d' % c for c in range(opts.contigs)], cuts, genome)
al = SeedAligner(reference, device=dev)
print('%d reads, %.0f bases each on average, reference %d bases%s' % (
    n_reads, rb.seq_off[-1] / n_reads, genome.size, ' in %d contigs' % opts.contigs if opts.contigs else ''))


def timed(fn):
    """-> (result, ms by HIP events around fn, ms of the seed kernel inside it)"""
    torch.cuda.synchronize(dev)
    ctx.timing_reset()
    ctx.timing_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    ctx.timing_enable(False)
    return out, e0.elapsed_time(e1), ctx.timing_read()['seed'][0]


for _ in range(2):   # warm-up: workspaces, the allocator's blocks, first launches
    al.align(rb)
    align_signal_batch(None, rb, kmer_model=km, aligner=al)
    align_signal_batch(None, rb, kmer_model=km, aligner=syn)

rows = {k: [] for k in ('seed', 'align', 'kernel', 'asb_seed', 'asb_syn')}
for _ in range(reps):
    _, ms, _ = timed(lambda: al.seed(rb))
    rows['seed'].append(ms)
    hits, ms, kern = timed(lambda: al.align(rb))
    rows['align'].append(ms)
    rows['kernel'].append(kern)
    _, ms, _ = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=al))
    rows['asb_seed'].append(ms)
    _, ms, _ = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=syn))
    rows['asb_syn'].append(ms)
med = {k: float(np.median(v)) for k, v in rows.items()}
ba = syn.get_base_alignments(rb)
same = not opts.contigs and all(np.array_equal(getattr(hits.base_alignments(), f), getattr(ba, f))
                                for f in ('read_idx', 'ref_idx', 'off', 'reverse'))
cells = int(np.diff(rb.seq_off).sum()) * (2 * al.params['band'] + 1)
print('SeedAligner.seed (step 1, torch)              %8.2f ms' % med['seed'])
print('SeedAligner.align (seed + kernel + gathers)   %8.2f ms  (%.0f k reads/s)' % (med['align'], n_reads / med['align']))
print('  of which the extension kernel               %8.2f ms  (%.2f G band cells/s)' % (
    med['kernel'], cells / med['kernel'] / 1e6))
print('align_signal_batch, SeedAligner               %8.2f ms' % med['asb_seed'])
print('align_signal_batch, SyntheticBatchAligner     %8.2f ms' % med['asb_syn'])
print('pairs equal to the simulated truth: %s; aligned %d / %d' % (
    same if not opts.contigs else 'n/a (reads across a join keep one side)', int(hits.aligned.sum()), n_reads))
