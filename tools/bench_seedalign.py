"""SeedAligner on N bench-shaped reads (cfg2_align: 400 +- 40 bases on a 10 000-base reference, both strands, the
simulated signal of ``synthetic.make_read_batch``): ``SeedAligner.align`` with the seeding (torch) and the extension
kernel (``nvk_seed_extend_dev``) timed apart, and ``align_signal_batch`` with ``SeedAligner`` against the same call with
``SyntheticBatchAligner``.  HIP events after a warm-up; the figures are the median of ``--reps`` runs.
``--contigs C`` cuts the same genome into C equal contigs (a ``ReferenceSet``: the bounded entry of the kernel, the
contig rule, k-mers across the joins left out) for the same reads; reads that cross a join then align to one side.
``--chain`` runs the aligner with ``chain=1`` and times its stages apart: the seeding with the strand's seeds, their
sort, the chain kernel (``nvk_seed_chain_dev``) and the extension along the chain (``nvk_seed_extend_path_dev``).
``--band W`` sets the band's half-width.  ``--length L`` and / or ``--deletion-rate D`` replace the reads by
``synthetic.make_error_read_batch``'s: L +- L / 10 bases (default 400) with substitutions 0.03, insertions 0.01 and
deletions D (default 0.05) on a reference of at least 10 L bases, so that the diagonal drifts by about (D - 0.01) L;
they carry no signal, so the ``align_signal_batch`` rows are left out and the share of the true pairs that come back
is printed instead, with the bytes of the traceback store.
`python tools/bench_seedalign.py [N] [--reps R] [--contigs C] [--chain] [--band W] [--length L] [--deletion-rate D]`."""
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
parser.add_argument('--chain', action='store_true')
parser.add_argument('--band', type=int, default=None)
parser.add_argument('--length', type=int, default=None)
parser.add_argument('--deletion-rate', type=float, default=None)
opts = parser.parse_args()
n_reads, reps = opts.n_reads, opts.reps

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
ctx = km.context
error_reads = opts.length is not None or opts.deletion_rate is not None
if error_reads:
    length = 400 if opts.length is None else opts.length
    genome = np.random.default_rng(7).integers(0, 4, max(10000, 10 * length)).astype(np.int32)
    rb, truth, _ = synthetic.make_error_read_batch(
        n_reads, genome, seed=7, length=length, spread=length // 10, substitution_rate=0.03, insertion_rate=0.01,
        deletion_rate=0.05 if opts.deletion_rate is None else opts.deletion_rate)
    syn = None
else:
    rb, syn, genome = synthetic.make_read_batch(n_reads, synthetic.load_model_arrays(), seed=7)
dev = torch.device('cuda', ctx.device)
reference = genome
if opts.contigs:
    from nadavca_amd.refset import ReferenceSet  # noqa: E402
    cuts = np.linspace(0, genome.size, opts.contigs + 1).astype(np.int64)
    reference = ReferenceSet(['contig%d' % c for c in range(opts.contigs)], cuts, genome)
params = dict(chain=1) if opts.chain else {}
if opts.band is not None:
    params['band'] = opts.band
al = SeedAligner(reference, device=dev, **params)
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


def chain_stages():
    """The stages of ``align`` with chain=1, one by one: -> ms of (strand_seeds, sort_seeds, chain kernel, extension
    along the path), the kernels by the library's timer"""
    from nadavca_amd.device import seed_chain_dev, seed_extend_path_dev
    p = al.params
    (strand, diagonal, _, rd, si, sp), ms_seeds, _ = timed(lambda: al.strand_seeds(rb))
    (seed_off, si, sp), ms_sort, _ = timed(lambda: al.sort_seeds(rb.n, rd, si, sp))
    q_off = torch.from_numpy(rb.seq_off).to(dev)
    query = torch.from_numpy(rb.sequence).to(dev)
    strips = torch.div(q_off[1:] - q_off[:-1] + 63, 64, rounding_mode='floor')
    strip_off = torch.zeros(rb.n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(strips, 0, out=strip_off[1:])
    strip_diag = torch.repeat_interleave(diagonal.to(torch.int32), strips).contiguous()
    lo = hi = None
    if al.reference_set is not None:
        _, lo, hi = al.contig_of(rb, strand, diagonal)
    _, _, ms_chain = timed(lambda: seed_chain_dev(ctx, q_off, strand, seed_off, si, sp, strip_off, strip_diag, p['k'],
                                                  p['band'], p['max_gap']))
    _, _, ms_ext = timed(lambda: seed_extend_path_dev(ctx, query, q_off, al._ref, strand, strip_off, strip_diag,
                                                      p['band'], p['match'], p['mismatch'], p['gap_open'],
                                                      p['gap_extend'], p['min_score'], lo, hi))
    return ms_seeds, ms_sort, ms_chain, ms_ext, int(seed_off[-1])


for _ in range(2):   # warm-up: workspaces, the allocator's blocks, first launches
    al.align(rb)
    if opts.chain:
        chain_stages()
    if not error_reads:
        align_signal_batch(None, rb, kmer_model=km, aligner=al)
        align_signal_batch(None, rb, kmer_model=km, aligner=syn)

rows = {k: [] for k in ('seed', 'align', 'kernel', 'asb_seed', 'asb_syn', 'c_seeds', 'c_sort', 'c_chain', 'c_ext')}
n_seeds = 0
for _ in range(reps):
    _, ms, _ = timed(lambda: al.seed(rb))
    rows['seed'].append(ms)
    hits, ms, kern = timed(lambda: al.align(rb))
    rows['align'].append(ms)
    rows['kernel'].append(kern)
    if opts.chain:
        *stages, n_seeds = chain_stages()
        for k, ms in zip(('c_seeds', 'c_sort', 'c_chain', 'c_ext'), stages):
            rows[k].append(ms)
    if not error_reads:
        _, ms, _ = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=al))
        rows['asb_seed'].append(ms)
        _, ms, _ = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=syn))
        rows['asb_syn'].append(ms)
med = {k: float(np.median(v)) for k, v in rows.items() if v}
band = al.params['band']
lens = np.diff(rb.seq_off)
cells = int(lens.sum()) * (2 * band + 1)
store = int((((lens + 63) // 64)[hits.strand >= 0]).sum()) * ((2 * band + 8) // 8) * 64 * 4
print('SeedAligner.seed (step 1, torch)              %8.2f ms' % med['seed'])
print('SeedAligner.align (seed + kernel%s + gathers)  %8.2f ms  (%.0f k reads/s)' % (
    's' if opts.chain else '', med['align'], n_reads / med['align']))
print('  of which the %s               %8.2f ms  (%.2f G band cells/s)' % (
    'seed kernels    ' if opts.chain else 'extension kernel', med['kernel'], cells / med['kernel'] / 1e6))
if opts.chain:
    print('stage by stage: seeding with the strand\'s seeds %8.2f ms' % med['c_seeds'])
    print('                sort of %9d seeds         %8.2f ms' % (n_seeds, med['c_sort']))
    print('                chain kernel                   %8.2f ms' % med['c_chain'])
    print('                extension along the chain      %8.2f ms' % med['c_ext'])
print('band %d, traceback store %d bytes' % (band, store))
if error_reads:
    key = lambda b: (np.repeat(np.arange(n_reads), np.diff(b.off)) * (int(lens.max()) + 1)
                     + b.read_idx.astype(np.int64)) * (genome.size + 1) + b.ref_idx.astype(np.int64)
    t = key(truth)
    print('share of the true pairs that come back: %.4f; aligned %d / %d' % (
        np.intersect1d(t, key(hits)).size / max(t.size, 1), int(hits.aligned.sum()), n_reads))
else:
    ba = syn.get_base_alignments(rb)
    same = not opts.contigs and all(np.array_equal(getattr(hits.base_alignments(), f), getattr(ba, f))
                                    for f in ('read_idx', 'ref_idx', 'off', 'reverse'))
    print('align_signal_batch, SeedAligner               %8.2f ms' % med['asb_seed'])
    print('align_signal_batch, SyntheticBatchAligner     %8.2f ms' % med['asb_syn'])
    print('pairs equal to the simulated truth: %s; aligned %d / %d' % (
        same if not opts.contigs else 'n/a (reads across a join keep one side)', int(hits.aligned.sum()), n_reads))
