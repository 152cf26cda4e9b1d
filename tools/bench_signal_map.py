"""signal_map_batch on N bench-shaped reads (cfg2_align: 400 +- 40 bases on a 10 000-base reference, both strands, the
simulated signal of ``synthetic.make_read_batch``): its stages timed apart — upload, normalisation, event detection
(``nvk_event_flags_dev``, the prefix sums, ``nvk_event_levels_dev``), the k-mer tables with the rescale by moments, the
alignment kernel (``nvk_event_align_dev``) — then the whole call, beside ``align_signal_batch`` with ``SeedAligner`` on
the same batch from the simulator's table and from the rebuilt one.  HIP events after a warm-up; the figures are the
median of ``--reps`` runs.  `python tools/bench_signal_map.py [N] [--reps R] [--band 64|128]`."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import defaults, signal_map_batch, synthetic  # noqa: E402
from nadavca_amd.align_signal import align_signal_batch  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.readbatch import ReadBatch  # noqa: E402
from nadavca_amd.seedalign import SeedAligner  # noqa: E402
from nadavca_amd.signal_map import signal_map_stages  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('n_reads', nargs='?', type=int, default=10000)
parser.add_argument('--reps', type=int, default=5)
parser.add_argument('--band', type=int, default=128)
opts = parser.parse_args()

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
dev = torch.device('cuda', km.context.device)
rb, _, genome = synthetic.make_read_batch(opts.n_reads, synthetic.load_model_arrays(), seed=7)
bare = ReadBatch.from_signals(rb.raw_signal, rb.sig_off, rb.sequence, rb.seq_off)
al = SeedAligner(genome, device=dev)
STAGES = ('upload', 'normalise', 'events', 'rescale', 'align')
args = (2, 5.0, 0.02, opts.band, 0.5, math.log(0.01), math.log(1e-10))


def staged():
    """-> (the stages' tensors, ms per stage by HIP events)"""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
    torch.cuda.synchronize(dev)
    marks[0].record()
    at = iter(marks[1:])
    st = signal_map_stages(bare, km, *args, timer=lambda name: next(at).record())
    torch.cuda.synchronize(dev)
    return st, [a.elapsed_time(b) for a, b in zip(marks, marks[1:])]


def timed(fn):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return out, e0.elapsed_time(e1)


whole = lambda: signal_map_batch(bare, kmer_model=km, band=opts.band)
for _ in range(2):   # warm-up: workspaces, the allocator's blocks, first launches
    staged()
    rebuilt = whole().read_batch(bare)
    align_signal_batch(None, rb, kmer_model=km, aligner=al)
    align_signal_batch(None, rebuilt, kmer_model=km, aligner=al)

rows = {k: [] for k in STAGES + ('whole', 'asb_table', 'asb_rebuilt')}
for _ in range(opts.reps):
    st, ms = staged()
    for k, v in zip(STAGES, ms):
        rows[k].append(v)
    sm, ms = timed(whole)
    rows['whole'].append(ms)
    a, ms = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=al))
    rows['asb_table'].append(ms)
    b, ms = timed(lambda: align_signal_batch(None, rebuilt, kmer_model=km, aligner=al))
    rows['asb_rebuilt'].append(ms)
med = {k: float(np.median(v)) for k, v in rows.items()}
n_ev, n_base = int(st.ev_off[-1]), int(rb.seq_off[-1])
cells = (n_ev + n_base + opts.n_reads) * opts.band
print('%d reads, %.0f bases and %.0f events each on average, %.0f samples; band %d' % (
    opts.n_reads, n_base / opts.n_reads, n_ev / opts.n_reads, rb.sig_off[-1] / opts.n_reads, opts.band))
print('upload (raw signal, sequence, offsets)         %8.2f ms' % med['upload'])
print('normalise (nvk_normalize_groups_dev)           %8.2f ms' % med['normalise'])
print('events (flags, prefix sums, levels)            %8.2f ms' % med['events'])
print('k-mer tables and rescale by moments            %8.2f ms' % med['rescale'])
print('alignment kernel (nvk_event_align_dev)         %8.2f ms  (%.2f G band cells/s)' % (
    med['align'], cells / med['align'] / 1e6))
print('signal_map_batch, the whole call               %8.2f ms  (%.0f k reads/s)' % (
    med['whole'], opts.n_reads / med['whole']))
print('align_signal_batch, simulator\'s table          %8.2f ms  (%d aligned)' % (med['asb_table'], a.n_aligned))
print('align_signal_batch, rebuilt table              %8.2f ms  (%d aligned)' % (med['asb_rebuilt'], b.n_aligned))
print('mapped %d / %d reads; %.4f of the bases have a row' % (sm.n_mapped, sm.n, sm.map_off[-1] / max(n_base, 1)))
