"""signal_locate_batch on N bench-shaped reads (400 +- 40 bases, both strands, the simulated signal of
``synthetic.make_read_batch``) against a random genome of ``--genome`` bases: its stages timed apart — upload,
normalisation, event detection, the column tables, the rescale with the chunk cut, the operator with its reduction
(``nvk_signal_locate_dev`` in parts under the block-table cap) — the operator alone in cells/s, the whole call, and the
chain signal_locate_batch -> signal_map_batch -> align_signal_batch beside ``align_signal_batch`` from the simulator's
table and true alignment.  HIP events after a warm-up; the figures are the median of ``--reps`` runs.
`python tools/bench_signal_locate.py [N] [--genome L] [--max-events Q] [--reps R]`."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import defaults, locate, signal_locate_batch, signal_map_batch, synthetic  # noqa: E402
from nadavca_amd.align_signal import align_signal_batch  # noqa: E402
from nadavca_amd.device import signal_locate_dev  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.readbatch import ReadBatch  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('n_reads', nargs='?', type=int, default=10000)
parser.add_argument('--genome', type=int, default=10000)
parser.add_argument('--max-events', type=int, default=128)
parser.add_argument('--reps', type=int, default=3)
opts = parser.parse_args()

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
ctx = km.context
dev = torch.device('cuda', ctx.device)
rb, true_aligner, genome = synthetic.make_read_batch(opts.n_reads, synthetic.load_model_arrays(), seed=7,
                                                     genome_length=opts.genome)
bare = ReadBatch.from_signals(rb.raw_signal, rb.sig_off, np.zeros(0, np.int32), np.zeros(rb.n + 1, np.int64))
targets = locate.target_tables(genome)
STAGES = ('upload', 'normalise', 'events', 'tables', 'rescale', 'locate')
args = (opts.max_events, 32, 0.5, 0.02, 0.5, math.log(0.01), 2, 5.0, 0.02)


def staged():
    """-> (the stages' tensors, ms per stage by HIP events)"""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
    torch.cuda.synchronize(dev)
    marks[0].record()
    at = iter(marks[1:])
    st = locate.signal_locate_stages(bare, targets, km, *args, timer=lambda name: next(at).record())
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


def operator_alone(st):
    """The operator on as many of the queries as one part takes, without the reduction"""
    per = max(1, locate.table_cap(ctx) // max(st.n_blocks * locate.TABLE_BYTES, 1))
    nq = min(per, int(st.q_off.numel()) - 1)
    hi = int(st.q_off[nq])
    q_off = st.q_off[:nq + 1].contiguous()
    _, ms = timed(lambda: signal_locate_dev(ctx, st.q_level[:hi], q_off, st.mu, st.ac, st.mc, st.col_off,
                                            opts.max_events, *st.costs, math.log(0.01)))
    return hi * int(st.mu.numel()), ms


whole = lambda: signal_locate_batch(bare, genome, kmer_model=km, max_events=opts.max_events)


def chain():
    loc = whole()
    rb1 = loc.read_batch(bare)
    rb2 = signal_map_batch(rb1, kmer_model=km).read_batch(rb1)
    return loc, align_signal_batch(None, rb2, kmer_model=km, aligner=loc.aligner())


staged()   # warm-up: workspaces, the allocator's blocks, first launches
chain()
align_signal_batch(None, rb, kmer_model=km, aligner=true_aligner)
rows = {k: [] for k in STAGES + ('operator', 'whole', 'chain', 'asb_table')}
for _ in range(opts.reps):
    st, ms = staged()
    for k, v in zip(STAGES, ms):
        rows[k].append(v)
    cells, ms = operator_alone(st)
    rows['operator'].append(ms)
    loc, ms = timed(whole)
    rows['whole'].append(ms)
    (_, b), ms = timed(chain)
    rows['chain'].append(ms)
    a, ms = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=true_aligner))
    rows['asb_table'].append(ms)
med = {k: float(np.median(v)) for k, v in rows.items()}
n_ev, n_q, n_col = int(st.ev_off[-1]), int(st.q_off.numel()) - 1, int(st.mu.numel())
wide = opts.max_events > 128
T, V = 1024, 512 if wide else 768
table = n_q * st.n_blocks * locate.TABLE_BYTES
print('%d reads, %.0f events and %.0f samples each on average; genome %d bases, %d columns in %d blocks; max_events %d: '
      '%d queries' % (opts.n_reads, n_ev / opts.n_reads, rb.sig_off[-1] / opts.n_reads, opts.genome, n_col, st.n_blocks,
                      opts.max_events, n_q))
print('upload (raw signal, reference, offsets)        %9.2f ms' % med['upload'])
print('normalise (nvk_normalize_groups_dev)           %9.2f ms' % med['normalise'])
print('events (flags, prefix sums, levels)            %9.2f ms' % med['events'])
print('column tables of both strands                  %9.2f ms' % med['tables'])
print('rescale onto the pooled columns, chunk cut     %9.2f ms' % med['rescale'])
print('operator and reduction, %3d part(s)            %9.2f ms' % (st.parts, med['locate']))
print('operator alone, one part                       %9.2f ms  (%.1f G cells/s; tile %d columns, %d valid: share '
      '%.2f)' % (med['operator'], cells / med['operator'] / 1e6, T, V, V / T))
print('block table %.1f MB under a cap of %.1f MB' % (table / 1e6, locate.table_cap(ctx) / 1e6))
print('signal_locate_batch, the whole call            %9.2f ms  (%.1f k reads/s)' % (
    med['whole'], opts.n_reads / med['whole']))
print('locate -> signal_map -> align_signal_batch     %9.2f ms  (%d located, %d aligned)' % (
    med['chain'], loc.n_located, b.n_aligned))
print('align_signal_batch, simulator\'s table          %9.2f ms  (%d aligned)' % (med['asb_table'], a.n_aligned))
