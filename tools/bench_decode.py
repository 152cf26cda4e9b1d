"""decode_batch on N bench-shaped reads (400 +- 40 bases, both strands, the simulated signal of
``synthetic.make_read_batch``) over a random genome of ``--genome`` bases: its stages timed apart — upload,
normalisation, event detection, the rescale onto the table's means, the operator (``nvk_viterbi_decode_dev``: the sweep
and the walk back of every part under the workspace cap) — the operator alone in cell updates per second (4^k per
event), the traceback store's bytes and parts, the whole call, and the chain decode_batch -> ``SeedAligner(k=10)`` ->
align_signal_batch beside ``align_signal_batch`` with the same aligner from the simulator's own sequences and tables.
HIP events after a warm-up; the figures are the median of ``--reps`` runs.  ``--qualities``: also the forward-backward
operator of ``decode_batch(qualities=True)`` (``nvk_kmer_posterior_dev``) -- its forward and backward launches apart,
its parts and row-store bytes with the bytes-over-bandwidth floor -- and the whole call with qualities beside the plain
one of the same session.  ``--fit R``: also ``decode_batch(fit=R)`` -- the E-step operator (``nvk_kmer_expectations_dev``)
of every round and of the closing pass with its forward and counts launches apart, the host's share of the fit (the
M-steps, the copies, the levels and tables of every round), and the whole call with the fit beside the plain one.
`python tools/bench_decode.py [N] [--genome L] [--reps R] [--qualities] [--fit R] [--limit-gib G]`."""
import argparse
import inspect
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nadavca_amd import decode, decode_batch, decode_fit, defaults, synthetic  # noqa: E402
from nadavca_amd.align_signal import align_signal_batch  # noqa: E402
from nadavca_amd.device import kmer_posterior_dev, viterbi_decode_dev  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.readbatch import ReadBatch  # noqa: E402
from nadavca_amd.seedalign import SeedAligner  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('n_reads', nargs='?', type=int, default=10000)
parser.add_argument('--genome', type=int, default=100000)
parser.add_argument('--reps', type=int, default=3)
parser.add_argument('--qualities', action='store_true')
parser.add_argument('--fit', type=int, default=0, help='rounds of decode_batch(fit=R) to time (0: none)')
parser.add_argument('--limit-gib', type=float, default=0.0, help='workspace limit of the context (0: the default caps)')
opts = parser.parse_args()

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
ctx = km.context
if opts.limit_gib > 0:
    ctx.set_workspace_limit(int(opts.limit_gib * 2 ** 30))
dev = torch.device('cuda', ctx.device)
rb, _, genome = synthetic.make_read_batch(opts.n_reads, synthetic.load_model_arrays(), seed=7,
                                          genome_length=opts.genome)
bare = ReadBatch.from_signals(rb.raw_signal, rb.sig_off, np.zeros(0, np.int32), np.zeros(rb.n + 1, np.int64))
seed = SeedAligner(genome, k=10)
STAGES = ('upload', 'normalise', 'events', 'rescale', 'decode')
defaults_of = inspect.signature(decode_batch).parameters   # the staged run takes decode_batch's own defaults
args = tuple(defaults_of[name].default for name in ('p_stay', 'p_skip', 'sigma_scale', 'min_events', 'window',
                                                    'threshold', 'var_floor'))


def staged():
    """-> (the stages' tensors, ms per stage by HIP events)"""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
    torch.cuda.synchronize(dev)
    marks[0].record()
    at = iter(marks[1:])
    st = decode.decode_stages(bare, km, *args, timer=lambda name: next(at).record())
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
    return timed(lambda: viterbi_decode_dev(ctx, st.scaled, st.ev_off, km.get_k(), km.get_central_position(), st.mean,
                                            st.ac, st.mc, *st.costs, st.status_in, st.cap_off))[1]


def posterior_alone(st):
    """-> (ms of the call, (ms of the forward launches, ms of the backward launches), parts)"""
    out, ms = timed(lambda: kmer_posterior_dev(ctx, st.scaled, st.ev_off, km.get_k(), km.get_central_position(), st.mean,
                                               st.ac, st.mc, *decode.transition_weights(args[0], args[1]),
                                               st.status_in, timing=True))
    return ms, out[4], out[3]


def fit_alone(st):
    """-> (ms of the fit, per E-step (forward ms, counts ms), the DecodeFit)"""
    launches = []
    fit, ms = timed(lambda: decode_fit.fit_on_device(st, km, opts.fit, decode_fit.FIT_PARAMS, args[2], args[0], args[1],
                                                     timer=lambda name, t: launches.append(t)))
    return ms, list(zip(launches[0::2], launches[1::2])), fit


whole = lambda: decode_batch(bare, kmer_model=km)
whole_f = lambda: decode_batch(bare, kmer_model=km, fit=opts.fit)
whole_q = lambda: decode_batch(bare, kmer_model=km, qualities=True)


def chain():
    dec = whole()
    return dec, align_signal_batch(None, dec.read_batch(bare), kmer_model=km, aligner=seed)


staged()   # warm-up: workspaces, the allocator's blocks, first launches
chain()
align_signal_batch(None, rb, kmer_model=km, aligner=seed)
rows = {k: [] for k in STAGES + ('operator', 'whole', 'chain', 'asb_table', 'post', 'forward', 'backward', 'whole_q')}
if opts.qualities:
    whole_q()
if opts.fit:
    whole_f()
fit_rows = []
for _ in range(opts.reps):
    st, ms = staged()
    for k, v in zip(STAGES, ms):
        rows[k].append(v)
    rows['operator'].append(operator_alone(st))
    dec, ms = timed(whole)
    rows['whole'].append(ms)
    (_, b), ms = timed(chain)
    rows['chain'].append(ms)
    a, ms = timed(lambda: align_signal_batch(None, rb, kmer_model=km, aligner=seed))
    rows['asb_table'].append(ms)
    if opts.qualities:
        ms, (fwd, bwd), post_parts = posterior_alone(st)
        rows['post'].append(ms)
        rows['forward'].append(fwd)
        rows['backward'].append(bwd)
        rows['whole_q'].append(timed(whole_q)[1])
    if opts.fit:
        ms, launches, fitted = fit_alone(st)
        fit_rows.append([ms] + [t for pair in launches for t in pair] + [timed(whole_f)[1]])
med = {k: float(np.median(v)) for k, v in rows.items() if v}
k = km.get_k()
n_ev = st.ev_off.cpu().numpy()
decoded = n_ev[1:] - n_ev[:-1]
decoded = decoded[st.ok.cpu().numpy()]
cells = int(decoded.sum()) * 4 ** k
store = decode.traceback_bytes(decoded, k)
print('%d reads, %.0f events and %.0f samples each on average; k = %d, %d states; genome %d bases'
      % (opts.n_reads, n_ev[-1] / opts.n_reads, rb.sig_off[-1] / opts.n_reads, k, 4 ** k, opts.genome))
print('upload (raw signal, offsets, the table)        %9.2f ms' % med['upload'])
print('normalise (nvk_normalize_groups_dev)           %9.2f ms' % med['normalise'])
print('events (flags, prefix sums, levels)            %9.2f ms' % med['events'])
print('rescale onto the table\'s means, capacities     %9.2f ms' % med['rescale'])
print('operator, %3d part(s)                          %9.2f ms' % (st.parts, med['decode']))
print('operator alone                                 %9.2f ms  (%.1f G cell updates/s; traceback store %.1f MB, '
      '%.1f GB/s written)' % (med['operator'], cells / med['operator'] / 1e6, store / 1e6,
                              store / med['operator'] / 1e6))
print('decode_batch, the whole call                   %9.2f ms  (%.1f k reads/s; %d decoded, %.2f bases per event)' % (
    med['whole'], opts.n_reads / med['whole'], dec.n_decoded, dec.n_bases.sum() / max(int(dec.n_events.sum()), 1)))
print('decode -> SeedAligner(k=10) -> align_signal    %9.2f ms  (%d aligned)' % (med['chain'], b.n_aligned))
print('align_signal_batch, simulator\'s sequences      %9.2f ms  (%d aligned)' % (med['asb_table'], a.n_aligned))
if opts.qualities:
    HBM_GBS = 8000.0   # the MI355X's HBM3E peak, GB/s
    rows_b = decode.row_store_bytes(decoded, k)
    print('posterior operator alone, %3d part(s)          %9.2f ms  (forward launches %.2f ms, backward launches %.2f ms; '
          '%.1f G cell updates/s each way)' % (post_parts, med['post'], med['forward'], med['backward'],
                                               cells / med['post'] / 1e6 * 2))
    print('    row store %.1f GB written and read back: %.1f GB/s forward, %.1f GB/s backward; floor at %.0f GB/s: %.1f ms '
          'each way' % (rows_b / 1e9, rows_b / med['forward'] / 1e6, rows_b / med['backward'] / 1e6, HBM_GBS,
                        rows_b / HBM_GBS / 1e6))
    print('decode_batch(qualities=True), the whole call   %9.2f ms  (%.1f k reads/s; plain call above: %.2f ms)'
          % (med['whole_q'], opts.n_reads / med['whole_q'], med['whole']))
if opts.fit:
    med_f = np.median(np.array(fit_rows), axis=0)
    print('fit alone, %d round(s) and the closing pass       %9.2f ms  (%d part(s) per E-step; sigma_scale %.4f, p_stay %.4f, '
          'p_skip %.5f)' % (opts.fit, med_f[0], fitted.parts, fitted.sigma_scale, fitted.p_stay, fitted.p_skip))
    for r in range(opts.fit + 1):
        print('    %s: forward launches %8.2f ms, counts launches %8.2f ms'
              % ('round %d' % (r + 1) if r < opts.fit else 'closing', med_f[1 + 2 * r], med_f[2 + 2 * r]))
    print('    host share (M-steps, copies, levels and tables)  %7.2f ms' % (med_f[0] - med_f[1:-1].sum()))
    print('decode_batch(fit=%d), the whole call               %9.2f ms  (%.1f k reads/s; plain call above: %.2f ms)'
          % (opts.fit, med_f[-1], opts.n_reads / med_f[-1], med['whole']))
