"""estimate_kmer_model's rounds on N synthetic reads (synthetic.make_read_batch, int16 raw data, the packaged 6-mer
table with every mean shifted by N(0, 0.25) and every sigma x 1.5 as the start).  Per round: the alignment (the device
half of align_signal_batch) and the two statistics passes, wall time, the time in the `kmer` kernels (ctx.timing_read)
and the bandwidth those kernels reach against the bytes they must move: 8 B per sample of a counted event and pass,
plus per event and pass the events read (8 B), key / value / length written (24 B) and read back by the reduction
with the sort order (32 B).  `python tools/bench_train.py [N] [rounds]`."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nadavca_amd import dtw, synthetic, defaults  # noqa: E402
from nadavca_amd.batchflow import align_batch, load_config  # noqa: E402
from nadavca_amd.kmer_train import kmer_stats_dev  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
n_reads = int(args[0]) if args else 10000
rounds = int(args[1]) if len(args) > 1 else 3
model = synthetic.load_model_arrays()
k, central, alphabet, mean, sigma = model
t0 = time.perf_counter()
rb, aligner, _ = synthetic.make_read_batch(n_reads, model, seed=7)
print('built %d reads (%.0f samples each on average) in %.1f s' % (n_reads, rb.sig_off[-1] / n_reads,
                                                                   time.perf_counter() - t0))
rng = np.random.default_rng(8)
km = dtw.KmerModel(k, central, alphabet, mean + rng.normal(0.0, 0.25, mean.size), sigma * 1.5)
ctx = km.context
config = load_config(defaults.CONFIG_FILE)
align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)   # warm-up: workspaces, first touch
for r in range(rounds):
    ctx.synchronize()
    t = time.perf_counter()
    res = align_batch(rb, config, km, defaults.RENORM_ROUNDS, aligner)
    dbatch, events, status = res.stage.dbatch, res.events, res.status
    ctx.synchronize()
    t_align = time.perf_counter() - t
    ctx.timing_reset()
    ctx.timing_enable(True)
    t = time.perf_counter()
    S, N, e = (x.cpu().numpy() for x in kmer_stats_dev(ctx, dbatch, events, status, k, central, alphabet, 5))
    seen = N > 0
    m = np.zeros(S.size)
    m[seen] = S[seen] / N[seen]
    Q = kmer_stats_dev(ctx, dbatch, events, status, k, central, alphabet, 5, level=m)[0].cpu().numpy()
    ctx.synchronize()
    t_stats = time.perf_counter() - t
    ctx.timing_enable(False)
    kmer_ms, launches = ctx.timing_read()['kmer']
    n_events = dbatch.total_ref
    bytes_moved = 2 * (8 * int(N.sum()) + (8 + 24 + 32) * n_events)
    upd = e >= 10
    new_mean, new_sigma = km.mean.copy(), km.sigma.copy()
    new_mean[upd] = m[upd]
    new_sigma[upd] = np.maximum(np.sqrt(Q[upd] / N[upd]), 0.05)
    print('round %d: align %.1f ms, statistics %.1f ms wall, kmer kernels %.3f ms (%d launches), %.1f M counted '
          'events, %.1f M samples, %.1f GB/s; %d k-mers updated, max events per k-mer %d'
          % (r, t_align * 1e3, t_stats * 1e3, kmer_ms, launches, e.sum() / 1e6, N.sum() / 1e6,
             bytes_moved / (kmer_ms * 1e-3) / 1e9 if kmer_ms > 0 else 0.0, int(upd.sum()), int(e.max())))
    km = dtw.KmerModel(k, central, alphabet, new_mean, new_sigma, context=ctx)
