"""estimate_decode_model on N bench-shaped reads (400 +- 40 bases, both strands, the simulated signal of
``synthetic.make_read_batch``): per round the launches of its operator (``nvk_kmer_state_moments_dev``: forward, moments
and reduce, summed over the parts), the parts and the bytes of the slabs, the fit's E-steps before it, and the whole
call; as the yardstick the counts sweep (``nvk_kmer_expectations_dev``) and the backward sweep
(``nvk_kmer_posterior_dev``) on the same levels in the same session.  HIP events after a warm-up.
``--quality``: instead, the 300 leader-padded reads of the test suite from the packaged table with its means displaced by
N(0, (0.15 spread)^2): mean identity of ``decode_batch``'s sequences to the true ones and the share of reads with at
least three exact 10-mer seeds, with the displaced table and with the re-estimated one (and with the packaged one).
`python tools/bench_decode_train.py [N] [--rounds R] [--fit F] [--limit-gib G] [--quality]`."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from nadavca_amd import decode_batch, decode_train, defaults, estimate_decode_model, synthetic  # noqa: E402
from nadavca_amd.device import kmer_expectations_dev, kmer_posterior_dev  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.rawsignal import gaussian_constants, transition_weights  # noqa: E402
from nadavca_amd.readbatch import ReadBatch  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('n_reads', nargs='?', type=int, default=10000)
parser.add_argument('--rounds', type=int, default=2)
parser.add_argument('--fit', type=int, default=1)
parser.add_argument('--limit-gib', type=float, default=0.0, help='workspace limit of the context (0: the default caps)')
parser.add_argument('--quality', action='store_true')
opts = parser.parse_args()

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
ctx = km.context
if opts.limit_gib > 0:
    ctx.set_workspace_limit(int(opts.limit_gib * 2 ** 30))
dev = torch.device('cuda', ctx.device)
k = km.get_k()


def timed(fn):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return out, e0.elapsed_time(e1)


def quality():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import decode_ref as D
    import signal_map_ref as R
    rb, _, _, (raw, sig_off, _) = R.quality_batch(synthetic.load_model_arrays())
    bare = ReadBatch.from_signals(raw, sig_off, np.zeros(0, np.int32), np.zeros(rb.n + 1, np.int64))
    truths = D.read_sequences(rb)
    true = np.asarray(km.mean, dtype=np.float64)
    moved = true + np.random.default_rng(7).normal(0.0, 0.15 * float(np.std(true)), true.size)
    start = KmerModel(k, km.get_central_position(), 4, moved, np.asarray(km.sigma), context=ctx)

    def report(name, model, **kw):
        dec = decode_batch(bare, kmer_model=model, fit=1, fit_params=('scale',), **kw)
        seqs = [dec.sequence[dec.seq_off[r]:dec.seq_off[r + 1]] for r in range(rb.n)]
        ident = np.array([D.identity(t, s) for t, s in zip(truths, seqs)])
        votes = np.array([D.seed_votes(t, s) for t, s in zip(truths, seqs)])
        print('%-28s decoded %d of %d; mean identity %.4f; share of reads with >= 3 seeds %.4f; RMS error of the means '
              '%.4f' % (name, dec.n_decoded, rb.n, ident.mean(), (votes >= 3).mean(),
                        float(np.sqrt(np.mean((np.asarray(model.mean) - true) ** 2)))))

    report('packaged table', km)
    report('displaced means', start)
    est = estimate_decode_model(bare, kmer_model=start, rounds=opts.rounds, fit=opts.fit)
    print('estimate_decode_model(rounds=%d, fit=%d): objective %s; states updated per round %s; RMS error of the updated '
          'states %.4f -> %.4f'
          % (opts.rounds, opts.fit, ' '.join('%.1f' % v for v in est.objective),
             [h['kmers_updated'] for h in est.history],
             float(np.sqrt(np.mean((moved[est.updated] - true[est.updated]) ** 2))),
             float(np.sqrt(np.mean((est.mean[est.updated] - true[est.updated]) ** 2)))))
    report('re-estimated table', est.model)
    report('re-estimated, fit_start', est.model, fit_start=est.fit)


def bench():
    rb, _, _ = synthetic.make_read_batch(opts.n_reads, synthetic.load_model_arrays(), seed=7, genome_length=100000)
    bare = ReadBatch.from_signals(rb.raw_signal, rb.sig_off, np.zeros(0, np.int32), np.zeros(rb.n + 1, np.int64))
    mean, sigma = np.asarray(km.mean, dtype=np.float64), np.asarray(km.sigma, dtype=np.float64)
    scaled, ev_off, status_in, ok = decode_train.train_stages(bare, ctx, mean, 32, 2, 5.0, 0.02)
    n_events = (ev_off[1:] - ev_off[:-1]).cpu().numpy()
    tables = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (mean,) + gaussian_constants(sigma, 1.0)]
    w = transition_weights(0.7, 0.01)
    launches = []
    steps = decode_train.device_steps(ctx, scaled, ev_off, status_in, k, timer=lambda name, ms: launches.append((name, ms)))
    args = (n_events, ok.cpu().numpy(), mean, sigma, opts.rounds, opts.fit, ('scale',), ('mean',), 8.0, 0.05, 1.0, 0.7,
            0.01)
    decode_train.train_loop(*steps, *args[:4], 1, *args[5:])   # warm-up: workspaces, the allocator's blocks
    del launches[:]
    out, ms_loop = timed(lambda: decode_train.train_loop(*steps, *args))
    history = out[6]
    print('%d reads, %.0f events each on average (%d processed); k = %d, %d states'
          % (opts.n_reads, n_events.mean(), int(ok.sum()), k, 4 ** k))
    # the launches in call order: per round the fit's E-steps (fit + 1 of them), then the operator; then the closing call
    at = 0
    for r in range(opts.rounds + 1):
        if r < opts.rounds and opts.fit > 0:
            fit_ms = launches[at:at + 2 * (opts.fit + 1)]
            at += len(fit_ms)
            print('round %d  fit: %d E-steps, forward launches %9.2f ms, counts launches %9.2f ms'
                  % (r + 1, opts.fit + 1, sum(ms for name, ms in fit_ms if name == 'fit forward'),
                     sum(ms for name, ms in fit_ms if name == 'fit counts')))
        f, m, red = (ms for _, ms in launches[at:at + 3])
        at += 3
        print('%s  operator: forward launches %9.2f ms, moments launches %9.2f ms, reduce launches %7.3f ms%s'
              % ('round %d' % (r + 1) if r < opts.rounds else 'closing', f, m, red,
                 '  (%d parts, %d states updated)' % (history[r]['parts'], history[r]['kmers_updated'])
                 if r < opts.rounds else ''))
    assert at == len(launches) or opts.fit == 0
    # the slabs: the largest part's reads times 3 S doubles (parts of about equal size)
    parts = history[-1]['parts']
    per_part = -(-opts.n_reads // parts)
    print('slabs: 3 x %d doubles per read, %.1f MB for a part of %d reads; row store %.1f GB over %d parts'
          % (4 ** k, per_part * 3 * 4 ** k * 8 / 1e6, per_part, float(n_events[ok.cpu().numpy()].sum()) * 8 * 4 ** k / 1e9,
             parts))
    print('train_loop on the device, %d round(s) with fit=%d and the closing call   %9.2f ms' % (opts.rounds, opts.fit,
                                                                                                ms_loop))
    exp = kmer_expectations_dev(ctx, scaled, ev_off, k, *tables, *w, status_in, timing=True)
    post = kmer_posterior_dev(ctx, scaled, ev_off, k, km.get_central_position(), *tables, *w, status_in, timing=True)
    print('yardstick, same session: nvk_kmer_expectations_dev forward %9.2f ms, counts %9.2f ms (%d parts); '
          'nvk_kmer_posterior_dev forward %9.2f ms, backward %9.2f ms (%d parts)'
          % (exp[4][0], exp[4][1], exp[3], post[4][0], post[4][1], post[3]))
    _, ms = timed(lambda: estimate_decode_model(bare, kmer_model=km, rounds=opts.rounds, fit=opts.fit))
    print('estimate_decode_model(rounds=%d, fit=%d), the whole call                   %9.2f ms' % (opts.rounds, opts.fit, ms))


quality() if opts.quality else bench()
