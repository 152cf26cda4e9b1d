"""detect_meth per read against detect_meth_batch on N synthetic reads (pattern CG by default), with
align_signal_batch on the same reads as the yardstick of the alignment the two share.  Wall time, time in the
library's kernels (ctx.timing_read: all kernels, and the meth kernels on their own) and reads/s; the batch form's
CSV writing is timed on its own.  The per-read detect_meth writes its CSV inside its loop, so its figure includes
the writing.  `python tools/bench_meth.py [N] [pattern] [--skip-per-read]`."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nadavca_amd import synthetic, defaults, _lib  # noqa: E402
from nadavca_amd.alignment import ApproximateAligner  # noqa: E402
from nadavca_amd.align_signal import align_signal_batch  # noqa: E402
from nadavca_amd.detect_meth import detect_meth, detect_meth_batch  # noqa: E402
from nadavca_amd.kmer_model import KmerModel  # noqa: E402
from nadavca_amd.readbatch import ReadBatch, BaseAlignmentBatch, SyntheticBatchAligner  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
n_reads = int(args[0]) if args else 2000
pattern = args[1] if len(args) > 1 else 'CG'
per_read = '--skip-per-read' not in sys.argv

km = KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)
model = synthetic.load_model_arrays()
seed = 7
genome = np.random.default_rng(seed).integers(0, 4, 10000).astype(np.int32)
t0 = time.perf_counter()
specs = [synthetic.make_read_spec(np.random.default_rng([seed, i]), genome, model, i) for i in range(n_reads)]
for s in specs:   # int16 ADC counts, as fast5 files hold them (the same samples for both forms)
    s['raw_signal'] = np.rint(s['raw_signal']).astype(np.int16)
reads = synthetic.reads_from_specs(specs)
rb = ReadBatch.from_reads(reads)
bms = [np.asarray(s['base_mapping'], dtype=np.int64).reshape(-1, 2) for s in specs]
ba = BaseAlignmentBatch(np.concatenate([b[:, 0] for b in bms]), np.concatenate([b[:, 1] for b in bms]),
                        np.concatenate([[0], np.cumsum([len(b) for b in bms])]), [s['reverse'] for s in specs])
batch_aligner = SyntheticBatchAligner(genome, ba)
read_aligner = synthetic.make_synthetic_aligner(ApproximateAligner, np.array(list('ACGT'))[genome])
print('built %d reads (%.0f samples, %.0f bases each on average) in %.1f s' % (
    n_reads, rb.sig_off[-1] / n_reads, rb.seq_off[-1] / n_reads, time.perf_counter() - t0))
ctx = km.context
tmp = tempfile.mkdtemp()


def timed(name, fn):
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    t = time.perf_counter()
    out = fn()
    ctx.synchronize()
    dt = time.perf_counter() - t
    ctx.timing_enable(False)
    timing = ctx.timing_read()
    kern = sum(ms for ms, _ in timing.values())
    print('%-34s %9.1f ms wall, %7.1f ms in kernels (meth %.2f ms), %9.0f reads/s' % (
        name, dt * 1e3, kern, timing['meth'][0], n_reads / dt))
    return out


# warm-up: workspaces, first touch, the model's tables
warm = ReadBatch.from_reads(reads[:64])
detect_meth_batch(None, warm, pattern, kmer_model=km,
                  aligner=SyntheticBatchAligner(genome, BaseAlignmentBatch(
                      ba.read_idx[:ba.off[64]], ba.ref_idx[:ba.off[64]], ba.off[:65], ba.reverse[:64])))

for rep in range(2):
    timed('align_signal_batch', lambda: align_signal_batch(None, rb, kmer_model=km, aligner=batch_aligner))
    mb = timed('detect_meth_batch (no CSV)', lambda: detect_meth_batch(None, rb, pattern, kmer_model=km,
                                                                       aligner=batch_aligner))
    path = os.path.join(tmp, 'batch.csv')
    t = time.perf_counter()
    mb.write_csv(path)
    dt = time.perf_counter() - t
    print('%-34s %9.1f ms wall, %d rows' % ('MethBatch.write_csv', dt * 1e3, len(mb)))
if per_read:
    path = os.path.join(tmp, 'per_read.csv')
    timed('detect_meth (per read, with CSV)', lambda: detect_meth(None, reads, pattern, path, kmer_model=km,
                                                                  aligner=read_aligner))
    with open(path) as f:
        print('%-34s %d rows' % ('detect_meth CSV', sum(1 for _ in f) - 1))
