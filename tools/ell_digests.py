#!/usr/bin/env python3
"""SHA-256 digests of what the log-likelihood kernels write, for comparing two builds bit for bit.

usage: ell_digests.py [--root REPOSITORY]     (default: the repository this script lies in)

Runs, with model wobbling off and on, the 40 cases of tests/variant_cases.ell_cases (one per built ell_kernel), its
ell_too_wide_case and one batch of 64 reads of bench.py's cfg3_snps shape at min event length 2, and prints one line
per run: the case, a digest of the output arrays — the matrix, or the totals and the hypotheses' values — and of the
per-read status.  A refactor of csrc/kernels_ell.hip moves no floating-point operation, so the listing of the tree
before and after it are equal line for line; run both on one machine in one session (the `log` of another toolchain may
differ in the last bit, which is why no listing is kept in the repository).  --root runs another checkout's package
and cases with this script.
"""
import argparse
import hashlib
import os
import sys

import numpy as np


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    import torch
    import variant_cases as vc
    from nadavca_amd import dtw, synthetic, _lib
    from nadavca_amd.device import DeviceBatch, estimate_log_likelihoods_dev

    ctx = _lib.default_context()
    device = torch.device('cuda', ctx.device)
    models = {}

    def model_of(arrays):
        if id(arrays) not in models:
            models[id(arrays)] = (dtw.KmerModel(*arrays, context=ctx), arrays)
        return models[id(arrays)][0]

    def full(name, batch, bw, mel, mg, w):
        ll, st = estimate_log_likelihoods_dev(DeviceBatch(batch, device), bw, mel, mg, w)
        print('%-22s w%d  ll %s  status %s' % (name, w, digest(ll.cpu().numpy()), digest(st.cpu().numpy())), flush=True)

    for case in vc.ell_cases() + [vc.ell_too_wide_case()]:
        mg = model_of(case['model'])
        k, central, alphabet = case['model'][:3]
        bw, mel, kind, reads = case['bandwidth'], case['mel'], case['kind'], case['reads']
        tup = vc.reads_of(reads)
        refs = [np.asarray(r['reference']) for r in reads]
        for w in (False, True):
            if kind == 'full':
                full(case['name'], dtw.FlatBatch(tup), bw, mel, mg, w)
                continue
            if kind == 'listed':
                lists = [np.stack([np.repeat(np.arange(r.size), alphabet), np.tile(np.arange(alphabet), r.size)], 1)
                         for r in refs]                          # every (p, b), b == ref[p] included
                lists[0] = lists[0][::-1]
                lists[3] = lists[3][:0]
                run = dtw.estimate_hypotheses_batch
            elif kind == 'joint':
                lists = [vc.joint_list(r, k, central, alphabet, case['lanes']) for r in refs]
                lists.append(lists[-1] + [vc.joint_one_row_more(refs[-1], k, central, alphabet)])
                run = dtw.estimate_joint_hypotheses_batch
            else:
                lists = [vc.edit_list(r, c['approximate_alignment'], k, central, alphabet, case['lanes'])
                         for r, c in zip(refs, reads)]
                lists.append(lists[-1] + [vc.edit_one_row_more(refs[-1], k, central, alphabet)])
                run = dtw.estimate_edit_hypotheses_batch
            # (joint, edit: the last read once more with a hypothesis of one row too many, which refuses it)
            total, got, st = run(tup + [tup[-1]] * (len(lists) - len(tup)), lists, bw, mel, mg, w, on_error='status',
                                 return_status=True)
            hyp = np.concatenate([np.asarray(g, dtype=np.float64).reshape(-1) for g in got] + [np.zeros(0)])
            print('%-22s w%d  total %s  hyp %s  status %s' % (case['name'], w, digest(np.asarray(total)), digest(hyp),
                                                              digest(np.asarray(st))), flush=True)

    wl = dict(synthetic.WORKLOADS['cfg3_snps'])
    wl.pop('n_reads', None)
    wl.pop('reference_length', None)
    model = synthetic.load_model_arrays()
    batch = synthetic.make_batch(64, model, seed=1000, **wl)
    for w in (False, True):
        full('cfg3_64_reads', batch, wl['bandwidth'], 2, model_of(model), w)


if __name__ == '__main__':
    main()
