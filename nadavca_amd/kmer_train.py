"""Re-estimate the k-mer table from aligned reads: ``estimate_kmer_model``.

Every score of the engine rests on the table's ``mean[A^k]`` and ``sigma[A^k]``, in the units the kernels read
(samples normalised by median/MAD, then linearly re-fitted by the renorm loop).  This module produces a table in those
units from a ReadBatch and a batch aligner, by hard EM: align the batch with the current table (``align_batch``, the
device half of ``align_signal_batch``, unchanged), take per-k-mer sample statistics over the final events and the
finally rescaled signal, update the k-mers seen often enough, and align again.

The statistics (the M-step) are two device passes, exact and deterministic; their contract is in
include/nadavca_hip.h (nvk_kmer_event_stats_dev):

* pass 1: per counted event the ``np.sum`` of its samples and its length; per k-mer S (``np.sum`` of its events'
  sums in batch order), N (samples), e (events); ``m = S / N``;
* pass 2: per counted event the ``np.sum`` of its squared deviations from ``m`` of its k-mer; per k-mer Q;
  ``sigma = sqrt(Q / N)``.

The stable sort of the event keys and the gather of the values into that order are torch's; every floating-point sum
is a kernel's, in numpy's order.
"""
import os

import numpy as np

from . import defaults

MAX_K = 12   # largest k estimate_kmer_model / expand_kmer_model serve (a 4^12 table: 16.7 M k-mers)


def _check_kmer_args(k, central, alphabet, max_k=MAX_K):
    if int(k) != k or int(central) != central or int(alphabet) != alphabet:
        raise ValueError('k, central and alphabet must be integers')
    k, central, alphabet = int(k), int(central), int(alphabet)
    if not 1 <= k <= max_k:
        raise ValueError('k = %d outside 1..%d' % (k, max_k))
    if not 0 <= central < k:
        raise ValueError('central = %d outside 0..k-1 (k = %d)' % (central, k))
    if not 1 <= alphabet <= 64 or alphabet ** k > (1 << 31):
        raise ValueError('alphabet = %d with k = %d: the table must hold at most 2^31 k-mers' % (alphabet, k))
    return k, central, alphabet


def kmer_stats_dev(context, dbatch, events, status, k, central, alphabet, trim=5, level=None):
    """Per-k-mer statistics of the counted events of ``dbatch`` (a device.DeviceBatch; ``events`` and ``status`` as
    ``refine_alignment_dev`` returns them) over ``dbatch.signal``.  Without ``level``: pass 1, -> (S f64, N int64,
    e int64) device tensors of alphabet^k entries (0 where nothing was counted).  With ``level`` (alphabet^k means,
    numpy or tensor): pass 2, -> (Q f64, N, e), Q the sums of squared deviations from ``level``."""
    import torch
    from .device import kmer_event_stats_dev, kmer_reduce_dev
    k, central, alphabet = _check_kmer_args(k, central, alphabet, max_k=31)
    if int(trim) != trim or trim < 0:
        raise ValueError('trim must be an integer >= 0')
    n_kmers = alphabet ** k
    dev = dbatch.device
    if level is not None:
        level = torch.as_tensor(level, dtype=torch.float64).to(dev).reshape(-1).contiguous()
        if int(level.numel()) != n_kmers:
            raise ValueError('level holds %d values, the table %d' % (int(level.numel()), n_kmers))
    key, val, length = kmer_event_stats_dev(dbatch, context, events, status, k, central, alphabet, int(trim), level)
    key, order = torch.sort(key, stable=True)
    return kmer_reduce_dev(context, key, val[order], length[order], n_kmers)


def save_kmer_model_npz(path, k, central, alphabet, mean, sigma):
    """Write a table in the packaged layout (default/kmer_model.npz): int64 scalars ``k``, ``central_pos``,
    ``alphabet_size`` and float64 ``mean`` / ``sigma`` of alphabet^k entries.  ``KmerModel.load_from_hdf5`` reads
    it back; it picks that branch by the suffix, so ``path`` must end in ``.npz``."""
    if not str(os.fspath(path)).endswith('.npz'):
        raise ValueError('save_kmer_model_npz: %r does not end in .npz (KmerModel.load_from_hdf5 would read it as '
                         'HDF5)' % (path,))
    k, central, alphabet = _check_kmer_args(k, central, alphabet, max_k=31)
    mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
    sigma = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
    if mean.size != alphabet ** k or sigma.size != alphabet ** k:
        raise ValueError('mean / sigma hold %d / %d values, the table %d' % (mean.size, sigma.size, alphabet ** k))
    np.savez(path, k=np.int64(k), central_pos=np.int64(central), alphabet_size=np.int64(alphabet), mean=mean,
             sigma=sigma)


def expand_kmer_model(k0, central0, alphabet, mean0, sigma0, k, central):
    """A k-mer table from a k0-mer one: every k-mer takes the values of the k0-mer embedded in it at offset
    ``central - central0`` (its central base on the k0-mer's).  Needs ``central >= central0`` and
    ``k - central >= k0 - central0``.  -> (mean, sigma) float64 arrays of alphabet^k entries."""
    k0, central0, alphabet = _check_kmer_args(k0, central0, alphabet)
    k, central, _ = _check_kmer_args(k, central, alphabet)
    off = central - central0
    if off < 0 or k - central < k0 - central0:
        raise ValueError('a %d-mer with central %d cannot hold the %d-mer with central %d at its centre'
                         % (k, central, k0, central0))
    mean0 = np.asarray(mean0, dtype=np.float64).reshape(-1)
    sigma0 = np.asarray(sigma0, dtype=np.float64).reshape(-1)
    if mean0.size != alphabet ** k0 or sigma0.size != alphabet ** k0:
        raise ValueError('mean0 / sigma0 hold %d / %d values, the table %d' % (mean0.size, sigma0.size,
                                                                              alphabet ** k0))
    ids = np.arange(alphabet ** k, dtype=np.int64)
    sub = (ids // alphabet ** (k - off - k0)) % alphabet ** k0
    return mean0[sub], sigma0[sub]


def extend_kmer_model(k, central, mean, sigma, base=1, levels=None):
    """The 4-letter table ``mean`` / ``sigma`` (4^k entries) laid out as a 5-letter one (id = sum b_m * 5^(k-1-m), the
    indexing of ``synthetic.kmer_ids`` with alphabet 5): a k-mer over codes 0..3 keeps its values, a k-mer containing
    code 4 (the modified base) takes those of the k-mer with ``base`` (default 1: C) in place of every 4.  ``levels``:
    known levels that override, ``{id5: (mean, sigma)}`` or a tuple of arrays ``(ids5, means, sigmas)``.
    -> (mean5, sigma5) float64 arrays of 5^k entries — the table ``call_mods_batch`` takes (``save_kmer_model_npz``
    writes it)."""
    k, central, _ = _check_kmer_args(k, central, 5)
    if int(base) != base or not 0 <= base <= 3:
        raise ValueError('base = %r outside 0..3' % (base,))
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if mean.size != 4 ** k or sigma.size != 4 ** k:
        raise ValueError('mean / sigma hold %d / %d values, the 4-letter table %d' % (mean.size, sigma.size, 4 ** k))
    ids = np.arange(5 ** k, dtype=np.int64)
    id4 = np.zeros_like(ids)
    for m in range(k):
        d = (ids // 5 ** (k - 1 - m)) % 5
        id4 = id4 * 4 + np.where(d == 4, int(base), d)
    mean5, sigma5 = mean[id4], sigma[id4]
    if levels is not None:
        if isinstance(levels, dict):
            at = np.array(list(levels.keys()), dtype=np.int64)
            vals = np.array([levels[i] for i in levels], dtype=np.float64).reshape(-1, 2)
            lm, ls = vals[:, 0], vals[:, 1]
        else:
            at, lm, ls = (np.asarray(x).reshape(-1) for x in levels)
            at = at.astype(np.int64)
        if at.size and (at.min() < 0 or at.max() >= 5 ** k):
            raise ValueError('levels: a k-mer id outside 0..%d' % (5 ** k - 1))
        if lm.size != at.size or ls.size != at.size:
            raise ValueError('levels: ids, means and sigmas differ in length')
        mean5[at], sigma5[at] = lm, ls
    return mean5, sigma5


class KmerModelEstimate:
    """What ``estimate_kmer_model`` returns.  ``model``: the final KmerModel; numpy arrays of the final table
    (``mean``, ``sigma``) and of the last round (``events``, ``samples``: counted per k-mer; ``updated``: the k-mers
    that round replaced); ``history``: per round a dict of ``reads`` (in the batch), ``aligned`` (with an approximate
    alignment), ``status_ok`` (status 0 after the alignment), ``events`` (counted), ``kmers_updated`` and
    ``rms_mean_change`` (over the updated k-mers)."""

    def __init__(self, model, k, central, alphabet, mean, sigma, events, samples, updated, history):
        self.model, self.k, self.central, self.alphabet = model, k, central, alphabet
        self.mean, self.sigma, self.events, self.samples, self.updated = mean, sigma, events, samples, updated
        self.history = history

    def save(self, path):
        """The table as ``.npz`` in the packaged layout (save_kmer_model_npz)."""
        save_kmer_model_npz(path, self.k, self.central, self.alphabet, self.mean, self.sigma)


def estimate_kmer_model(read_batch, aligner, kmer_model=defaults.KMER_MODEL_FILE, config=defaults.CONFIG_FILE,
                        rounds=2, renorm_rounds=defaults.RENORM_ROUNDS, min_events=10, min_sigma=0.05, trim=5):
    """Re-estimate ``kmer_model`` (a KmerModel or a file for ``KmerModel.load_from_hdf5``) from ``read_batch`` (a
    ReadBatch) and ``aligner`` (the batch-aligner contract of ``align_signal_batch``).  Each of ``rounds`` rounds runs
    ``align_signal_batch``'s device half with the current table, takes both statistics passes over the signal after
    the last rescale with the final events and status, then gives every k-mer with at least ``min_events`` counted
    events ``mean = m`` and ``sigma = max(sigma, min_sigma)``; every other k-mer keeps its values bit for bit.  Bases
    within ``trim`` of either end of a read's aligned part are not counted.  -> KmerModelEstimate."""
    from .batchflow import align_batch, load_config, load_kmer_model
    from .kmer_model import KmerModel
    for name, v, lo in (('rounds', rounds, 1), ('renorm_rounds', renorm_rounds, 0), ('min_events', min_events, 1),
                        ('trim', trim, 0)):
        if isinstance(v, bool) or int(v) != v or v < lo:
            raise ValueError('%s must be an integer >= %d, not %r' % (name, lo, v))
    if not (np.isfinite(min_sigma) and min_sigma > 0):
        raise ValueError('min_sigma must be a finite number > 0, not %r' % (min_sigma,))
    config, kmer_model = load_config(config), load_kmer_model(kmer_model)
    k, central, alphabet = _check_kmer_args(kmer_model.get_k(), kmer_model.get_central_position(),
                                            kmer_model.get_alphabet_size())
    context = kmer_model.context
    mean = np.array(kmer_model.mean, dtype=np.float64)
    sigma = np.array(kmer_model.sigma, dtype=np.float64)
    if mean.size != alphabet ** k:
        raise ValueError('the table holds %d k-mers, alphabet^k is %d' % (mean.size, alphabet ** k))
    current = kmer_model
    history = []
    n_kmers = alphabet ** k
    for _ in range(int(rounds)):
        res = align_batch(read_batch, config, current, int(renorm_rounds), aligner)
        aligned = res.stage.n_live
        stats = lambda level=None: kmer_stats_dev(context, res.stage.dbatch, res.events, res.status, k, central,
                                                  alphabet, trim, level)
        if aligned == 0:
            S, N, e = np.zeros(n_kmers), np.zeros(n_kmers, dtype=np.int64), np.zeros(n_kmers, dtype=np.int64)
            status_ok = 0
        else:
            status_ok = int((res.status == 0).sum())
            S, N, e = (t.cpu().numpy() for t in stats())
        seen = N > 0
        m = np.zeros(n_kmers)
        m[seen] = S[seen] / N[seen]
        Q = stats(m)[0].cpu().numpy() if aligned else np.zeros(n_kmers)
        updated = e >= int(min_events)
        new_mean, new_sigma = mean.copy(), sigma.copy()
        new_mean[updated] = m[updated]
        new_sigma[updated] = np.maximum(np.sqrt(Q[updated] / N[updated]), float(min_sigma))
        change = float(np.sqrt(np.mean((new_mean[updated] - mean[updated]) ** 2))) if updated.any() else 0.0
        history.append(dict(reads=int(read_batch.n), aligned=aligned, status_ok=status_ok, events=int(e.sum()),
                            kmers_updated=int(updated.sum()), rms_mean_change=change))
        mean, sigma = new_mean, new_sigma
        current = KmerModel(k, central, alphabet, mean, sigma, context=context)
    return KmerModelEstimate(current, k, central, alphabet, mean, sigma, e, N, updated, history)
