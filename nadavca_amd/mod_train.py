"""Train the modified-base k-mer levels from reads: ``estimate_mod_model``.

``call_mods_batch`` needs a table whose k-mers with the modified base (code 4, ``M``) carry real levels.  This module
estimates them from a ReadBatch of a sample that is modified wholly (``labels='all'``, an M.SssI-style control) or in
part (``labels='em'``, a native sample), by EM around the existing alignment:

* align the batch with the current table against the CANONICAL reference (``align_batch``, unchanged).  The reference
  is never rewritten with ``M``: event borders next to a modified base come from canonical levels.  That is a limit of
  this trainer, not of the table it writes;
* E-step: per read and per occurrence of the pattern, gamma = the probability that the read carries ``M`` there.
  ``'all'``: 1.  ``'em'``: the site ratios of ``call_mods_batch``'s own code path (``call_mods.score_sites``) and
  gamma = sigmoid(llr + log(pi / (1 - pi))), in f64 on the device;
* M-step: every event whose k-mer window holds 1 .. 4 sites is counted under each non-empty subset of them, with the
  subset's probability as its weight, into the k-mer that subset spells (include/nadavca_hip.h: nvk_mod_kmer_rows_dev
  has the contract; two kernels, a stable sort and a gather between them).  ``update_mod_levels`` turns the sums into
  levels;
* with ``fit_fraction``, pi becomes the mean gamma.

Only k-mers that hold ``mod_code`` are ever written; every other entry of the table keeps its bits.
"""
import math

import numpy as np

from . import defaults, _lib
from .kmer_train import _check_kmer_args, save_kmer_model_npz


def holds_code(k, alphabet, code):
    """bool (alphabet^k,): the k-mer ids with ``code`` at one place or more."""
    ids = np.arange(int(alphabet) ** int(k), dtype=np.int64)
    has = np.zeros(ids.size, dtype=bool)
    for m in range(int(k)):
        has |= (ids // int(alphabet) ** m) % int(alphabet) == int(code)
    return has


def update_mod_levels(mean, sigma, key, sums, k, alphabet, mod_code, min_weight, min_sigma):
    """The update rule of ``estimate_mod_model``, plain numpy.  ``mean`` / ``sigma``: the current table (alphabet^k);
    ``key`` int64 (n,): distinct k-mer ids; ``sums`` f64 (n, 4): their W, Nw, Sd, Sq as nvk_mod_kmer_reduce_dev writes
    them (Sd, Sq: weighted sums of the samples' deviations from ``mean[key]`` and of their squares).  A k-mer that
    holds ``mod_code`` and has W >= ``min_weight`` gets
        mean  = mean[key] + Sd / Nw
        sigma = max(sqrt(max(Sq / Nw - (Sd / Nw)^2, 0)), min_sigma)
    (Nw > 0 is asked too; the kernel's rows have n >= 1, so W > 0 implies it) and every other entry keeps its bits.
    -> (mean, sigma, updated bool, weight f64, samples f64), all alphabet^k; weight and samples are W and Nw laid out
    densely (0 where a k-mer has no row)."""
    mean = np.array(mean, dtype=np.float64).reshape(-1)
    sigma = np.array(sigma, dtype=np.float64).reshape(-1)
    n_kmers = int(alphabet) ** int(k)
    if mean.size != n_kmers or sigma.size != n_kmers:
        raise ValueError('mean / sigma hold %d / %d values, the table %d' % (mean.size, sigma.size, n_kmers))
    key = np.asarray(key, dtype=np.int64).reshape(-1)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 4)
    if sums.shape[0] != key.size or (key.size and (key.min() < 0 or key.max() >= n_kmers)) or \
            np.unique(key).size != key.size:
        raise ValueError('update_mod_levels: keys must be distinct ids of the table, one row of sums each')
    if not (min_weight > 0 and np.isfinite(min_sigma) and min_sigma > 0):
        raise ValueError('update_mod_levels: min_weight and min_sigma must be > 0')
    weight, samples = np.zeros(n_kmers), np.zeros(n_kmers)
    weight[key], samples[key] = sums[:, 0], sums[:, 1]
    sel = holds_code(k, alphabet, mod_code)[key] & (sums[:, 0] >= float(min_weight)) & (sums[:, 1] > 0)
    at = key[sel]
    shift = sums[sel, 2] / sums[sel, 1]
    var = np.maximum(sums[sel, 3] / sums[sel, 1] - shift * shift, 0.0)
    updated = np.zeros(n_kmers, dtype=bool)
    updated[at] = True
    mean[at] = mean[at] + shift
    sigma[at] = np.maximum(np.sqrt(var), float(min_sigma))
    return mean, sigma, updated, weight, samples


class ModModelEstimate:
    """What ``estimate_mod_model`` returns.  ``model``: the final KmerModel; ``k``, ``central``, ``alphabet``; numpy
    arrays of the final table (``mean``, ``sigma``) and of the last round, dense over the table: ``weight`` (W, the sum
    of the weights of a k-mer's rows), ``samples`` (Nw, its weighted sample count) and ``updated`` (the k-mers that
    round wrote); ``fraction``: the share of modified sites the next round would assume; ``gamma``: the last round's
    per-site probabilities, in the row order of ``call_mods_batch``; ``history``: per round a dict of ``reads`` (in the
    batch), ``aligned`` (with an approximate alignment), ``status_ok`` (status 0 after the alignment), ``sites``
    (scored), ``fraction`` (after the round), ``rows`` (of the statistics), ``windows_skipped`` (bases with more than
    4 sites in their window), ``kmers_updated`` and ``rms_mean_change`` (over the updated k-mers)."""

    def __init__(self, model, k, central, alphabet, mean, sigma, weight, samples, updated, fraction, gamma, history):
        self.model, self.k, self.central, self.alphabet = model, k, central, alphabet
        self.mean, self.sigma, self.weight, self.samples, self.updated = mean, sigma, weight, samples, updated
        self.fraction, self.gamma, self.history = fraction, gamma, history

    def save(self, path):
        """The table as ``.npz`` in the packaged layout (save_kmer_model_npz)."""
        save_kmer_model_npz(path, self.k, self.central, self.alphabet, self.mean, self.sigma)


def site_gammas(res, config, kmer_model, codes, mod_offset, mod_code, labels, fraction, joint, max_joint):
    """The E-step on the BatchAlignment ``res`` (``res.stage.n_live > 0``).  -> (site_off int64 (n_live + 1,), pos
    int32, gamma f64): the scored sites per live read and their probabilities, device tensors, in the row order of
    ``call_mods_batch``."""
    import torch
    from .call_mods import find_sites, score_sites
    from .readbatch import contig_local_range
    stage = res.stage
    if labels == 'all':
        sa, dbatch = stage.sa, stage.dbatch
        start, end = contig_local_range(sa, stage.reference)
        site_off, _, pos, _, _ = find_sites(dbatch.reference, dbatch.ref_off, start, end, sa.reverse, codes, mod_offset,
                                            kmer_model.get_k(), keep=res.status == _lib.READ_OK,
                                            total_ref=dbatch.total_ref)
        return site_off, pos, torch.ones(int(pos.numel()), dtype=torch.float64, device=pos.device)
    sc = score_sites(res, config, kmer_model, codes, mod_offset, mod_code, joint, max_joint, fraction)
    owner, pos, llr = sc.owner[sc.ok], sc.pos[sc.ok], sc.llr[sc.ok]
    site_off = torch.zeros(stage.n_live + 1, dtype=torch.int64, device=pos.device)
    torch.cumsum(torch.bincount(owner, minlength=stage.n_live), 0, out=site_off[1:])
    gamma = torch.sigmoid(llr + math.log(fraction / (1.0 - fraction)))
    return site_off, pos.contiguous(), gamma


def estimate_mod_model(read_batch, aligner, kmer_model, pattern='CG', mod_offset=0, mod_code=4, labels='em', rounds=4,
                       fraction=0.5, fit_fraction=True, joint=True, max_joint=4, min_weight=10.0, min_sigma=0.05,
                       trim=5, config=defaults.CONFIG_FILE, renorm_rounds=defaults.RENORM_ROUNDS):
    """Estimate the levels of the k-mers that hold ``mod_code`` from ``read_batch`` (a ReadBatch) and ``aligner`` (the
    batch-aligner contract of ``align_signal_batch``; one over a ``ReferenceSet`` works as it is, the table being
    global).  ``kmer_model``: a KmerModel (or a file) whose alphabet holds ``mod_code`` — a 4-letter table is refused
    as ``call_mods_batch`` refuses it; ``kmer_train.extend_kmer_model(k, central, mean, sigma)`` without levels
    (M = C) is the usual start.  Each of ``rounds`` rounds aligns, takes gamma per occurrence of ``pattern`` in the
    reads with status 0 (``labels`` 'all': 1, a wholly modified sample, no likelihood call; 'em': from the site ratios
    of ``call_mods_batch(joint=joint, max_joint=max_joint, site_prior=fraction)`` and the prior ``fraction``), takes
    the weighted statistics over the final events and the finally rescaled signal (bases within ``trim`` of either end
    of a read's aligned part are not counted) and updates every k-mer holding ``mod_code`` whose weight reaches
    ``min_weight`` (``update_mod_levels``).  With ``fit_fraction`` and 'em', ``fraction`` becomes the mean gamma,
    clipped to [1e-3, 1 - 1e-3], for the next round.  ``rounds=n`` equals n chained ``rounds=1`` calls, each seeded with
    the previous ``model`` and ``fraction``, bit for bit.  -> ModModelEstimate."""
    from .batchflow import align_batch, load_config, load_kmer_model
    from .detect_meth import pattern_codes
    from .device import mod_kmer_stats_dev
    from .kmer_model import KmerModel
    for name, v, lo in (('rounds', rounds, 1), ('renorm_rounds', renorm_rounds, 0), ('trim', trim, 0)):
        if isinstance(v, bool) or int(v) != v or v < lo:
            raise ValueError('estimate_mod_model: %s must be an integer >= %d, not %r' % (name, lo, v))
    if labels not in ('all', 'em'):
        raise ValueError("estimate_mod_model: labels must be 'all' or 'em', not %r" % (labels,))
    if not (np.isfinite(min_weight) and min_weight > 0):
        raise ValueError('estimate_mod_model: min_weight must be a finite number > 0, not %r' % (min_weight,))
    if not (np.isfinite(min_sigma) and min_sigma > 0):
        raise ValueError('estimate_mod_model: min_sigma must be a finite number > 0, not %r' % (min_sigma,))
    if not 0.0 < float(fraction) < 1.0:
        raise ValueError('estimate_mod_model: fraction %r outside the open interval (0, 1)' % (fraction,))
    if int(max_joint) != max_joint or not 1 <= max_joint <= 8:
        raise ValueError('estimate_mod_model: max_joint %r outside 1 .. 8' % (max_joint,))
    config, kmer_model = load_config(config), load_kmer_model(kmer_model)
    k, central, alphabet = _check_kmer_args(kmer_model.get_k(), kmer_model.get_central_position(),
                                            kmer_model.get_alphabet_size())
    if int(mod_code) != mod_code or not 4 <= mod_code < alphabet:
        raise ValueError('call_mods_batch: the k-mer table has %d letters and no modified base with code %r '
                         '(kmer_train.extend_kmer_model makes a 5-letter table from a canonical one)'
                         % (alphabet, mod_code))
    codes = pattern_codes(pattern)
    if not 0 <= int(mod_offset) < len(codes):
        raise ValueError('estimate_mod_model: mod_offset %r outside the pattern %r' % (mod_offset, pattern))
    import torch
    context = kmer_model.context
    mean = np.array(kmer_model.mean, dtype=np.float64).reshape(-1)
    sigma = np.array(kmer_model.sigma, dtype=np.float64).reshape(-1)
    n_kmers = alphabet ** k
    if mean.size != n_kmers:
        raise ValueError('the table holds %d k-mers, alphabet^k is %d' % (mean.size, n_kmers))
    current, fraction = kmer_model, float(fraction)
    history = []
    for _ in range(int(rounds)):
        res = align_batch(read_batch, config, current, int(renorm_rounds), aligner)
        aligned = res.stage.n_live
        key, sums = np.zeros(0, dtype=np.int64), np.zeros((0, 4))
        gamma = np.zeros(0)
        status_ok = rows = skipped = 0
        if aligned:
            status_ok = int((res.status == _lib.READ_OK).sum())
            site_off, pos, g = site_gammas(res, config, current, codes, mod_offset, mod_code, labels, fraction, joint,
                                           max_joint)
            stats = mod_kmer_stats_dev(context, res.stage.dbatch, res.events, res.status, k, central, alphabet,
                                       int(trim), site_off, pos, g, int(mod_code),
                                       torch.from_numpy(mean).to(res.stage.dbatch.device))
            key, sums = stats['key'].cpu().numpy(), stats['sums'].cpu().numpy()
            rows, skipped = stats['rows'], stats['windows_skipped']
            if fit_fraction and labels == 'em' and int(g.numel()):
                fraction = min(max(float(g.mean()), 1e-3), 1.0 - 1e-3)
            gamma = g.cpu().numpy()
        new_mean, new_sigma, updated, weight, samples = update_mod_levels(mean, sigma, key, sums, k, alphabet, mod_code,
                                                                          min_weight, min_sigma)
        change = float(np.sqrt(np.mean((new_mean[updated] - mean[updated]) ** 2))) if updated.any() else 0.0
        history.append(dict(reads=int(read_batch.n), aligned=aligned, status_ok=status_ok, sites=int(gamma.size),
                            fraction=fraction, rows=rows, windows_skipped=skipped, kmers_updated=int(updated.sum()),
                            rms_mean_change=change))
        mean, sigma = new_mean, new_sigma
        current = KmerModel(k, central, alphabet, mean, sigma, context=context)
    return ModModelEstimate(current, k, central, alphabet, mean, sigma, weight, samples, updated, fraction, gamma,
                            history)
