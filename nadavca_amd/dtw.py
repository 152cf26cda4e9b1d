"""``nadavca_amd.dtw`` — the drop-in for the reference's pybind11 module ``nadavca.dtw``
(/root/reference/nadavca/dtw/dtwmodule.cpp:10-29), backed by HIP kernels for gfx950.

Per-read surface (same names, keywords and return shapes as the reference):
    KmerModel(k, central_position, alphabet_size, mean, sigma)
        .get_k() .get_central_position() .get_expected_signal(reference, context_before, context_after)
    refine_alignment(signal, reference, context_before, context_after, approximate_alignment,
                     bandwidth, min_event_length, kmer_model, model_transitions) -> R x 2 ints, or []
    estimate_log_likelihoods(..., model_wobbling) -> R x alphabet floats

Batched surface (what the estimator uses; one launch for many reads):
    refine_alignment_batch(reads, ...)            reads = list of per-read argument tuples
    estimate_log_likelihoods_batch(reads, ...)
    estimate_hypotheses_batch(reads, hypotheses, ...)   listed substitutions only
    estimate_joint_hypotheses_batch(reads, hypotheses, ...)   listed SETS of substitutions, each scored as a whole
    estimate_edit_hypotheses_batch(reads, edits, ...)   listed insertions / deletions (p, d, s)

All compute goes through libnadavca_hip.so; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from .batchflow import check_status
from ._lib import READ_OK, READ_NO_PATH, READ_BAD_INPUT, READ_BAD_BAND, READ_TOO_WIDE  # noqa: F401


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _i32(a):
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


class FlatBatch:
    """Host-side flat batch (layout of include/nadavca_hip.h)."""

    def __init__(self, reads):
        """reads: iterable of (signal, reference, context_before, context_after, approximate_alignment)."""
        sig, ref, cb, ca, anc = [], [], [], [], []
        for s, r, b, a, al in reads:
            sig.append(_f64(s))
            ref.append(_i32(r))
            cb.append(_i32(b))
            ca.append(_i32(a))
            al = _i32(al)
            if al.size % 2:
                raise ValueError('approximate_alignment must have shape (A, 2)')
            anc.append(al)
        self.n = len(sig)
        cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False) if xs else np.zeros(0, dtype=dt)
        self.signal = cat(sig, np.float64)
        self.reference = cat(ref, np.int32)
        self.context_before = cat(cb, np.int32)
        self.context_after = cat(ca, np.int32)
        self.anchors = cat(anc, np.int32)
        self.sig_off = _offsets([x.size for x in sig])
        self.ref_off = _offsets([x.size for x in ref])
        self.cb_off = _offsets([x.size for x in cb])
        self.ca_off = _offsets([x.size for x in ca])
        self.anc_off = _offsets([x.size // 2 for x in anc])

    @classmethod
    def from_arrays(cls, signal, sig_off, reference, ref_off, context_before, cb_off, context_after,
                    ca_off, anchors, anc_off):
        self = cls.__new__(cls)
        self.n = len(sig_off) - 1
        self.signal = _f64(signal)
        self.reference = _i32(reference)
        self.context_before = _i32(context_before)
        self.context_after = _i32(context_after)
        self.anchors = _i32(anchors)
        for name, v in (('sig_off', sig_off), ('ref_off', ref_off), ('cb_off', cb_off),
                        ('ca_off', ca_off), ('anc_off', anc_off)):
            setattr(self, name, np.ascontiguousarray(v, dtype=np.int64))
        return self

    def pointers(self):
        return [_ptr(self.signal), _ptr(self.sig_off), _ptr(self.reference), _ptr(self.ref_off),
                _ptr(self.context_before), _ptr(self.cb_off), _ptr(self.context_after), _ptr(self.ca_off),
                _ptr(self.anchors), _ptr(self.anc_off)]


class KmerModel:
    """Device-resident k-mer table (reference: dtw.KmerModel, kmer_model.cpp:6-14)."""

    def __init__(self, k, central_position, alphabet_size, mean, sigma, context=None):
        self._lib = _lib.load()
        self.context = context or _lib.default_context()
        mean, sigma = _f64(mean), _f64(sigma)
        if mean.size != sigma.size:
            raise ValueError('mean and sigma differ in length')
        self.k, self.central_position, self.alphabet_size = int(k), int(central_position), int(alphabet_size)
        h = C.c_void_p()
        _lib.check(self._lib.nvk_model_create(self.context.handle, self.k, self.central_position,
                                              self.alphabet_size, _ptr(mean), _ptr(sigma), mean.size,
                                              C.byref(h)), 'nvk_model_create')
        self.handle = h
        self.mean, self.sigma = mean, sigma

    def get_k(self):
        return self.k

    def get_central_position(self):
        return self.central_position

    def get_alphabet_size(self):
        return self.alphabet_size

    def get_expected_signal(self, reference, context_before, context_after):
        out = self.get_expected_signal_batch([(reference, context_before, context_after)])
        return out[0]

    def get_expected_signal_batch(self, items):
        """items: list of (reference, context_before, context_after) -> list of f64 arrays."""
        ref = [_i32(r) for r, _, _ in items]
        cb = [_i32(b) for _, b, _ in items]
        ca = [_i32(a) for _, _, a in items]
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int32)
        r, b, a = cat(ref), cat(cb), cat(ca)
        for name, v in (('reference', r), ('context_before', b), ('context_after', a)):
            if v.size and (int(v.min()) < 0 or int(v.max()) >= self.alphabet_size):
                raise ValueError('get_expected_signal: %s holds a base code outside 0..%d'
                                 % (name, self.alphabet_size - 1))
        ro, bo, ao = _offsets([x.size for x in ref]), _offsets([x.size for x in cb]), _offsets([x.size for x in ca])
        out = np.zeros(r.size, dtype=np.float64)
        _lib.check(self._lib.nvk_expected_signal_batch(self.handle, len(items), _ptr(r), _ptr(ro), _ptr(b),
                                                       _ptr(bo), _ptr(a), _ptr(ao), _ptr(out)),
                   'nvk_expected_signal_batch')
        return [out[ro[i]:ro[i + 1]] for i in range(len(items))]

    @staticmethod
    def load_from_npz(filename, context=None):
        z = np.load(filename)
        return KmerModel(int(z['k']), int(z['central_pos']), int(z['alphabet_size']), z['mean'], z['sigma'],
                         context=context)

    def close(self):
        if getattr(self, 'handle', None):
            self._lib.nvk_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# batched operators
# ------------------------------------------------------------------------------------------------
def refine_alignment_flat(batch, bandwidth, min_event_length, kmer_model, model_transitions, on_error='raise'):
    """-> (events int32 (sum R, 2), status int32 (n,)) for a FlatBatch.  on_error='status': per-read
    failures (status < 0) are left to the caller instead of raised."""
    lib = _lib.load()
    events = np.zeros((int(batch.ref_off[-1]), 2), dtype=np.int32)
    status = np.zeros(batch.n, dtype=np.int32)
    _lib.check(lib.nvk_refine_alignment_batch(kmer_model.handle, batch.n, *batch.pointers(), int(bandwidth),
                                              int(min_event_length), int(bool(model_transitions)),
                                              _ptr(events), _ptr(status)), 'nvk_refine_alignment_batch')
    if on_error == 'raise':
        check_status('refine_alignment', status)
    return events, status


class RefineStream:
    """``refine_alignment`` over a stream of FlatBatches with the PCIe copies behind the kernels
    (nvk_refine_alignment_submit / _wait, include/nadavca_hip.h): ``submit`` uploads a batch and returns at once
    while the previous batch's kernels still run, ``wait`` hands back (events, status, tie flags) of a ticket.
    Keep at most a few batches in flight (one lane each; the library has three)."""

    def __init__(self, kmer_model, bandwidth, min_event_length, model_transitions):
        self._lib = _lib.load()
        self.kmer_model = kmer_model
        self.args = (int(bandwidth), int(min_event_length), int(bool(model_transitions)))
        self._pending = {}

    def submit(self, batch, out=None):
        """``out``: (events int32 (sum R, 2), status int32 (n,), tie flags int32 (n,)) arrays to reuse — fresh
        arrays are page-faulted in while the results arrive, which shows in a tight loop."""
        if out is None:
            out = (np.zeros((int(batch.ref_off[-1]), 2), dtype=np.int32), np.zeros(batch.n, dtype=np.int32),
                   np.zeros(batch.n, dtype=np.int32))
        events, status, ties = out
        assert events.size == 2 * int(batch.ref_off[-1]) and status.size == batch.n and ties.size == batch.n
        t = C.c_int64(-1)
        _lib.check(self._lib.nvk_refine_alignment_submit(self.kmer_model.handle, batch.n, *batch.pointers(),
                                                         *self.args, _ptr(events), _ptr(status), _ptr(ties),
                                                         C.byref(t)), 'nvk_refine_alignment_submit')
        self._pending[t.value] = (batch, events, status, ties)   # (keeps the host arrays alive until wait)
        return t.value

    def wait(self, ticket):
        batch, events, status, ties = self._pending.pop(ticket)
        _lib.check(self._lib.nvk_refine_alignment_wait(self.kmer_model.handle, int(ticket)),
                   'nvk_refine_alignment_wait')
        return events, status, ties


def estimate_log_likelihoods_flat(batch, bandwidth, min_event_length, kmer_model, model_wobbling,
                                  on_error='raise'):
    """-> (ll f64 (sum R, alphabet), status int32 (n,)) for a FlatBatch."""
    lib = _lib.load()
    alpha = kmer_model.alphabet_size
    ll = np.zeros((int(batch.ref_off[-1]), alpha), dtype=np.float64)
    status = np.zeros(batch.n, dtype=np.int32)
    _lib.check(lib.nvk_estimate_log_likelihoods_batch(kmer_model.handle, batch.n, *batch.pointers(),
                                                      int(bandwidth), int(min_event_length),
                                                      int(bool(model_wobbling)), _ptr(ll), _ptr(status)),
               'nvk_estimate_log_likelihoods_batch')
    if on_error == 'raise':
        check_status('estimate_log_likelihoods', status)
    return ll, status


def refine_alignment_batch(reads, bandwidth, min_event_length, kmer_model, model_transitions,
                           on_error='raise', return_status=False):
    """reads: list of (signal, reference, context_before, context_after, approximate_alignment).
    -> list of (R, 2) int arrays; an empty (0, 2) array where the band holds no valid path (and, with
    on_error='status', where the read was refused: return_status=True also returns the status array)."""
    batch = reads if isinstance(reads, FlatBatch) else FlatBatch(reads)
    events, status = refine_alignment_flat(batch, bandwidth, min_event_length, kmer_model, model_transitions,
                                           on_error=on_error)
    out = []
    for j in range(batch.n):
        if status[j] == READ_OK:
            out.append(events[batch.ref_off[j]:batch.ref_off[j + 1]])
        else:
            out.append(np.zeros((0, 2), dtype=np.int32))
    return (out, status) if return_status else out


def estimate_log_likelihoods_batch(reads, bandwidth, min_event_length, kmer_model, model_wobbling):
    batch = reads if isinstance(reads, FlatBatch) else FlatBatch(reads)
    ll, _ = estimate_log_likelihoods_flat(batch, bandwidth, min_event_length, kmer_model, model_wobbling)
    return [ll[batch.ref_off[j]:batch.ref_off[j + 1]] for j in range(batch.n)]


def _listed_hypotheses(what, dev_fn, batch, off, lists, unfit, params, on_error, return_status):
    """What ``<what>_batch`` does once its Python lists are flat.  ``off``: the reads' offsets into the hypotheses;
    ``lists``: what ``dev_fn`` (the operator in nadavca_amd/device.py) takes behind ``hyp_off``, as (int64 array, dtype)
    pairs — np.int64: offsets, passed as they are; np.int32: values, which must fit 32 bits (ValueError naming
    ``unfit``); ``params``: (bandwidth, min_event_length, kmer_model, model_wobbling).
    -> (total, list of the reads' slices of hyp[, status])."""
    if batch.n == 0:
        out = (np.zeros(0), [])
        return out + (np.zeros(0, dtype=np.int32),) if return_status else out
    for a, dtype in lists:
        if dtype == np.int32 and a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
            raise ValueError('%s_batch: %s does not fit 32 bits' % (what, unfit))
    import torch
    from .device import DeviceBatch
    dbatch = DeviceBatch(batch, torch.device('cuda', params[2].context.device))
    total, hyp, status = dev_fn(dbatch, *params, torch.from_numpy(off),
                                *[torch.from_numpy(a.astype(dtype, copy=False)) for a, dtype in lists])
    total, hyp, status = total.cpu().numpy(), hyp.cpu().numpy(), status.cpu().numpy()
    if on_error == 'raise':
        check_status(what, status)
    out = (total, [hyp[off[j]:off[j + 1]] for j in range(batch.n)])
    return out + (status,) if return_status else out


def estimate_hypotheses_batch(reads, hypotheses, bandwidth, min_event_length, kmer_model, model_wobbling,
                              on_error='raise', return_status=False):
    """``estimate_log_likelihoods_batch`` for a list of substitutions per read instead of the whole matrix.  reads:
    as there (or a FlatBatch); hypotheses: per read an (m, 2) integer array of (position, substituted base) rows, in
    any order, duplicates allowed, possibly empty.  -> (total f64 (n,), list of f64 (m,) arrays): ``total[j]`` the
    read's log-likelihood without a substitution, entry h of read j the value ``[p, b]`` of its full matrix (the
    hypotheses that are not listed are never run; nvk_estimate_hypotheses_batch_dev).  A position or base out of
    range fails its read (READ_BAD_INPUT: ValueError, or with on_error='status' NaN values and, with
    return_status=True, the status array as a third result)."""
    from .device import estimate_hypotheses_dev
    batch = reads if isinstance(reads, FlatBatch) else FlatBatch(reads)
    if len(hypotheses) != batch.n:
        raise ValueError('estimate_hypotheses_batch: %d hypothesis lists for %d reads' % (len(hypotheses), batch.n))
    hyps = [np.asarray(h, dtype=np.int64).reshape(-1, 2) for h in hypotheses]
    flat = np.concatenate(hyps + [np.zeros((0, 2), dtype=np.int64)])
    return _listed_hypotheses('estimate_hypotheses', estimate_hypotheses_dev, batch,
                              _offsets([h.shape[0] for h in hyps]), [(flat[:, 0], np.int32), (flat[:, 1], np.int32)],
                              'a position or base', (bandwidth, min_event_length, kmer_model, model_wobbling),
                              on_error, return_status)


def estimate_joint_hypotheses_batch(reads, hypotheses, bandwidth, min_event_length, kmer_model, model_wobbling,
                                    on_error='raise', return_status=False):
    """``estimate_hypotheses_batch`` for hypotheses that hold several substitutions.  hypotheses: per read a list of
    (m, 2) integer arrays of (position, substituted base) rows with strictly ascending positions, m >= 0 (no row: the
    read's total), in any order, duplicates allowed.  -> (total f64 (n,), list of f64 (number of hypotheses,) arrays):
    entry h of read j is its log-likelihood with ALL of h's substitutions applied: the rows the first to the last of
    them influence are re-run once and closed as a single substitution's are (nvk_estimate_joint_hypotheses_batch_dev;
    rows with b == reference[p] change nothing).  A position or base out of range, positions that do not ascend or a
    hypothesis that re-runs more than 14 rows fails its read (READ_BAD_INPUT: ValueError, or with on_error='status'
    NaN values and, with return_status=True, the status array as a third result)."""
    from .device import estimate_joint_hypotheses_dev
    batch = reads if isinstance(reads, FlatBatch) else FlatBatch(reads)
    if len(hypotheses) != batch.n:
        raise ValueError('estimate_joint_hypotheses_batch: %d hypothesis lists for %d reads'
                         % (len(hypotheses), batch.n))
    hyps = [[np.asarray(h, dtype=np.int64).reshape(-1, 2) for h in hs] for hs in hypotheses]
    sub_off = _offsets([h.shape[0] for hs in hyps for h in hs])
    flat = np.concatenate([h for hs in hyps for h in hs] + [np.zeros((0, 2), dtype=np.int64)])
    return _listed_hypotheses('estimate_joint_hypotheses', estimate_joint_hypotheses_dev, batch,
                              _offsets([len(hs) for hs in hyps]),
                              [(sub_off, np.int64), (flat[:, 0], np.int32), (flat[:, 1], np.int32)],
                              'a position or base', (bandwidth, min_event_length, kmer_model, model_wobbling),
                              on_error, return_status)


def estimate_edit_hypotheses_batch(reads, edits, bandwidth, min_event_length, kmer_model, model_wobbling,
                                   on_error='raise', return_status=False):
    """``estimate_hypotheses_batch`` for insertions and deletions.  edits: per read a list of ``(p, d, s)``: delete
    ``reference[p .. p+d)`` and put the letters ``s`` (a sequence of base codes, possibly empty) in its place; any
    order, duplicates allowed.  -> (total f64 (n,), list of f64 (number of edits,) arrays): entry h of read j is its
    log-likelihood under the edited reference, the total ``estimate_log_likelihoods`` has for it — with the band of
    the edited reference mapped from the read's own, not recomputed, and ``(p, 0, ())`` the read's total
    (nvk_estimate_edit_hypotheses_batch_dev).  An edit without a base of the read on either side (p < 1 or
    p + d > R - 1), d outside 0 .. 255, a letter out of range or an edit that re-runs more than 14 rows fails its read
    (READ_BAD_INPUT: ValueError, or with on_error='status' NaN values and, with return_status=True, the status array
    as a third result)."""
    from .device import estimate_edit_hypotheses_dev
    batch = reads if isinstance(reads, FlatBatch) else FlatBatch(reads)
    if len(edits) != batch.n:
        raise ValueError('estimate_edit_hypotheses_batch: %d edit lists for %d reads' % (len(edits), batch.n))
    flat = [e for es in edits for e in es]
    letters = [np.asarray(s, dtype=np.int64).reshape(-1) for _, _, s in flat]
    pd = np.array([[p, d] for p, d, _ in flat], dtype=np.int64).reshape(-1, 2)
    ins = np.concatenate(letters + [np.zeros(0, dtype=np.int64)])
    return _listed_hypotheses('estimate_edit_hypotheses', estimate_edit_hypotheses_dev, batch,
                              _offsets([len(es) for es in edits]),
                              [(pd[:, 0], np.int32), (pd[:, 1], np.int32),
                               (_offsets([s.size for s in letters]), np.int64), (ins, np.int32)],
                              'a position, length or letter',
                              (bandwidth, min_event_length, kmer_model, model_wobbling), on_error, return_status)


# ------------------------------------------------------------------------------------------------
# per-read operators (reference signatures)
# ------------------------------------------------------------------------------------------------
def refine_alignment(signal, reference, context_before, context_after, approximate_alignment, bandwidth,
                     min_event_length, kmer_model, model_transitions):
    return refine_alignment_batch([(signal, reference, context_before, context_after, approximate_alignment)],
                                  bandwidth, min_event_length, kmer_model, model_transitions)[0]


def estimate_log_likelihoods(signal, reference, context_before, context_after, approximate_alignment,
                             bandwidth, min_event_length, kmer_model, model_wobbling):
    return estimate_log_likelihoods_batch(
        [(signal, reference, context_before, context_after, approximate_alignment)],
        bandwidth, min_event_length, kmer_model, model_wobbling)[0]
