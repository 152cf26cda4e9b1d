"""Device-resident batches: torch tensors used purely as HBM buffers for the ``*_dev`` entry
points of the C-ABI (inputs already in HBM when the call starts; see include/nadavca_hip.h)."""
import ctypes as C

import numpy as np

from . import _lib


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _one(t):
    """``t``, or a placeholder element where it is empty: the C-ABI takes no NULL for a batch that has reads"""
    import torch
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def _opt(t, n):
    """The pointer of an optional per-read array: NULL for None and for a batch without reads"""
    return _dp(t) if t is not None and n > 0 else C.c_void_p(0)


def to_host(t):
    """A device tensor as a numpy array through page-locked host memory (torch keeps a cache of such blocks, so a
    caller that drops the previous batch's result gets the block back: no page faults on fresh memory, the copy at
    PCIe speed).  Meant for the large results of the batch workflows (96 MB of rows per 10 000 reads); small ones
    go ``.cpu()``."""
    import torch
    if t.numel() < (1 << 18):
        return t.cpu().numpy()
    try:
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    except RuntimeError:
        return t.cpu().numpy()
    h.copy_(t)
    return h.numpy()


class DeviceBatch:
    """A flat batch (nadavca_amd.dtw.FlatBatch / synthetic.Batch layout) copied to one GPU.

    ``plan_token`` names the batch's geometry to the library (include/nadavca_hip.h: plan once, sweep again): the
    first ``refine_alignment_dev`` of the batch plans it, later ones with the same settings sweep from that plan for
    as long as the context holds it.  ``signal`` may be rewritten or replaced between calls; see
    ``geometry_changed``."""

    GEOMETRY = ('sig_off', 'reference', 'ref_off', 'context_before', 'cb_off', 'context_after', 'ca_off', 'anchors',
                'anc_off', 'n', 'total_signal', 'total_ref', 'total_anchors')

    def __setattr__(self, name, value):
        object.__setattr__(self, name, value)
        if name in self.GEOMETRY and 'plan_token' in self.__dict__:   # (a geometry field replaced after construction)
            self.geometry_changed()

    def geometry_changed(self):
        """Take a new plan token: the next ``refine_alignment_dev`` plans again.  To be called after the VALUES of a
        geometry field were changed in place — ``sig_off``, ``reference``, ``ref_off``, ``context_before``,
        ``cb_off``, ``context_after``, ``ca_off``, ``anchors``, ``anc_off`` (the planner reads all of them; the counts
        ``n`` and ``total_*`` follow from the offsets).  Assigning a new tensor to one of these attributes does it by
        itself; ``signal`` is no geometry."""
        object.__setattr__(self, 'plan_token', _lib.plan_token_new())

    def __init__(self, batch, device):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.n = int(batch.n)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.signal = up(batch.signal, np.float64)
        self.sig_off = up(batch.sig_off, np.int64)
        self.reference = up(batch.reference, np.int32)
        self.ref_off = up(batch.ref_off, np.int64)
        self.context_before = up(batch.context_before, np.int32)
        self.cb_off = up(batch.cb_off, np.int64)
        self.context_after = up(batch.context_after, np.int32)
        self.ca_off = up(batch.ca_off, np.int64)
        self.anchors = up(batch.anchors, np.int32)
        self.anc_off = up(batch.anc_off, np.int64)
        self.total_signal = int(batch.sig_off[-1])
        self.total_ref = int(batch.ref_off[-1])
        self.total_anchors = int(batch.anc_off[-1])
        self.geometry_changed()
        torch.cuda.synchronize(self.device)

    @classmethod
    def from_windows(cls, signal_dev, sa, device):
        """The DP inputs of ``readbatch.signal_alignments()`` (a SignalAlignmentBatch of tensors on ``device``)
        with every read's signal window gathered ON THE DEVICE out of ``signal_dev`` (the normalised signals of
        all reads end to end, f64 device tensor): no per-read array crosses PCIe."""
        import torch
        self = cls.__new__(cls)
        self.torch = torch
        self.device = torch.device(device)
        dev = self.device
        self.n = int(sa.live.numel())
        win_len = sa.win_len.to(dev)
        sig_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(win_len, 0)])
        self.sig_off = sig_off
        self.total_signal = int(sig_off[-1])
        # source index of every window sample: its position in the batch + (window start - batch offset)
        idx = torch.repeat_interleave(sa.win_start.to(dev) - sig_off[:-1], win_len, output_size=self.total_signal)
        idx += torch.arange(self.total_signal, dtype=torch.int64, device=dev)
        self.signal = signal_dev[idx]
        del idx
        nz = lambda t, m: t.to(dev).contiguous() if t.numel() else torch.zeros(m, dtype=t.dtype, device=dev)
        self.reference = nz(sa.reference, 1)
        self.ref_off = sa.ref_off.to(dev).contiguous()
        self.context_before = nz(sa.context_before, 1)
        self.cb_off = sa.cb_off.to(dev).contiguous()
        self.context_after = nz(sa.context_after, 1)
        self.ca_off = sa.ca_off.to(dev).contiguous()
        self.anchors = nz(sa.anchors.reshape(-1), 2)
        self.anc_off = sa.anc_off.to(dev).contiguous()
        self.total_ref = int(sa.ref_off[-1])
        self.total_anchors = int(sa.anc_off[-1])
        self.geometry_changed()
        return self

    def pointers(self):
        return [_dp(self.signal), _dp(self.sig_off), _dp(self.reference), _dp(self.ref_off),
                _dp(self.context_before), _dp(self.cb_off), _dp(self.context_after), _dp(self.ca_off),
                _dp(self.anchors), _dp(self.anc_off)]

    def algorithmic_bytes_align(self, band_cells):
        """B_align summed over the batch: 20*C + 8*N + 8*A + 4*(R+ctx) + 24*R."""
        ctx = int(self.context_before.numel() + self.context_after.numel())
        return (20 * int(band_cells) + 8 * self.total_signal + 8 * self.total_anchors
                + 4 * (self.total_ref + ctx) + 24 * self.total_ref)

    def algorithmic_bytes_snp(self, band_cells):
        """B_snp: 32*C' + 8*N + 8*A + 4*(R+ctx) + 32*R."""
        ctx = int(self.context_before.numel() + self.context_after.numel())
        return (32 * int(band_cells) + 8 * self.total_signal + 8 * self.total_anchors
                + 4 * (self.total_ref + ctx) + 32 * self.total_ref)


def refine_alignment_dev(dbatch, bandwidth, min_event_length, kmer_model, model_transitions,
                         events=None, status=None):
    """Device in, device out: -> (events int32 (sum R, 2), status int32 (n,)) torch tensors.  The batch's plan token
    goes with the call, so a batch aligned again with the same settings is not planned again (DeviceBatch)."""
    torch = dbatch.torch
    lib = _lib.load()
    if events is None:
        events = torch.zeros((dbatch.total_ref, 2), dtype=torch.int32, device=dbatch.device)
    if status is None:
        status = torch.zeros(dbatch.n, dtype=torch.int32, device=dbatch.device)
    _lib.check(lib.nvk_refine_alignment_batch_dev_keyed(
        kmer_model.handle, dbatch.n, dbatch.total_signal, dbatch.total_ref, dbatch.total_anchors,
        *dbatch.pointers(), int(bandwidth), int(min_event_length), int(bool(model_transitions)),
        _dp(events), _dp(status), getattr(dbatch, 'plan_token', 0)), 'nvk_refine_alignment_batch_dev_keyed')
    return events, status


def estimate_log_likelihoods_dev(dbatch, bandwidth, min_event_length, kmer_model, model_wobbling,
                                 ll=None, status=None):
    torch = dbatch.torch
    lib = _lib.load()
    if ll is None:
        ll = torch.zeros((dbatch.total_ref, kmer_model.alphabet_size), dtype=torch.float64, device=dbatch.device)
    if status is None:
        status = torch.zeros(dbatch.n, dtype=torch.int32, device=dbatch.device)
    _lib.check(lib.nvk_estimate_log_likelihoods_batch_dev(
        kmer_model.handle, dbatch.n, dbatch.total_signal, dbatch.total_ref, dbatch.total_anchors,
        *dbatch.pointers(), int(bandwidth), int(min_event_length), int(bool(model_wobbling)),
        _dp(ll), _dp(status)), 'nvk_estimate_log_likelihoods_batch_dev')
    return ll, status


def _listed_hypotheses_dev(name, dbatch, bandwidth, min_event_length, kmer_model, model_wobbling, n_hyp, hyp_off,
                           lists):
    """The C-ABI call ``name`` of a listed-hypothesis operator.  ``lists``: what it takes between ``hyp_off`` and
    ``out_total``, in that order: an int (a second level's total) as it is, a (tensor, dtype) pair as a contiguous
    tensor of that dtype on the batch's device.  -> (total f64 (n,), hyp f64 (n_hyp,), status int32 (n,)), the values
    NaN wherever the kernel writes none."""
    torch = dbatch.torch
    lib = _lib.load()
    dev = dbatch.device

    def coerce(t, dtype):
        t = t.to(device=dev, dtype=dtype).contiguous()
        # (a placeholder element: the C-ABI's pointers of an empty list are never read)
        return t if t.numel() else torch.zeros(1, dtype=dtype, device=dev)
    lists = [x if isinstance(x, int) else coerce(*x) for x in [(hyp_off, torch.int64)] + list(lists)]
    total = torch.full((dbatch.n,), float('nan'), dtype=torch.float64, device=dev)
    hyp = torch.full((n_hyp,), float('nan'), dtype=torch.float64, device=dev)
    status = torch.zeros(dbatch.n, dtype=torch.int32, device=dev)
    _lib.check(getattr(lib, name)(
        kmer_model.handle, dbatch.n, dbatch.total_signal, dbatch.total_ref, dbatch.total_anchors,
        *dbatch.pointers(), int(bandwidth), int(min_event_length), int(bool(model_wobbling)),
        n_hyp, *[x if isinstance(x, int) else _dp(x) for x in lists], _dp(total), _dp(hyp if n_hyp else total),
        _dp(status)), name)
    return total, hyp, status


def estimate_hypotheses_dev(dbatch, bandwidth, min_event_length, kmer_model, model_wobbling, hyp_off, hyp_pos,
                            hyp_base):
    """``estimate_log_likelihoods_dev`` for a LIST of substitutions: read j's hypotheses are entries
    ``hyp_off[j] .. hyp_off[j+1]`` (int64 (n+1,)) of ``hyp_pos`` / ``hyp_base`` (int32: position in the read's
    reference part, substituted base) — device tensors.  -> (total f64 (n,), hyp f64 (n_hyp,), status int32 (n,)):
    ``hyp[h]`` is the entry ``[p, b]`` of the read's full matrix, ``total[j]`` the read's log-likelihood without a
    substitution.  The unlisted hypotheses are never run; a read with a position or base out of range gets
    READ_BAD_INPUT (include/nadavca_hip.h: nvk_estimate_hypotheses_batch_dev).  Values of reads with a negative
    status are NaN."""
    n_hyp = int(hyp_pos.numel())
    if int(hyp_base.numel()) != n_hyp or int(hyp_off.numel()) != dbatch.n + 1:
        raise ValueError('estimate_hypotheses_dev: hyp_pos and hyp_base go together, hyp_off has one entry per read '
                         'and one more')
    i32 = dbatch.torch.int32
    return _listed_hypotheses_dev('nvk_estimate_hypotheses_batch_dev', dbatch, bandwidth, min_event_length, kmer_model,
                                  model_wobbling, n_hyp, hyp_off, [(hyp_pos, i32), (hyp_base, i32)])


def estimate_joint_hypotheses_dev(dbatch, bandwidth, min_event_length, kmer_model, model_wobbling, hyp_off, sub_off,
                                  sub_pos, sub_base):
    """``estimate_hypotheses_dev`` for hypotheses of SEVERAL substitutions: read j's hypotheses are
    ``hyp_off[j] .. hyp_off[j+1]`` (int64 (n+1,)), hypothesis h's substitutions the entries ``sub_off[h] ..
    sub_off[h+1]`` (int64 (n_hyp+1,)) of ``sub_pos`` / ``sub_base`` (int32, positions strictly ascending within a
    hypothesis) — device tensors.  -> (total f64 (n,), hyp f64 (n_hyp,), status int32 (n,)): ``hyp[h]`` is the read's
    log-likelihood with all of h's substitutions applied (rows first .. last of the first and last one re-run and
    closed as one substitution is; a hypothesis without an effective substitution gives ``total``).  A read with a
    position or base out of range, positions that do not ascend or a hypothesis that re-runs more than 14 rows gets
    READ_BAD_INPUT (include/nadavca_hip.h: nvk_estimate_joint_hypotheses_batch_dev).  Values of reads with a negative
    status are NaN."""
    n_hyp, n_sub = int(sub_off.numel()) - 1, int(sub_pos.numel())
    if int(sub_base.numel()) != n_sub or int(hyp_off.numel()) != dbatch.n + 1 or n_hyp < 0:
        raise ValueError('estimate_joint_hypotheses_dev: sub_pos and sub_base go together, hyp_off has one entry per '
                         'read and one more, sub_off one per hypothesis and one more')
    i32, i64 = dbatch.torch.int32, dbatch.torch.int64
    return _listed_hypotheses_dev('nvk_estimate_joint_hypotheses_batch_dev', dbatch, bandwidth, min_event_length,
                                  kmer_model, model_wobbling, n_hyp, hyp_off,
                                  [n_sub, (sub_off, i64), (sub_pos, i32), (sub_base, i32)])


def estimate_edit_hypotheses_dev(dbatch, bandwidth, min_event_length, kmer_model, model_wobbling, hyp_off, edit_pos,
                                 edit_del, ins_off, ins_base):
    """``estimate_hypotheses_dev`` for insertions and deletions: read j's hypotheses are ``hyp_off[j] .. hyp_off[j+1]``
    (int64 (n+1,)); hypothesis h deletes ``edit_del[h]`` bases of the read's reference part from ``edit_pos[h]`` on
    and puts the letters ``ins_off[h] .. ins_off[h+1]`` (int64 (n_hyp+1,)) of ``ins_base`` in their place (int32) —
    device tensors.  -> (total f64 (n,), hyp f64 (n_hyp,), status int32 (n,)): ``hyp[h]`` is the read's
    log-likelihood under the edited part (its rows around the edit re-run with k-mers and bands read through the
    edit's index map, closed on band last + 1; no deletion and no letter gives ``total``).  A read with an edit that
    leaves no base in front of it (p < 1) or behind it (p + d > R - 1), a negative d or one above 255, a letter out of
    range or a re-run of more than 14 rows gets READ_BAD_INPUT (include/nadavca_hip.h:
    nvk_estimate_edit_hypotheses_batch_dev).  Values of reads with a negative status are NaN."""
    n_hyp, n_ins = int(edit_pos.numel()), int(ins_base.numel())
    if int(edit_del.numel()) != n_hyp or int(ins_off.numel()) != n_hyp + 1 or int(hyp_off.numel()) != dbatch.n + 1:
        raise ValueError('estimate_edit_hypotheses_dev: edit_pos and edit_del go together, hyp_off has one entry per '
                         'read and one more, ins_off one per hypothesis and one more')
    i32, i64 = dbatch.torch.int32, dbatch.torch.int64
    return _listed_hypotheses_dev('nvk_estimate_edit_hypotheses_batch_dev', dbatch, bandwidth, min_event_length,
                                  kmer_model, model_wobbling, n_hyp, hyp_off,
                                  [(edit_pos, i32), (edit_del, i32), n_ins, (ins_off, i64), (ins_base, i32)])


# ---- host steps adjacent to the path, on the device (include/nadavca_hip.h) --------
def normalize_groups_dev(context, raw, grp_off, out=None):
    """``Read.normalize_reads`` for groups of samples laid end to end (torch f64 / int64 tensors on the
    context's device): -> (normalised signal, (n_groups, 2) tensor of (centre, scale))."""
    import torch
    lib = _lib.load()
    n_groups = int(grp_off.numel()) - 1
    if out is None:
        out = torch.empty_like(raw)
    cs = torch.zeros((max(n_groups, 0), 2), dtype=torch.float64, device=raw.device)
    _lib.check(lib.nvk_normalize_groups_dev(context.handle, n_groups, _dp(raw), _dp(grp_off), _dp(out),
                                            _dp(cs)), 'nvk_normalize_groups_dev')
    return out, cs


def select_hist_dev(context, x):
    """-> local_hist(mode, centre, prefix, pass) over a device tensor of samples, for distributed.pooled_median:
    256 counts per call (int64 cuda tensor, ready for the all-reduce), nvk_select_hist_dev."""
    import torch
    lib = _lib.load()

    def local_hist(mode, centre, prefix, p):
        h = torch.zeros(256, dtype=torch.int64, device=x.device)
        _lib.check(lib.nvk_select_hist_dev(context.handle, _dp(x), int(x.numel()), int(mode), float(centre),
                                           C.c_uint64(int(prefix)), int(p), _dp(h)), 'nvk_select_hist_dev')
        return h
    return local_hist


def normalize_apply_dev(context, x, centre, scale, out=None):
    """clip((x - centre) / scale, -5, 5) on the device (read.py:80-81 with a given shift and scale)."""
    import torch
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.nvk_normalize_apply_dev(context.handle, _dp(x), int(x.numel()), float(centre), float(scale),
                                           _dp(out)), 'nvk_normalize_apply_dev')
    return out


def expected_levels_dev(dbatch, kmer_model, with_contexts=True):
    """``KmerModel.get_expected_signal`` for every read of the batch -> f64 (sum R,).  Without contexts
    the k-mers at the ends are padded with base 0, as ``get_expected_signal(bases, [], [])`` does
    (align_signal.py:63)."""
    torch = dbatch.torch
    lib = _lib.load()
    out = torch.zeros(dbatch.total_ref, dtype=torch.float64, device=dbatch.device)
    if with_contexts:
        cb, cbo, ca, cao = dbatch.context_before, dbatch.cb_off, dbatch.context_after, dbatch.ca_off
    else:
        cb = ca = torch.zeros(1, dtype=torch.int32, device=dbatch.device)
        cbo = cao = torch.zeros(dbatch.n + 1, dtype=torch.int64, device=dbatch.device)
    _lib.check(lib.nvk_expected_signal_batch_dev(
        kmer_model.handle, dbatch.n, dbatch.total_ref, _dp(dbatch.reference), _dp(dbatch.ref_off),
        _dp(cb), _dp(cbo), _dp(ca), _dp(cao), _dp(out)), 'nvk_expected_signal_batch_dev')
    return out


def event_means_dev(dbatch, context, events, status=None):
    """Mean of the batch's signal over every event of ``events`` (as returned by
    ``refine_alignment_dev``) -> f64 (sum R,); equals ``numpy.mean`` of the same samples bit for bit."""
    torch = dbatch.torch
    lib = _lib.load()
    out = torch.zeros(dbatch.total_ref, dtype=torch.float64, device=dbatch.device)
    _lib.check(lib.nvk_event_means_dev(
        context.handle, dbatch.n, dbatch.total_ref, _dp(dbatch.signal), _dp(dbatch.sig_off), _dp(events),
        _dp(dbatch.ref_off), _opt(status, dbatch.n), _dp(out)),
        'nvk_event_means_dev')
    return out


def linfit_rescale_dev(dbatch, context, expected, means, status=None):
    """Per read: least-squares line of ``means`` on ``expected`` and ``signal = (signal - intercept) /
    slope`` in place on the batch's signal -> (n, 2) tensor of (slope, intercept)."""
    torch = dbatch.torch
    lib = _lib.load()
    fit = torch.zeros((dbatch.n, 2), dtype=torch.float64, device=dbatch.device)
    _lib.check(lib.nvk_linfit_rescale_dev(
        context.handle, dbatch.n, _dp(expected), _dp(means), _dp(dbatch.ref_off),
        _opt(status, dbatch.n), _dp(dbatch.signal), _dp(dbatch.sig_off),
        _dp(fit)), 'nvk_linfit_rescale_dev')
    return fit


def spline_fit_dev(context, means, expected, ref_off, status=None):
    """The fit of ``Read.tweak_signal_normalization`` (read.py:83-93: keep |expected - mean| <= 1, sort,
    ``splrep(..., s=len)``) for every read on the device.  means / expected: f64 device tensors, read j at
    [ref_off[j], ref_off[j+1]); status: int32 per read or None (reads with status != 0 are not fitted).
    -> (t (n, 8), c (n, 8), fit int32 (n,)): fit 0 = fitted (coefficients equal scipy's), 1 = fewer than 4 usable
    events, 2 = outside the polynomial case (include/nadavca_hip.h: nvk_spline_fit_dev)."""
    import torch
    lib = _lib.load()
    n = int(ref_off.numel()) - 1
    t = torch.empty((n, 8), dtype=torch.float64, device=means.device)
    c = torch.empty((n, 8), dtype=torch.float64, device=means.device)
    fit = torch.empty(n, dtype=torch.int32, device=means.device)
    _lib.check(lib.nvk_spline_fit_dev(
        context.handle, n, int(means.numel()), _dp(means), _dp(expected), _dp(ref_off),
        _opt(status, n), _dp(t), _dp(c), _dp(fit)), 'nvk_spline_fit_dev')
    return t, c, fit


def splev_groups_dev(context, x, grp_off, t, c, knot_off, degree, out=None):
    """``scipy.interpolate.splev`` for groups of samples laid end to end, one spline (its knots ``t`` and
    coefficients ``c`` between ``knot_off[g]`` and ``knot_off[g+1]``) per group -> values (torch f64)."""
    import torch
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.nvk_splev_groups_dev(context.handle, int(grp_off.numel()) - 1, _dp(x), _dp(grp_off), _dp(t),
                                        _dp(c), _dp(knot_off), int(degree), _dp(out)), 'nvk_splev_groups_dev')
    return out


def refine_renorm_loop_dev(dbatch, bandwidth, min_event_length, kmer_model, model_transitions,
                           renorm_rounds):
    """The renormalise / re-align loop of ``align_signal`` (align_signal.py:55-80) for a whole batch
    without leaving the device: align; then for round r = 0 .. renorm_rounds-1: even r — per-event
    means, linear re-fit against the model's expected levels (empty contexts), rescale the signal;
    odd r — align again.  -> (events, status, [fit tensors of the even rounds]).  ``dbatch.signal`` is
    rescaled in place."""
    context = kmer_model.context
    events, status = refine_alignment_dev(dbatch, bandwidth, min_event_length, kmer_model, model_transitions)
    expected, fits = None, []
    for r in range(int(renorm_rounds)):
        if r % 2 == 0:
            if expected is None:
                expected = expected_levels_dev(dbatch, kmer_model, with_contexts=False)
            means = event_means_dev(dbatch, context, events, status)
            fits.append(linfit_rescale_dev(dbatch, context, expected, means, status))
        else:
            # a read that lost its path stays lost (the reference raises on it at this point)
            new_events, new_status = refine_alignment_dev(dbatch, bandwidth, min_event_length, kmer_model,
                                                          model_transitions)
            keep = status != 0
            new_status[keep] = status[keep]
            events, status = new_events, new_status
    return events, status, fits


def meth_scores_dev(context, reference, ref_off, means, expected, status, pattern):
    """``calculate_meth_scores`` + ``maxs3`` (detect_meth.py:21-65) for every read of a batch, on the device:
    the scorable occurrences of ``pattern`` (base codes, a sequence or a tensor; a code outside 0..3 never
    matches) in the reference parts ``reference`` / ``ref_off`` (int32 / int64 device tensors), scored from the
    per-base event ``means`` (``event_means_dev``: NaN = empty event) and ``expected`` levels (f64 device tensors,
    one value per base); ``status``: int32 per read or None.  Count, prefix sum, emit (include/nadavca_hip.h:
    nvk_meth_count_dev / nvk_meth_scores_dev).
    -> (occ_off int64 (n+1,), position int64 (n_occ,), scores f64 (n_occ, 11), aggregate f64 (n_occ,)) device
    tensors; read j's occurrences are [occ_off[j], occ_off[j+1]), in ascending position."""
    import torch
    lib = _lib.load()
    dev = means.device
    n = int(ref_off.numel()) - 1
    total_ref = int(means.numel())   # (``reference`` may hold a placeholder element when it is empty)
    if isinstance(pattern, torch.Tensor):
        pat = pattern.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    else:
        pat = torch.from_numpy(np.asarray(pattern, dtype=np.int32).reshape(-1)).to(dev)
    m = int(pat.numel())
    if m == 0:
        pat = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _opt(status, n)
    count = torch.zeros(max(n, 0), dtype=torch.int64, device=dev)
    _lib.check(lib.nvk_meth_count_dev(context.handle, n, total_ref, _dp(reference), _dp(ref_off), _dp(means), st,
                                      _dp(pat), m, _dp(count)), 'nvk_meth_count_dev')
    occ_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=occ_off[1:])
    n_occ = int(occ_off[-1])
    pos = torch.empty(n_occ, dtype=torch.int64, device=dev)
    scores = torch.empty((n_occ, 11), dtype=torch.float64, device=dev)
    agg = torch.empty(n_occ, dtype=torch.float64, device=dev)
    if n_occ:
        _lib.check(lib.nvk_meth_scores_dev(context.handle, n, total_ref, _dp(reference), _dp(ref_off), _dp(means),
                                           _dp(expected), st, _dp(pat), m, _dp(occ_off), _dp(pos), _dp(scores),
                                           _dp(agg)), 'nvk_meth_scores_dev')
    return occ_off, pos, scores, agg


def seed_extend_dev(context, query, q_off, reference, strand, diagonal, band, match, mismatch, gap_open, gap_extend,
                    min_score, ref_lo=None, ref_hi=None):
    """The extension stage of the seed aligner (nadavca_amd/seedalign.py) for every read of a batch, on the device:
    banded affine-gap local alignment of read j (``query`` / ``q_off``: int32 codes / int64 offsets) against strand
    ``strand[j]`` (0 forward, 1 reverse complement, -1 skip) of ``reference`` (int32 codes, forward) around diagonal
    ``diagonal[j]``, traceback and matched pairs (include/nadavca_hip.h: nvk_seed_extend_dev).  Device tensors.
    ``ref_lo`` / ``ref_hi`` (int32 per read, both or neither): the read's cells lie in the columns
    ref_lo[j] <= j < ref_hi[j] of its strand (nvk_seed_extend_bounded_dev); None: the whole reference.
    -> (score i32 (n,), end i32 (n, 2), count i32 (n,), pairs i32 (total, 2)); read j's pairs are
    pairs[q_off[j] : q_off[j] + count[j]], ascending (the other rows are unspecified)."""
    import torch
    lib = _lib.load()
    dev = query.device
    n = int(q_off.numel()) - 1
    total = int(query.numel())
    G = int(reference.numel())
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    query, reference, strand, diagonal = i32(query), i32(reference), i32(strand), i32(diagonal)
    q_off = q_off.to(device=dev, dtype=torch.int64).contiguous()
    # (a placeholder element where an array is empty: the C-ABI takes no NULL for a batch that has reads)
    if total == 0:
        query = torch.zeros(1, dtype=torch.int32, device=dev)
    if G == 0:
        reference = torch.zeros(1, dtype=torch.int32, device=dev)
    hit = torch.zeros((max(n, 0), 4), dtype=torch.int32, device=dev)
    pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
    scoring = (int(band), int(match), int(mismatch), int(gap_open), int(gap_extend), int(min_score))
    if ref_lo is None and ref_hi is None:
        _lib.check(lib.nvk_seed_extend_dev(context.handle, n, total, _dp(query), _dp(q_off), _dp(reference), G,
                                           _dp(strand), _dp(diagonal), *scoring, _dp(hit), _dp(pairs)),
                   'nvk_seed_extend_dev')
    else:
        if ref_lo is None or ref_hi is None or int(ref_lo.numel()) != n or int(ref_hi.numel()) != n:
            raise ValueError('seed_extend_dev: ref_lo and ref_hi go together, one value per read each')
        ref_lo, ref_hi = i32(ref_lo), i32(ref_hi)
        if n == 0:
            ref_lo = ref_hi = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.nvk_seed_extend_bounded_dev(context.handle, n, total, _dp(query), _dp(q_off), _dp(reference),
                                                   G, _dp(strand), _dp(diagonal), _dp(ref_lo), _dp(ref_hi), *scoring,
                                                   _dp(hit), _dp(pairs)), 'nvk_seed_extend_bounded_dev')
    return hit[:, 0], hit[:, 1:3], hit[:, 3], pairs[:total]


def seed_chain_dev(context, q_off, strand, seed_off, seed_i, seed_p, strip_off, strip_diag, k, band, max_gap,
                   lookback=64):
    """The chaining stage of the seed aligner for every read of a batch, on the device (include/nadavca_hip.h:
    nvk_seed_chain_dev): read j's seeds ``seed_i`` / ``seed_p`` [seed_off[j], seed_off[j+1]), on its strand and sorted
    by (p, i), are chained, and the chain's anchors give the band centre of each strip of 64 read rows.
    ``strip_off`` (int64, the running sum of ceil(m_j / 64)) and ``strip_diag`` (int32, one centre per strip) are
    device tensors; ``strip_diag`` is WRITTEN IN PLACE for the reads that have a chain and left alone for the others
    (no strand, no seeds), so it comes in filled with the centres those are to keep.
    -> (chain score i32 (n,), anchors i32 (n,))."""
    import torch
    lib = _lib.load()
    dev = q_off.device
    n = int(q_off.numel()) - 1
    if strip_diag.dtype != torch.int32 or not strip_diag.is_contiguous() or strip_diag.device != dev:
        raise ValueError('seed_chain_dev: strip_diag is written in place: a contiguous int32 tensor on the device')
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    i64 = lambda t: t.to(device=dev, dtype=torch.int64).contiguous()
    q_off, seed_off, strip_off = i64(q_off), i64(seed_off), i64(strip_off)
    strand, seed_i, seed_p = i32(strand), i32(seed_i), i32(seed_p)
    n_seeds, n_strips = int(seed_i.numel()), int(strip_diag.numel())
    if int(seed_p.numel()) != n_seeds or int(seed_off.numel()) != n + 1 or int(strip_off.numel()) != n + 1 or \
            int(strand.numel()) != n:
        raise ValueError('seed_chain_dev: one strand per read, n + 1 offsets each, as many seed_p as seed_i')
    total = int(q_off[-1]) if n >= 0 else 0
    # (a placeholder element where an array is empty: the C-ABI takes no NULL for a batch that has reads)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros((max(n, 0), 2), dtype=torch.int32, device=dev)
    _lib.check(lib.nvk_seed_chain_dev(context.handle, n, total, _dp(q_off), _dp(strand if n else one), n_seeds,
                                      _dp(seed_off), _dp(seed_i if n_seeds else one), _dp(seed_p if n_seeds else one),
                                      int(k), int(band), int(max_gap), int(lookback), n_strips, _dp(strip_off),
                                      _dp(strip_diag if n_strips else one), _dp(out if n else one)),
               'nvk_seed_chain_dev')
    return out[:, 0], out[:, 1]


def seed_extend_path_dev(context, query, q_off, reference, strand, strip_off, strip_diag, band, match, mismatch,
                         gap_open, gap_extend, min_score, ref_lo=None, ref_hi=None):
    """``seed_extend_dev`` with a band that follows a path (include/nadavca_hip.h: nvk_seed_extend_path_dev): row i of
    read j is centred on ``strip_diag[strip_off[j] + i // 64]`` (``strip_off`` int64, the running sum of
    ceil(m_j / 64); ``strip_diag`` int32) instead of one diagonal per read.  ``ref_lo`` / ``ref_hi`` and what is
    returned as there."""
    import torch
    lib = _lib.load()
    dev = query.device
    n = int(q_off.numel()) - 1
    total = int(query.numel())
    G = int(reference.numel())
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    query, reference, strand, strip_diag = i32(query), i32(reference), i32(strand), i32(strip_diag)
    q_off = q_off.to(device=dev, dtype=torch.int64).contiguous()
    strip_off = strip_off.to(device=dev, dtype=torch.int64).contiguous()
    n_strips = int(strip_diag.numel())
    if int(strip_off.numel()) != n + 1:
        raise ValueError('seed_extend_path_dev: strip_off holds n + 1 offsets')
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    if total == 0:
        query = one
    if G == 0:
        reference = one
    if n_strips == 0:
        strip_diag = one
    if (ref_lo is None) != (ref_hi is None) or (ref_lo is not None and (int(ref_lo.numel()) != n or
                                                                        int(ref_hi.numel()) != n)):
        raise ValueError('seed_extend_path_dev: ref_lo and ref_hi go together, one value per read each')
    lo = hi = C.c_void_p(0)
    if ref_lo is not None:
        ref_lo, ref_hi = (i32(ref_lo), i32(ref_hi)) if n else (one, one)
        lo, hi = _dp(ref_lo), _dp(ref_hi)
    hit = torch.zeros((max(n, 0), 4), dtype=torch.int32, device=dev)
    pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
    _lib.check(lib.nvk_seed_extend_path_dev(context.handle, n, total, _dp(query), _dp(q_off), _dp(reference), G,
                                            _dp(strand), n_strips, _dp(strip_off), _dp(strip_diag), lo, hi, int(band),
                                            int(match), int(mismatch), int(gap_open), int(gap_extend), int(min_score),
                                            _dp(hit), _dp(pairs)), 'nvk_seed_extend_path_dev')
    return hit[:, 0], hit[:, 1:3], hit[:, 3], pairs[:total]


# ---- Chunk score accumulation and posterior, device-resident (estimator.py:199-236) ---------------------
def consensus_accumulate_dev(context, dbatch, ll, chunk_start, reverse, status, normalization_event_length,
                             ref_len, acc=None, cov=None):
    """Normalise, strand-correct and scatter-add the per-read log-likelihood rows ``ll`` (as written by
    ``estimate_log_likelihoods_dev``) into the per-position sums ``acc`` (ref_len, alphabet) f64 and the
    coverage ``cov`` (ref_len,) i64 — torch tensors on the batch's device, created zeroed when not given,
    accumulated into otherwise.  chunk_start i64 (n,), reverse i32 (n,), status i32 (n,) device tensors; ``status``
    None: every read counts."""
    torch = dbatch.torch
    lib = _lib.load()
    alpha = int(ll.shape[1])
    if acc is None:
        acc = torch.zeros((int(ref_len), alpha), dtype=torch.float64, device=dbatch.device)
    if cov is None:
        cov = torch.zeros(int(ref_len), dtype=torch.int64, device=dbatch.device)
    _lib.check(lib.nvk_consensus_accumulate_dev(
        context.handle, dbatch.n, dbatch.total_ref, alpha, _dp(ll), _dp(dbatch.reference), _dp(dbatch.ref_off),
        _dp(chunk_start), _dp(reverse), _opt(status, dbatch.n), float(normalization_event_length), int(ref_len),
        _dp(acc), _dp(cov)), 'nvk_consensus_accumulate_dev')
    return acc, cov


def posterior_segments_dev(context, ll, reference_num, seg_off, k, snp_prior, out=None):
    """``_compute_posterior`` for groups of positions laid end to end (device tensors: ll (len, alphabet) f64,
    reference_num (len,) i32, seg_off (n_segments + 1,) i64) -> posterior (len, alphabet) f64."""
    import torch
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(ll)
    _lib.check(lib.nvk_posterior_segments_dev(
        context.handle, int(ll.shape[0]), int(seg_off.numel()) - 1, _dp(seg_off), int(ll.shape[1]), int(k),
        float(snp_prior), _dp(ll), _dp(reference_num), _dp(out)), 'nvk_posterior_segments_dev')
    return out


# ---- per-k-mer sample statistics of k-mer table training (nadavca_amd/kmer_train.py) ----------------------------
def kmer_event_stats_dev(dbatch, context, events, status, k, central, alphabet, trim, level=None):
    """Per event of ``dbatch``'s reads: (key int64 (sum R,), value f64, length int64) device tensors — the k-mer key of
    a counted event or -1, its sample count, and np.sum of its samples of ``dbatch.signal`` (``level`` None) or of
    their squared deviations from ``level[key]`` (include/nadavca_hip.h: nvk_kmer_event_stats_dev)."""
    torch = dbatch.torch
    lib = _lib.load()
    n = max(dbatch.total_ref, 0)
    key = torch.empty(n, dtype=torch.int64, device=dbatch.device)
    val = torch.empty(n, dtype=torch.float64, device=dbatch.device)
    length = torch.empty(n, dtype=torch.int64, device=dbatch.device)
    _lib.check(lib.nvk_kmer_event_stats_dev(
        context.handle, dbatch.n, dbatch.total_ref, _dp(dbatch.signal), _dp(dbatch.sig_off), _dp(events),
        _dp(dbatch.ref_off), _dp(dbatch.reference), _dp(dbatch.context_before), _dp(dbatch.cb_off),
        _dp(dbatch.context_after), _dp(dbatch.ca_off), _opt(status, dbatch.n),
        int(k), int(central), int(alphabet), int(trim), _dp(level) if level is not None else C.c_void_p(0),
        _dp(key), _dp(val), _dp(length)), 'nvk_kmer_event_stats_dev')
    return key, val, length


def kmer_reduce_dev(context, key, val, length, n_kmers):
    """Per k-mer id 0 .. n_kmers: (np.sum of ``val`` over its run of ``key``, the sum of their ``length``, their
    number) as (f64, int64, int64) device tensors (nvk_kmer_reduce_dev).  ``key``: the event keys after a stable
    ascending sort; ``val`` and ``length`` gathered into the same order."""
    import torch
    lib = _lib.load()
    dev = key.device
    out_sum = torch.empty(int(n_kmers), dtype=torch.float64, device=dev)
    out_samples = torch.empty(int(n_kmers), dtype=torch.int64, device=dev)
    out_events = torch.empty(int(n_kmers), dtype=torch.int64, device=dev)
    _lib.check(lib.nvk_kmer_reduce_dev(context.handle, int(key.numel()), int(n_kmers), _dp(key), _dp(val),
                                       _dp(length), _dp(out_sum), _dp(out_samples), _dp(out_events)),
               'nvk_kmer_reduce_dev')
    return out_sum, out_samples, out_events


# ---- weighted per-k-mer statistics of modified-base table training (nadavca_amd/mod_train.py) --------------------
MOD_COLUMNS = ('w', 'n', 'sd', 'sq')


def mod_kmer_rows_dev(dbatch, context, events, status, k, central, alphabet, trim, site_off, site_pos, site_gamma,
                      mod_code, level):
    """Per base of ``dbatch``'s reads with 1 .. 4 of its read's sites in its k-mer window, one row per non-empty subset
    of them (include/nadavca_hip.h: nvk_mod_kmer_rows_dev has the contract; its two calls and the cumulative sum
    between them).  ``site_off`` int64 (n + 1,), ``site_pos`` int32 (strictly ascending within a read, inside the
    read's reference part), ``site_gamma`` f64 in [0, 1], ``level`` f64 (alphabet^k,): device tensors; what they hold is
    checked here (ValueError).
    -> (key int64 (rows,), val f64 (rows, 4): w, n, sd, sq, row_off int64 (sum R + 1,), windows_skipped int)."""
    torch = dbatch.torch
    lib = _lib.load()
    dev = dbatch.device
    n, total = dbatch.n, max(dbatch.total_ref, 0)
    site_off = site_off.to(device=dev, dtype=torch.int64).contiguous()
    site_pos = site_pos.to(device=dev, dtype=torch.int32).contiguous()
    site_gamma = site_gamma.to(device=dev, dtype=torch.float64).contiguous()
    level = level.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    n_sites = int(site_pos.numel())
    if int(level.numel()) != int(alphabet) ** int(k):
        raise ValueError('mod_kmer_rows_dev: level holds %d values, the table %d' % (int(level.numel()),
                                                                                    int(alphabet) ** int(k)))
    if int(site_off.numel()) != n + 1 or int(site_gamma.numel()) != n_sites:
        raise ValueError('mod_kmer_rows_dev: site_off holds %d offsets for %d reads, site_gamma %d values for %d sites'
                         % (int(site_off.numel()), n, int(site_gamma.numel()), n_sites))
    if n_sites:
        if not bool(((site_gamma >= 0.0) & (site_gamma <= 1.0)).all()):     # (false for a NaN too)
            raise ValueError('mod_kmer_rows_dev: a site_gamma outside [0, 1] or not finite')
        if not (int(site_off[0]) == 0 and int(site_off[-1]) == n_sites and bool((site_off[1:] >= site_off[:-1]).all())):
            raise ValueError('mod_kmer_rows_dev: site_off does not start at 0, decreases or does not end at the number '
                             'of sites')
        owner = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), site_off[1:] - site_off[:-1],
                                        output_size=n_sites)
        length = (dbatch.ref_off[1:] - dbatch.ref_off[:-1])[owner]
        if not bool(((site_pos >= 0) & (site_pos < length)).all()):
            raise ValueError('mod_kmer_rows_dev: a site position outside its read\'s reference part')
        if not bool(((owner[1:] != owner[:-1]) | (site_pos[1:] > site_pos[:-1])).all()):
            raise ValueError('mod_kmer_rows_dev: site positions are not strictly ascending within a read')
    else:       # (a placeholder element: the C-ABI takes no NULL for a batch that has reads)
        site_pos = torch.zeros(1, dtype=torch.int32, device=dev)
        site_gamma = torch.zeros(1, dtype=torch.float64, device=dev)
    skipped = C.c_int64(0)
    head = (context.handle, dbatch.n, dbatch.total_ref, _dp(dbatch.signal), _dp(dbatch.sig_off), _dp(events),
            _dp(dbatch.ref_off), _dp(dbatch.reference), _dp(dbatch.context_before), _dp(dbatch.cb_off),
            _dp(dbatch.context_after), _dp(dbatch.ca_off), _opt(status, dbatch.n),
            int(k), int(central), int(alphabet), int(trim), n_sites, _dp(site_off), _dp(site_pos), _dp(site_gamma),
            int(mod_code), _dp(level))
    count = torch.zeros(total, dtype=torch.int64, device=dev)
    _lib.check(lib.nvk_mod_kmer_rows_dev(*head, 0, C.c_void_p(0), _dp(count), C.c_void_p(0), C.c_void_p(0),
                                         C.byref(skipped)), 'nvk_mod_kmer_rows_dev')
    row_off = torch.zeros(total + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=row_off[1:])
    n_rows = int(row_off[-1])
    key = torch.empty(n_rows, dtype=torch.int64, device=dev)
    val = torch.empty((n_rows, len(MOD_COLUMNS)), dtype=torch.float64, device=dev)
    if n_rows:
        _lib.check(lib.nvk_mod_kmer_rows_dev(*head, n_rows, _dp(row_off), C.c_void_p(0), _dp(key), _dp(val),
                                             C.byref(skipped)), 'nvk_mod_kmer_rows_dev')
    return key, val, row_off, int(skipped.value)


def mod_kmer_reduce_dev(context, val, run_off):
    """Per run of ``run_off`` (int64 (n_keys + 1,): the runs of the distinct keys >= 0 among the rows in stable key
    order; ``val`` f64 (rows, 4) gathered into that order): (sums f64 (n_keys, 4): W, Nw, Sd, Sq, rows int64 (n_keys,))
    device tensors (nvk_mod_kmer_reduce_dev)."""
    import torch
    lib = _lib.load()
    dev = val.device
    n_keys = int(run_off.numel()) - 1
    if n_keys < 0 or val.dim() != 2 or int(val.shape[1]) != len(MOD_COLUMNS):
        raise ValueError('mod_kmer_reduce_dev: val must be (rows, 4) and run_off hold at least one offset')
    val = val.to(torch.float64).contiguous()
    run_off = run_off.to(device=dev, dtype=torch.int64).contiguous()
    sums = torch.empty((n_keys, len(MOD_COLUMNS)), dtype=torch.float64, device=dev)
    rows = torch.empty(n_keys, dtype=torch.int64, device=dev)
    _lib.check(lib.nvk_mod_kmer_reduce_dev(context.handle, int(val.shape[0]), n_keys, _dp(val), _dp(run_off),
                                           _dp(sums), _dp(rows)), 'nvk_mod_kmer_reduce_dev')
    return sums, rows


def mod_kmer_stats_dev(context, dbatch, events, status, k, central, alphabet, trim, site_off, site_pos, site_gamma,
                       mod_code, level):
    """The weighted statistics of every k-mer that a site's window can turn into: the rows from one kernel, a stable
    sort of their keys, a gather and the runs of the keys (torch: plumbing), the per-run sums from another.
    -> dict of device tensors ``key`` int64 (n_keys,) ascending, ``sums`` f64 (n_keys, 4): W, Nw, Sd, Sq, ``count``
    int64 (n_keys,), and the ints ``rows`` and ``windows_skipped``."""
    import torch
    key, val, _, skipped = mod_kmer_rows_dev(dbatch, context, events, status, k, central, alphabet, trim, site_off,
                                             site_pos, site_gamma, mod_code, level)
    skey, order = torch.sort(key, stable=True)
    sval = val[order]
    n_neg = (skey < 0).sum().reshape(1)
    ukey, counts = torch.unique_consecutive(skey[skey >= 0], return_counts=True)
    run_off = torch.cat([n_neg, n_neg + torch.cumsum(counts, 0)])
    sums, count = mod_kmer_reduce_dev(context, sval, run_off)
    return dict(key=ukey, sums=sums, count=count, rows=int(key.numel()), windows_skipped=skipped)


# ---- per-site allele mixtures (nadavca_amd/allele_fractions.py) -------------------------------------------------
def allele_rows_dev(context, dbatch, ll, chunk_start, reverse, status, event_length, ref_len):
    """Per read-major row of ``ll``: (key int64 (sum R,), val f64 (sum R, alphabet)) device tensors — the row's global
    reference position (-1 where it does not count) and its normalised, strand-corrected log-likelihood ratios in
    forward columns (include/nadavca_hip.h: nvk_allele_rows_dev)."""
    torch = dbatch.torch
    lib = _lib.load()
    alpha = int(ll.shape[1])
    n = max(dbatch.total_ref, 0)
    key = torch.empty(n, dtype=torch.int64, device=dbatch.device)
    val = torch.empty((n, alpha), dtype=torch.float64, device=dbatch.device)
    _lib.check(lib.nvk_allele_rows_dev(
        context.handle, dbatch.n, dbatch.total_ref, alpha, _dp(ll), _dp(dbatch.reference), _dp(dbatch.ref_off),
        _dp(chunk_start), _dp(reverse), _opt(status, dbatch.n), float(event_length),
        int(ref_len), _dp(key), _dp(val)), 'nvk_allele_rows_dev')
    return key, val


def allele_solve_dev(context, key, val, ref_codes):
    """Per position of ``ref_codes`` (int32 device tensor) and base: (fraction, lrt, ll_half, ll_full f64 (L, alphabet),
    coverage int64 (L,)) device tensors (nvk_allele_solve_dev).  ``key``: the rows' keys after a stable ascending
    sort; ``val`` (rows, alphabet) gathered into the same order."""
    import torch
    lib = _lib.load()
    dev = ref_codes.device
    L, alpha = int(ref_codes.numel()), int(val.shape[1])
    out = [torch.empty((L, alpha), dtype=torch.float64, device=dev) for _ in range(4)]
    cov = torch.empty(L, dtype=torch.int64, device=dev)
    _lib.check(lib.nvk_allele_solve_dev(context.handle, int(key.numel()), L, alpha, _dp(key), _dp(val),
                                        _dp(ref_codes), *[_dp(t) for t in out], _dp(cov)), 'nvk_allele_solve_dev')
    return out[0], out[1], out[2], out[3], cov


def allele_fractions_dev(context, dbatch, ll, chunk_start, reverse, status, event_length, ref_codes):
    """The allele mixture of every reference position from the per-read rows ``ll`` (as written by
    ``estimate_log_likelihoods_dev``): rows and keys from one kernel, a stable sort by position and a gather (torch:
    plumbing), the per-position solve in another (include/nadavca_hip.h: nvk_allele_rows_dev has the contract).
    chunk_start i64 (n,), reverse i32 (n,), status i32 (n,) or None, ref_codes i32 (L,): device tensors.
    -> (fraction, lrt, ll_half, ll_full f64 (L, alphabet), coverage int64 (L,)) device tensors."""
    _, val, sorted_key, order = allele_sorted_rows_dev(context, dbatch, ll, chunk_start, reverse, status, event_length,
                                                       int(ref_codes.numel()))
    return allele_solve_dev(context, sorted_key, val[order], ref_codes)


def allele_sorted_rows_dev(context, dbatch, ll, chunk_start, reverse, status, event_length, ref_len):
    """``allele_rows_dev`` and the stable ascending sort of its keys: -> (key, val, sorted_key, order) device tensors,
    ``key`` and ``val`` read-major as written, ``sorted_key = key[order]``.  ``val[order]`` is what
    ``allele_solve_dev`` and the site kernels of the phasing take."""
    import torch
    key, val = allele_rows_dev(context, dbatch, ll, chunk_start, reverse, status, event_length, ref_len)
    sorted_key, order = torch.sort(key, stable=True)
    return key, val, sorted_key, order


# ---- phasing and haplotype tags (nadavca_amd/phase.py; include/nadavca_hip.h: nvk_phase_links_dev) ----------------
def phase_links_dev(context, site_lo, site_hi, site_alt, chain, row_read, sorted_val, clip):
    """Per site: (link f64 (S,), shared int64 (S,)) device tensors (nvk_phase_links_dev).  site_lo / site_hi i64 (S,):
    the sites' ranges in the sorted rows; site_alt, chain i32 (S,); row_read i64 (rows,): the read of every sorted row;
    sorted_val f64 (rows, alphabet)."""
    import torch
    lib = _lib.load()
    S = int(site_lo.numel())
    link = torch.zeros(S, dtype=torch.float64, device=site_lo.device)
    shared = torch.zeros(S, dtype=torch.int64, device=site_lo.device)
    _lib.check(lib.nvk_phase_links_dev(context.handle, S, int(sorted_val.shape[1]), _dp(site_lo), _dp(site_hi),
                                       _dp(site_alt), _dp(chain), _dp(row_read), _dp(sorted_val), float(clip),
                                       _dp(link), _dp(shared)), 'nvk_phase_links_dev')
    return link, shared


def _phase_tag(entry, context, ref_off, chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma,
               clip):
    """The two tag entries (``entry``: the symbol's name): the same arguments, the same results."""
    import torch
    lib = _lib.load()
    n, S = int(ref_off.numel()) - 1, int(site_pos.numel())
    dev = ref_off.device
    block = torch.full((n,), -1, dtype=torch.int64, device=dev)
    llr = torch.zeros(n, dtype=torch.float64, device=dev)
    count = torch.zeros(n, dtype=torch.int64, device=dev)
    _lib.check(getattr(lib, entry)(context.handle, n, S, int(val.shape[1]), _dp(ref_off), _dp(chunk_start),
                                   _dp(reverse), _dp(key), _dp(val), _dp(site_pos), _dp(site_alt), _dp(site_block),
                                   _dp(site_sigma), float(clip), _dp(block), _dp(llr), _dp(count)), entry)
    return block, llr, count


def phase_tag_dev(context, ref_off, chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma, clip):
    """Per read: (read_block int64 (n,), read_llr f64 (n,), read_sites int64 (n,)) device tensors (nvk_phase_tag_dev)
    from the READ-MAJOR ``key`` / ``val`` of ``allele_rows_dev``; -1 / 0 / 0 for a read without a site.  ref_off i64
    (n + 1,), chunk_start i64 (n,), reverse i32 (n,); site_pos, site_block i64 (S,), site_alt, site_sigma i32 (S,)."""
    return _phase_tag('nvk_phase_tag_dev', context, ref_off, chunk_start, reverse, key, val, site_pos, site_alt,
                      site_block, site_sigma, clip)


def phase_votes_dev(context, site_lo, site_hi, site_alt, site_block, site_sigma, row_read, sorted_val, read_block,
                    read_llr, clip):
    """Per site: (vote f64 (S,), n_agree int64 (S,), n_against int64 (S,)) device tensors (nvk_phase_votes_dev): the
    leave-one-out vote of the reads tagged in the site's block.  Arguments as for ``phase_links_dev`` and as
    ``phase_tag_dev`` returns them."""
    import torch
    lib = _lib.load()
    S = int(site_lo.numel())
    dev = site_lo.device
    vote = torch.zeros(S, dtype=torch.float64, device=dev)
    agree = torch.zeros(S, dtype=torch.int64, device=dev)
    against = torch.zeros(S, dtype=torch.int64, device=dev)
    _lib.check(lib.nvk_phase_votes_dev(context.handle, S, int(sorted_val.shape[1]), _dp(site_lo), _dp(site_hi),
                                       _dp(site_alt), _dp(site_block), _dp(site_sigma), _dp(row_read),
                                       _dp(sorted_val), _dp(read_block), _dp(read_llr), float(clip), _dp(vote),
                                       _dp(agree), _dp(against)), 'nvk_phase_votes_dev')
    return vote, agree, against


def phase_blocks(link, shared, chain, min_shared, min_link):
    """Blocks and starting phase from the links (integer work, torch on the tensors' device): site s is joined to
    s - 1 iff chain, shared >= min_shared and |link| >= min_link.  -> (block int64 (S,): the index of the block's
    first site, sigma int32 (S,): +1 at a block's first site, then sigma[s - 1] * (+1 if link > 0 else -1))."""
    import torch
    S = int(link.numel())
    joined = (chain != 0) & (shared >= int(min_shared)) & (link.abs() >= float(min_link))
    joined[:1] = False
    idx = torch.arange(S, dtype=torch.int64, device=link.device)
    block = torch.cummax(torch.where(joined, torch.zeros_like(idx), idx), 0).values if S else idx
    turns = torch.cumsum((joined & ~(link > 0)).to(torch.int64), 0)
    sigma = (1 - 2 * ((turns - turns[block]) & 1)).to(torch.int32)
    return block, sigma


def check_span(what, span):
    """``span`` as ``phase_reads_batch`` takes it -> int in 1 .. 8, or ValueError."""
    if isinstance(span, bool) or not isinstance(span, (int, np.integer)) or not 1 <= span <= 8:
        raise ValueError('%s: span %r is not an integer in 1 .. 8' % (what, span))
    return int(span)


def phase_span_links_dev(context, site_lo, site_hi, site_alt, site_first, row_read, sorted_val, clip, span):
    """Per site and w = 1 .. span: (link f64 (S, span), shared int64 (S, span)) device tensors
    (nvk_phase_span_links_dev): column w - 1 holds the link between the sites s - w and s, 0 where s - w lies before
    site_first[s].  site_first i64 (S,): the first site of every site's contig; the other arguments as for
    ``phase_links_dev``."""
    import torch
    lib = _lib.load()
    S, span = int(site_lo.numel()), check_span('phase_span_links_dev', span)
    link = torch.zeros((S, span), dtype=torch.float64, device=site_lo.device)
    shared = torch.zeros((S, span), dtype=torch.int64, device=site_lo.device)
    _lib.check(lib.nvk_phase_span_links_dev(context.handle, S, span, int(sorted_val.shape[1]), _dp(site_lo),
                                            _dp(site_hi), _dp(site_alt), _dp(site_first), _dp(row_read),
                                            _dp(sorted_val), float(clip), _dp(link), _dp(shared)),
               'nvk_phase_span_links_dev')
    return link, shared


def phase_tag_blocks_dev(context, ref_off, chunk_start, reverse, key, val, site_pos, site_alt, site_block, site_sigma,
                         clip):
    """``phase_tag_dev`` for ANY block array (nvk_phase_tag_blocks_dev): a read's block is the one with the largest |H|
    over all of the read's sites in that block, the smallest block index on ties.  Arguments and results as there."""
    return _phase_tag('nvk_phase_tag_blocks_dev', context, ref_off, chunk_start, reverse, key, val, site_pos, site_alt,
                      site_block, site_sigma, clip)


def phase_forest(link, shared, site_first, min_shared, min_link):
    """Parents, blocks and starting phase from the span links (integer work, torch on the tensors' device, CPU tensors
    included).  link f64 (S, span), shared int64 (S, span), site_first int64 (S,).  Candidate w = 1 .. span of site s
    qualifies when s - w >= site_first[s], shared >= min_shared and |link| >= min_link; parent[s] = s - w* for the
    qualifying candidate with the largest |link| (the smallest w on ties), -1 without one.  A parent is an earlier
    site, so this is a forest; roots and signs come from pointer jumping in ceil(log2 S) gathers.
    -> (parent int64 (S,), block int64 (S,): the root, sigma int32 (S,): the product of (+1 if link > 0 else -1) along
    the path to the root).  With span 1 block and sigma are ``phase_blocks``'."""
    import torch
    S, span = int(link.shape[0]), int(link.shape[1])
    dev = link.device
    idx = torch.arange(S, dtype=torch.int64, device=dev)
    w = torch.arange(1, span + 1, dtype=torch.int64, device=dev)
    ok = (idx[:, None] - w[None, :] >= site_first.to(torch.int64)[:, None]) & (shared >= int(min_shared)) \
        & (link.abs() >= float(min_link))
    if S == 0 or span == 0:
        return idx - 1, idx, torch.ones(S, dtype=torch.int32, device=dev)
    mag = torch.where(ok, link.abs(), torch.full_like(link, -1.0))
    top = mag.max(dim=1).values
    has = top >= 0.0
    # the smallest w among the candidates that reach the maximum
    w_star = torch.where(ok & (mag == top[:, None]), w[None, :].expand(S, span),
                         torch.full((S, span), span + 1, dtype=torch.int64, device=dev)).min(dim=1).values
    w_star = torch.where(has, w_star, torch.ones_like(w_star))
    parent = torch.where(has, idx - w_star, torch.full_like(idx, -1))
    chosen = link.gather(1, (w_star - 1)[:, None])[:, 0]
    ptr = torch.where(has, parent, idx)
    turn = (has & ~(chosen > 0)).to(torch.int64)         # the parity of the -1 links on the path from s to ptr[s]
    for _ in range(max(S - 1, 1).bit_length()):
        turn = turn ^ turn[ptr]
        ptr = ptr[ptr]
    return parent, ptr, (1 - 2 * turn).to(torch.int32)


def phase_sites_dev(context, ref_off, chunk_start, reverse, key, val, sorted_key, sorted_val, order, site_pos, site_alt,
                    chain, clip, min_shared, min_link, rounds, *, span=1):
    """The whole phasing loop on the device (include/nadavca_hip.h: nvk_phase_links_dev has the contract): links,
    blocks and starting phase, ``rounds`` rounds of tag / vote / flip, the final tag and vote.  ``key`` / ``val``:
    the read-major rows of ``allele_sorted_rows_dev``, ``sorted_key`` / ``order`` its sort, ``sorted_val = val[order]``;
    site_pos i64 (S,) global and strictly ascending, site_alt i32 (S,), chain i32 (S,).  -> dict of device tensors:
    link, shared, block, sigma, vote, n_agree, n_against (S,), read_block, read_llr, read_sites (n,) and flips
    int64 (rounds,).
    ``span`` = 1: every site is linked to the site before it only.  ``span`` = 2 .. 8 (nvk_phase_span_links_dev has
    the contract): every site is linked to the ``span`` sites before it, back to the last site with chain 0, and
    joined to the strongest qualifying one (``phase_forest``); the tags come from nvk_phase_tag_blocks_dev, since a
    block is no interval then.  The dict gains parent int64 (S,), span_link f64 and span_shared int64 (S, span); link
    and shared stay the column of the site before."""
    import torch
    span = check_span('phase_sites_dev', span)
    site_pos, site_alt, chain = site_pos.contiguous(), site_alt.contiguous(), chain.contiguous()
    # the read of every sorted row: the last read whose offset is <= the row's read-major index
    row_read = (torch.searchsorted(ref_off, order, right=True) - 1).contiguous()
    site_lo = torch.searchsorted(sorted_key, site_pos).contiguous()
    site_hi = torch.searchsorted(sorted_key, site_pos, right=True).contiguous()
    more = {}
    if span == 1:
        link, shared = phase_links_dev(context, site_lo, site_hi, site_alt, chain, row_read, sorted_val, clip)
        block, sigma = phase_blocks(link, shared, chain, min_shared, min_link)
        tag_dev = phase_tag_dev
    else:
        idx = torch.arange(int(site_pos.numel()), dtype=torch.int64, device=site_pos.device)
        # the last site at or before s whose chain is 0 (site 0 opens a chain whatever its flag)
        site_first = torch.cummax(torch.where(chain != 0, torch.zeros_like(idx), idx), 0).values.contiguous() \
            if idx.numel() else idx
        span_link, span_shared = phase_span_links_dev(context, site_lo, site_hi, site_alt, site_first, row_read,
                                                      sorted_val, clip, span)
        parent, block, sigma = phase_forest(span_link, span_shared, site_first, min_shared, min_link)
        block, sigma = block.contiguous(), sigma.contiguous()
        link, shared = span_link[:, 0].contiguous(), span_shared[:, 0].contiguous()
        more = dict(parent=parent, span_link=span_link, span_shared=span_shared)
        tag_dev = phase_tag_blocks_dev
    flips = []
    for r in range(int(rounds) + 1):
        read_block, read_llr, read_sites = tag_dev(context, ref_off, chunk_start, reverse, key, val, site_pos,
                                                   site_alt, block, sigma, clip)
        vote, agree, against = phase_votes_dev(context, site_lo, site_hi, site_alt, block, sigma, row_read, sorted_val,
                                               read_block, read_llr, clip)
        if r == int(rounds):
            break
        flip = vote * sigma < 0
        flips.append(flip.sum())
        sigma = torch.where(flip, -sigma, sigma)
        sigma = (sigma * sigma[block]).contiguous()
    flips = torch.stack(flips) if flips else torch.zeros(0, dtype=torch.int64, device=link.device)
    return dict(link=link, shared=shared, block=block, sigma=sigma, vote=vote, n_agree=agree, n_against=against,
                read_block=read_block, read_llr=read_llr, read_sites=read_sites, flips=flips, **more)


# ---- per-site modification frequencies over sets of rows (nadavca_amd/phase_mods.py) -------------------------------
def mod_site_solve_dev(context, site_lo, site_hi, val, group, set_mask, clip):
    """Per (site, set): (count int64, fraction f64, ll f64), each (S, n_sets), device tensors (include/nadavca_hip.h:
    nvk_mod_site_solve_dev).  site_lo / site_hi i64 (S,): the sites' ranges of rows; val f64 (rows,): the rows'
    log-likelihood ratios; group i32 (rows,) or None (every row is group 0); set_mask: 1 .. 8 integers in 0 .. 2^32 - 1,
    set q holds the rows whose group's bit is set in ``set_mask[q]``."""
    import torch
    lib = _lib.load()
    dev = site_lo.device
    masks = [int(m) for m in np.asarray(set_mask).reshape(-1)]
    if any(not 0 <= m < 1 << 32 for m in masks):
        raise ValueError('mod_site_solve_dev: a set mask outside 0 .. 2^32 - 1')
    S, n_rows, Q = int(site_lo.numel()), int(val.numel()), len(masks)
    if int(site_hi.numel()) != S or (group is not None and int(group.numel()) != n_rows):
        raise ValueError('mod_site_solve_dev: site_hi or group does not match site_lo or val in length')
    if site_lo.dtype != torch.int64 or site_hi.dtype != torch.int64 or val.dtype != torch.float64 \
            or (group is not None and group.dtype != torch.int32):
        raise ValueError('mod_site_solve_dev: site_lo / site_hi int64, val float64, group int32')
    # uint32 bit patterns held in an int32 tensor
    mask = torch.from_numpy(np.array(masks, dtype=np.uint32).view(np.int32)).to(dev)
    count = torch.zeros((S, Q), dtype=torch.int64, device=dev)
    fraction = torch.zeros((S, Q), dtype=torch.float64, device=dev)
    ll = torch.zeros((S, Q), dtype=torch.float64, device=dev)
    site_lo, site_hi, val = site_lo.contiguous(), site_hi.contiguous(), val.contiguous()
    group = None if group is None else group.contiguous()
    _lib.check(lib.nvk_mod_site_solve_dev(
        context.handle, S, n_rows, _dp(site_lo), _dp(site_hi), _opt(val, n_rows), _opt(group, n_rows), Q, _dp(mask),
        float(clip), _dp(count), _dp(fraction), _dp(ll)), 'nvk_mod_site_solve_dev')
    return count, fraction, ll


# ---- per-site event-level pile-up (nadavca_amd/site_levels.py) --------------------------------------------------
SITE_COLUMNS = ('level', 'stdv', 'dwell', 'resid')


def site_level_rows_dev(context, dbatch, events, expected, chunk_start, reverse, status, trim, ref_len):
    """Per base of ``dbatch``'s reads: (key int64 (sum R,), val f64 (sum R, 4)) device tensors — 2 * global position +
    strand of a counted base or -1, and np.mean, np.std and the length of its event over ``dbatch.signal`` and the
    mean's distance from ``expected`` (include/nadavca_hip.h: nvk_site_level_rows_dev)."""
    torch = dbatch.torch
    lib = _lib.load()
    n = max(dbatch.total_ref, 0)
    key = torch.empty(n, dtype=torch.int64, device=dbatch.device)
    val = torch.empty((n, len(SITE_COLUMNS)), dtype=torch.float64, device=dbatch.device)
    _lib.check(lib.nvk_site_level_rows_dev(
        context.handle, dbatch.n, dbatch.total_ref, _dp(dbatch.signal), _dp(dbatch.sig_off), _dp(events),
        _dp(dbatch.ref_off), _dp(expected), _dp(chunk_start), _dp(reverse),
        _opt(status, dbatch.n), int(trim), int(ref_len), _dp(key), _dp(val)),
        'nvk_site_level_rows_dev')
    return key, val


def site_moments_dev(context, key, val, n_keys):
    """Per key 0 .. n_keys: (count int64 (n_keys,), mean f64 (n_keys, n_val), m2 f64 (n_keys, n_val)) device tensors:
    the rows of the key, and per column their mean and their sum of squared deviations from it
    (nvk_site_moments_dev).  ``key``: the rows' keys after a stable ascending sort; ``val`` (rows, n_val) gathered into
    the same order."""
    import torch
    lib = _lib.load()
    dev = val.device
    n_keys, n_val = int(n_keys), int(val.shape[1])
    count = torch.empty(n_keys, dtype=torch.int64, device=dev)
    mean = torch.empty((n_keys, n_val), dtype=torch.float64, device=dev)
    m2 = torch.empty((n_keys, n_val), dtype=torch.float64, device=dev)
    _lib.check(lib.nvk_site_moments_dev(context.handle, int(key.numel()), n_keys, n_val, _dp(key), _dp(val),
                                        _dp(count), _dp(mean), _dp(m2)), 'nvk_site_moments_dev')
    return count, mean, m2


def site_levels_dev(context, dbatch, events, expected, chunk_start, reverse, status, trim, ref_len):
    """The pile-up of the reads' event levels per (reference position, strand): rows and keys from one kernel, a stable
    sort by key and a gather (torch: plumbing), the per-key moments in another (include/nadavca_hip.h:
    nvk_site_level_rows_dev has the contract).  events i32 (sum R, 2), expected f64 (sum R,), chunk_start i64 (n,),
    reverse i32 (n,), status i32 (n,) or None: device tensors.
    -> (count int64 (2 ref_len,), mean, m2 f64 (2 ref_len, 4), key, val): key 2 P + strand; ``key`` / ``val``: the
    rows in read order, before the sort."""
    import torch
    key, val = site_level_rows_dev(context, dbatch, events, expected, chunk_start, reverse, status, trim, ref_len)
    skey, order = torch.sort(key, stable=True)
    count, mean, m2 = site_moments_dev(context, skey, val[order], 2 * int(ref_len))
    return count, mean, m2, key, val


# ---- per-site rank tests between two samples (nadavca_amd/site_ranks.py) -----------------------------------------
MAX_SITE_ROWS = 1 << 20          # n + m per site stays below this: the tie sum of t^3 - t is an exact int64


def sort_site_rows(key, val):
    """The rows of one sample for nvk_site_rank_tests_dev: rows with key < 0 or a NaN value dropped, the rest sorted
    ascending by (key, value) — a stable argsort by value, then a stable argsort by key (torch: plumbing).
    -> (key int64, val f64) contiguous device tensors."""
    import torch
    keep = (key >= 0) & ~torch.isnan(val)
    key, val = key[keep], val[keep]
    by_val = torch.argsort(val, stable=True)
    key, val = key[by_val], val[by_val]
    by_key = torch.argsort(key, stable=True)
    return key[by_key].contiguous(), val[by_key].contiguous()


def common_sites(key_a, key_b, min_coverage):
    """The ascending keys with at least ``min_coverage`` rows in BOTH sorted key tensors, on the device, and the
    largest n + m among them (0 when there is none; one number crosses to the host, and only where the two samples
    together hold MAX_SITE_ROWS rows or more)."""
    import torch
    ua, ca = torch.unique_consecutive(key_a, return_counts=True)
    ub, cb = torch.unique_consecutive(key_b, return_counts=True)
    ua, ca, ub, cb = ua[ca >= min_coverage], ca[ca >= min_coverage], ub[cb >= min_coverage], cb[cb >= min_coverage]
    in_b = torch.isin(ua, ub, assume_unique=True)
    site_key = ua[in_b].contiguous()
    largest = 0
    if int(key_a.numel()) + int(key_b.numel()) >= MAX_SITE_ROWS and int(site_key.numel()) > 0:
        largest = int((ca[in_b] + cb[torch.isin(ub, ua, assume_unique=True)]).max())
    return site_key, largest


def _two_sample_sites(entry, noun, finite_only, key_a, val_a, key_b, val_b, min_coverage):
    """What ``site_rank_tests_dev`` and ``site_mixture_tests_dev`` do before their kernel: the check of
    ``min_coverage``, ``sort_site_rows`` per sample (``finite_only``: rows with +-inf dropped too), ``common_sites`` and
    the 2^20 guard (``entry`` and ``noun`` name the caller and its tests in the messages).
    -> (key_a, val_a, key_b, val_b, site_key), sorted."""
    import torch
    if int(min_coverage) != min_coverage or min_coverage < 1:
        raise ValueError('%s: min_coverage %r is not an integer >= 1' % (entry, min_coverage))
    if finite_only:
        finite_a, finite_b = torch.isfinite(val_a), torch.isfinite(val_b)
        key_a, val_a, key_b, val_b = key_a[finite_a], val_a[finite_a], key_b[finite_b], val_b[finite_b]
    key_a, val_a = sort_site_rows(key_a, val_a)
    key_b, val_b = sort_site_rows(key_b, val_b)
    site_key, largest = common_sites(key_a, key_b, int(min_coverage))
    if largest >= MAX_SITE_ROWS:
        raise ValueError('%s: a site holds %d rows in the two samples together; the %s tests serve fewer than 2^20 '
                         'per site' % (entry, largest, noun))
    return key_a, val_a, key_b, val_b, site_key


def site_rank_tests_dev(context, key_a, val_a, key_b, val_b, min_coverage, exact_cells):
    """Per-site rank tests between two samples' rows of ONE event column (include/nadavca_hip.h:
    nvk_site_rank_tests_dev has the contract).  key int64 (rows,) (a key < 0: not counted) and val f64 (rows,) per
    sample, unsorted device tensors.  Rows with key < 0 or a NaN value are dropped; the rest are sorted by (key,
    value); the sites are the keys with at least ``min_coverage`` rows in both samples; a site whose two pile-ups hold
    2^20 rows or more together is a ValueError (the kernel's tie sum is an exact int64 below that); then ONE kernel
    call.  ``exact_cells``: the exact KS p-value is computed where min(n, m) <= 255 and n m <= exact_cells.
    -> (site_key, n_a, n_b, ks_plus, ks_minus, u2, tie int64 (sites,), ks_p f64 (sites,)) device tensors, site_key
    ascending."""
    import torch
    lib = _lib.load()
    if int(exact_cells) != exact_cells or exact_cells < 0:
        raise ValueError('site_rank_tests_dev: exact_cells %r is not an integer >= 0' % (exact_cells,))
    key_a, val_a, key_b, val_b, site_key = _two_sample_sites('site_rank_tests_dev', 'rank', False, key_a, val_a, key_b,
                                                             val_b, min_coverage)
    n_sites = int(site_key.numel())
    dev = val_a.device
    ints = [torch.empty(n_sites, dtype=torch.int64, device=dev) for _ in range(6)]
    ks_p = torch.empty(n_sites, dtype=torch.float64, device=dev)
    _lib.check(lib.nvk_site_rank_tests_dev(
        context.handle, int(key_a.numel()), _dp(key_a), _dp(val_a), int(key_b.numel()), _dp(key_b), _dp(val_b),
        n_sites, _dp(site_key), int(exact_cells), *[_dp(t) for t in ints], _dp(ks_p)), 'nvk_site_rank_tests_dev')
    return (site_key, *ints, ks_p)


# ---- per-site mixture tests between two samples (nadavca_amd/site_mixtures.py) -----------------------------------
SITE_MIX_COUNTS, SITE_MIX_FIT = 5, 17        # the columns of nvk_site_mixture_tests_dev's two tables


def site_mixture_tests_dev(context, key_a, val_a, key_b, val_b, min_coverage, iterations, min_sd_ratio):
    """Per-site two-component mixture fits over two samples' rows of ONE event column (include/nadavca_hip.h:
    nvk_site_mixture_tests_dev has the contract).  key int64 (rows,) (a key < 0: not counted) and val f64 (rows,) per
    sample, unsorted device tensors.  Rows with key < 0 or a value that is not finite are dropped (a mixture cannot
    hold +-inf, which the rank tests keep); the rest are sorted by (key, value) (``sort_site_rows``); the sites are the
    keys with at least ``min_coverage`` rows in both samples (``common_sites``); a site whose two pile-ups hold 2^20
    rows or more together is a ValueError, as for the rank tests; then ONE kernel call.
    -> (site_key int64 (sites,), counts int64 (sites, 5), fit f64 (sites, 17)) device tensors, site_key ascending; the
    columns as the contract lists them."""
    import torch
    lib = _lib.load()
    if int(iterations) != iterations or not 1 <= iterations <= 1024:
        raise ValueError('site_mixture_tests_dev: iterations %r is not an integer in 1 .. 1024' % (iterations,))
    if not 0.0 < min_sd_ratio <= 1.0:
        raise ValueError('site_mixture_tests_dev: min_sd_ratio %r is not in (0, 1]' % (min_sd_ratio,))
    key_a, val_a, key_b, val_b, site_key = _two_sample_sites('site_mixture_tests_dev', 'mixture', True, key_a, val_a,
                                                             key_b, val_b, min_coverage)
    n_sites = int(site_key.numel())
    dev = val_a.device
    counts = torch.empty((n_sites, SITE_MIX_COUNTS), dtype=torch.int64, device=dev)
    fit = torch.empty((n_sites, SITE_MIX_FIT), dtype=torch.float64, device=dev)
    _lib.check(lib.nvk_site_mixture_tests_dev(
        context.handle, int(key_a.numel()), _dp(key_a), _dp(val_a), int(key_b.numel()), _dp(key_b), _dp(val_b),
        n_sites, _dp(site_key), int(iterations), float(min_sd_ratio), _dp(counts), _dp(fit)),
        'nvk_site_mixture_tests_dev')
    return site_key, counts, fit


# ---- signal_map_batch: event detection and event alignment (include/nadavca_hip.h) ----------------------------
def event_flags_dev(context, signal, sig_off, window, threshold, var_floor):
    """Where events start in the reads' normalised signals (f64 / int64 device tensors, read j at
    [sig_off[j], sig_off[j+1])) -> int32 (total,) : 1 at a border, else 0 (nvk_event_flags_dev)."""
    import torch
    lib = _lib.load()
    n, total = int(sig_off.numel()) - 1, int(signal.numel())
    flags = torch.zeros(max(total, 1), dtype=torch.int32, device=sig_off.device)
    if total == 0:
        signal = torch.zeros(1, dtype=torch.float64, device=sig_off.device)
    _lib.check(lib.nvk_event_flags_dev(context.handle, n, total, _dp(signal), _dp(sig_off), int(window),
                                       float(threshold), float(var_floor), _dp(flags)), 'nvk_event_flags_dev')
    return flags[:total]


def event_levels_dev(context, signal, sig_off, ev_pos):
    """The events that start at the flat positions ``ev_pos`` (int64, ascending) -> (start int32: the first sample,
    counted inside the read; length int32; level f64: the mean of the samples), nvk_event_levels_dev."""
    import torch
    lib = _lib.load()
    dev = sig_off.device
    n, total, n_ev = int(sig_off.numel()) - 1, int(signal.numel()), int(ev_pos.numel())
    start = torch.zeros(max(n_ev, 1), dtype=torch.int32, device=dev)
    length = torch.zeros(max(n_ev, 1), dtype=torch.int32, device=dev)
    level = torch.zeros(max(n_ev, 1), dtype=torch.float64, device=dev)
    if n_ev:
        _lib.check(lib.nvk_event_levels_dev(context.handle, n, total, _dp(signal), _dp(sig_off), n_ev, _dp(ev_pos),
                                            _dp(start), _dp(length), _dp(level)), 'nvk_event_levels_dev')
    return start[:n_ev], length[:n_ev], level[:n_ev]


def event_align_dev(context, level, ev_off, mu, ac, mc, base_off, l_stay, l_step, status_in, band, trim_cost,
                    skip_cost):
    """The adaptive-banded alignment of every read's events (``level`` / ``ev_off``) to its bases' k-mer levels and
    Gaussian constants (``mu``, ``ac``, ``mc`` / ``base_off``), nvk_event_align_dev.  Device tensors; ``l_stay`` /
    ``l_step``: f64 per read; ``status_in``: int32 per read or None.
    -> (hit int32 (n, 4): status, events, first event, last event; score f64 (n,); base_event int32 (bases,))."""
    import torch
    lib = _lib.load()
    dev = ev_off.device
    n, n_ev, n_base = int(ev_off.numel()) - 1, int(level.numel()), int(mu.numel())
    hit = torch.zeros((max(n, 0), 4), dtype=torch.int32, device=dev)
    score = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
    base_event = torch.zeros(max(n_base, 1), dtype=torch.int32, device=dev)
    _lib.check(lib.nvk_event_align_dev(context.handle, n, n_ev, _dp(_one(level)), _dp(ev_off), n_base, _dp(_one(mu)),
                                       _dp(_one(ac)), _dp(_one(mc)), _dp(base_off), _dp(_one(l_stay)),
                                       _dp(_one(l_step)), _opt(status_in, n), int(band), float(trim_cost),
                                       float(skip_cost), _dp(hit), _dp(score), _dp(base_event)), 'nvk_event_align_dev')
    return hit, score[:n], base_event[:n_base]


# ---- signal_locate_batch: the dense subsequence alignment (include/nadavca_hip.h) -----------------------------
def signal_locate_dev(context, level, q_off, mu, ac, mc, col_off, max_events, l_stay, l_step, l_skip, trim_cost):
    """Every query's events (``level`` / ``q_off``, rescaled) against every column of every target (``mu``, ``ac``,
    ``mc`` / ``col_off``), nvk_signal_locate_dev.  Device tensors.  -> (score f64 (queries, blocks), hit int32
    (queries, blocks, 4): end column, last event, start column, first event), the blocks of 256 columns numbered over
    all targets."""
    import torch
    lib = _lib.load()
    dev = q_off.device
    nq, nt = int(q_off.numel()) - 1, int(col_off.numel()) - 1
    n_ev, n_col = int(level.numel()), int(mu.numel())
    lens = col_off[1:] - col_off[:-1]
    n_blocks = int(((lens + (_lib.LOC_BLOCK - 1)) // _lib.LOC_BLOCK).sum()) if nt > 0 else 0
    score = torch.zeros((max(nq, 0), n_blocks), dtype=torch.float64, device=dev)
    hit = torch.zeros((max(nq, 0), n_blocks, 4), dtype=torch.int32, device=dev)
    _lib.check(lib.nvk_signal_locate_dev(context.handle, nq, n_ev, _dp(_one(level)), _dp(q_off), nt, n_col,
                                         _dp(_one(mu)), _dp(_one(ac)), _dp(_one(mc)), _dp(col_off), int(max_events),
                                         float(l_stay), float(l_step), float(l_skip), float(trim_cost), n_blocks,
                                         _dp(_one(score)), _dp(_one(hit))), 'nvk_signal_locate_dev')
    return score, hit


# ---- decode_batch: the k-mer HMM Viterbi decode (include/nadavca_hip.h) ---------------------------------------
def viterbi_decode_dev(context, level, ev_off, k, central, mean, ac, mc, l_stay, l_step, l_skip, status_in, cap_off):
    """The best path of every read's events (``level`` / ``ev_off``, rescaled) over the 4^k states of the table
    (``mean``, ``ac``, ``mc``), nvk_viterbi_decode_dev.  Device tensors; ``status_in``: int32 per read or None;
    ``cap_off``: int64 (n + 1), where each read's bases are written (k + 2 (E - 1) entries at least).
    -> (hit int32 (n, 4): status, events, bases, end state; score f64 (n,); seq int32 and base_event int32, both laid
    out by ``cap_off``; the number of parts the traceback store was cut into)."""
    import torch
    lib = _lib.load()
    dev = ev_off.device
    n, n_ev = int(ev_off.numel()) - 1, int(level.numel())
    total_cap = int(cap_off[-1]) if n > 0 else 0
    hit = torch.zeros((max(n, 0), 4), dtype=torch.int32, device=dev)
    score = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
    seq = torch.zeros(max(total_cap, 1), dtype=torch.int32, device=dev)
    base_event = torch.zeros(max(total_cap, 1), dtype=torch.int32, device=dev)
    parts = C.c_int64(0)
    _lib.check(lib.nvk_viterbi_decode_dev(context.handle, n, n_ev, _dp(_one(level)), _dp(ev_off), int(k),
                                          int(central), _dp(mean), _dp(ac), _dp(mc), float(l_stay), float(l_step),
                                          float(l_skip), _opt(status_in, n), total_cap, _dp(cap_off), _dp(hit),
                                          _dp(score), _dp(seq), _dp(base_event), C.byref(parts)),
               'nvk_viterbi_decode_dev')
    return hit, score[:n], seq[:total_cap], base_event[:total_cap], int(parts.value)


def _kmer_sweeps_dev(entry, context, level, ev_off, k, mean, ac, mc, weights, status_in, out, n_ms, pos=None):
    """One of the three operators on the k-mer forward-backward (``entry``: its symbol; ``out``: its own output tensor,
    zeroed; ``n_ms``: how many launches it times; ``pos``: the posterior entry's)
    -> (z (n, 2), status (n,), parts, ms)"""
    import torch
    lib = _lib.load()
    dev = ev_off.device
    n, n_ev = int(ev_off.numel()) - 1, int(level.numel())
    z = torch.zeros((max(n, 1), 2), dtype=torch.float64, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    parts, ms = C.c_int64(0), (C.c_double * n_ms)()
    _lib.check(getattr(lib, entry)(context.handle, n, n_ev, _dp(_one(level)), _dp(ev_off), int(k),
                                   *(() if pos is None else (int(pos),)), _dp(mean), _dp(ac), _dp(mc),
                                   *(float(w) for w in weights), _opt(status_in, n), _dp(out), _dp(z), _dp(status),
                                   C.byref(parts), C.cast(ms, C.POINTER(C.c_double)) if n_ms else None), entry)
    return z[:n], status[:n], int(parts.value), tuple(float(t) for t in ms)


def kmer_posterior_dev(context, level, ev_off, k, pos, mean, ac, mc, w_stay, w_step, w_skip, status_in, timing=False):
    """The forward-backward sums of every read's events (``level`` / ``ev_off``, rescaled) over the 4^k states of the
    table (``mean``, ``ac``, ``mc``), nvk_kmer_posterior_dev.  Device tensors; ``pos``: the letter position of the state
    the marginals are taken over (first base = 0); ``w_stay`` / ``w_step`` / ``w_skip``: the moves' linear weights;
    ``status_in``: int32 per read or None.
    -> (marg f64 (events, 4): per event the posterior of each letter at ``pos``; z f64 (n, 2): the scaled sum of the
    last forward row and its binary exponent, log Z = log(z[:, 0]) + z[:, 1] ln 2; status int32 (n,); the number of
    parts the row store was cut into) and, with ``timing``, the milliseconds of the forward and backward launches."""
    import torch
    n_ev = int(level.numel())
    marg = torch.zeros((max(n_ev, 1), 4), dtype=torch.float64, device=ev_off.device)
    z, status, parts, ms = _kmer_sweeps_dev('nvk_kmer_posterior_dev', context, level, ev_off, k, mean, ac, mc,
                                            (w_stay, w_step, w_skip), status_in, marg, 2 * bool(timing), pos)
    out = (marg[:n_ev], z, status, parts)
    return out + (ms,) if timing else out


def kmer_expectations_dev(context, level, ev_off, k, mean, ac, mc, w_stay, w_step, w_skip, status_in, timing=False):
    """The E-step of a Baum-Welch fit on every read's events, nvk_kmer_expectations_dev: the arguments of
    ``kmer_posterior_dev`` without ``pos``.
    -> (stats f64 (n, 10): per read M0, Mx, Mxx, Mm, Mxm, Mmm (the posterior-weighted moments of the levels x against the
    states' means, each term times the state's mc), N_stay, N_step, N_skip (the expected moves) and the number of events
    whose every emission sits on the floor; a read that is not processed has zeros; z and status as
    ``kmer_posterior_dev``'s, z bit for bit; the number of parts) and, with ``timing``, the milliseconds of the forward
    and counts launches."""
    import torch
    n = int(ev_off.numel()) - 1
    stats = torch.zeros((max(n, 1), 10), dtype=torch.float64, device=ev_off.device)
    z, status, parts, ms = _kmer_sweeps_dev('nvk_kmer_expectations_dev', context, level, ev_off, k, mean, ac, mc,
                                            (w_stay, w_step, w_skip), status_in, stats, 2 * bool(timing))
    out = (stats[:n], z, status, parts)
    return out + (ms,) if timing else out


def kmer_state_moments_dev(context, level, ev_off, k, mean, ac, mc, w_stay, w_step, w_skip, status_in, timing=False):
    """The per-state E-step of a Baum-Welch re-estimation of the table, nvk_kmer_state_moments_dev: the arguments of
    ``kmer_expectations_dev``.
    -> (moments f64 (3, 4^k): per state the posterior weight G0 of the batch's events, G1 = SUM g x and G2 = SUM g x^2
    over them, the reads that were processed summed in ascending order; z and status as ``kmer_posterior_dev``'s, z bit
    for bit; the number of parts) and, with ``timing``, the milliseconds of the forward, moments and reduce launches."""
    import torch
    moments = torch.zeros((3, 4 ** int(k)), dtype=torch.float64, device=ev_off.device)
    z, status, parts, ms = _kmer_sweeps_dev('nvk_kmer_state_moments_dev', context, level, ev_off, k, mean, ac, mc,
                                            (w_stay, w_step, w_skip), status_in, moments, 3 * bool(timing))
    out = (moments, z, status, parts)
    return out + (ms,) if timing else out


# ---- count_repeats_batch: the Viterbi path over a chain with a loop (include/nadavca_hip.h) -------------------
def repeat_count_dev(context, level, items, mu, ac, mc, st_off, chain_par, l_stay, l_step, l_skip, trim_cost,
                     status_in=None, timing=False):
    """Every item's events (``items`` int64 (n, 3): chain, ev_lo, ev_hi into ``level``, rescaled) over its chain of
    states (``mu``, ``ac``, ``mc`` / ``st_off``; ``chain_par`` int32 (chains, 4): lp_from, lp_to, m1, m2),
    nvk_repeat_count_dev.  Device tensors; ``status_in``: int32 per item or None.
    -> (hit int32 (n, 8): status, events, first event, last event, loops, i1, i2, 0; score f64 (n, 4): end value,
    S(last, N-1), v1, v2) and, with ``timing``, the milliseconds of the launches."""
    import torch
    lib = _lib.load()
    dev = st_off.device
    n, n_chains = int(items.shape[0]), int(st_off.numel()) - 1
    hit = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    score = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    ms = C.c_double(0.0)
    _lib.check(lib.nvk_repeat_count_dev(context.handle, n, _dp(_one(items.reshape(-1))), int(level.numel()),
                                        _dp(_one(level)), n_chains, int(mu.numel()), _dp(_one(mu)), _dp(_one(ac)),
                                        _dp(_one(mc)), _dp(st_off), _dp(_one(chain_par.reshape(-1))), float(l_stay),
                                        float(l_step), float(l_skip), float(trim_cost), _opt(status_in, n),
                                        _dp(_one(hit.reshape(-1))), _dp(_one(score.reshape(-1))),
                                        C.byref(ms) if timing else None), 'nvk_repeat_count_dev')
    return (hit, score, float(ms.value)) if timing else (hit, score)


def repeat_likelihoods_dev(context, level, items, mu, ac, mc, st_off, chain_par, w_stay, w_step, w_skip, w_trim, layers,
                           status_in=None, timing=False):
    """The likelihood of every item's events summed over the paths that go round its chain's loop exactly c times, for
    c = 0 .. ``layers`` - 1, nvk_repeat_likelihoods_dev: the arguments of ``repeat_count_dev`` with the moves' and the
    trim's linear weights (the numbers whose logs that call takes).
    -> (z f64 (n, layers), x f64 (n,): log L(loops = c) = log(z[:, c]) + x ln 2; status int32 (n,)) and, with
    ``timing``, the milliseconds of the launches."""
    import torch
    lib = _lib.load()
    dev = st_off.device
    n, n_chains, layers = int(items.shape[0]), int(st_off.numel()) - 1, int(layers)
    z = torch.zeros((n, max(layers, 1)), dtype=torch.float64, device=dev)
    x = torch.zeros(n, dtype=torch.float64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ms = C.c_double(0.0)
    _lib.check(lib.nvk_repeat_likelihoods_dev(context.handle, n, _dp(_one(items.reshape(-1))), int(level.numel()),
                                              _dp(_one(level)), n_chains, int(mu.numel()), _dp(_one(mu)),
                                              _dp(_one(ac)), _dp(_one(mc)), _dp(st_off),
                                              _dp(_one(chain_par.reshape(-1))), float(w_stay), float(w_step),
                                              float(w_skip), float(w_trim), layers, _opt(status_in, n),
                                              _dp(_one(z.reshape(-1))), _dp(_one(x)), _dp(_one(status)),
                                              C.byref(ms) if timing else None), 'nvk_repeat_likelihoods_dev')
    return (z, x, status, float(ms.value)) if timing else (z, x, status)
