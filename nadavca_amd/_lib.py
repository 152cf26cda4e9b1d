"""ctypes binding of nadavca_amd/csrc/libnadavca_hip.so (ABI: include/nadavca_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C nadavca_amd/csrc``.
There is no fallback: a missing library or a missing GPU raises.
"""
import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libnadavca_hip.so')

NVK_OK = 0
NVK_ERR_NO_DEVICE = -1
NVK_ERR_INVALID = -2
NVK_ERR_HIP = -3
NVK_ERR_UNSUPPORTED = -4
NVK_ERR_NOMEM = -5

READ_OK = 0
READ_NO_PATH = 1
READ_BAD_INPUT = -1
READ_BAD_BAND = -2
READ_TOO_WIDE = -3

MAP_OK, MAP_NO_EVENTS, MAP_LOST = 0, 1, 2   # NVK_MAP_*: per-read status of signal_map_batch
LOC_OK, LOC_NO_EVENTS, LOC_AMBIGUOUS = 0, 1, 2   # NVK_LOC_*: per-read status of signal_locate_batch
LOC_BLOCK, LOC_MAX_EVENTS = 256, 256   # NVK_LOC_BLOCK, NVK_LOC_MAX_EVENTS
DEC_OK, DEC_NO_EVENTS = 0, 1   # NVK_DEC_*: per-read status of decode_batch
REP_OK, REP_NO_EVENTS, REP_NO_PATH = 0, 1, 2   # NVK_REP_*: per-item status of count_repeats_batch
REP_MAX_STATES = 256   # NVK_REP_MAX_STATES
REP_MAX_LAYERS = 128   # NVK_REP_MAX_LAYERS

TIE_EXACT = 1   # nvk_last_tie_flags: some path comparison of the read met two exactly equal scores
TIE_NEAR = 2    # ... two scores closer than 2^-24 relative (beyond the class below)
TIE_PLATEAU = 8  # structural mark: two adjacent bases with the same k-mer level (boundary unidentifiable)
TIE_ULP = 4     # ... two scores within 64 ulps of the reference's log value, not equal (where its rounding may decide)

K_PLAN, K_ALIGN, K_ELL_SWEEP, K_ELL_HYP, K_EXPECTED, K_CONSENSUS, K_POSTERIOR, K_RENORM, K_METH, K_SEED, K_KMER, \
    K_ALLELE, K_SITE = range(13)
KERNEL_NAMES = ['plan', 'align', 'ell_sweep', 'ell_hyp', 'expected', 'consensus', 'posterior', 'renorm', 'meth',
                'seed', 'kmer', 'allele', 'site']

_vp = C.c_void_p
_i64 = C.c_int64
_int = C.c_int
_dbl = C.c_double

# what the *_batch_dev operators on a device batch start with: model, n_reads, 3 totals, 10 array pointers, bandwidth,
# min_event_length and the operator's switch
_BATCH_DEV = [_vp, _i64, _i64, _i64, _i64] + [_vp] * 10 + [_int, _int, _int]


def _kmer_sweeps(pos=False):
    """The three operators on the k-mer forward-backward: context, n_reads, total_events, level, ev_off, k (and
    ``pos``), the table, the three weights, status_in, the operator's output, out_z, out_status, out_parts, out_ms"""
    return [_vp, _i64, _i64, _vp, _vp, _int] + [_int] * pos + [_vp] * 3 + [_dbl] * 3 + [_vp] * 4 \
        + [C.POINTER(_i64), C.POINTER(_dbl)]


# every symbol include/nadavca_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    'nvk_last_error': (C.c_char_p, []),
    'nvk_device_count': (_int, []),
    'nvk_ctx_create': (_int, [_int, C.POINTER(_vp)]),
    'nvk_ctx_destroy': (None, [_vp]),
    'nvk_ctx_synchronize': (_int, [_vp]),
    'nvk_ctx_stream': (_vp, [_vp]),
    'nvk_ctx_set_slots': (_int, [_vp, _int]),
    'nvk_timing_enable': (_int, [_vp, _int]),
    'nvk_timing_reset': (_int, [_vp]),
    'nvk_timing_read': (_int, [_vp, _int, C.POINTER(_dbl), C.POINTER(_i64)]),
    'nvk_last_batch_stats': (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    'nvk_last_retry_count': (_int, [_vp, C.POINTER(_i64)]),
    'nvk_last_tie_count': (_int, [_vp, C.POINTER(_i64)]),
    'nvk_last_tie_counts': (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    'nvk_last_tie_flags': (_int, [_vp, _i64, _vp]),
    'nvk_ctx_set_workspace_limit': (_int, [_vp, _i64]),
    'nvk_last_launches': (_int, [_vp, _int, _vp, C.POINTER(_int)]),
    'nvk_last_read_skews': (_int, [_vp, _i64, _vp, _vp]),
    'nvk_built_sweep_variants': (_int, [_int, _vp, C.POINTER(_int)]),
    'nvk_selftest_wave_max': (_int, [_vp, _vp, _i64, _vp]),
    'nvk_model_create': (_int, [_vp, _int, _int, _int, _vp, _vp, _i64, C.POINTER(_vp)]),
    'nvk_model_destroy': (None, [_vp]),
    'nvk_model_info': (_int, [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    'nvk_expected_signal_batch': (_int, [_vp, _i64] + [_vp] * 7),
    'nvk_expected_signal_batch_dev': (_int, [_vp, _i64, _i64] + [_vp] * 7),
    'nvk_refine_alignment_batch': (_int, [_vp, _i64] + [_vp] * 10 + [_int, _int, _int, _vp, _vp]),
    'nvk_refine_alignment_submit': (_int, [_vp, _i64] + [_vp] * 10 + [_int, _int, _int, _vp, _vp, _vp, C.POINTER(_i64)]),
    'nvk_refine_alignment_wait': (_int, [_vp, _i64]),
    'nvk_refine_alignment_batch_dev': (_int, _BATCH_DEV + [_vp, _vp]),
    'nvk_plan_token_new': (C.c_uint64, []),
    'nvk_refine_alignment_batch_dev_keyed': (_int, _BATCH_DEV + [_vp, _vp, C.c_uint64]),
    'nvk_last_plan_reused': (_int, [_vp, C.POINTER(_int)]),
    'nvk_estimate_log_likelihoods_batch': (_int, [_vp, _i64] + [_vp] * 10 + [_int, _int, _int, _vp, _vp]),
    'nvk_estimate_log_likelihoods_batch_dev': (_int, _BATCH_DEV + [_vp, _vp]),
    'nvk_estimate_hypotheses_batch_dev': (_int, _BATCH_DEV + [_i64] + [_vp] * 6),
    'nvk_estimate_joint_hypotheses_batch_dev': (_int, _BATCH_DEV + [_i64, _vp, _i64] + [_vp] * 6),
    'nvk_estimate_edit_hypotheses_batch_dev': (_int, _BATCH_DEV + [_i64, _vp, _vp, _vp, _i64] + [_vp] * 5),
    'nvk_consensus_accumulate_dev': (_int, [_vp, _i64, _i64, _int] + [_vp] * 6 + [_dbl, _i64, _vp, _vp]),
    'nvk_posterior_segments_dev': (_int, [_vp, _i64, _i64, _vp, _int, _int, _dbl, _vp, _vp, _vp]),
    'nvk_normalize_groups_dev': (_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    'nvk_select_hist_dev': (_int, [_vp, _vp, _i64, _int, _dbl, C.c_uint64, _int, _vp]),
    'nvk_normalize_apply_dev': (_int, [_vp, _vp, _i64, _dbl, _dbl, _vp]),
    'nvk_event_means_dev': (_int, [_vp, _i64, _i64] + [_vp] * 6),
    'nvk_linfit_rescale_dev': (_int, [_vp, _i64] + [_vp] * 7),
    'nvk_splev_groups_dev': (_int, [_vp, _i64] + [_vp] * 5 + [_int, _vp]),
    'nvk_spline_fit_dev': (_int, [_vp, _i64, _i64] + [_vp] * 7),
    'nvk_meth_count_dev': (_int, [_vp, _i64, _i64] + [_vp] * 5 + [_i64, _vp]),
    'nvk_meth_scores_dev': (_int, [_vp, _i64, _i64] + [_vp] * 6 + [_i64] + [_vp] * 4),
    'nvk_seed_extend_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp] + [_int] * 6 + [_vp, _vp]),
    'nvk_seed_extend_bounded_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp] + [_int] * 6
                                    + [_vp, _vp]),
    'nvk_seed_chain_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp] + [_int] * 4 + [_i64, _vp, _vp, _vp]),
    'nvk_seed_extend_path_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp] + [_int] * 6
                                 + [_vp, _vp]),
    'nvk_kmer_event_stats_dev': (_int, [_vp, _i64, _i64] + [_vp] * 10 + [_int] * 4 + [_vp] * 4),
    'nvk_kmer_reduce_dev': (_int, [_vp, _i64, _i64] + [_vp] * 6),
    'nvk_mod_kmer_rows_dev': (_int, [_vp, _i64, _i64] + [_vp] * 10 + [_int] * 4 + [_i64, _vp, _vp, _vp, _int, _vp, _i64]
                              + [_vp] * 5),
    'nvk_mod_kmer_reduce_dev': (_int, [_vp, _i64, _i64] + [_vp] * 4),
    'nvk_allele_rows_dev': (_int, [_vp, _i64, _i64, _int] + [_vp] * 6 + [_dbl, _i64, _vp, _vp]),
    'nvk_allele_solve_dev': (_int, [_vp, _i64, _i64, _int] + [_vp] * 8),
    'nvk_phase_links_dev': (_int, [_vp, _i64, _int] + [_vp] * 6 + [_dbl, _vp, _vp]),
    'nvk_phase_tag_dev': (_int, [_vp, _i64, _i64, _int] + [_vp] * 9 + [_dbl, _vp, _vp, _vp]),
    'nvk_phase_votes_dev': (_int, [_vp, _i64, _int] + [_vp] * 9 + [_dbl, _vp, _vp, _vp]),
    'nvk_phase_span_links_dev': (_int, [_vp, _i64, _int, _int] + [_vp] * 6 + [_dbl, _vp, _vp]),
    'nvk_phase_tag_blocks_dev': (_int, [_vp, _i64, _i64, _int] + [_vp] * 9 + [_dbl, _vp, _vp, _vp]),
    'nvk_mod_site_solve_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _int, _vp, _dbl, _vp, _vp, _vp]),
    'nvk_site_level_rows_dev': (_int, [_vp, _i64, _i64] + [_vp] * 8 + [_int, _i64, _vp, _vp]),
    'nvk_site_moments_dev': (_int, [_vp, _i64, _i64, _int] + [_vp] * 5),
    'nvk_site_rank_tests_dev': (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64] + [_vp] * 7),
    'nvk_site_mixture_tests_dev': (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _int, _dbl, _vp, _vp]),
    'nvk_event_flags_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _int, _dbl, _dbl, _vp]),
    'nvk_event_levels_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'nvk_event_align_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _i64] + [_vp] * 7 + [_int, _dbl, _dbl, _vp, _vp, _vp]),
    'nvk_signal_locate_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64] + [_vp] * 4 + [_int] + [_dbl] * 4
                              + [_i64, _vp, _vp]),
    'nvk_viterbi_decode_dev': (_int, [_vp, _i64, _i64, _vp, _vp, _int, _int, _vp, _vp, _vp, _dbl, _dbl, _dbl, _vp, _i64]
                               + [_vp] * 5 + [C.POINTER(_i64)]),
    'nvk_kmer_posterior_dev': (_int, _kmer_sweeps(pos=True)),
    'nvk_kmer_expectations_dev': (_int, _kmer_sweeps()),
    'nvk_kmer_state_moments_dev': (_int, _kmer_sweeps()),
    'nvk_repeat_count_dev': (_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64] + [_vp] * 5 + [_dbl] * 4 + [_vp] * 3
                             + [C.POINTER(_dbl)]),
    'nvk_repeat_likelihoods_dev': (_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64] + [_vp] * 5 + [_dbl] * 4 + [_int]
                                   + [_vp] * 4 + [C.POINTER(_dbl)]),
}

LAUNCH_SWEEP, LAUNCH_EXACT, LAUNCH_ELL = 1, 2, 3   # nvk_launch_rec.op
LAUNCH_OPS = {LAUNCH_SWEEP: 'sweep', LAUNCH_EXACT: 'exact', LAUNCH_ELL: 'ell'}
ELL_KINDS = ['full', 'listed', 'joint', 'edit']       # nvk_launch_rec.kind of an 'ell' record (NVK_ELL_*)
LAUNCH_CAP = 8


class LaunchRec(C.Structure):
    """nvk_launch_rec (include/nadavca_hip.h, launch report)."""
    _fields_ = [(n, C.c_int32) for n in ('op', 'mel', 'transitions', 'waves', 'period', 'kind', 'c', 'H', 'SR',
                                         'lds_bytes')] + [('reads', _i64), ('chunks', _i64)]


_lib = None
_lock = threading.Lock()


class NadavcaHipError(RuntimeError):
    pass


def _torch_runtime_first():
    """PyTorch-ROCm ships its own copy of the HIP runtime; this library links the system one.  Both can
    live in one process only if torch's touches the device first — otherwise the first
    ``tensor.to('cuda')`` after a kernel call of this library fails with "No HIP GPUs are available".
    So torch's runtime is initialised before this library makes its first HIP call (torch is the
    package's plumbing for device memory anyway, nadavca_amd/device.py)."""
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:  # no torch, or no device: this library reports the latter itself
        pass


def load():
    """Load libnadavca_hip.so (once) and attach the prototypes.  Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        _torch_runtime_first()
        if not os.path.isfile(LIB_PATH):
            raise NadavcaHipError(
                'HIP library not built: %s is missing (run __graft_entry__.build() or '
                '`make -C nadavca_amd/csrc`). There is no CPU fallback.' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc, what):
    if rc != NVK_OK:
        lib = load()
        msg = lib.nvk_last_error()
        msg = msg.decode('utf-8', 'replace') if msg else ''
        if rc == NVK_ERR_INVALID:
            raise ValueError('%s: %s' % (what, msg))
        raise NadavcaHipError('%s failed (%d): %s' % (what, rc, msg))


class Context:
    """One per process/GPU: owns the HIP stream, the workspaces and the timers."""

    def __init__(self, device=0):
        lib = load()
        self._lib = lib
        h = _vp()
        check(lib.nvk_ctx_create(int(device), C.byref(h)), 'nvk_ctx_create')
        self.handle = h
        self.device = int(device)
        self.workspace_limit = 0   # what set_workspace_limit was last given (0: the library's default)

    def synchronize(self):
        check(self._lib.nvk_ctx_synchronize(self.handle), 'nvk_ctx_synchronize')

    def set_slots(self, slots):
        check(self._lib.nvk_ctx_set_slots(self.handle, int(slots)), 'nvk_ctx_set_slots')

    def timing_enable(self, on=True):
        check(self._lib.nvk_timing_enable(self.handle, int(bool(on))), 'nvk_timing_enable')

    def timing_reset(self):
        check(self._lib.nvk_timing_reset(self.handle), 'nvk_timing_reset')

    def timing_read(self):
        out = {}
        for kid, name in enumerate(KERNEL_NAMES):
            ms, n = _dbl(), _i64()
            check(self._lib.nvk_timing_read(self.handle, kid, C.byref(ms), C.byref(n)), 'nvk_timing_read')
            out[name] = (ms.value, n.value)
        return out

    def last_batch_stats(self):
        a, b, c = _i64(), _i64(), _i64()
        check(self._lib.nvk_last_batch_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)),
              'nvk_last_batch_stats')
        d = _i64()
        check(self._lib.nvk_last_retry_count(self.handle, C.byref(d)), 'nvk_last_retry_count')
        e = _i64()
        check(self._lib.nvk_last_tie_count(self.handle, C.byref(e)), 'nvk_last_tie_count')
        f, g, h = _i64(), _i64(), _i64()
        check(self._lib.nvk_last_tie_counts(self.handle, C.byref(f), C.byref(g), C.byref(h)), 'nvk_last_tie_counts')
        return dict(band_cells=a.value, wave_steps=b.value, spill_bytes=c.value, reads_redone_exact=d.value,
                    reads_tie_ambiguous=e.value, reads_tie_exact=f.value, reads_tie_near=g.value,
                    reads_tie_ulp=h.value)

    def last_plan_reused(self):
        """Whether the last refine_alignment call on this context swept from the plan an earlier call with the same
        batch token left (include/nadavca_hip.h: plan once, sweep again) and so launched no planner."""
        r = _int()
        check(self._lib.nvk_last_plan_reused(self.handle, C.byref(r)), 'nvk_last_plan_reused')
        return bool(r.value)

    def last_tie_flags(self, n_reads):
        """Per read of the last refine_alignment batch: TIE_EXACT | TIE_NEAR | TIE_ULP where a path comparison fell
        inside the tie margin (include/nadavca_hip.h, parity contract)."""
        import numpy as np
        out = np.zeros(int(n_reads), dtype=np.int32)
        check(self._lib.nvk_last_tie_flags(self.handle, int(n_reads), _vp(out.ctypes.data)), 'nvk_last_tie_flags')
        return out

    def last_launches(self):
        """The launch report of the last device-pointer refine_alignment / log-likelihood call on this context
        (include/nadavca_hip.h): one dict per launch class with op ('sweep' | 'exact' | 'ell'), mel, transitions,
        waves, period, kind (an 'ell' record: 'full' | 'listed' | 'joint' | 'edit'; an 'exact' one: 'retry' | 'all'),
        c, H, SR, lds_bytes, reads, chunks.  Empty after a host-pointer call."""
        recs = (LaunchRec * LAUNCH_CAP)()
        n = _int()
        check(self._lib.nvk_last_launches(self.handle, LAUNCH_CAP, C.cast(recs, _vp), C.byref(n)), 'nvk_last_launches')
        if n.value > LAUNCH_CAP:
            raise NadavcaHipError('nvk_last_launches: %d launch classes, %d kept' % (n.value, LAUNCH_CAP))
        out = []
        for r in recs[:n.value]:
            d = {name: int(getattr(r, name)) for name, _ in LaunchRec._fields_}
            d['op'] = LAUNCH_OPS[d['op']]
            if d['op'] == 'ell':
                d['kind'] = ELL_KINDS[d['kind']]
            elif d['op'] == 'exact':
                d['kind'] = 'retry' if d['kind'] else 'all'
            else:
                d['kind'] = None
            out.append(d)
        return out

    def last_read_skews(self, n_reads):
        """-> (c, cw) int32 arrays: per read of the last device-pointer call that planned reads on this context the
        planner's wavefront skew and, for a read swept by a team of waves, its team skew (else 0)."""
        import numpy as np
        c = np.zeros(int(n_reads), dtype=np.int32)
        cw = np.zeros(int(n_reads), dtype=np.int32)
        check(self._lib.nvk_last_read_skews(self.handle, int(n_reads), _vp(c.ctypes.data), _vp(cw.ctypes.data)),
              'nvk_last_read_skews')
        return c, cw

    def selftest_wave_max(self, rows):
        """nvk_selftest_wave_max: ``rows`` int32 [n, 64] -> int32 [n], what wave_max_i (csrc/wave.h), the function
        behind the sweeps' rescale decision, returns for each row of 64 lanes."""
        import numpy as np
        import torch
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 2 or rows.shape[1] != 64:
            raise ValueError('selftest_wave_max: rows must be [n, 64]')
        dev = torch.device('cuda', self.device)
        d_in = torch.from_numpy(rows).to(dev)
        d_out = torch.zeros(rows.shape[0], dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        check(self._lib.nvk_selftest_wave_max(self.handle, _vp(d_in.data_ptr()), rows.shape[0], _vp(d_out.data_ptr())),
              'nvk_selftest_wave_max')
        return d_out.cpu().numpy()

    def set_workspace_limit(self, nbytes):
        check(self._lib.nvk_ctx_set_workspace_limit(self.handle, int(nbytes)), 'nvk_ctx_set_workspace_limit')
        self.workspace_limit = int(nbytes)

    def close(self):
        if getattr(self, 'handle', None):
            self._lib.nvk_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_token_new():
    """A fresh batch token (nvk_plan_token_new): process-wide, never 0.  Needs no GPU."""
    return int(load().nvk_plan_token_new())


def built_sweep_variants():
    """-> sorted list of (mel, transitions, waves, period): the sweep kernel pairs select_sweeps
    (csrc/kernels_align3.hip) has, as the library itself enumerates them.  Needs no GPU."""
    import numpy as np
    lib = load()
    n = _int()
    check(lib.nvk_built_sweep_variants(0, None, C.byref(n)), 'nvk_built_sweep_variants')
    out = np.zeros((max(n.value, 1), 4), dtype=np.int32)
    check(lib.nvk_built_sweep_variants(n.value, _vp(out.ctypes.data), C.byref(n)), 'nvk_built_sweep_variants')
    return sorted((int(a), bool(b), int(c), int(d)) for a, b, c, d in out[:n.value])


_default_ctx = {}


def default_context(device=None):
    """Process-wide context for ``device`` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get('LOCAL_RANK', '0'))
        lib = load()
        n = lib.nvk_device_count()
        if n > 0:
            device %= n
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
