"""What the batch workflows over a ``ReadBatch`` share (``align_signal_batch``, ``estimate_snps_batch``,
``detect_meth_batch``, ``estimate_kmer_model``): loading of their arguments, the device stage in front of the kernels
(``device_stage``: upload, normalise, approximate alignment, windows), the alignment on top of it (``align_batch``),
the likelihood rows of the SNP-style workflows (``likelihood_rows``), the closing step of the workflows that score
listed hypotheses on an alignment (``hypothesis_rows``), the one policy for per-read kernel status (``check_status``)
and the segment index of flat layouts (``seg_index``)."""
import os
import sys

import numpy as np
import yaml

from . import _lib


def load_config(config):
    """A loaded configuration passes through; a path is read as YAML."""
    if isinstance(config, (str, os.PathLike)):
        with open(config, 'r') as file:
            return yaml.safe_load(file)
    return config


def load_kmer_model(kmer_model):
    """A KmerModel passes through; a path goes to ``KmerModel.load_from_hdf5``."""
    if isinstance(kmer_model, (str, os.PathLike)):
        from .kmer_model import KmerModel
        return KmerModel.load_from_hdf5(os.fspath(kmer_model))
    return kmer_model


def seg_index(off, total=None):
    """Segments laid end to end, segment s at [off[s], off[s+1]) (int64 tensor, any device) -> (owner, inner): the
    segment of every flat position 0..off[-1] and the position inside it.  ``total``: off[-1] where the caller holds
    it as a Python int; without it the value is read from ``off``, which on a GPU waits for the device (as
    repeat_interleave itself would without ``output_size``)."""
    import torch
    if total is None:
        total = int(off[-1])
    segments = torch.arange(off.numel() - 1, dtype=torch.int64, device=off.device)
    owner = torch.repeat_interleave(segments, off[1:] - off[:-1], output_size=total)
    inner = torch.arange(total, dtype=torch.int64, device=off.device) - off[:-1][owner]
    return owner, inner


def check_status(what, status, index=None, too_wide='raise'):
    """Per-read failures of a batch kernel.  ``status``: NVK_READ_* codes, numpy array or torch tensor; ``index``: the
    reads' names in messages (the batch forms pass ``live``; default: their positions).  Invalid input raises
    ValueError naming the first 8 such reads.  A band wider than the compiled kernels serve (READ_TOO_WIDE: a limit of
    this build, not bad input) follows ``too_wide``: 'raise' -> NadavcaHipError, as the per-read operators raise;
    'skip' -> a note on stderr, the read stays in ``status`` like one without a path (the batch workflows); 'invalid'
    -> invalid input like the rest, codes not shown (ProbabilityEstimator.refine_and_renormalize, which always did)."""
    if not bool((status < 0).any()):
        return
    host = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    status = host(status)
    named = lambda rows: (rows if index is None else host(index)[rows]).tolist()
    wide = status == _lib.READ_TOO_WIDE
    if too_wide == 'invalid':
        raise ValueError('%s: invalid input for read(s) %s' % (what, named(np.nonzero(status < 0)[0][:8])))
    bad = np.nonzero((status < 0) & ~wide)[0][:8]
    if bad.size:
        raise ValueError('%s: invalid input for read(s) %s (status %s)' % (what, named(bad), status[bad].tolist()))
    first = named(np.nonzero(wide)[0][:8])
    if too_wide == 'skip':
        sys.stderr.write('%s: %d read(s) skipped, band wider than the compiled kernels serve (first: %s)\n'
                         % (what, int(wide.sum()), first))
        return
    raise _lib.NadavcaHipError('%s: the band of read(s) %s is wider than the compiled kernels serve '
                               '(INTEGRATION.md, limits)' % (what, first))


class DeviceStage:
    """What ``device_stage`` leaves on the device.  ``norm``: the normalised signals of all reads (f64, layout of
    ``raw_signal``); ``group_off``: the offsets of the groups they were normalised in ('read': the reads' ``sig_off``;
    'pooled': [0, total]; 'ranks': None); ``sa``: the readbatch.SignalAlignmentBatch; ``n_live``: the reads with an
    anchor; ``dbatch``: their windows as a device.DeviceBatch (None when ``n_live == 0``); ``reference``: what ``sa``
    was made against, base codes or a refset.ReferenceSet."""
    __slots__ = ('norm', 'group_off', 'sa', 'n_live', 'dbatch', 'reference')

    def contig_names(self):
        """The contigs' names where ``reference`` is a ReferenceSet (the batch results' ``contig_names``), else None."""
        from .refset import ReferenceSet
        return list(self.reference.names) if isinstance(self.reference, ReferenceSet) else None


def device_stage(read_batch, reference_num, config, kmer_model, aligner, mode, group=None):
    """The raw signals of ``read_batch`` to the device in their own dtype, widened and normalised there in place —
    ``mode`` 'read': per read (align_signal.py:54); 'pooled': one median / MAD over all reads (estimate_snps.py:61);
    'ranks': the same over the shards of all ranks of ``group`` — then the approximate-alignment stage
    (``get_base_alignments``, ``signal_alignments`` against ``reference_num``, or against the aligner's
    ``reference_set`` when it has one: its pairs are contig-local then) and the windows.  -> DeviceStage."""
    import torch
    from . import readbatch
    from .device import DeviceBatch, normalize_groups_dev
    context = kmer_model.context
    device = torch.device('cuda', context.device)
    rb, st = read_batch, DeviceStage()
    raw = torch.from_numpy(rb.raw_signal).to(device)
    if raw.dtype != torch.float64:
        raw = raw.to(torch.float64)
    total = int(rb.sig_off[-1])
    st.group_off = None
    if mode in ('read', 'pooled'):
        st.group_off = (torch.from_numpy(rb.sig_off).to(device) if mode == 'read'
                        else torch.tensor([0, total], dtype=torch.int64, device=device))
        st.norm, _ = normalize_groups_dev(context, raw, st.group_off, out=raw)
    elif mode == 'ranks':
        from . import distributed as D
        from .device import select_hist_dev, normalize_apply_dev
        # exact distributed median and MAD (256 counts per pass cross ranks)
        centre, scale = D.pooled_centre_scale(select_hist_dev(context, raw), total, device=device, group=group)
        st.norm = normalize_apply_dev(context, raw, centre, scale, out=raw)
    else:
        raise ValueError("device_stage: mode 'read', 'pooled' or 'ranks'")
    ba = aligner.get_base_alignments(rb)
    st.reference = reference_num
    if getattr(aligner, 'reference_set', None) is not None:
        st.reference = aligner.reference_set
    st.sa = readbatch.signal_alignments(rb, ba, config['bandwidth'], st.reference, kmer_model.get_k(),
                                        kmer_model.get_central_position(), device=device)
    st.n_live = int(st.sa.live.numel())
    st.dbatch = DeviceBatch.from_windows(st.norm, st.sa, device) if st.n_live else None
    return st


def likelihood_rows(stage, config, kmer_model, fit_workers=0, spline_fit='device'):
    """What ``estimate_snps_batch`` and ``estimate_allele_fractions_batch`` run on a 'pooled' (or 'ranks') stage with
    live reads: the spline tweak of the signal normalisation when ``config`` asks for it, then the per-read
    log-likelihood rows, a band wider than the kernels serve skipped (``check_status``).
    -> (ll f64 (sum R, alphabet), status int32 (n_live,), reads the tweak fitted or None): device tensors."""
    from .device import estimate_log_likelihoods_dev
    fitted = None
    if config['tweak_signal_normalization']:
        from .splinefit import tweak_signal_normalization
        fitted = tweak_signal_normalization(kmer_model.context, kmer_model, stage.dbatch, config, fit_workers,
                                            spline_fit)
    ll, status = estimate_log_likelihoods_dev(stage.dbatch, config['bandwidth'], config['min_event_length'],
                                              kmer_model, config['model_wobbling'])
    check_status('estimate_log_likelihoods', status, stage.sa.live, too_wide='skip')
    return ll, status, fitted


def hypothesis_rows(what, res, status, owner):
    """What ``call_mods_batch`` and ``call_indels_batch`` do once operator ``what`` has scored their hypotheses on the
    BatchAlignment ``res``.  ``status``: the operator's per live read; ``owner``: the live read of every hypothesis
    (device tensors).  A read that did not align keeps the alignment's status, a band wider than the kernels serve is
    skipped (``check_status``).  -> (status int32 (n_live,) device tensor, live as a numpy array, mask of the
    hypotheses whose read is READ_OK)."""
    import torch
    status = torch.where(res.status != _lib.READ_OK, res.status, status)
    check_status(what, status, res.stage.sa.live, too_wide='skip')
    return status, res.stage.sa.live.cpu().numpy(), (status == _lib.READ_OK)[owner]


class BatchAlignment:
    """What ``align_batch`` returns.  ``stage``: the DeviceStage (``stage.dbatch.signal`` rescaled by every fit,
    ``stage.norm`` NOT rescaled); ``events`` / ``status``: the final events and per-read status of the live reads,
    device tensors (None when ``stage.n_live == 0``); ``fits``: the linear fits, one (n_live, 2) tensor per re-fit."""
    __slots__ = ('stage', 'events', 'status', 'fits')

    def __init__(self, stage, events=None, status=None, fits=()):
        self.stage, self.events, self.status, self.fits = stage, events, status, list(fits)


def align_batch(read_batch, config, kmer_model, renorm_rounds, aligner):
    """The device half of ``align_signal_batch``, which ``detect_meth_batch`` and ``estimate_kmer_model`` build on
    too: the stage with per-read normalisation, then the renormalise / re-align loop.  ``config`` loaded,
    ``kmer_model`` a KmerModel.  -> BatchAlignment."""
    from .device import refine_renorm_loop_dev
    if aligner is None:
        raise ValueError('align_signal_batch needs a batch aligner (BWA has no batch adapter offline)')
    stage = device_stage(read_batch, aligner.reference_num, config, kmer_model, aligner, 'read')
    if stage.n_live == 0:
        return BatchAlignment(stage)
    events, status, fits = refine_renorm_loop_dev(stage.dbatch, config['bandwidth'], config['min_event_length'],
                                                  kmer_model, config['model_transitions'], renorm_rounds)
    check_status('refine_alignment', status, stage.sa.live, too_wide='skip')
    return BatchAlignment(stage, events, status, fits)
