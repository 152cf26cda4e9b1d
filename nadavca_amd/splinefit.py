"""``Read.tweak_signal_normalization`` (/root/reference/nadavca/read.py:83-94) for many reads.

The FIT on the host, with scipy: per read, keep the events whose mean lies within 1 of the model's expected level,
sort the pairs by mean and fit FITPACK's smoothing spline (``scipy.interpolate.splrep(means, expected,
s=len(means))``).  Since round 3 the batch path fits on the device (``nvk_spline_fit_dev``, csrc/splfit.h: under that
filter and that ``s`` FITPACK never gets past its first trial, the least-squares cubic); the host fit is what serves a
read the kernel reports as outside that case, the per-read ``Read.tweak_signal_normalization``, and
``estimate_snps_batch(spline_fit='host')`` — the cross-check of the kernel (~0.25 ms per read; the reads are
independent, so the fits are spread over worker processes: scipy holds the GIL inside the call).  At the end, the
whole step for a device.DeviceBatch (``tweak_signal_normalization``) and the one place that applies splines to it."""
import numpy as np


def fit_one(observed, levels):
    """-> (t, c) of the cubic smoothing spline, or None when fewer than 4 usable events remain."""
    from scipy import interpolate
    with np.errstate(invalid='ignore'):
        keep = np.abs(levels - observed) <= 1      # an empty event has mean NaN and drops out
    xs, ys = observed[keep], levels[keep]
    if xs.size < 4:
        return None
    order = np.lexsort((ys, xs))
    t, c, _ = interpolate.splrep(xs[order], ys[order], s=len(xs))
    return t, c[:len(t)]


def _fit_chunk(args):
    means, expected, off = args
    return [fit_one(means[off[j]:off[j + 1]], expected[off[j]:off[j + 1]]) for j in range(len(off) - 1)]


_POOL = {}


def _pool(workers):
    """A process pool started with ``spawn`` (the parent holds a HIP context: never fork it); kept for the life
    of the process, the workers import numpy and scipy only."""
    if workers not in _POOL:
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        _POOL[workers] = ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context('spawn'))
    return _POOL[workers]


class FitHandle:
    """Fits of one set of reads under way (``submit_fits``); ``result()`` -> (t, c, knot_off, fitted) as
    ``fit_splines`` returns them."""

    def __init__(self, n, jobs, futures, local, means, expected, ref_off, workers):
        self.n, self.jobs, self.futures, self.local = n, jobs, futures, local
        self._retry = (means, expected, ref_off, workers)

    def result(self):
        results = [None] * self.n
        try:
            for (part, _), fut in zip(self.jobs, self.futures):
                for j, r in zip(part, fut.result()):
                    results[j] = r
        except Exception as exc:   # e.g. a main module the workers cannot import (interactive session)
            import sys
            means, expected, ref_off, workers = self._retry
            sys.stderr.write('nadavca_amd.splinefit: worker pool unusable (%s); fitting in this process\n' % exc)
            bad = _POOL.pop(workers, None)
            if bad is not None:
                bad.shutdown(wait=False, cancel_futures=True)
            for part, _ in self.jobs:
                for j in part:
                    results[j] = fit_one(means[ref_off[j]:ref_off[j + 1]], expected[ref_off[j]:ref_off[j + 1]])
        for j in self.local:
            means, expected, ref_off, _ = self._retry
            results[j] = fit_one(means[ref_off[j]:ref_off[j + 1]], expected[ref_off[j]:ref_off[j + 1]])
        return pack_results(results)


def pack_results(results):
    """per-read (t, c) or None -> (t, c, knot_off, fitted) laid end to end"""
    fitted = np.array([r is not None for r in results], dtype=bool)
    lens = np.array([len(r[0]) if r is not None else 0 for r in results], dtype=np.int64)
    knot_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    t = np.concatenate([r[0] for r in results if r is not None]) if fitted.any() else np.zeros(0)
    c = np.concatenate([r[1] for r in results if r is not None]) if fitted.any() else np.zeros(0)
    return t, c, knot_off, fitted


def merge_host_fits(means, expected, ref_off, t8, c8, fit):
    """The device's fits (t8, c8: (n, 8); fit: 0 fitted, 1 no fit, 2 outside the kernel's case) with the reads of
    class 2 fitted here by FITPACK -> (t, c, knot_off, fitted) as ``fit_splines`` returns them."""
    results = []
    for j in range(len(fit)):
        if fit[j] == 0:
            results.append((t8[j], c8[j]))
        elif fit[j] == 1:
            results.append(None)
        else:
            results.append(fit_one(means[ref_off[j]:ref_off[j + 1]], expected[ref_off[j]:ref_off[j + 1]]))
    return pack_results(results)


def submit_fits(means, expected, ref_off, usable, workers=0):
    """Start the fits of the usable reads and return at once: -> FitHandle.  With ``workers`` > 1 the reads go to
    the worker processes in runs (the caller goes on — e.g. launches the kernels of the previous chunk of reads —
    and collects with ``result()``); otherwise they are fitted in this process when ``result()`` is called."""
    n = len(ref_off) - 1
    idx = np.nonzero(usable)[0]
    if not (workers and workers > 1 and idx.size >= 4 * workers):
        return FitHandle(n, [], [], list(idx), means, expected, ref_off, workers)
    parts = np.array_split(idx, workers * 2)
    jobs = []
    for part in parts:
        if part.size == 0:
            continue
        lo, hi = int(ref_off[part[0]]), int(ref_off[part[-1] + 1])    # contiguous range covering the part
        off = np.concatenate([[ref_off[j] - lo for j in part], [ref_off[part[-1] + 1] - lo]])
        # (parts are runs of consecutive usable reads only where nothing in between is unusable; otherwise
        # cut per read)
        if np.array_equal(part, np.arange(part[0], part[-1] + 1)):
            jobs.append((part, (means[lo:hi], expected[lo:hi], off)))
        else:
            for j in part:
                a, b = int(ref_off[j]), int(ref_off[j + 1])
                jobs.append((np.array([j]), (means[a:b], expected[a:b], np.array([0, b - a]))))
    try:
        pool = _pool(workers)
        futures = [pool.submit(_fit_chunk, j[1]) for j in jobs]
    except Exception:
        return FitHandle(n, [], [], list(idx), means, expected, ref_off, workers)
    return FitHandle(n, jobs, futures, [], means, expected, ref_off, workers)


def fit_splines(means, expected, ref_off, usable, workers=0):
    """means / expected: f64 (sum R,) per-event means and expected levels of all reads end to end, read j at
    [ref_off[j], ref_off[j+1]); usable bool (n,): reads to fit.  -> (t, c, knot_off, fitted bool (n,)): knots
    and coefficients of the fitted reads end to end (read j's at [knot_off[j], knot_off[j+1]), empty when not
    fitted).  ``workers`` > 1: that many processes."""
    return submit_fits(means, expected, ref_off, usable, workers).result()


def apply_splines_dev(context, dbatch, t, c, knot_off, unfitted):
    """``signal = splev(signal, spline of its read)`` in place on ``dbatch.signal`` (read.py:94; the kernel restates
    FITPACK's evaluation).  Device tensors: read j's knots and coefficients at [knot_off[j], knot_off[j+1]) of ``t``
    and ``c`` — a valid spline for EVERY read, a placeholder where ``unfitted[j]`` (bool): those reads keep their
    samples (the reference would fail on them), saved before the kernel and put back after it."""
    import torch
    from .device import splev_groups_dev
    keep = saved = None
    if bool(unfitted.any()):
        keep = torch.repeat_interleave(unfitted, dbatch.sig_off[1:] - dbatch.sig_off[:-1],
                                       output_size=dbatch.total_signal)
        saved = dbatch.signal[keep]
    splev_groups_dev(context, dbatch.signal, dbatch.sig_off, t, c, knot_off, 3, out=dbatch.signal)
    if keep is not None:
        dbatch.signal[keep] = saved


def apply_host_fits(context, dbatch, fits):
    """``apply_splines_dev`` for fits made on the host (``fits`` as ``fit_splines`` returns them): uploaded with the
    identity on [-5, 5] as the placeholder of the reads without a fit."""
    import torch
    t, c, knot_off, fitted = fits
    ident = np.array([-5.0] * 4 + [5.0] * 4), np.array([-5.0, -5.0 / 3, 5.0 / 3, 5.0, 0.0, 0.0, 0.0, 0.0])
    parts = [(t[a:b], c[a:b]) if f else ident for a, b, f in zip(knot_off, knot_off[1:], fitted)]
    koff2 = np.cumsum([0] + [len(p[0]) for p in parts], dtype=np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dbatch.device)
    apply_splines_dev(context, dbatch, up(np.concatenate([p[0] for p in parts])),
                      up(np.concatenate([p[1] for p in parts])), up(koff2), up(~fitted))


def tweak_signal_normalization(context, kmer_model, dbatch, config, fit_workers=0, spline_fit='device'):
    """``Read.tweak_signal_normalization`` (read.py:83-94) for the batch, in place on its signal: pre-alignment
    without transition rows, expected levels, per-event means, the fit, the evaluation — five kernels, nothing on
    the host (``spline_fit='device'``: nvk_spline_fit_dev restates the pass of FITPACK's ``curfit`` that decides
    these fits and checks per read that it does).  A read the kernel reports as outside that case (fit == 2: NaN
    levels, all means equal) is fitted by FITPACK itself, as is everything with ``spline_fit='host'`` (scipy in
    ``fit_workers`` processes — the path of rounds 1-2, kept as the cross-check of the kernel).
    -> number of reads fitted."""
    import torch
    from .device import refine_alignment_dev, expected_levels_dev, event_means_dev, spline_fit_dev
    bw, mel = config['bandwidth'], config['min_event_length']
    ev0, st0 = refine_alignment_dev(dbatch, bw, mel, kmer_model, False)
    expected = expected_levels_dev(dbatch, kmer_model, with_contexts=True)
    means = event_means_dev(dbatch, context, ev0, st0)
    if spline_fit == 'device':
        t, c, fit = spline_fit_dev(context, means, expected, dbatch.ref_off, st0)
        if not bool((fit == 2).any()):
            # the splines as the kernel left them: 8 knots + 8 coefficients per read, placeholders included
            knot_off = torch.arange(dbatch.n + 1, dtype=torch.int64, device=dbatch.device) * 8
            apply_splines_dev(context, dbatch, t.reshape(-1), c.reshape(-1), knot_off, fit != 0)
            return int((fit == 0).sum())
        fits = merge_host_fits(means.cpu().numpy(), expected.cpu().numpy(), dbatch.ref_off.cpu().numpy(),
                               t.cpu().numpy(), c.cpu().numpy(), fit.cpu().numpy())
    elif spline_fit == 'host':
        fits = fit_splines(means.cpu().numpy(), expected.cpu().numpy(), dbatch.ref_off.cpu().numpy(),
                           st0.cpu().numpy() == 0, workers=fit_workers)
    else:
        raise ValueError("spline_fit: 'device' or 'host'")
    apply_host_fits(context, dbatch, fits)
    return int(fits[3].sum())
