"""The kernels of ``signal_map_batch`` against their CPU restatements (tests/host_shims/events_host.cpp,
eventalign_host.cpp, which tests/test_signal_map_cpu.py holds to plain Python), bit for bit: every integer, every f64
level and score, both band widths — on the constructed cases of tests/signal_map_ref.py and on the 300-read batch of
the quality tests; a run under a workspace cap that cuts the batch against the uncut one; bad arguments."""
import ctypes as C
import math

import numpy as np
import pytest

import signal_map_ref as R

pytestmark = pytest.mark.gpu
TRIM, SKIP = math.log(0.01), math.log(1e-10)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp('signal_map'))


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def dev(a, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to('cuda')


def same(a, b):
    """bit for bit (NaN and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('case', R.detector_cases(), ids=lambda c: c[0])
def test_detector_kernels_equal_the_restatement(host, ctx, case):
    from nadavca_amd import device
    _, signal, sig_off, w, threshold, var_floor = case
    x, off = dev(signal, np.float64), dev(sig_off, np.int64)
    flags = device.event_flags_dev(ctx, x, off, w, threshold, var_floor)
    want = host.flags(signal, sig_off, w, threshold, var_floor)
    assert same(flags.cpu().numpy(), want)
    ev_pos = np.nonzero(want)[0].astype(np.int64)
    got = device.event_levels_dev(ctx, x, off, dev(ev_pos))
    for g, e in zip(got, host.levels(signal, sig_off, ev_pos)):
        assert same(g.cpu().numpy(), e)


def gpu_align(ctx, packed, band, trim, skip, status_in=None):
    from nadavca_amd import device
    d = {k: dev(v) for k, v in packed.items()}
    st = None if status_in is None else dev(status_in, np.int32)
    hit, score, be = device.event_align_dev(ctx, d['level'], d['ev_off'], d['mu'], d['ac'], d['mc'], d['base_off'],
                                            d['l_stay'], d['l_step'], st, band, trim, skip)
    return hit.cpu().numpy(), score.cpu().numpy(), be.cpu().numpy()


@pytest.mark.parametrize('band', [64, 128])
def test_alignment_kernel_equals_the_restatement_on_the_small_cases(host, ctx, band):
    named = R.small_align_cases()
    for grid in (False, True):
        packed = R.pack_align_cases([c for name, c in named if name.startswith('grid') == grid])
        trim, skip = R.GRID_COSTS if grid else (TRIM, SKIP)
        # one read handed a status, which it reports without being aligned
        status_in = np.zeros(packed['ev_off'].size - 1, dtype=np.int32)
        status_in[2] = R.MAP_NO_EVENTS
        want = host.align(band=band, trim_cost=trim, skip_cost=skip, status_in=status_in, **packed)
        got = gpu_align(ctx, packed, band, trim, skip, status_in)
        for g, e in zip(got, want):
            assert same(g, e)
        assert want[0][2].tolist() == [R.MAP_NO_EVENTS, packed['ev_off'][3] - packed['ev_off'][2], -1, -1]
        assert {0, R.MAP_LOST} <= set(want[0][:, 0].tolist())


@pytest.fixture(scope='module')
def model():
    from nadavca_amd import synthetic
    return synthetic.load_model_arrays()


@pytest.fixture(scope='module')
def km():
    from nadavca_amd import defaults
    from nadavca_amd.kmer_model import KmerModel
    return KmerModel.load_from_hdf5(defaults.KMER_MODEL_FILE)


@pytest.mark.parametrize('band', [64, 128])
def test_alignment_kernel_on_cut_and_empty_reads(host, ctx, model, band):
    """Reads whose band is steered by the scores: a whole read, three with 100 bases of signal cut out (lost), one
    without events and one without bases, in one batch."""
    parts = [R.cut_read(model, cut_from=c) for c in (30, 100, 180)]
    raws = [parts[0][2]] + [p[0] for p in parts] + [np.zeros(0, np.int16), parts[0][2][:400]]
    seqs = [parts[0][1]] + [p[1] for p in parts] + [parts[0][1][:50], np.zeros(0, np.int32)]
    res = R.cpu_signal_map(host, np.concatenate(raws), R.offsets([r.size for r in raws]), np.concatenate(seqs),
                           R.offsets([s.size for s in seqs]), model, band=band)
    assert res['status'].tolist() == [0, 2, 2, 2, 1, 1]
    packed = {k: res[k] for k in ('mu', 'ac', 'mc', 'l_stay', 'l_step', 'ev_off')}
    packed.update(level=res['scaled'], base_off=R.offsets([s.size for s in seqs]))
    got = gpu_align(ctx, packed, band, TRIM, SKIP, res['status_in'])
    want = host.align(band=band, trim_cost=TRIM, skip_cost=SKIP, status_in=res['status_in'], **packed)
    for g, e in zip(got, want):
        assert same(g, e)


@pytest.fixture(scope='module')
def batch(model):
    rb, aligner, true_starts, padded = R.quality_batch(model)
    return rb, true_starts, padded


@pytest.mark.parametrize('band', [64, 128])
@pytest.mark.parametrize('padded', [False, True])
def test_kernels_equal_the_restatements_on_the_300_read_batch(host, ctx, km, batch, band, padded):
    """Stage by stage on what the previous stage left on the device: flags, events, alignment."""
    from nadavca_amd.readbatch import ReadBatch
    from nadavca_amd.signal_map import signal_map_stages
    rb, true_starts, (raw2, sig_off2, lead) = batch
    if padded:
        rb = ReadBatch.from_signals(raw2, sig_off2, rb.sequence, rb.seq_off)
    st = signal_map_stages(rb, km, 2, 5.0, 0.02, band, 0.5, TRIM, SKIP)
    h = lambda t: t.cpu().numpy()
    norm, flags = h(st.norm), h(st.flags)
    assert same(flags, host.flags(norm, rb.sig_off, 2, 5.0, 0.02))
    ev_pos = np.nonzero(flags)[0].astype(np.int64)
    assert same(h(st.ev_pos), ev_pos) and same(h(st.ev_off), np.searchsorted(ev_pos, rb.sig_off).astype(np.int64))
    for g, e in zip((st.ev_start, st.ev_len, st.ev_level), host.levels(norm, rb.sig_off, ev_pos)):
        assert same(h(g), e)
    hit, score, be = host.align(h(st.scaled), h(st.ev_off), h(st.mu), h(st.ac), h(st.mc), rb.seq_off, h(st.l_stay),
                                h(st.l_step), band, TRIM, SKIP, h(st.status_in))
    assert same(h(st.hit), hit) and same(h(st.path_score), score) and same(h(st.base_event), be)
    assert (hit[:, 0] == 0).all()
    # the stages in torch agree with their numpy restatement: the k-mer tables bit for bit, the moments closely
    mu, ac, mc = R.base_tables(rb.sequence, rb.seq_off, (km.k, km.central_position, km.alphabet_size, km.mean,
                                                         km.sigma), 0.5)
    assert same(h(st.mu), mu) and np.allclose(h(st.ac), ac, rtol=1e-15, atol=0) and np.allclose(h(st.mc), mc, rtol=1e-15)


def test_a_workspace_cap_that_cuts_the_batch_changes_nothing(ctx, km, batch):
    from nadavca_amd import device
    from nadavca_amd.signal_map import signal_map_stages
    rb, _, _ = batch
    st = signal_map_stages(rb, km, 2, 5.0, 0.02, 128, 0.5, TRIM, SKIP)
    args = (st.scaled, st.ev_off, st.mu, st.ac, st.mc, st.seq_off, st.l_stay, st.l_step, st.status_in)
    words = (np.diff(rb.seq_off) + np.diff(st.ev_off.cpu().numpy()) + 1) * 4 * 8
    cap = int(3.5 * words.max())      # three reads fit a part, four never do
    assert words.sum() > 50 * cap
    for band in (64, 128):
        ref = device.event_align_dev(ctx, *args, band, TRIM, SKIP)
        ctx.set_workspace_limit(cap)
        try:
            got = device.event_align_dev(ctx, *args, band, TRIM, SKIP)
        finally:
            ctx.set_workspace_limit(0)
        for g, e in zip(got, ref):
            assert same(g.cpu().numpy(), e.cpu().numpy())
    assert same(ref[0].cpu().numpy(), st.hit.cpu().numpy())


def test_bad_arguments_return_invalid(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    x = torch.zeros(10, dtype=torch.float64, device='cuda')
    i32 = torch.zeros(40, dtype=torch.int32, device='cuda')
    off = lambda *v: torch.tensor(v, dtype=torch.int64, device='cuda')
    good, h = off(0, 4, 10), ctx.handle
    flags = lambda c, n, tot, sig, o, w, th, vf, out: lib.nvk_event_flags_dev(c, n, tot, sig, o, w, th, vf, out)
    assert flags(h, 2, 10, p(x), p(good), 2, 5.0, 0.02, p(i32)) == _lib.NVK_OK
    for bad in (off(1, 4, 10), off(0, 6, 4), off(0, 4, 9)):       # not from 0, decreasing, not ending at the total
        assert flags(h, 2, 10, p(x), p(bad), 2, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(null, 2, 10, p(x), p(good), 2, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, null, p(good), 2, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, p(x), null, 2, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, p(x), p(good), 2, 5.0, 0.02, null) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, p(x), p(good), 0, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, p(x), p(good), 2, 0.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, p(x), p(good), 2, 5.0, 0.0, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, -1, 10, p(x), p(good), 2, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_INVALID
    assert flags(h, 2, 10, p(x), p(good), 9, 5.0, 0.02, p(i32)) == _lib.NVK_ERR_UNSUPPORTED
    pos = off(0, 4)
    levels = lambda c, o, n_ev, ev, a, b, d: lib.nvk_event_levels_dev(c, 2, 10, p(x), o, n_ev, ev, a, b, d)
    assert levels(h, p(good), 2, p(pos), p(i32), p(i32[16:]), p(x)) == _lib.NVK_OK
    assert levels(h, p(off(0, 4, 11)), 2, p(pos), p(i32), p(i32[16:]), p(x)) == _lib.NVK_ERR_INVALID
    assert levels(h, p(good), 11, p(pos), p(i32), p(i32[16:]), p(x)) == _lib.NVK_ERR_INVALID
    assert levels(h, p(good), 2, null, p(i32), p(i32[16:]), p(x)) == _lib.NVK_ERR_INVALID
    assert levels(h, p(good), 2, p(pos), null, p(i32[16:]), p(x)) == _lib.NVK_ERR_INVALID
    assert levels(null, p(good), 2, p(pos), p(i32), p(i32[16:]), p(x)) == _lib.NVK_ERR_INVALID
    y, cost = torch.zeros(10, dtype=torch.float64, device='cuda'), torch.zeros(2, dtype=torch.float64, device='cuda')
    base, score = off(0, 3, 6), torch.zeros(2, dtype=torch.float64, device='cuda')

    def align(c=h, lev=p(x), eo=p(good), mu=p(y), bo=p(base), ls=p(cost), band=64, trim=-1.0, skip=-2.0, hit=p(i32),
              sc=p(score), be=p(i32[16:]), n_ev=10, n_base=6):
        return lib.nvk_event_align_dev(c, 2, n_ev, lev, eo, n_base, mu, mu, mu, bo, ls, ls, null, band, trim, skip,
                                       hit, sc, be)
    assert align() == _lib.NVK_OK
    for kw in (dict(c=null), dict(lev=null), dict(eo=null), dict(mu=null), dict(bo=null), dict(ls=null),
               dict(hit=null), dict(sc=null), dict(be=null), dict(eo=p(off(0, 4, 9))), dict(bo=p(off(1, 3, 6))),
               dict(bo=p(off(0, 7, 6))), dict(n_ev=-1), dict(trim=1.0), dict(skip=float('nan')),
               dict(trim=float('-inf'))):
        assert align(**kw) == _lib.NVK_ERR_INVALID, kw
    assert align(band=96) == _lib.NVK_ERR_UNSUPPORTED
