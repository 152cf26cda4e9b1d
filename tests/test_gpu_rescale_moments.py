"""``rawsignal.rescale_by_moments_dev``, the one rescale of ``signal_map_batch`` (a target per read),
``signal_locate_batch`` and ``decode_batch`` (one target for every read): which reads take part, and what comes out
for those that do and for those that do not, on five hand-made reads.  The medians and MADs are taken from
``normalize_groups_dev``'s own second return value, so the test is about how they are combined — (level - med_e) *
(mad_l / mad_e) + med_l, a rounding per operation, which numpy's f64 repeats bit for bit — not about the selection,
which has its own tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MIN_EVENTS = 4
# events per read: none; three of one level (MAD 0); MIN_EVENTS - 1; MIN_EVENTS; many
N_EVENTS = [0, 3, MIN_EVENTS - 1, MIN_EVENTS, 200]
N_TARGET = [7, 5, 9, 0, 11]          # the per-read form's groups: read 3 has none


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope='module')
def reads():
    rng = np.random.default_rng(5)
    level = [np.zeros(0), np.full(3, 0.375), np.array([-0.5, 0.25, 1.5]), np.array([0.75, -1.25, 0.5, 2.0]),
             rng.normal(0.1, 1.3, 200)]
    assert [x.size for x in level] == N_EVENTS
    target = rng.normal(90.0, 12.0, sum(N_TARGET))
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(level), off(N_EVENTS), target, off(N_TARGET)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def run(ctx, reads, pooled, **kw):
    """-> (scaled, shift, scale, ok) of the device, and the same from numpy out of the device's medians and MADs"""
    from nadavca_amd.device import _one, normalize_groups_dev
    from nadavca_amd.rawsignal import rescale_by_moments_dev
    level, ev_off, target, target_off = reads
    if pooled:
        target_off = np.array([0, target.size], dtype=np.int64)
    got = [x.cpu().numpy() for x in rescale_by_moments_dev(ctx, dev(level), dev(ev_off), dev(target), dev(target_off),
                                                           **kw)]
    cs_e = normalize_groups_dev(ctx, dev(level), dev(ev_off))[1].cpu().numpy()
    cs_l = normalize_groups_dev(ctx, _one(dev(target)), dev(target_off))[1].cpu().numpy()
    if pooled:
        cs_l = np.repeat(cs_l, len(N_EVENTS), axis=0)
    want = []
    for r in range(len(N_EVENTS)):
        x = level[ev_off[r]:ev_off[r + 1]]
        if cs_e[r, 1] > 0:
            scale = cs_l[r, 1] / cs_e[r, 1]
            want.append(((x - cs_e[r, 0]) * scale + cs_l[r, 0], cs_l[r, 0] - cs_e[r, 0] * scale, scale))
        else:
            want.append(None)
    return got, want


def check(reads, got, want, ok):
    level, ev_off = reads[:2]
    scaled, shift, scale, got_ok = got
    assert got_ok.dtype == np.bool_ and got_ok.tolist() == ok
    assert scaled.shape == level.shape and scaled.dtype == np.float64
    for r, takes_part in enumerate(ok):
        mine = scaled[ev_off[r]:ev_off[r + 1]]
        if takes_part:
            assert mine.tobytes() == want[r][0].tobytes(), r
            assert shift[r].tobytes() == np.float64(want[r][1]).tobytes(), r
            assert scale[r].tobytes() == np.float64(want[r][2]).tobytes(), r
            assert scale[r] > 0 and not np.array_equal(mine, level[ev_off[r]:ev_off[r + 1]])
        else:
            assert np.array_equal(mine, level[ev_off[r]:ev_off[r + 1]]), r
            assert scale[r] == 1.0 and shift[r] == 0.0, r


def test_a_target_per_read(ctx, reads):
    """signal_map_batch's form: at least one event, a MAD above 0, a target that is not empty"""
    got, want = run(ctx, reads, pooled=False)
    check(reads, got, want, [False, False, True, False, True])
    got, want = run(ctx, reads, pooled=False, min_events=MIN_EVENTS)
    check(reads, got, want, [False, False, False, False, True])


def test_one_target_for_every_read(ctx, reads):
    """signal_locate_batch's and decode_batch's form: at least ``min_events`` events, a MAD above 0"""
    got, want = run(ctx, reads, pooled=True, min_events=MIN_EVENTS)
    check(reads, got, want, [False, False, False, True, True])
    got, want = run(ctx, reads, pooled=True)
    check(reads, got, want, [False, False, True, True, True])
    keep = np.array([True, True, True, False, True])
    got, want = run(ctx, reads, pooled=True, min_events=MIN_EVENTS, ok_extra=dev(keep))
    check(reads, got, want, [False, False, False, False, True])


def test_an_empty_target_leaves_every_read_out(ctx, reads):
    level, ev_off, target, _ = reads
    got, want = run(ctx, (level, ev_off, target[:0], None), pooled=True, min_events=MIN_EVENTS)
    check(reads, got, want, [False] * 5)
