"""GPU tests of the span entries (csrc/kernels_phase.hip) through the C-ABI on constructed rows, no DP: the span links
against nvk_phase_links_dev (the one-column instantiation of the same kernel against the 2-, 4- and 8-column ones:
column 1, bit for bit; the chain form against the site_first form; site 0 with its chain flag set) and against the numpy
restatement (tests/phase_span_ref.py), the tags over arbitrary block arrays against nvk_phase_tag_dev on interval
blocks (bit for bit) and against the restatement on interleaved ones, the whole loop of
``device.phase_sites_dev(span=3)``, and the invalid-argument returns.  The builders are those of
tests/test_gpu_phase_kernels.py."""
import ctypes as C

import numpy as np
import pytest

import phase_ref
import phase_span_ref
from phase_span_ref import first_of_chain
from test_gpu_phase_kernels import CHAIN, CLIP, MIN_LINK, MIN_SHARED, build_case, build_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


class Rows:
    """A case's rows on the device with the sort (torch: plumbing) and what the site kernels take."""

    def __init__(self, ctx, case):
        import torch
        self.dev = torch.device('cuda', ctx.device)
        self.case = case
        up = self.up
        self.key, self.val = up(case['key']), up(case['val'])
        self.ref_off, self.start, self.reverse = up(case['ref_off']), up(case['start']), up(case['reverse'])
        self.site_pos, self.site_alt = up(case['site_pos']), up(case['site_alt'])
        self.sorted_key, self.order = torch.sort(self.key, stable=True)
        self.sorted_val = self.val[self.order].contiguous()
        self.row_read = (torch.searchsorted(self.ref_off, self.order, right=True) - 1).contiguous()
        self.lo = torch.searchsorted(self.sorted_key, self.site_pos).contiguous()
        self.hi = torch.searchsorted(self.sorted_key, self.site_pos, right=True).contiguous()

    def up(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def evidence(self):
        c = self.case
        return phase_ref.evidence(c['key'], c['val'], c['ref_off'], c['start'], c['reverse'], c['site_pos'],
                                  c['site_alt'], CLIP)

    def span_links(self, ctx, site_first, span):
        from nadavca_amd import device
        link, shared = device.phase_span_links_dev(ctx, self.lo, self.hi, self.site_alt, self.up(site_first),
                                                   self.row_read, self.sorted_val, CLIP, span)
        return link.cpu().numpy(), shared.cpu().numpy()

    def tag(self, ctx, block, sigma, blocks=True):
        from nadavca_amd import device
        entry = device.phase_tag_blocks_dev if blocks else device.phase_tag_dev
        got = entry(ctx, self.ref_off, self.start, self.reverse, self.key, self.val, self.site_pos, self.site_alt,
                    self.up(np.asarray(block, dtype=np.int64)), self.up(np.asarray(sigma, dtype=np.int32)), CLIP)
        return [t.cpu().numpy() for t in got]

    def loop(self, ctx, chain, rounds, **kw):
        from nadavca_amd import device
        got = device.phase_sites_dev(ctx, self.ref_off, self.start, self.reverse, self.key, self.val, self.sorted_key,
                                     self.sorted_val, self.order, self.site_pos, self.site_alt,
                                     self.up(np.asarray(chain, dtype=np.int32)), CLIP, MIN_SHARED, MIN_LINK, rounds,
                                     **kw)
        return {k: v.cpu().numpy() for k, v in got.items()}


def rows_of_dense(has, E, alpha, seed):
    """(has, E) over sites at 10, 20, ... as read-major rows: a read covers its first to its last site, a site inside
    that it has no evidence at gets a punctured row (key -1), a read without a site is dead; odd reads are reverse."""
    S = has.shape[1]
    site_pos = [10 * (s + 1) for s in range(S)]
    reads = []
    for i, h in enumerate(has):
        at = np.nonzero(h)[0]
        if at.size:
            reads.append((site_pos[at[0]] - 5, site_pos[at[-1]] - site_pos[at[0]] + 10, i % 2, True))
        else:
            reads.append((5, 20, i % 2, False))
    site_alt = [int(x) for x in np.random.default_rng(seed).integers(0, alpha, S)]
    return build_rows(reads, site_pos, site_alt, alpha, lambda i, s: E[i, s] if has[i, s] else None, seed + 1)


def sparse_case(seed):
    """20 sites with 0 .. 3 rows each: three reads over every site, each punctured at random; some sites have none."""
    rng = np.random.default_rng(seed)
    S = 20
    has = rng.random((3, S)) < 0.55
    has[:, [0, 7, 8, 19]] = False
    has[:, 4] = True
    E = rng.normal(0, 6, (3, S))
    site_pos = [10 * (s + 1) for s in range(S)]
    reads = [(5, 10 * S + 5, i % 2, True) for i in range(3)]
    site_alt = [int(x) for x in rng.integers(0, 4, S)]
    case = build_rows(reads, site_pos, site_alt, 4, lambda i, s: E[i, s] if has[i, s] else None, seed + 1)
    return case, has


@pytest.mark.parametrize('alpha', [4, 5])
def test_span_links_on_the_ten_site_case(ctx, alpha):
    from nadavca_amd import device
    rows = Rows(ctx, build_case(alpha, 40 + alpha))
    has, E = rows.evidence()
    assert has.sum(axis=0).tolist() == [200, 129, 65, 64, 63, 4, 9, 9, 9, 1]
    chain = np.array(CHAIN, dtype=np.int32)
    site_first = first_of_chain(chain)
    assert site_first.tolist() == [0] * 7 + [7] * 3
    old_link, old_shared = [t.cpu().numpy() for t in device.phase_links_dev(
        ctx, rows.lo, rows.hi, rows.site_alt, rows.up(chain), rows.row_read, rows.sorted_val, CLIP)]
    assert old_shared.tolist() == [0, 129, 65, 64, 62, 1, 3, 0, 9, 0]
    S = 10
    for span in (1, 2, 3, 8):
        link, shared = rows.span_links(ctx, site_first, span)
        assert link.shape == (S, span) and shared.shape == (S, span) and link.dtype == np.float64
        # column 1: the bits of nvk_phase_links_dev where the chain runs, 0 elsewhere
        assert np.array_equal(link[:, 0].view(np.int64), np.where(chain != 0, old_link, 0.0).view(np.int64))
        assert np.array_equal(shared[:, 0], np.where(chain != 0, old_shared, 0))
        want_link, want_shared = phase_span_ref.span_links(has, E, site_first, span)
        assert np.array_equal(shared, want_shared)
        same = phase_span_ref.close(link, want_link)
        assert same.all(), (span, link[~same][:4], want_link[~same][:4])
        outside = np.arange(S)[:, None] - np.arange(1, span + 1)[None, :] < site_first[:, None]
        assert (link[outside].view(np.int64) == 0).all() and (shared[outside] == 0).all() and outside.any()
        # a second call returns the same bits
        again = rows.span_links(ctx, site_first, span)
        assert np.array_equal(again[0].view(np.int64), link.view(np.int64)) and np.array_equal(again[1], shared)
    # span 8 sees the nested sites 0 .. 4 from site 4 and the pair without a shared read
    assert (shared[4, :4] >= 62).all() and (shared[4, 4:] == 0).all() and shared[9, 0] == 0 and link[9, 0] == 0.0
    assert (shared[:, 1:] > 0).sum() == 6            # sites 2, 3 and 4 over the nested sites before them


def test_span_links_on_sites_with_few_rows(ctx):
    case, has = sparse_case(7)
    rows = Rows(ctx, case)
    has2, E = rows.evidence()
    assert np.array_equal(has2, has) and set(has.sum(axis=0).tolist()) == {0, 1, 2, 3}
    chain = np.array([0] + [1] * 19, dtype=np.int32)
    chain[11] = 0
    site_first = first_of_chain(chain)
    for span in (1, 2, 3, 8):
        link, shared = rows.span_links(ctx, site_first, span)
        want_link, want_shared = phase_span_ref.span_links(has, E, site_first, span)
        assert np.array_equal(shared, want_shared) and phase_span_ref.close(link, want_link).all(), span
        empty = has.sum(axis=0) == 0
        assert (link[empty] == 0.0).all() and (shared[empty] == 0).all()
    assert (shared > 0).sum() > 20 and shared.max() == 3


def chain_links(ctx, rows, chain):
    from nadavca_amd import device
    return [t.cpu().numpy() for t in device.phase_links_dev(
        ctx, rows.lo, rows.hi, rows.site_alt, rows.up(np.asarray(chain, dtype=np.int32)), rows.row_read,
        rows.sorted_val, CLIP)]


@pytest.mark.parametrize('alpha', [4, 5])
def test_site_0_with_its_chain_flag_set(ctx, alpha):
    """nvk_phase_links_dev reads no site before site 0 whatever chain[0] says: 0.0 / 0 there, the other sites as with
    chain[0] = 0."""
    rows = Rows(ctx, build_case(alpha, 40 + alpha))
    link, shared = chain_links(ctx, rows, [1] * 10)
    want_link, want_shared = chain_links(ctx, rows, [0] + [1] * 9)
    assert link.view(np.int64)[0] == 0 and shared[0] == 0
    assert np.array_equal(link[1:].view(np.int64), want_link[1:].view(np.int64))
    assert np.array_equal(shared[1:], want_shared[1:]) and shared.tolist() == [0, 129, 65, 64, 62, 1, 3, 9, 9, 0]


@pytest.mark.parametrize('alpha', [4, 5])
def test_the_chain_form_and_the_site_first_form_agree(ctx, alpha):
    """nvk_phase_links_dev(chain) and nvk_phase_span_links_dev(site_first of that chain, span 1) are one kernel told
    the sites' first sites in two ways: every bit of link and shared agrees."""
    rows = Rows(ctx, build_case(alpha, 40 + alpha))
    breaks = [0, 1, 1, 0, 0, 1, 1, 1, 1, 1]             # two chain breaks in a row
    for chain in (CHAIN, [0] + [1] * 9, breaks):
        link, shared = chain_links(ctx, rows, chain)
        span_link, span_shared = rows.span_links(ctx, first_of_chain(chain), 1)
        assert span_link.shape == (10, 1) and span_shared.shape == (10, 1)
        assert np.array_equal(link.view(np.int64), span_link[:, 0].view(np.int64)), chain
        assert np.array_equal(shared, span_shared[:, 0]), chain
        served = np.array(chain) != 0
        assert (shared[~served] == 0).all() and (link[~served].view(np.int64) == 0).all()
        assert (shared[served] > 0).sum() >= 5
    assert shared.tolist() == [0, 129, 65, 0, 0, 1, 3, 9, 9, 0]


@pytest.mark.parametrize('alpha', [4, 5])
def test_tag_blocks_on_interval_blocks_is_the_tag_kernel(ctx, alpha):
    case = build_case(alpha, 40 + alpha)
    rows = Rows(ctx, case)
    has, E = rows.evidence()
    full = np.array([0] + [1] * 9, dtype=np.int32)
    for chain, rounds in ((case['chain'], 2), (case['chain'], 0), (full, 1)):
        ref = phase_ref.refine(has, E, chain, MIN_SHARED, MIN_LINK, rounds)
        old = rows.tag(ctx, ref['block'], ref['sigma'], blocks=False)
        new = rows.tag(ctx, ref['block'], ref['sigma'])
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[2], new[2])
        assert np.array_equal(old[1].view(np.int64), new[1].view(np.int64))
        assert np.array_equal(new[0], ref['read_block']) and np.array_equal(new[1], ref['read_llr'])
    assert (new[0] == -1).sum() >= 4 and np.unique(new[0]).size >= 4 and new[2].max() >= 4
    assert new[0][case['dead']] == -1 and new[1][case['dead']] == 0.0 and new[2][case['dead']] == 0


def check_tags(rows, ctx, has, E, block, sigma, label):
    want = phase_span_ref.tag_blocks(has, E, block, sigma)
    got = rows.tag(ctx, block, sigma)
    assert np.array_equal(got[0], want[0]), (label, got[0], want[0])
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), label + ': read_llr differs in some bit'
    assert np.array_equal(got[2], want[2]), label
    return want


def test_tag_blocks_on_interleaved_blocks(ctx):
    # the forest of the weak-site case: site 2 a singleton inside block 0
    has, E, _ = phase_span_ref.weak_site_case()
    ref = phase_span_ref.refine_span(has, E, np.zeros(6, dtype=np.int64), MIN_SHARED, MIN_LINK, 0, 3)
    assert ref['block'].tolist() == [0, 0, 2, 0, 0, 0]
    rows = Rows(ctx, rows_of_dense(has, E, 4, 3))
    has2, E2 = rows.evidence()
    assert np.array_equal(has2, has) and np.array_equal(E2, E)
    want = check_tags(rows, ctx, has, E, ref['block'], ref['sigma'], 'weak site')
    over_weak = has[:, 2] & (has[:, 1] | has[:, 3])
    assert over_weak.sum() > 20 and (want[0][over_weak] == 0).all() and (want[2][has[:, 1] & has[:, 3]] >= 2).all()
    # 20 seeded random forests over 20 sites, reads of 1 .. 20 sites with punctured rows and dead reads
    rng = np.random.default_rng(23)
    S, n = 20, 50
    most_blocks = punctured_members = dead = interleaved = 0
    for trial in range(20):
        span = (2, 3, 8)[trial % 3]
        link = np.round(rng.normal(0, 4, (S, span)), 1)
        shared = rng.integers(0, 8, (S, span))
        site_first = first_of_chain((rng.random(S) < 0.9).astype(np.int32))
        _, block, sigma, _ = phase_span_ref.forest(link, shared, site_first, (3, 6)[trial % 2], MIN_LINK)
        length = rng.integers(1, S + 1, n)
        length[0] = S
        first = (rng.random(n) * (S - length + 1)).astype(np.int64)
        cols = np.arange(S)[None, :]
        inside = (cols >= first[:, None]) & (cols < (first + length)[:, None])
        has = inside & (rng.random((n, S)) < 0.85)
        has[0], has[1] = True, False
        E = rng.normal(0, 5, (n, S))
        E[rng.random((n, S)) < 0.03] = 600.0
        E[rng.random((n, S)) < 0.03] = -np.inf
        rows = Rows(ctx, rows_of_dense(has, np.where(has, E, 0.0), 4, 100 + trial))
        has2, E2 = rows.evidence()
        assert np.array_equal(has2, has) and rows.case['reverse'].any() and not rows.case['reverse'].all()
        check_tags(rows, ctx, has2, E2, block, sigma, 'forest %d' % trial)
        per_read = [np.unique(block[h]).size for h in has]
        most_blocks = max(most_blocks, max(per_read))
        interleaved += any(np.unique(block[a:b + 1]).size > 1 for r in np.unique(block)
                           for a, b in [np.nonzero(block == r)[0][[0, -1]]])
        for i in range(n):
            at = np.nonzero(has[i])[0]
            if at.size >= 2:
                mid = np.arange(at[0], at[-1] + 1)
                mid = mid[~has[i, mid]]
                punctured_members += bool(np.isin(block[mid], block[at]).any())
        dead += int((~has.any(axis=1)).sum())
    assert most_blocks > 8 and punctured_members > 20 and dead >= 20 and interleaved >= 15, \
        (most_blocks, punctured_members, dead, interleaved)


def test_the_loop_with_span(ctx):
    # the weak-site case as rows
    has, E, truth = phase_span_ref.weak_site_case()
    rows = Rows(ctx, rows_of_dense(has, E, 4, 3))
    chain = [0, 1, 1, 1, 1, 1]
    ref = phase_span_ref.refine_span(has, E, first_of_chain(chain), MIN_SHARED, MIN_LINK, 2, 3)
    got = rows.loop(ctx, chain, 2, span=3)
    phase_span_ref.check_against(ref, got, 'weak site, span 3')
    assert got['block'].tolist() == [0, 0, 2, 0, 0, 0] and got['parent'].tolist() == [-1, 0, -1, 1, 3, 3]
    assert got['sigma'][[0, 1, 3, 5]].tolist() == truth[[0, 1, 3, 5]].tolist()
    assert got['span_link'].shape == (6, 3) and np.array_equal(got['link'], got['span_link'][:, 0])
    assert np.array_equal(got['shared'], got['span_shared'][:, 0])
    # span = 1 is the call without the keyword, bit for bit, and cuts the block
    plain, one = rows.loop(ctx, chain, 2), rows.loop(ctx, chain, 2, span=1)
    assert sorted(plain) == sorted(one) and 'parent' not in one and plain['block'].tolist() == [0, 0, 2, 3, 3, 3]
    for k in plain:
        assert plain[k].dtype == one[k].dtype and np.array_equal(plain[k].view(np.uint8), one[k].view(np.uint8)), k
    phase_ref.check_against(phase_ref.refine(has, E, chain, MIN_SHARED, MIN_LINK, 2), one, 'weak site, span 1')
    # the refinement case of tests/test_phase_cpu.py: with span 3 site c takes its strong link to a, not the one to b
    # that puts it at -1, and no vote has to flip it
    has, E = phase_ref.refinement_case()
    rows = Rows(ctx, rows_of_dense(has, E, 4, 5))
    ref = phase_span_ref.refine_span(has, E, np.zeros(3, dtype=np.int64), MIN_SHARED, MIN_LINK, 2, 3)
    assert ref['flips_per_round'] == [0, 0] and ref['sigma'].tolist() == [1, 1, 1] and ref['span_link'][2, 0] < -20
    got = rows.loop(ctx, [0, 1, 1], 2, span=3)
    # (the three reads over b and c end at H = 10 - 10 = 0 in exact arithmetic, as in tests/test_gpu_phase_kernels.py)
    phase_span_ref.check_against(ref, got, 'refinement, span 3', exact=('llr',))
    assert got['flips'].tolist() == [0, 0] and got['parent'].tolist() == [-1, 0, 0]
    # no site: nothing phased
    import torch
    none = torch.zeros(0, dtype=torch.int64, device=rows.dev)
    from nadavca_amd import device
    got = device.phase_sites_dev(ctx, rows.ref_off, rows.start, rows.reverse, rows.key, rows.val, rows.sorted_key,
                                 rows.sorted_val, rows.order, none, none.to(torch.int32), none.to(torch.int32), CLIP,
                                 MIN_SHARED, MIN_LINK, 2, span=3)
    assert got['parent'].numel() == 0 and tuple(got['span_link'].shape) == (0, 3) and got['flips'].tolist() == [0, 0]
    assert (got['read_block'] == -1).all() and got['read_block'].numel() == has.shape[0]


def test_c_abi_rejects_bad_arguments_and_no_sites(ctx):
    import torch
    from nadavca_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    i64, i32, f64 = torch.int64, torch.int32, torch.float64
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    S, n, rows = 2, 2, 30
    lo, hi = torch.tensor([0, 10], dtype=i64, device=dev), torch.tensor([10, 30], dtype=i64, device=dev)
    alt, first, sigma, block = z(S, i32), z(S, i64), z(S, i32) + 1, z(S, i64)
    row_read = torch.cat([torch.zeros(10, dtype=i64), torch.ones(20, dtype=i64)]).to(dev)
    val, key = z((rows, 4), f64), torch.cat([torch.arange(10), torch.arange(20)]).to(dev)
    off = torch.tensor([0, 10, 30], dtype=i64, device=dev)
    start, rev, pos = z(n, i64), z(n, i32), torch.tensor([3, 12], dtype=i64, device=dev)
    link, shared = z(S * 8, f64) + 7.0, z(S * 8, i64) + 7
    rblock, rllr, rsites = z(n, i64), z(n, f64), z(n, i64)

    def links(c=None, S_=S, alpha=4, clip=CLIP, span=2, a=(lo, hi, alt, first, row_read, val), o=(link, shared)):
        return lib.nvk_phase_span_links_dev(ctx.handle if c is None else c, S_, span, alpha, *[p(t) for t in a], clip,
                                            *[p(t) for t in o])

    def tag(c=None, n_=n, S_=S, alpha=4, clip=CLIP, a=(off, start, rev, key, val, pos, alt, block, sigma),
            o=(rblock, rllr, rsites)):
        return lib.nvk_phase_tag_blocks_dev(ctx.handle if c is None else c, n_, S_, alpha, *[p(t) for t in a], clip,
                                            *[p(t) for t in o])

    for entry in (links, tag):
        assert entry() == _lib.NVK_OK
        assert entry(c=C.c_void_p(0)) == _lib.NVK_ERR_INVALID
        for kw in (dict(alpha=1), dict(alpha=9), dict(clip=0.0), dict(clip=-1.0), dict(clip=float('nan')),
                   dict(clip=float('inf')), dict(S_=-1)):
            assert entry(**kw) == _lib.NVK_ERR_INVALID and lib.nvk_last_error(), (entry.__name__, kw)
        n_in = len(entry.__defaults__[-2])
        for j in range(n_in):
            a = list(entry.__defaults__[-2])
            a[j] = None
            assert entry(a=tuple(a)) == _lib.NVK_ERR_INVALID, (entry.__name__, j)
        for j in range(len(entry.__defaults__[-1])):
            o = list(entry.__defaults__[-1])
            o[j] = None
            assert entry(o=tuple(o)) == _lib.NVK_ERR_INVALID, (entry.__name__, j)
        # n_sites == 0 launches nothing and needs no array
        assert entry(S_=0, a=(None,) * n_in, o=(None,) * len(entry.__defaults__[-1])) == _lib.NVK_OK
    for span in (0, 9, -1):
        assert links(span=span) == _lib.NVK_ERR_INVALID and b'span' in lib.nvk_last_error()
    # every entry inside n_sites * span is written, nothing behind it
    link[:], shared[:] = 7.0, 7
    assert links(span=3) == _lib.NVK_OK
    assert link.tolist()[:6] == [0.0] * 6 and link.tolist()[6:] == [7.0] * 10
    assert shared.tolist()[:6] == [0] * 6 and shared.tolist()[6:] == [7] * 10
    assert tag(n_=-1) == _lib.NVK_ERR_INVALID
    assert tag(a=(torch.tensor([0, 31, 30], dtype=i64, device=dev), start, rev, key, val, pos, alt, block, sigma)) \
        == _lib.NVK_ERR_INVALID
