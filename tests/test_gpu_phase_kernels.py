"""GPU tests of the phase kernels (csrc/kernels_phase.hip) through the C-ABI on constructed rows, no DP: links, tags and
votes and the whole loop of ``device.phase_sites_dev`` against the numpy restatement (tests/phase_ref.py) under the
tolerances of ``phase_ref.check_against``, the same bits on a second call, the refinement case of the CPU test, and the
invalid-argument returns."""
import ctypes as C

import numpy as np
import pytest

import phase_ref

pytestmark = pytest.mark.gpu

CLIP, MIN_SHARED, MIN_LINK = 30.0, 3, 2.0
SITE_POS = [10, 20, 30, 40, 50, 60, 70, 80, 90, 150]
#            rows 200 129  65  64  63   4   9   9   9    1
CHAIN = [0, 1, 1, 1, 1, 1, 1, 0, 1, 1]        # 0 in the middle: sites 6 and 7 share 9 reads and are not linked


def build_rows(reads, site_pos, site_alt, alpha, evidence, seed):
    """Read-major rows as nvk_allele_rows_dev writes them.  ``reads``: (start, length, reverse, live) per read;
    ``evidence(i, s)``: the value of read i in the forward column site_alt[s] of its row of site_pos[s] (None: the
    row's key becomes -1).  Every other cell holds noise.  -> dict of host arrays."""
    rng = np.random.default_rng(seed)
    length = np.array([r[1] for r in reads], dtype=np.int64)
    ref_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    total = int(ref_off[-1])
    start = np.array([r[0] for r in reads], dtype=np.int64)
    reverse = np.array([r[2] for r in reads], dtype=np.int32)
    key = np.full(total, -1, dtype=np.int64)
    val = rng.normal(-20.0, 15.0, (total, alpha))
    for i, (c0, R, rev, live) in enumerate(reads):
        p = np.arange(R)
        if live:
            key[ref_off[i]:ref_off[i + 1]] = c0 + (R - 1 - p if rev else p)
        else:
            val[ref_off[i]:ref_off[i + 1]] = 0.0
        for s, P in enumerate(site_pos):
            if live and c0 <= P < c0 + R:
                row = ref_off[i] + (R - 1 - (P - c0) if rev else P - c0)
                e = evidence(i, s)
                if e is None:
                    key[row], val[row] = -1, 0.0
                else:
                    val[row, site_alt[s]] = e
    return dict(alpha=alpha, n=len(reads), ref_off=ref_off, start=start, reverse=reverse, key=key, val=val,
                site_pos=np.array(site_pos, dtype=np.int64), site_alt=np.array(site_alt, dtype=np.int32))


def build_case(alpha, seed):
    """Ten sites whose rows number 200, 129, 65, 64, 63, 4, 9, 9, 9 and 1.  Sites 0 .. 4 are nested (every read of site
    1 is one of site 0: a pair sharing all reads), site 5 shares exactly one read with site 4, sites 5 and 6 share three
    reads whose evidence at site 5 is 0.01 (a link far below min_link), chain is 0 at site 7, site 9 shares no read with
    site 8.  Reads without a site, a read whose keys are all -1, a read whose row of site 1 has the key -1, reads with
    sites in three blocks; odd reads are reverse.  Evidence of +-600 and -inf under a clip of 30."""
    rng = np.random.default_rng(seed)
    spans = [(5, 50)] * 62 + [(45, 20)] + [(5, 40)] * 2 + [(5, 30)] + [(5, 20)] * 64 + [(5, 10)] * 70 + [(5, 20)] \
        + [(66, 29)] * 6 + [(56, 39)] * 3 + [(140, 20)] + [(100, 20)] * 3 + [(5, 50)]
    punctured, dead = 62 + 1 + 2 + 1 + 64 + 70, len(spans) - 1
    order = rng.permutation(len(spans))
    punctured, dead = int(np.nonzero(order == punctured)[0][0]), int(np.nonzero(order == dead)[0][0])
    spans = [spans[j] for j in order]
    reads = [(c0, R, i % 2, i != dead) for i, (c0, R) in enumerate(spans)]
    truth = np.array([1, -1, -1, 1, -1, 1, 1, -1, 1, 1])
    hap = np.where(rng.random(len(reads)) < 0.5, 1, -1)
    site_alt = [int(x) for x in rng.integers(0, alpha, len(SITE_POS))]
    noise = rng.normal(0, 1.5, (len(reads), len(SITE_POS)))
    kind = rng.integers(0, 12, (len(reads), len(SITE_POS)))

    def evidence(i, s):
        if i == punctured and s == 1:
            return None
        if spans[i] == (56, 39) and s == 5:
            return 0.01 * hap[i]
        e = hap[i] * truth[s] * 6.0 + noise[i, s]
        if spans[i][0] == 5 and kind[i, s] == 0:       # (only reads inside one block: two runs would tie at the clip)
            return 600.0 if e > 0 else -600.0
        if spans[i][0] == 5 and kind[i, s] == 1 and e < 0:
            return -np.inf
        return e
    case = build_rows(reads, SITE_POS, site_alt, alpha, evidence, seed + 1)
    case.update(chain=np.array(CHAIN, dtype=np.int32), punctured=punctured, dead=dead, spans=spans)
    return case


@pytest.fixture(scope='module')
def ctx():
    from nadavca_amd import _lib
    return _lib.default_context()


def run_loop(ctx, case, rounds, chain=None):
    """The sort (torch: plumbing) and ``device.phase_sites_dev`` on the case's rows -> dict of numpy arrays."""
    import torch
    from nadavca_amd import device
    dev = torch.device('cuda', ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    key, val = up(case['key']), up(case['val'])
    sorted_key, order = torch.sort(key, stable=True)
    got = device.phase_sites_dev(ctx, up(case['ref_off']), up(case['start']), up(case['reverse']), key, val, sorted_key,
                                 val[order].contiguous(), order, up(case['site_pos']), up(case['site_alt']),
                                 up(case['chain'] if chain is None else chain), CLIP, MIN_SHARED, MIN_LINK, rounds)
    return {k: v.cpu().numpy() for k, v in got.items()}


def restated(case, rounds, chain=None):
    has, E = phase_ref.evidence(case['key'], case['val'], case['ref_off'], case['start'], case['reverse'],
                                case['site_pos'], case['site_alt'], CLIP)
    return has, E, phase_ref.refine(has, E, case['chain'] if chain is None else chain, MIN_SHARED, MIN_LINK, rounds)


@pytest.mark.parametrize('alpha', [4, 5])
def test_kernels_against_the_restatement(ctx, alpha):
    case = build_case(alpha, 40 + alpha)
    has, E, ref = restated(case, 2)
    # the case is what its description says, by the restatement alone
    assert has.sum(axis=0).tolist() == [200, 129, 65, 64, 63, 4, 9, 9, 9, 1]
    assert ref['shared'].tolist() == [0, 129, 65, 64, 62, 1, 3, 0, 9, 0]
    assert abs(ref['link'][6]) < 1.0 and ref['link'][7] == 0.0
    assert ref['block'].tolist() == [0, 0, 0, 0, 0, 5, 6, 7, 7, 9]
    assert ref['sigma'].tolist() == [1, -1, -1, 1, -1, 1, 1, 1, -1, 1]
    assert not has[case['dead']].any() and has[case['punctured']].tolist() == [True] + [False] * 9
    sites_of = has.sum(axis=1)
    blocks_of = np.array([np.unique(ref['block'][h]).size for h in has])
    assert (sites_of == 0).sum() >= 4 and (sites_of == 1).sum() >= 70 and (blocks_of == 3).sum() == 3
    assert (ref['read_block'] == -1).sum() == (sites_of == 0).sum() and (ref['read_sites'] >= 4).any()
    raw = case['val'][np.arange(case['val'].shape[0])[:, None], case['site_alt'][None, :]]
    assert (raw == 600.0).any() and (raw == -600.0).any() and np.isneginf(raw).any()
    assert (np.abs(E) == CLIP).sum() > 20 and case['reverse'].any() and not case['reverse'].all()
    got = run_loop(ctx, case, 2)
    phase_ref.check_against(ref, got, 'alphabet %d' % alpha)
    print('alphabet %d: margins %r' % (alpha, ref['margins']))
    assert got['read_llr'][case['dead']] == 0.0 and got['read_block'][case['dead']] == -1
    # a second call returns the same bits
    again = run_loop(ctx, case, 2)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    # every chain flag set: sites 6 and 7 are linked through their 9 shared reads, the others stay
    full = np.array([0] + [1] * 9, dtype=np.int32)
    _, _, ref_full = restated(case, 1, full)
    assert ref_full['block'].tolist() == [0, 0, 0, 0, 0, 5, 6, 6, 6, 9] and ref_full['shared'][7] == 9
    phase_ref.check_against(ref_full, run_loop(ctx, case, 1, full), 'alphabet %d, full chain' % alpha)


def test_refinement_flips_on_the_device(ctx):
    """The constructed case of tests/test_phase_cpu.py as rows: the link puts site c at -1, the vote flips it."""
    has, E = phase_ref.refinement_case()
    spans = {(True, True, False): (5, 20), (False, True, True): (15, 20), (True, True, True): (5, 30)}
    reads = [spans[tuple(h)] + (i % 2, True) for i, h in enumerate(has.tolist())]
    case = build_rows(reads, [10, 20, 30], [1, 3, 0], 4, lambda i, s: E[i, s], 3)
    case['chain'] = np.array([0, 1, 1], dtype=np.int32)
    has2, E2, ref = restated(case, 2)
    assert np.array_equal(has2, has) and np.array_equal(E2, E)
    assert ref['flips_per_round'] == [1, 0] and ref['sigma'].tolist() == [1, 1, 1]
    got = run_loop(ctx, case, 2)
    # the three reads over b and c end at H = 10 - 10 = 0 in exact arithmetic; the reads over a, b, c have
    # h = (10 + 0.1 - 10) - 0.1 = -3.6e-16 at b: one rounded subtraction from a read_llr that is equal bit for bit
    assert ref['margins']['llr'] == 0.0 and 0.0 < ref['margins']['h'] < 1e-15
    phase_ref.check_against(ref, got, 'refinement', exact=('llr', 'h'))
    assert got['flips'].tolist() == [1, 0] and got['sigma'].tolist() == [1, 1, 1]
    zero = run_loop(ctx, case, 0)
    assert zero['flips'].size == 0 and zero['sigma'].tolist() == [1, 1, -1]
    assert zero['vote'][2] == 50.0 and (zero['n_agree'][2], zero['n_against'][2]) == (3, 8)


def test_c_abi_rejects_bad_arguments_and_no_sites(ctx):
    import torch
    from nadavca_amd import _lib, device
    lib = _lib.load()
    dev = torch.device('cuda', ctx.device)
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    i64, i32, f64 = torch.int64, torch.int32, torch.float64
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    S, n, rows = 2, 2, 30
    lo, hi = torch.tensor([0, 10], dtype=i64, device=dev), torch.tensor([10, 30], dtype=i64, device=dev)
    alt, chain, sigma, block = z(S, i32), z(S, i32) + 1, z(S, i32) + 1, z(S, i64)
    row_read = torch.cat([torch.zeros(10, dtype=i64), torch.ones(20, dtype=i64)]).to(dev)
    val, key = z((rows, 4), f64), torch.cat([torch.arange(10), torch.arange(20)]).to(dev)
    off = torch.tensor([0, 10, 30], dtype=i64, device=dev)
    start, rev, pos = z(n, i64), z(n, i32), torch.tensor([3, 12], dtype=i64, device=dev)
    link, shared, vote, agree, against = z(S, f64), z(S, i64), z(S, f64), z(S, i64), z(S, i64)
    rblock, rllr, rsites = z(n, i64), z(n, f64), z(n, i64)

    def links(c=None, S_=S, alpha=4, clip=CLIP, a=(lo, hi, alt, chain, row_read, val), o=(link, shared)):
        return lib.nvk_phase_links_dev(ctx.handle if c is None else c, S_, alpha, *[p(t) for t in a], clip,
                                       *[p(t) for t in o])

    def tag(c=None, n_=n, S_=S, alpha=4, clip=CLIP, a=(off, start, rev, key, val, pos, alt, block, sigma),
            o=(rblock, rllr, rsites)):
        return lib.nvk_phase_tag_dev(ctx.handle if c is None else c, n_, S_, alpha, *[p(t) for t in a], clip,
                                     *[p(t) for t in o])

    def votes(c=None, S_=S, alpha=4, clip=CLIP, a=(lo, hi, alt, block, sigma, row_read, val, rblock, rllr),
              o=(vote, agree, against)):
        return lib.nvk_phase_votes_dev(ctx.handle if c is None else c, S_, alpha, *[p(t) for t in a], clip,
                                       *[p(t) for t in o])

    for entry in (links, tag, votes):
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
    assert tag(n_=-1) == _lib.NVK_ERR_INVALID
    assert tag(a=(torch.tensor([0, 31, 30], dtype=i64, device=dev), start, rev, key, val, pos, alt, block, sigma)) \
        == _lib.NVK_ERR_INVALID
    assert tag(a=(torch.tensor([1, 10, 30], dtype=i64, device=dev), start, rev, key, val, pos, alt, block, sigma)) \
        == _lib.NVK_ERR_INVALID
    # the wrappers with no site: nothing phased, every read untagged
    none = z(0, i64)
    sorted_key, order = torch.sort(key, stable=True)
    got = device.phase_sites_dev(ctx, off, start, rev, key, val, sorted_key, val[order].contiguous(), order, none,
                                 z(0, i32), z(0, i32), CLIP, MIN_SHARED, MIN_LINK, 2)
    assert got['link'].numel() == 0 and got['block'].numel() == 0 and got['flips'].tolist() == [0, 0]
    assert got['read_block'].tolist() == [-1, -1] and got['read_llr'].tolist() == [0.0, 0.0]
    assert got['read_sites'].tolist() == [0, 0]
