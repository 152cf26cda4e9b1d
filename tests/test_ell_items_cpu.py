"""CPU check behind nadavca_amd/csrc/ell_items.h, the packed hypotheses of the joint and the edit kind of ell_kernel
(csrc/kernels_ell.hip): the host build of the header (tests/host_shims/ell_items_host.cpp, a ctypes library) against
Python restatements of the two codes (include/nadavca_hip.h and the header's comments: a joint item has one nibble per
offset, bit 3 marks a substituted base, the last offset sits in nibble 15; an edit item has its letters in nibbles, i in
bits 52-55 and d in bits 56-63), of the rows a hypothesis re-runs (variant_cases.joint_rows / edit_rows) and of the edit
map, exhausted over the small cases; and the same cases once more through a stand-alone program built with the address
and undefined-behaviour sanitizers.  What the kernels do with the items is tests/test_gpu_joint_hypotheses.py,
tests/test_gpu_edit_hypotheses.py and tests/test_gpu_variant_census.py."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from variant_cases import JOINT_ROWS, edit_rows, joint_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, 'tests', 'host_shims')
PAD = 9              # ell_items_host.cpp: positions looked at on either side of the sequence
ALPHABET = 4
SHAPES = ((5, 2), (7, 3), (6, 0), (6, 5))   # (k, central)
MASK64 = (1 << 64) - 1


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp('ell_items')), 'ell_items_host.so')
    subprocess.run(['g++', '-O2', '-shared', '-fPIC', os.path.join(SHIMS, 'ell_items_host.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.ell_items_host_edit.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_longlong, C.c_void_p]
    lib.ell_items_host_edit.restype = C.c_longlong
    lib.ell_items_host_joint.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.ell_items_host_joint.restype = C.c_longlong
    return lib


def _fix(flat):
    """The code comes out of the shim as a signed 64-bit integer."""
    if len(flat) > 1:
        flat[1] &= MASK64
    return flat


_out = np.empty(4096, dtype=np.int64)


def got_edit(lib, case):
    R, k, central, p, d, s = case
    s = np.asarray(s, dtype=np.int32)
    n = lib.ell_items_host_edit(R, ALPHABET, k - central - 1, central, p, d, s.ctypes.data, len(s), _out.ctypes.data)
    return _fix(_out[:n].tolist())


def got_joint(lib, case):
    ref, k, central, h = case
    pos = np.asarray([x[0] for x in h], dtype=np.int32)
    base = np.asarray([x[1] for x in h], dtype=np.int32)
    n = lib.ell_items_host_joint(ref.ctypes.data, len(ref), ALPHABET, k - central - 1, central, pos.ctypes.data,
                                 base.ctypes.data, len(h), _out.ctypes.data)
    return _fix(_out[:n].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# edits
# ---------------------------------------------------------------------------------------------------------------------
def expected_edit(case):
    """What ell_items_host_edit writes, restated: the hypothesis (p, d, s) on a read of R bases."""
    R, k, central, p, d, s = case
    i, back, fwd = len(s), k - central - 1, central
    if not (1 <= p and 0 <= d <= 255 and i <= 13 and p + d <= R - 1 and all(0 <= x < ALPHABET for x in s)):
        return [0]
    rows = edit_rows(R, k, central, p, d, i)
    if rows > JOINT_ROWS:
        return [0]
    code = sum(x << (4 * t) for t, x in enumerate(s)) | i << 52 | d << 56
    R2 = R - d + i                                          # bases of ref' = ref[:p] + s + ref[p+d:]
    first, last = max(0, min(p - 1, p - back)), min(R2 - 1, p + i - 1 + fwd)
    # boundary row r of ref' as a row of the read's bands: itself before the edit; an inserted row starts where the last
    # row before the edit does and ends where the first one behind it does; behind the edit the read's r - i + d
    row = lambda r, inserted: r if r < p else inserted if r < p + i else r - i + d
    flat = [1, code, i, d, rows, first, last, last + 1 - i + d, 1]
    flat += [row(r, p - 1) for r in range(R2 + 1)] + [row(r, p + d) for r in range(R2 + 1)]
    for at in range(-PAD, R2 + PAD):
        flat += [-1, at] if at < p else [s[at - p], 0] if at < p + i else [-1, at - i + d]
    return flat


def seq_at(ref, cb, ca, idx):
    """ExtendedSequence::operator[] as csrc/kmer.h restates it: context_before | reference | context_after, 0 outside."""
    if idx < 0:
        return cb[idx + len(cb)] if idx + len(cb) >= 0 else 0
    if idx < len(ref):
        return ref[idx]
    return ca[idx - len(ref)] if idx - len(ref) < len(ca) else 0


def check_edit_reads_the_edited_sequence(case, flat, rng):
    """Every position of ref' = ref[:p] + s + ref[p+d:] read through the map is that sequence's base, and the positions
    outside it fall into the read's contexts as seq_at has them."""
    R, k, central, p, d, s = case
    ref = rng.integers(0, ALPHABET, R).tolist()
    cb, ca = rng.integers(0, ALPHABET, 3).tolist(), rng.integers(0, ALPHABET, 4).tolist()
    edited = ref[:p] + list(s) + ref[p + d:]
    R2 = len(edited)
    pairs = flat[9 + 2 * (R2 + 1):]
    assert len(pairs) == 2 * (R2 + 2 * PAD)
    for n, at in enumerate(range(-PAD, R2 + PAD)):
        letter, src = pairs[2 * n], pairs[2 * n + 1]
        assert (letter if letter >= 0 else seq_at(ref, cb, ca, src)) == seq_at(edited, cb, ca, at), (case, at)


def most_letters(k, central):
    """The longest insertion in a read's interior that JOINT_ROWS rows hold."""
    return max(i for i in range(14) if edit_rows(40, k, central, 20, 0, i) <= JOINT_ROWS)


def edit_cases():
    rng = np.random.default_rng(52)
    out = []
    for k, central in SHAPES:
        for R in (3, 4, 8, 20):
            for p in range(1, R):
                for d in range(0, R - p):
                    for i in (0, 1, 2, 13, 14):
                        out.append((R, k, central, p, d, rng.integers(0, ALPHABET, i).tolist()))
        for d in (255, 256):                                 # the code's field for d
            for p, i in ((1, 0), (7, 2), (300 - 1 - d, 1)):
                out.append((300, k, central, p, d, rng.integers(0, ALPHABET, i).tolist()))
        # an interior insertion of i letters re-runs i + k - 1 rows (one more where no position before the edit holds
        # its first base in its k-mer): JOINT_ROWS, and one more
        for i in (most_letters(k, central), most_letters(k, central) + 1):
            out.append((40, k, central, 20, 0, rng.integers(0, ALPHABET, i).tolist()))
    return out


def test_edit_items_equal_the_restatement(lib):
    rng = np.random.default_rng(53)
    accepted = refused = 0
    for case in edit_cases():
        flat = got_edit(lib, case)
        assert flat == expected_edit(case), case
        if flat[0]:
            check_edit_reads_the_edited_sequence(case, flat, rng)
        accepted += flat[0]
        refused += 1 - flat[0]
    assert accepted > 1500 and refused > 1000


def test_edit_refusals(lib):
    ok = lambda *case: got_edit(lib, case)[0]
    for k, central in SHAPES:
        assert all(not ok(R, k, central, p, 0, [1] * 14) for R in (3, 4, 8, 20) for p in range(1, R))   # 14 letters
        assert ok(300, k, central, 7, 255, [0, 3]) and not ok(300, k, central, 7, 256, [0, 3])
        i = most_letters(k, central)
        assert edit_rows(40, k, central, 20, 0, i) == JOINT_ROWS and ok(40, k, central, 20, 0, [2] * i)
        assert edit_rows(40, k, central, 20, 0, i + 1) == JOINT_ROWS + 1 and not ok(40, k, central, 20, 0, [2] * (i + 1))
        # a base of the read stays on either side
        assert not ok(8, k, central, 0, 1, []) and ok(8, k, central, 1, 6, []) and not ok(8, k, central, 1, 7, [])
        assert not ok(8, k, central, 8, 0, [1]) and not ok(8, k, central, 3, -1, [1])
        assert not ok(8, k, central, 3, 0, [ALPHABET]) and not ok(8, k, central, 3, 0, [0, -1])
        assert got_edit(lib, (8, k, central, 3, 0, []))[1] == 0          # (d, i) = (0, 0): code 0


# ---------------------------------------------------------------------------------------------------------------------
# joints
# ---------------------------------------------------------------------------------------------------------------------
def expected_joint(case):
    """What ell_items_host_joint writes, restated: the substitutions h = [(pos, base), ...] on the read `ref`."""
    ref, k, central, h = case
    R, back, fwd = len(ref), k - central - 1, central
    prev = -1
    for pos, b in h:
        if not (prev < pos < R and 0 <= b < ALPHABET):
            return [0]
        prev = pos
    eff = [(pos, b) for pos, b in h if b != ref[pos]]       # the no-op entries are dropped
    if eff and eff[-1][0] - eff[0][0] >= JOINT_ROWS:
        return [0]
    rows = joint_rows(h, ref, k, central)
    if rows > JOINT_ROWS:
        return [0]
    p1 = eff[0][0] if eff else 0
    span = eff[-1][0] - p1 if eff else 0
    code = sum((8 | b) << (4 * (pos - p1)) for pos, b in eff) | span << 60
    first, last = (max(0, p1 - back), min(R - 1, p1 + span + fwd)) if eff else (0, 0)
    subs = dict(eff)
    return [1, code, p1, span, rows, first, last, 1] + [subs.get(j, -1) for j in range(-PAD, R + PAD)]


def joint_cases():
    rng = np.random.default_rng(54)
    out = []
    for k, central in SHAPES:
        ref = rng.integers(0, ALPHABET, 20).astype(np.int32)
        for start in (0, 5):                                 # windows clipped at row 0, and near the read's end
            for n in (1, 2, 3):
                for offs in itertools.combinations(range(JOINT_ROWS), n):
                    shift = rng.integers(1, ALPHABET, n)
                    for noop in itertools.product((False, True), repeat=n):
                        out.append((ref, k, central, [(start + o, int(ref[start + o] + (0 if z else sh)) % ALPHABET)
                                                      for o, sh, z in zip(offs, shift, noop)]))
    return out


def test_joint_items_equal_the_restatement(lib):
    accepted = refused = empty = 0
    for case in joint_cases():
        flat = got_joint(lib, case)
        assert flat == expected_joint(case), case[1:]
        accepted += flat[0]
        refused += 1 - flat[0]
        empty += flat[0] and flat[1] == 0
    assert accepted > 5000 and refused > 1000 and empty > 1000   # (the table holds enough of each)


def test_joint_refusals(lib):
    for k, central in SHAPES:
        ref = np.arange(40, dtype=np.int32) % ALPHABET
        sub = lambda p: (p, int(ref[p] + 1) % ALPHABET)
        same = lambda p: (p, int(ref[p]))
        ok = lambda *h: got_joint(lib, (ref, k, central, list(h)))[0]
        span = JOINT_ROWS - k                                # interior: span + k rows
        assert ok(sub(10), sub(10 + span)) and not ok(sub(10), sub(10 + span + 1))
        assert not ok(sub(3), sub(3 + JOINT_ROWS)) and ok(sub(3), same(3 + JOINT_ROWS))   # offset 14; dropped, it is none
        assert ok(sub(36), sub(39)) and not ok(sub(36), (40, 1))                          # outside the read
        assert not ok(sub(5), sub(5)) and not ok(sub(6), sub(5)) and not ok((-1, 0))       # not strictly ascending
        assert not ok((5, ALPHABET)) and not ok((5, -1))
        flat = got_joint(lib, (ref, k, central, [same(4), same(30)]))                      # no effective substitution
        assert flat[:5] == [1, 0, 0, 0, 0]
        flat = got_joint(lib, (ref, k, central, [same(2), sub(9), sub(9 + span), same(39)]))
        assert flat[2:4] == [9, span] and flat[1] >> 60 == span                            # plast - p1: the top nibble


# ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_under_the_sanitizers(tmp_path):
    """tests/host_shims/ell_items_main.cpp: a plain program with its own main, address + undefined-behaviour sanitizers
    linked in; every case of the two tables goes through the header in it and comes out as the restatements have it."""
    flags = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run(['g++'] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('the toolchain has no sanitizer runtimes')   # (an empty program: nothing of the code under test)
    exe = str(tmp_path / 'ell_items_main')
    build = subprocess.run(['g++'] + flags + [os.path.join(SHIMS, 'ell_items_main.cpp'), '-o', exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    edits, joints = edit_cases(), joint_cases()
    ints = lambda v: ' '.join(str(int(x)) for x in v)
    cases = tmp_path / 'cases.txt'
    with open(cases, 'w') as f:
        for R, k, central, p, d, s in edits:
            f.write('E %d %d %d %d %d %d %d %s\n' % (R, ALPHABET, k - central - 1, central, p, d, len(s), ints(s)))
        for ref, k, central, h in joints:
            f.write('J %d %d %d %d %d %s %s %s\n' % (len(ref), ALPHABET, k - central - 1, central, len(h), ints(ref),
                                                     ints(x[0] for x in h), ints(x[1] for x in h)))
    run = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(edits) + len(joints)
    for line, case in zip(lines, edits + joints):
        expected = expected_edit(case) if len(case) == 6 else expected_joint(case)
        assert _fix([int(x) for x in line.split()]) == expected, case[1:]
