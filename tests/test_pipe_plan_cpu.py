"""CPU check behind nadavca_amd/csrc/pipe_plan.h, the host arithmetic of the pipelined host-pointer path
(csrc/pipeline.hip): the chunk schedule against a Python restatement of its rule — Python floats are the same IEEE
doubles, so equality is exact — on a table of edges and on seeded random batches; the pack layout (alignment, no
overlap, inside the total) with every subset of the payload arrays empty; the rebased offset arrays; and the edge table
once more through a stand-alone program built with the address and undefined-behaviour sanitizers.  What the lanes do
with these numbers on the GPU is tests/test_gpu_host_pipeline.py."""
import bisect
import itertools
import os
import subprocess

import numpy as np
import pytest

from pipe_plan_shim import MAX_CHUNKS, SHIMS, build_shim, shim_schedule

MIB = 1 << 20


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp('pipe_plan'))


def chunk_count(sig_off, asked, min_reads, floor_bytes):
    """Pieces the rule allows: as many as asked, unless that leaves a piece under ``floor_bytes`` of signal (8 bytes a
    sample) or under ``min_reads`` reads on average; never fewer than one."""
    n_reads = len(sig_off) - 1
    return max(1, min(asked, int(sig_off[-1]) * 8 // floor_bytes, n_reads // min_reads))


def restated_schedule(sig_off, asked, growth, min_reads, floor_bytes):
    """The rule of run_pipelined's comment: piece c's share of the signal is growth^c (a running product), its end
    is the first read whose offset reaches the cumulative share of the total, it takes at least one read, the last
    piece takes the rest, and pieces left without a read are dropped."""
    sig_off = [int(x) for x in sig_off]
    n_reads = len(sig_off) - 1
    pieces = chunk_count(sig_off, asked, min_reads, floor_bytes)
    weights = list(itertools.accumulate([growth] * (pieces - 1), lambda w, g: w * g, initial=1.0))
    whole = 0.0
    for w in weights:
        whole += w
    out, lo, share = [], 0, 0.0
    for c, w in enumerate(weights):
        share += w
        if c == pieces - 1:
            hi = n_reads
        else:
            target = int(float(sig_off[-1]) * (share / whole))
            hi = max(bisect.bisect_left(sig_off, target, lo, n_reads), lo + 1)
        hi = min(hi, n_reads)
        if hi > lo:
            out.append((lo, hi))
            lo = hi
    return out


def _off(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def edge_table():
    """(name, sig_off, chunks asked, growth, min_reads, floor_bytes)"""
    rng = np.random.default_rng(7)
    uniform = lambda n, lo=3000, hi=5000: rng.integers(lo, hi, n)
    t = []
    t.append(('one_read', _off([4000]), 3, 2.0, 1, 1024))
    t.append(('one_read_many_asked', _off([1 << 22]), 64, 2.0, 1, 8 * MIB))
    t.append(('no_signal', _off([0] * 9), 3, 2.0, 1, 8 * MIB))            # count 0, clamped to 1
    t.append(('min_reads_above_n', _off(uniform(50)), 4, 2.0, 51, 1024))
    first = uniform(40, 10, 20)
    first[0] = 99 * int(first[1:].sum())
    t.append(('first_read_has_99_percent', _off(first), 5, 2.0, 1, 64))   # later chunks: one read each
    last = uniform(40, 10, 20)
    last[-1] = 99 * int(last[:-1].sum())
    t.append(('last_read_has_99_percent', _off(last), 5, 2.0, 1, 64))     # chunk 0 takes everything: the rest skipped
    only = [0] * 30
    only[0] = 1000
    t.append(('all_signal_in_read_0', _off(only), 5, 2.0, 1, 64))
    only_last = [0] * 30
    only_last[-1] = 1000
    t.append(('all_signal_in_the_last_read', _off(only_last), 5, 2.0, 1, 64))
    zeros = [100] * 10 + [0] * 10 + [100] * 10                            # boundary of 2 equal chunks inside the run
    t.append(('zero_reads_on_a_boundary', _off(zeros), 2, 1.0, 1, 64))
    t.append(('zero_reads_on_every_boundary', _off(([100] * 3 + [0] * 4) * 8), 8, 1.0, 1, 64))
    t.append(('64_chunks_of_64_reads', _off([4096] * 64), 64, 1.0, 1, 64))
    t.append(('64_chunks_of_64_reads_growing', _off(uniform(64)), 64, 2.0, 1, 64))
    for g in (1.0, 2.0, 10.0):
        t.append(('growth_%g' % g, _off(uniform(1300, 400, 8000)), 5, g, 1, 64))
        t.append(('growth_%g_min_reads' % g, _off(uniform(1300, 400, 8000)), 5, g, 400, 64))
    sig = _off(uniform(600))                                              # ~2.4 M samples = ~18 MiB
    t.append(('floor_binds', sig, 5, 2.0, 1, 8 * MIB))                    # 2 pieces of at least 8 MiB
    t.append(('floor_does_not_bind', sig, 5, 2.0, 1, 2 * MIB))
    t.append(('floor_above_the_batch', sig, 5, 2.0, 1, 64 * MIB))
    return t


def check_properties(chunks, sig_off, asked, min_reads, floor_bytes):
    n_reads = len(sig_off) - 1
    assert chunks[0][0] == 0 and chunks[-1][1] == n_reads
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))            # in order, nothing left out
    assert all(hi > lo for lo, hi in chunks)                                # at least one read each
    assert 1 <= len(chunks) <= chunk_count(sig_off, asked, min_reads, floor_bytes)
    assert len(chunks) <= min(asked, MAX_CHUNKS)


@pytest.mark.parametrize('case', edge_table(), ids=[c[0] for c in edge_table()])
def test_schedule_edges_equal_the_restated_rule(lib, case):
    name, sig_off, asked, growth, min_reads, floor_bytes = case
    got = shim_schedule(lib, sig_off, asked, growth, min_reads, floor_bytes)
    assert got == restated_schedule(sig_off, asked, growth, min_reads, floor_bytes)
    check_properties(got, sig_off, asked, min_reads, floor_bytes)


def test_the_edges_are_what_their_names_say(lib):
    by_name = {c[0]: shim_schedule(lib, *c[1:]) for c in edge_table()}
    assert by_name['one_read'] == by_name['one_read_many_asked'] == [(0, 1)]
    assert by_name['no_signal'] == [(0, 9)]
    assert by_name['min_reads_above_n'] == [(0, 50)]
    assert by_name['first_read_has_99_percent'][:4] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert by_name['last_read_has_99_percent'] == [(0, 40)]
    assert by_name['all_signal_in_read_0'] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 30)]
    assert by_name['all_signal_in_the_last_read'] == [(0, 30)]
    assert by_name['zero_reads_on_a_boundary'] == [(0, 10), (10, 30)]      # the run goes to the later chunk
    assert len(by_name['zero_reads_on_every_boundary']) == 8
    assert by_name['64_chunks_of_64_reads'] == [(i, i + 1) for i in range(64)]
    assert len(by_name['floor_binds']) == 2 and len(by_name['floor_does_not_bind']) == 5
    assert by_name['floor_above_the_batch'] == [(0, 600)]
    for g in (1.0, 2.0, 10.0):
        assert len(by_name['growth_%g' % g]) == 5 and len(by_name['growth_%g_min_reads' % g]) == 3
    sizes = [hi - lo for lo, hi in by_name['growth_10']]
    assert sizes == sorted(sizes) and sizes[-1] > 1000


def test_schedule_random_cases_equal_the_restated_rule(lib):
    rng = np.random.default_rng(20250)
    several = 0
    for trial in range(2000):
        n_reads = int(rng.integers(1, 400))
        kind = trial % 4
        if kind == 0:
            lengths = rng.integers(0, 2000, n_reads)
        elif kind == 1:
            lengths = rng.integers(0, 3, n_reads) * rng.integers(0, 5000, n_reads)      # many empty reads
        elif kind == 2:
            lengths = np.rint(rng.lognormal(6, 2, n_reads)).astype(np.int64)            # a few reads hold most
        else:
            lengths = np.full(n_reads, int(rng.integers(0, 50)))
        sig_off = _off(lengths)
        asked = int(rng.integers(1, MAX_CHUNKS + 1))
        growth = int(rng.integers(100, 1001)) / 100.0
        min_reads = int(rng.choice([1, 1, 2, 7, 50, 500]))
        floor_bytes = int(rng.choice([1, 64, 4096, 1 << 16, 1 << 20]))
        got = shim_schedule(lib, sig_off, asked, growth, min_reads, floor_bytes)
        assert got == restated_schedule(sig_off, asked, growth, min_reads, floor_bytes), trial
        check_properties(got, sig_off, asked, min_reads, floor_bytes)
        several += len(got) > 2
    assert several > 600


def shim_layout(lib, n, tr, tb, ta, tn):
    at = np.zeros(9, dtype=np.uint64)
    total = lib.pipe_plan_host_layout(n, tr, tb, ta, tn, at.ctypes.data)
    return [int(x) for x in at], int(total)


def test_layout_keeps_arrays_apart_aligned_and_inside(lib):
    rng = np.random.default_rng(3)
    shapes = [(1, 1, 1, 1, 1), (1, 16, 16, 16, 8), (7, 15, 17, 33, 9), (1300, 500000, 2600, 3900, 300000)]
    shapes += [tuple(int(x) for x in rng.integers(1, 3000, 5)) for _ in range(200)]
    for n, tr, tb, ta, tn in shapes:
        for empty in itertools.product((False, True), repeat=4):             # every subset of the payload arrays
            tr_, tb_, ta_, tn_ = (0 if e else v for e, v in zip(empty, (tr, tb, ta, tn)))
            at, total = shim_layout(lib, n, tr_, tb_, ta_, tn_)
            sizes = [(n + 1) * 8] * 5 + [tr_ * 4, tb_ * 4, ta_ * 4, tn_ * 8]
            assert at[0] == 0 and all(a % 16 == 0 for a in at)
            # (an empty array still gets a 64-byte granule of its own: no kernel argument aliases its neighbour)
            ends = [a + (s if s else 64) for a, s in zip(at, sizes)]
            assert all(e <= b for e, b in zip(ends, at[1:])) and ends[-1] <= total
            assert len(set(at)) == 9
            assert total <= sum(sizes) + 9 * 64 + 4 * 64                      # ... and no more than padding on top


def test_rebased_offsets_start_at_zero_and_keep_the_differences(lib):
    rng = np.random.default_rng(4)
    n_reads = 500
    offs = [_off(rng.integers(0, hi, n_reads) * (rng.random(n_reads) < keep)) for hi, keep in
            ((5000, 1.0), (800, 1.0), (4, 0.5), (5, 0.5), (300, 0.8))]
    for a, b in [(0, 500), (0, 1), (499, 500), (17, 18), (100, 357), (1, 499)] + \
            [tuple(sorted(int(x) for x in rng.choice(501, 2, replace=False))) for _ in range(100)]:
        n = b - a
        tot = [int(o[b] - o[a]) for o in offs]
        at, total = shim_layout(lib, n, tot[1], tot[2], tot[3], tot[4])
        buf = np.full(total, 0xAB, dtype=np.uint8)
        lib.pipe_plan_host_rebase(*[o.ctypes.data for o in offs], a, n, np.array(at, dtype=np.uint64).ctypes.data,
                                  buf.ctypes.data)
        written = np.zeros(total, dtype=bool)
        for q in range(5):
            got = buf[at[q]:at[q] + (n + 1) * 8].view(np.int64)
            assert got[0] == 0 and got[-1] == tot[q]
            assert np.array_equal(np.diff(got), np.diff(offs[q][a:b + 1]))
            written[at[q]:at[q] + (n + 1) * 8] = True
        assert np.all(buf[~written] == 0xAB)                                 # nothing written beside the five arrays


def test_edge_table_under_the_sanitizers(lib, tmp_path):
    """tests/host_shims/pipe_plan_main.cpp: a plain program with its own main, address + undefined-behaviour
    sanitizers linked in; the edge table goes through the header in it and comes out as the restated rule has it."""
    exe = str(tmp_path / 'pipe_plan_main')
    build = subprocess.run(['g++', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=all', os.path.join(SHIMS, 'pipe_plan_main.cpp'), '-o', exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if build.returncode != 0:
        if 'asan' in build.stdout or 'ubsan' in build.stdout or 'sanitize' in build.stdout:
            pytest.skip('the toolchain has no sanitizer runtimes')
        raise AssertionError(build.stdout)
    table = edge_table()
    cases = tmp_path / 'cases.txt'
    with open(cases, 'w') as f:
        for name, sig_off, asked, growth, min_reads, floor_bytes in table:
            f.write('%d %d %r %d %d %s\n' % (len(sig_off) - 1, asked, float(growth), min_reads, floor_bytes,
                                             ' '.join(str(int(x)) for x in sig_off)))
    run = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(table)
    for line, (name, sig_off, asked, growth, min_reads, floor_bytes) in zip(lines, table):
        v = [int(x) for x in line.split()]
        got = list(zip(v[1::2], v[2::2]))
        assert v[0] == len(got) and got == restated_schedule(sig_off, asked, growth, min_reads, floor_bytes), name
