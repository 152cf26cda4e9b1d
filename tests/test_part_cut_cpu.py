"""CPU check behind nadavca_amd/csrc/part_cut.h, the host arithmetic that cuts a batch into parts under a workspace cap
(seed extension, event alignment, Viterbi decode, k-mer posteriors): ``cut_parts`` against a plain-Python restatement
of its rule, with exact integer equality, on a table of edges and on seeded random offset arrays; the properties the
callers rely on; and the edge table once more through a stand-alone program built with the address and
undefined-behaviour sanitizers.  What the kernels do with the parts on the GPU is the small-workspace tests of
tests/test_gpu_decode_kernels.py, test_gpu_posterior_kernels.py and test_gpu_signal_map_kernels.py."""
import os
import subprocess

import numpy as np
import pytest

from part_cut_shim import SHIMS, build_shim, shim_cut


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp('part_cut'))


def restated_cut(off, cap):
    """The rule in words: reads join the current part one after another; a read that would take the part above ``cap``
    units starts the next one, unless the part is still empty (a read larger than the cap is a part of one).  ``need``
    is the largest part's units, at least 1.  No reads: the cut is [0, 0]."""
    sizes = [int(b) - int(a) for a, b in zip(off[:-1], off[1:])]
    cut, held, count, need = [0], 0, 0, 1
    for r, size in enumerate(sizes):
        if count > 0 and held + size > cap:
            need = max(need, held)
            cut.append(r)
            held, count = 0, 0
        held += size
        count += 1
    return cut + [len(sizes)], max(need, held)


def _off(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def decode_shape():
    """Offsets like the decode kernel test's k = 6 batch: 64 reads, 256 words of traceback per event but the first"""
    events = np.random.default_rng(11).integers(150, 900, 64)
    return _off((events - 1) * 256)


def edge_table():
    """(name, off, cap)"""
    t = [('no_reads', _off([]), 100), ('no_reads_cap_0', _off([]), 0)]
    t += [('one_read', _off([40]), 100), ('one_read_above_the_cap', _off([400]), 100), ('one_empty_read', _off([0]), 0)]
    t += [('all_reads_empty', _off([0] * 9), 5), ('all_reads_empty_cap_0', _off([0] * 9), 0)]
    t += [('cap_0', _off([3, 0, 0, 2, 1, 0]), 0)]
    same = _off([10] * 6)
    t += [('cap_one_below_a_read', same, 9), ('cap_a_read', same, 10), ('cap_one_above_a_read', same, 11),
          ('cap_one_below_two_reads', same, 19), ('cap_two_reads', same, 20)]
    mixed = _off([5, 80, 3, 0, 2, 90, 90, 1, 1, 70, 4])
    t += [('cap_below_the_largest_reads', mixed, 10), ('cap_the_total', mixed, int(mixed[-1])),
          ('cap_one_below_the_total', mixed, int(mixed[-1]) - 1), ('cap_above_the_total', mixed, 1 << 40)]
    dec = decode_shape()
    t += [('decode_third', dec, int(dec[-1]) // 3), ('decode_seventh', dec, int(dec[-1]) // 7),
          ('decode_below_the_largest_read', dec, int(np.diff(dec).max()) - 1)]
    return t


def check_properties(off, cap, cut, need):
    n = len(off) - 1
    units = lambda a, b: int(off[b]) - int(off[a])
    assert cut[0] == 0 and cut[-1] == n and len(cut) >= 2
    if n == 0:
        assert cut == [0, 0] and need == 1
        return
    assert all(a < b for a, b in zip(cut, cut[1:]))                          # strictly ascending: no empty part
    parts = list(zip(cut, cut[1:]))
    assert all(units(a, b) <= cap or b - a == 1 for a, b in parts)           # fits the cap, or is a single read
    # greedy: a part with the next part's first read would not have fitted
    assert all(units(a, b + 1) > cap for a, b in parts[:-1])
    assert need == max([1] + [units(a, b) for a, b in parts])


@pytest.mark.parametrize('case', edge_table(), ids=[c[0] for c in edge_table()])
def test_edges_equal_the_restated_rule(lib, case):
    name, off, cap = case
    cut, need = shim_cut(lib, off, cap)
    assert (cut, need) == restated_cut(off, cap)
    check_properties(off, cap, cut, need)


def test_the_edges_are_what_their_names_say(lib):
    by_name = {name: shim_cut(lib, off, cap) for name, off, cap in edge_table()}
    assert by_name['no_reads'] == by_name['no_reads_cap_0'] == ([0, 0], 1)
    assert by_name['one_read'] == ([0, 1], 40) and by_name['one_read_above_the_cap'] == ([0, 1], 400)
    assert by_name['one_empty_read'] == ([0, 1], 1)
    assert by_name['all_reads_empty'] == by_name['all_reads_empty_cap_0'] == ([0, 9], 1)
    # (empty reads join an empty part; a part above the cap takes no further read, not even an empty one)
    assert by_name['cap_0'] == ([0, 1, 3, 4, 5, 6], 3)
    assert by_name['cap_one_below_a_read'] == by_name['cap_a_read'] == (list(range(7)), 10)
    assert by_name['cap_one_above_a_read'] == by_name['cap_one_below_two_reads'] == (list(range(7)), 10)
    assert by_name['cap_two_reads'] == ([0, 2, 4, 6], 20)
    assert by_name['cap_below_the_largest_reads'] == ([0, 1, 2, 5, 6, 7, 9, 10, 11], 90)
    assert by_name['cap_the_total'] == by_name['cap_above_the_total'] == ([0, 11], 346)
    assert len(by_name['cap_one_below_the_total'][0]) == 3
    assert len(by_name['decode_third'][0]) - 1 >= 3 and len(by_name['decode_seventh'][0]) - 1 >= 7
    assert by_name['decode_below_the_largest_read'][0] != list(range(65))    # small reads still share a part ...
    dec = decode_shape()
    assert by_name['decode_below_the_largest_read'][1] == int(np.diff(dec).max())   # ... and the largest is one alone


def test_random_cases_equal_the_restated_rule(lib):
    rng = np.random.default_rng(20251)
    several = alone = 0
    for trial in range(600):
        n = int(rng.integers(0, 65))
        kind = trial % 4
        if kind == 0:
            sizes = rng.integers(0, 2000, n)
        elif kind == 1:
            sizes = rng.integers(0, 3, n) * rng.integers(0, 5000, n)                    # many empty reads
        elif kind == 2:
            sizes = np.rint(rng.lognormal(6, 2, n)).astype(np.int64)                    # a few reads hold most
        else:
            sizes = np.full(n, int(rng.integers(0, 50)))
        off = _off(sizes)
        top = int(sizes.max()) if n else 0
        cap = int(rng.choice([0, 1, max(top - 1, 0), top, top + 1, int(off[-1]) // 3, int(off[-1]), 1 << 40,
                              int(rng.integers(0, max(int(off[-1]), 1) + 1))]))
        cut, need = shim_cut(lib, off, cap)
        assert (cut, need) == restated_cut(off, cap), trial
        check_properties(off, cap, cut, need)
        several += len(cut) > 3
        alone += n > 0 and need > cap
    assert several > 150 and alone > 50


def test_edge_table_under_the_sanitizers(lib, tmp_path):
    """tests/host_shims/part_cut_main.cpp: a plain program with its own main, address + undefined-behaviour sanitizers
    linked in; the edge table goes through the header in it and comes out as the restated rule has it."""
    exe = str(tmp_path / 'part_cut_main')
    build = subprocess.run(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(SHIMS, 'part_cut_main.cpp'), '-o', exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if build.returncode != 0:
        if 'asan' in build.stdout or 'ubsan' in build.stdout or 'sanitize' in build.stdout:
            pytest.skip('the toolchain has no sanitizer runtimes')
        raise AssertionError(build.stdout)
    table = edge_table()
    cases = tmp_path / 'cases.txt'
    with open(cases, 'w') as f:
        for name, off, cap in table:
            f.write('%d %d %s\n' % (len(off) - 1, cap, ' '.join(str(int(x)) for x in off)))
    run = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(table)
    for line, (name, off, cap) in zip(lines, table):
        v = [int(x) for x in line.split()]
        assert v[1] == len(v) - 2 and (v[2:], v[0]) == restated_cut(off, cap), name
