"""CPU check behind nadavca_amd/csrc/plan_key.h, the comparison that decides whether a refine_alignment call may sweep
from the plan its context holds (csrc/api.hip: plan once, sweep again): an equal key matches, a key that differs in any
single field does not, token 0 never matches and neither does a cleared key — through a g++ shim
(tests/host_shims/plan_key_host.cpp), and the same table once more in a stand-alone program built with the address and
undefined-behaviour sanitizers.  What the library does with the answer on the GPU is tests/test_gpu_plan_reuse.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SHIMS = os.path.join(ROOT, 'tests', 'host_shims')
FIELDS = ('token', 'model_id', 'bandwidth', 'mel', 'transitions', 'rows_written', 'n_reads', 'total_signal',
          'total_ref', 'total_anchors', 'sig_off', 'reference', 'ref_off', 'ctx_before', 'cb_off', 'ctx_after',
          'ca_off', 'anchors', 'anc_off')
FLAGS = ('transitions', 'rows_written')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp('plan_key')), 'plan_key_host.so')
    subprocess.run(['g++', '-O2', '-shared', '-fPIC', os.path.join(SHIMS, 'plan_key_host.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    for fn in (lib.plan_key_host_matches, lib.plan_key_host_matches_cleared):
        fn.argtypes = [C.c_void_p, C.c_void_p]
        fn.restype = C.c_int
    assert lib.plan_key_host_fields() == len(FIELDS)
    return lib


def _key(**change):
    """A key with every field set and no two fields alike, ``change`` applied."""
    v = {name: 0x7f0000001000 + 4096 * i if i >= 10 else 1000 + 16 * i for i, name in enumerate(FIELDS)}
    v.update(transitions=1, rows_written=0)
    v.update(change)
    return np.array([v[name] for name in FIELDS], dtype=np.int64)


def _matches(lib, held, want, fn='plan_key_host_matches'):
    return bool(getattr(lib, fn)(held.ctypes.data, want.ctypes.data))


def test_an_equal_key_matches(lib):
    assert _matches(lib, _key(), _key())
    assert _matches(lib, _key(token=2 ** 63 - 1), _key(token=2 ** 63 - 1))


@pytest.mark.parametrize('field', FIELDS)
def test_every_single_differing_field_refuses(lib, field):
    base = _key()
    at = FIELDS.index(field)
    others = [1 - int(base[at])] if field in FLAGS else [int(base[at]) + 1, int(base[at]) - 1, 0,
                                                         int(base[at]) + (1 << 32)]
    for value in others:
        if field in ('bandwidth', 'mel') and value >= 1 << 31:
            continue   # (32-bit fields)
        other = _key(**{field: value})
        assert not _matches(lib, base, other), (field, value)
        assert not _matches(lib, other, base), (field, value)
        assert _matches(lib, other, other) == (field != 'token' or value != 0)


def test_token_zero_refuses(lib):
    zero = _key(token=0)
    assert not _matches(lib, zero, zero)
    assert not _matches(lib, zero, _key()) and not _matches(lib, _key(), zero)


def test_a_cleared_key_refuses(lib):
    assert not _matches(lib, _key(), _key(), fn='plan_key_host_matches_cleared')
    # (... whatever is asked of it: cleared fields equal those of an all-zero request, whose token is 0)
    nothing = np.zeros(len(FIELDS), dtype=np.int64)
    assert not _matches(lib, _key(), nothing, fn='plan_key_host_matches_cleared')
    assert not _matches(lib, nothing, nothing)


def test_the_table_under_the_sanitizers(tmp_path):
    """tests/host_shims/plan_key_main.cpp: a plain program with its own main, address + undefined-behaviour sanitizers
    linked in, that walks the same table; exit status 0 passes."""
    exe = str(tmp_path / 'plan_key_main')
    build = subprocess.run(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(SHIMS, 'plan_key_main.cpp'), '-o', exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if build.returncode != 0:
        if 'asan' in build.stdout or 'ubsan' in build.stdout or 'sanitize' in build.stdout:
            pytest.skip('the toolchain has no sanitizer runtimes')
        raise AssertionError(build.stdout)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert '%d fields ok' % len(FIELDS) in run.stdout
