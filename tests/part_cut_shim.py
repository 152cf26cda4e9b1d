"""The host build of nadavca_amd/csrc/part_cut.h (tests/host_shims/part_cut_host.cpp) as a ctypes library, for
tests/test_part_cut_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, 'tests', 'host_shims')


def build_shim(directory):
    """-> ctypes library of tests/host_shims/part_cut_host.cpp, built into ``directory``."""
    so = os.path.join(str(directory), 'part_cut_host.so')
    subprocess.run(['g++', '-O2', '-shared', '-fPIC', os.path.join(SHIMS, 'part_cut_host.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.part_cut_host.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.part_cut_host.restype = C.c_longlong
    return lib


def shim_cut(lib, off, cap):
    """-> (cut as a list, need) as cut_parts cuts the reads at ``off`` under ``cap`` units."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(off) - 1
    cut = np.full(n + 2, -1, dtype=np.int64)
    n_cut = C.c_longlong(0)
    need = lib.part_cut_host(off.ctypes.data, n, int(cap), cut.ctypes.data, C.addressof(n_cut))
    return [int(x) for x in cut[:n_cut.value]], int(need)
