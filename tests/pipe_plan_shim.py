"""The host build of nadavca_amd/csrc/pipe_plan.h (tests/host_shims/pipe_plan_host.cpp) as a ctypes library, shared by
tests/test_pipe_plan_cpu.py and tests/test_gpu_host_pipeline.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, 'tests', 'host_shims')
MAX_CHUNKS = 64          # pipe_plan::MAX_CHUNKS, the clamp of NADAVCA_E2E_CHUNKS
FLOOR_BYTES = 8 << 20    # the floor run_pipelined passes: a chunk holds at least 8 MiB of signal


def build_shim(directory):
    """-> ctypes library of tests/host_shims/pipe_plan_host.cpp, built into ``directory``."""
    so = os.path.join(str(directory), 'pipe_plan_host.so')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC',
                    os.path.join(SHIMS, 'pipe_plan_host.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.pipe_plan_host_schedule.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_double, C.c_longlong,
                                            C.c_longlong, C.c_void_p]
    lib.pipe_plan_host_schedule.restype = C.c_longlong
    lib.pipe_plan_host_layout.argtypes = [C.c_longlong] * 5 + [C.c_void_p]
    lib.pipe_plan_host_layout.restype = C.c_ulonglong
    lib.pipe_plan_host_rebase.argtypes = [C.c_void_p] * 5 + [C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.pipe_plan_host_rebase.restype = None
    return lib


def shim_schedule(lib, sig_off, n_chunks, growth, min_reads, floor_bytes=FLOOR_BYTES):
    """-> [(lo, hi), ...] as pipe_plan::chunk_schedule cuts the batch."""
    sig_off = np.ascontiguousarray(sig_off, dtype=np.int64)
    bounds = np.full(2 * MAX_CHUNKS, -1, dtype=np.int64)
    made = lib.pipe_plan_host_schedule(sig_off.ctypes.data, len(sig_off) - 1, int(n_chunks), float(growth),
                                       int(min_reads), int(floor_bytes), bounds.ctypes.data)
    return [(int(bounds[2 * c]), int(bounds[2 * c + 1])) for c in range(made)]
