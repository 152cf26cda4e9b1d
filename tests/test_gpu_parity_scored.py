"""Every built kernel of refine_alignment through the scored gate of the parity contract (include/nadavca_hip.h):
per read, the events equal the CPU oracle's, or the read carries NVK_TIE_ULP | NVK_TIE_NEAR AND its path scores as
well as the reference's on the reference's own path objective, to within NVK_TIE_ULPS ulps of the reference's log
score per differing row, in 80-bit arithmetic (fuzz_cases.classify_difference); a 'flat-plateau' difference needs
the plateau mark as well.  The contract is test_gpu_parity_full._fuzz_contract, run here on the smallest shapes that
reach each kernel variant (select_sweeps, kernels_align3.hip; the exact kernel, kernels_align.hip):

* one wave per read: min event length 0-4 x transition rows on/off;
* teams of four waves: min event length 0, 2, 4 x transition rows on/off, a narrow read in the same batch;
* few-level k-mer models, where differences really occur, and the PLATEAU table of tests/plan_cases.py;
* the exact kernel (NADAVCA_ALIGN_KERNEL=1), in a child process, on all of these.

Each campaign prints its reads, the differing reads per class and the largest deficit / margin."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 20261019
NO_CAP = 1.0   # these campaigns check every read; the caps on the differing share belong to test_gpu_parity_full


def _plan():
    """label -> (batch generator, seed, iterations)"""
    from fuzz_cases import make_fuzz_batch, make_plateau_batch, make_run_batch, make_team_shape_batch
    return {'one wave per read': (make_run_batch, SEED, 10),
            'teams of four waves': (make_team_shape_batch, SEED, 6),
            'few-level models': (make_fuzz_batch, 20261004, 40),
            'plateau table': (make_plateau_batch, SEED, 8)}


def _campaign(oracle_port, label):
    from test_gpu_parity_full import _fuzz_contract
    make, seed, iters = _plan()[label]
    return _fuzz_contract(make, seed, iters, oracle_port, label, NO_CAP)


def _campaigns(oracle_port):
    """Every campaign of this file -> {label: stats of _fuzz_contract}."""
    return {label: _campaign(oracle_port, label) for label in _plan()}


def test_one_wave_per_read_kernels(oracle_port):
    """16 reads of 3-140 bases, bandwidth 8-60, on the packaged 6-mer model for each of min event length 0-4 x
    transition rows on/off; half of the reads homopolymer-rich, half quantised to 1/12."""
    assert _campaign(oracle_port, 'one wave per read')['reads'] == 160


def test_team_kernels(oracle_port):
    """The team reads of tests/plan_cases.py (300 and 90 bases, bandwidth 200) with a narrow read beside them, min
    event length 0, 2, 4 x transition rows on/off."""
    assert _campaign(oracle_port, 'teams of four waves')['reads'] == 20


def test_few_level_models(oracle_port):
    """Random k-mer models of few levels (make_fuzz_batch, 40 iterations) and the PLATEAU table: the reads on
    which the engine really differs from the reference, so the ones the score test has to explain."""
    st = _campaign(oracle_port, 'few-level models')
    assert st['reads'] > 150
    assert _campaign(oracle_port, 'plateau table')['reads'] == 16


def test_exact_kernel(oracle_port):
    """NADAVCA_ALIGN_KERNEL=1 sends every read to the exact scaled-number kernel (the fast kernels' fallback).  The
    variable is read at call time, so the campaigns run in a fresh child process that has it set from the start."""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")\n'
            'from oracle.oracle import Oracle\n'
            'import test_gpu_parity_scored as t\n'
            'st = t._campaigns(Oracle("port"))\n'
            'assert all(s["reads"] > 0 for s in st.values())\n'
            'print("EXACT-KERNEL-OK")\n' % (ROOT, ROOT))
    env = dict(os.environ, NADAVCA_ALIGN_KERNEL='1')
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and 'EXACT-KERNEL-OK' in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
