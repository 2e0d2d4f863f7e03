"""CPU: the surface of the device-resident action plans (cc4_run_plan_device) -- the three entry points through header, library and binding, the
Python methods, the plan kernels in the build's resource table, and the host-side unpacking of packed observation rows."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

PLAN_SYMBOLS = ('cc4_run_plan_device', 'cc4_plan_kernel_for', 'cc4_unpack_rows_device')


def test_plan_entry_points_are_declared_exported_and_bound():
    from cage_challenge_4_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'cc4.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in PLAN_SYMBOLS:
        assert re.search(r'\b' + s + r'\s*\(', txt), f'{s} is not declared in include/cc4.h'
        assert hasattr(lib, s), f'{s} is not exported by libcc4.so'
        assert s in _lib.SIGNATURES, f'{s} is not bound in _lib.py'
    assert len(_lib.SIGNATURES['cc4_run_plan_device'][1]) == 7
    assert f'#define CC4_OBS_PACKED_BYTES {_lib.OBS_PACKED_BYTES}' in open(os.path.join(ROOT, 'include', 'cc4.h')).read()


def test_python_surface_exists():
    from cage_challenge_4_amd import CC4VecEnv
    assert callable(getattr(CC4VecEnv, 'run_plan', None)) and callable(getattr(CC4VecEnv, 'plan_kernel_for', None))
    torch_env = pytest.importorskip('cage_challenge_4_amd.torch_env')
    assert callable(getattr(torch_env.CC4TorchVecEnv, 'step_plan', None))


def test_plan_kernels_are_in_the_resource_table_at_their_parents_occupancy():
    """profiles/kernel_resources.txt is written by build() from the compilations that made the library: the plan builds are there, within the
    register budget of six waves per SIMD (<= 80 VGPRs) like the kernels they are builds of."""
    rows = {}
    for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')):
        m = re.match(r'_Z(\d+)(\S+)\s+vgpr\s+(\d+)', ln)       # Itanium mangling: the length of the name, then the name
        if m:
            rows.setdefault(m.group(2)[:int(m.group(1))], int(m.group(3)))
    for plan, parent in (('k_run_philox1p', 'k_run_philox1'), ('k_run_pcgp', 'k_run_pcg')):
        assert plan in rows and parent in rows, (plan, sorted(rows))
        assert rows[plan] <= 80 and rows[parent] <= 80, (plan, rows[plan], rows[parent])
    for helper in ('k_plan_collect', 'k_plan_finish', 'k_unpack_rows'):
        assert helper in rows, helper


def test_plan_unit_is_built_with_the_library():
    """The plan build is an entry of its own in a unit the Makefile lists (build() lints every listed unit's ISA with tools/isa_scan.py and fails on a
    finding); the headline kernel's unit knows nothing of it."""
    csrc = os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc')
    src = open(os.path.join(csrc, 'cc4_k_plan.hip')).read()
    assert 'k_run_philox1p' in src and 'persist_loop<false, false, false, true>' in src
    assert re.search(r'^UNITS\s*=.*\bcc4_k_plan\b', open(os.path.join(csrc, 'Makefile')).read(), flags=re.M)
    assert 'PlanArgs' not in open(os.path.join(csrc, 'cc4_k_run1.hip')).read()


def test_unpack_obs_rows_inverts_the_packing():
    from cage_challenge_4_amd.vec_env import unpack_obs_rows
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 3, size=(3, 4, 578)).astype(np.uint8)
    padded = np.zeros((3, 4, 592), np.uint8)
    padded[..., :578] = vals
    q = padded.reshape(3, 4, 148, 4)
    packed = (q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)).astype(np.uint8)
    assert np.array_equal(unpack_obs_rows(packed), vals)
