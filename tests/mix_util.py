"""Helpers of the opponent-mix tests (tests/test_opponent_mix*.py): per-episode opponent classes on oracle rows and device handles."""
import ctypes

import numpy as np

from cage_challenge_4_amd import _lib as L

KEEP, DEFAULT = L.POLICY_KEEP, L.POLICY_DEFAULT
COMBOS = [(r, g, b) for r in range(4) for g in range(2) for b in range(2)]      # all 16 assignable (red, green, blue) classes


def policy_bits(red, green, blue):
    """The `policy` argument of the oracle's regenerations for a handle of these classes (policy_bits, csrc/cc4_api.hip)."""
    return (red & 3) | (0x10 if green else 0) | (0x20 if blue else 0)


def _ptr(row):
    return row.ctypes.data_as(ctypes.c_void_p) if isinstance(row, np.ndarray) else ctypes.c_void_p(row)


def row_set(row, red, green, blue):
    """cc4_row_set_policies on a hot row: a uint8 array (edited in place) or an address (an oracle's row).  Returns the call's result."""
    return int(L.load().cc4_row_set_policies(_ptr(row), int(red), int(green), int(blue)))


def row_get(row):
    """cc4_row_get_policies: (live, assigned) as tuples (red, green, blue)."""
    live, assigned = (ctypes.c_int8 * 3)(), (ctypes.c_int8 * 3)()
    assert L.load().cc4_row_get_policies(_ptr(row), live, assigned) == 0
    return tuple(live), tuple(assigned)


def assign_offset():
    """The byte of the hot row that holds the assignment: found from what cc4_row_set_policies changes in an all-zero row, not assumed."""
    row = np.zeros(L.load().cc4_state_bytes(), np.uint8)
    assert row_set(row, 3, 1, 1) == 0
    at = np.nonzero(row)[0]
    assert at.size == 1, at
    return int(at[0])


def oracle_row(ora, i):
    return ora.lib.cc4o_state_ptr(ora._h, int(i))


def oracle_assign(ora, i, red, green, blue):
    """Edit episode i of an OracleVecEnv as cc4_set_policies edits a device row."""
    assert row_set(oracle_row(ora, i), red, green, blue) == 0, (i, red, green, blue)


def without_assignment(rows):
    """Hot rows ([..., cc4_state_bytes] uint8) with the assignment byte cleared: what a mixed and a uniform handle must agree in."""
    rows = np.array(rows, copy=True)
    rows[..., assign_offset()] = 0
    return rows


def run_plan_packed(env, plan):
    """cc4_run_plan_device on a CC4VecEnv with the recorded observations left packed (2 bits per value): (rewards [k, n] float32, dones [k, n] uint8,
    packed [k, n, 148] uint8).  CC4VecEnv.run_plan unpacks them to 578 bytes per row, which at 6656 episodes x 100 steps is most of a test's time."""
    from cage_challenge_4_amd.vec_env import Staged, as_actions
    plan = as_actions(plan, env.num_envs, 0)
    k, n = plan.shape[:2]
    vp = ctypes.c_void_p
    b_rew, b_pk, b_done = 4 * k * n, L.OBS_PACKED_BYTES * k * n, k * n
    with Staged(env._dev, [plan, (b_rew + b_pk + b_done, 16)]) as st:
        d_out = st.ptr(1).value
        rc = env.lib.cc4_run_plan_device(env._h, k, st.ptr(0), None, vp(d_out), vp(d_out + b_rew + b_pk), vp(d_out + b_rew))
        rc2 = env.lib.cc4_synchronize(env._h)
        env._chk(rc or rc2, 'cc4_run_plan_device')
        out = st.down(1, np.empty(b_rew + b_pk + b_done, np.uint8))
    return (out[:b_rew].view(np.float32).reshape(k, n), out[b_rew + b_pk:].reshape(k, n), out[b_rew:b_rew + b_pk].reshape(k, n, L.OBS_PACKED_BYTES))


def final_outputs(env):
    """The handle's outputs as they stand (no error check: a strict=False handle): observations, reward, done, error words, action masks."""
    vp = ctypes.c_void_p
    env.synchronize()
    env._chk(env.lib.cc4_fetch(env._h, *env._p_out), 'cc4_fetch')
    env._chk(env.lib.cc4_get_action_mask(env._h, env._mask.ctypes.data_as(vp)), 'cc4_get_action_mask')
    return env._obs.copy(), env._rew.copy(), env._done.copy(), env._err.copy(), env._mask.copy()
