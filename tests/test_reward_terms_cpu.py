"""CPU: the reward terms -- which zone, which kind, whose Restore (include/cc4.h cc4_reward_terms_device; the definition: csrc/cc4_reward_terms.h).

* The surface: header, exports, bindings, constants, the kernel's resource row as committed in profiles/kernel_resources.txt (build() rewrites
  that file from the compiler's metadata of every build).
* tests/cpp/reward_terms_check.cpp, a program with its own main: built here with the host compiler at -O1 with the address and
  undefined-behaviour sanitizers and run as a child process (never loaded into Python), on crafted rows and records in heap blocks of exactly
  their size.
* On the oracle, whose engine is the same header the kernels compile: every scripted fixture recorded from the reference (brm and reward after
  every step entry), the three BlueRewardMachine fixtures cell by cell, 16 episodes x 300 steps in both RNG modes with both identities at every
  step, and the stale cases -- a step that did not record, a Restore stamp of the previous episode, the built-in blue policy's Restore, a Restore
  submitted while busy."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from cage_challenge_4_amd import blue_view as BV
from cage_challenge_4_amd import reward_terms as RT
from oracle_binding import OracleVecEnv
import reward_terms_util as U
import test_scripted as TS
from cpp_check import build_and_run

SRC = os.path.join(ROOT, 'tests', 'cpp', 'reward_terms_check.cpp')


def test_surface_header_exports_bindings_constants_and_resources():
    import ctypes
    from cage_challenge_4_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in (('cc4_enable_reward_terms', 2), ('cc4_reward_terms_enabled', 1), ('cc4_reward_terms_device', 7), ('cc4_reward_terms_from_row', 5)):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert f'#define CC4_REWARD_SUBNETS {RT.SUBNETS}\n' in txt and RT.SUBNETS == 9
    assert f'#define CC4_REWARD_COLS {RT.COLS}\n' in txt and RT.COLS == 4
    assert f'#define CC4_REWARD_WORDS {RT.NWORDS}\n' in txt and RT.NWORDS == 16
    assert sorted(RT.TERM_COLUMNS.values()) == list(range(4)) and sorted(RT.WORDS.values()) == list(range(16))
    assert RT.ZONE_OF_SUBNET == (0, 1, 2, 3, -1, 4, 4, 4, -1) and len(RT.SUBNET_NAMES) == 9
    from cage_challenge_4_amd.wrappers import SUBNET_NAMES, BLUE_SUBNETS
    assert list(RT.SUBNET_NAMES) == list(SUBNET_NAMES)
    for s, name in enumerate(RT.SUBNET_NAMES):
        owners = [b for b in range(5) if name in BLUE_SUBNETS[b]]
        assert owners == ([RT.ZONE_OF_SUBNET[s]] if RT.ZONE_OF_SUBNET[s] >= 0 else []), name
    for name, c in RT.TERM_COLUMNS.items():          # the header's table names every column, in order
        assert re.search(rf'\*\s+{c} {name}\b', txt), name
    rows = [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if 'k_reward_terms' in ln]
    assert len(rows) == 1 and rows[0].rstrip().endswith('cc4_k_reward.hip'), rows
    assert re.search(r'scratch\s+0 vgpr_spill\s+0 sgpr_spill\s+0 ', rows[0]), rows[0]
    assert 4 * 36 <= int(re.search(r'lds_static\s+(\d+)', rows[0]).group(1)) <= 1280, rows[0]      # the 36 cells; one of LDS's 1280-byte granules


def test_importing_the_module_imports_neither_torch_nor_the_oracle():
    code = ("import sys; import cage_challenge_4_amd; from cage_challenge_4_amd import reward_terms; "
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.') or 'oracle' in m]; assert not bad, bad")
    run = subprocess.run([sys.executable, '-c', 'import sys; sys.path.insert(0, %r); ' % ROOT + code], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


def test_serial_statement_on_crafted_rows_under_the_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300, flags=['-ffp-contract=off'])
    assert ' 0 mismatches' in run.stdout, run.stdout


# ------------------------------------------------------------------------------------------------ the reference's scripted tests, on the oracle
def _replay(env, case):
    for e in U.replay_scripted(env, case, TS._records):
        terms, words = RT.from_row(env.get_state(0), env.get_cold(0), case['steps'])
        yield e, terms, words


@pytest.mark.parametrize('name', TS.NAMES)
def test_brm_and_reward_of_every_scripted_step_recorded_from_the_reference(name):
    fx = TS._load(name)
    total = 0
    for case in fx['cases']:
        env = OracleVecEnv(1, steps=case['steps'], red_policy=case['red_policy'], green_policy=case['green_policy'])
        for k, (e, terms, words) in enumerate(_replay(env, case)):
            ex, where = e['expect'], (name, case.get('note', ''), k)
            assert words[0] == 1, where
            assert words[3] == ex['brm'] and words[3] + words[4] == ex['reward'], (where, words[:5].tolist(), ex['brm'], ex['reward'])
            U.check_identities(terms[None], words[None], np.array([ex['reward']], np.float32), where)
            total += 1
        env.close()
    assert total > 0


@pytest.mark.parametrize('name,col,steps,nonzero', U.BRM_FIXTURES)
def test_the_blue_reward_machine_fixtures_cell_by_cell(name, col, steps, nonzero):
    """Sleeping red and green classes, one submitted action per step: the only non-zero penalty is [host // 17 of the submitted record, its
    kind], it equals brm, and a failed action counts as an event whatever its weight."""
    fx = TS._load(name)
    n = nz = zero_weight_events = 0
    for case in fx['cases']:
        assert case['red_policy'] == 1 and case['green_policy'] == 1
        env = OracleVecEnv(1, steps=case['steps'], red_policy=1, green_policy=1)
        for k, (e, terms, words) in enumerate(_replay(env, case)):
            want = U.brm_cells(e, col)
            assert np.array_equal(terms, want), ((name, case.get('note', ''), k), terms.tolist(), want.tolist())
            zero_weight_events += int(want[:, 3].any() and e['expect']['brm'] == 0)
            n += 1
            nz += e['expect']['brm'] != 0
        env.close()
    assert (n, nz) == (steps, nonzero)
    assert zero_weight_events >= 1, 'no charged event with weight 0 in this fixture'


# ------------------------------------------------------------------------------------------------ trajectories
@pytest.mark.parametrize('mode', [1, 0], ids=['counter', 'numpy'])
def test_both_identities_on_16_episodes_of_300_steps(mode):
    n, T, seed = 16, 300, 77
    ora = OracleVecEnv(n, steps=500, rng_mode=mode)
    ora.reset(seeds=seed)
    share = dict(lwf=0, asf=0, ria=0, restore=0)
    for t in range(T):
        obs, rew, done, info = ora.step_ex(U.blue_mix(seed, t, n), None, None, None)
        assert not info['err'].any()
        terms, words = U.from_rows(ora, range(n), 500)
        assert (words[:, 0] == 1).all() and (words[:, 1] == t + 1).all(), t
        U.check_identities(terms, words, rew, (mode, t))
        share['lwf'] += int((terms[..., 0].sum(1) != 0).sum()); share['asf'] += int((terms[..., 1].sum(1) != 0).sum())
        share['ria'] += int((terms[..., 2].sum(1) != 0).sum()); share['restore'] += int((words[:, 4] != 0).sum())
    ora.close()
    print('share of episode-steps with a non-zero term, mode', mode, {k: round(v / (n * T), 4) for k, v in share.items()})
    for k, v in share.items():          # not vacuous: every kind occurs on at least 1 % of the compared episode-steps
        assert v >= 0.01 * n * T, (k, v, share)


# ------------------------------------------------------------------------------------------------ staleness
def _tw(ora, e=0):
    return RT.from_row(ora.get_state(e), ora.get_cold(e), ora.steps)


@pytest.mark.parametrize('mode', [1, 0], ids=['counter', 'numpy'])
def test_a_step_that_did_not_record_leaves_valid_0_and_zeros(mode):
    ora = OracleVecEnv(2, steps=60, rng_mode=mode)
    ora.reset(seeds=500)
    terms, words = _tw(ora)
    assert words[0] == 0 and not terms.any() and words[1] == 0, 'a fresh episode'
    some = 0
    for t in range(12):
        _, rew, _, _ = ora.step_ex(U.blue_mix(500, t, 2), None, None, None)
        terms, words = _tw(ora)
        assert words[0] == 1 and words[3] + words[4] == rew[0]
        some += int(terms.any())
        ora.step(U.blue_mix(501, t, 2))                    # the fast path: no record of this step
        terms, words = _tw(ora)
        assert words[0] == 0 and words[1] == 2 * t + 2 and not terms.any() and not words[3:].any(), t
        assert RT.from_row(ora.get_state(0), None, 60)[1][0] == 0          # no cold row
    assert some >= 3
    # cc4_edit_state(SE_SET_STEP): the row's step count no longer is the record's
    ora.step_ex(U.blue_mix(500, 99, 2), None, None, None)
    assert _tw(ora)[1][0] == 1
    SE_SET_STEP = 7
    assert ora.edit_state(0, SE_SET_STEP, 40) >= 0
    terms, words = _tw(ora)
    assert words[0] == 0 and words[1] == 40 and not terms.any() and not words[3:].any()
    ora.close()


@pytest.mark.parametrize('recorded_between', [True, False], ids=['all-recorded', 'fast-steps-between'])
@pytest.mark.parametrize('mode', [1, 0], ids=['counter', 'numpy'])
def test_a_restore_stamp_does_not_outlive_its_episode(mode, recorded_between):
    """A Restore on the first step of a 12-step episode that runs to done, is regenerated, and takes a first step without Restore: cost 0.  Both
    first steps carry stamp 1; with fast steps in between nothing after the first step touches the record but the regeneration."""
    ora = OracleVecEnv(1, steps=12, rng_mode=mode)
    ora.reset(seeds=900)
    act = np.full((1, 5), -1, np.int32)
    act[0, 2] = U.restore_code(ora, 0, 2)
    _, rew, done, _ = ora.step_ex(act, None, None, None)
    terms, words = _tw(ora)
    assert words[0] == 1 and words[4] == -1 and words[13] == -1 and words[7] == terms[2, :3].sum() - 1 and words[3] + words[4] == rew[0]
    none = np.full((1, 5), -1, np.int32)
    while not done[0]:
        _, rew, done, _ = ora.step_ex(none, None, None, None) if recorded_between else ora.step(none)
        if recorded_between:
            terms, words = _tw(ora)
            assert words[0] == 1 and words[4] == 0 and not words[11:].any(), 'the Restore is charged once, on submission'
    ora.reset(seeds=None, env_mask=np.array([True]))
    terms, words = _tw(ora)
    assert words[0] == 0 and words[1] == 0 and not terms.any()
    _, rew, done, _ = ora.step_ex(none, None, None, None)
    terms, words = _tw(ora)
    assert words[0] == 1 and words[1] == 1 and words[4] == 0 and not words[11:].any() and words[3] == rew[0], words.tolist()
    ora.close()


def test_the_built_in_blue_policy_is_not_charged_and_a_restore_while_busy_is():
    # blue_policy = 1, nothing submitted: cc4BlueRandomAgent chooses Restore now and then; the reward machine charges submitted actions only
    ora = OracleVecEnv(4, steps=100, rng_mode=0, blue_policy=1)
    ora.reset(seeds=300)
    chosen = 0
    for t in range(40):
        _, rew, _, _ = ora.step_ex(None, None, None, None)
        for e in range(4):
            terms, words = _tw(ora, e)
            assert words[0] == 1 and words[4] == 0 and not words[11:].any() and words[3] == rew[e], (t, e)
            scal = BV.from_row(ora.get_state(e))[1]
            chosen += int(((scal[:, 1] == BV.RESTORE) & (scal[:, 3] == 4)).sum())          # queued this step: four of five ticks left
    assert chosen >= 3, chosen
    ora.close()
    # a Restore submitted while the agent is busy with the first one is dropped by the queue and charged all the same
    ora = OracleVecEnv(1, steps=100, rng_mode=1)
    ora.reset(seeds=301)
    act = np.full((1, 5), -1, np.int32)
    act[0, 4] = U.restore_code(ora, 0, 4)
    act[0, 0] = U.restore_code(ora, 0, 0)
    for t in range(3):
        _, rew, _, _ = ora.step_ex(act, None, None, None)
        terms, words = _tw(ora)
        scal = BV.from_row(ora.get_state(0))[1]
        assert scal[4, 0] == 1 and scal[4, 3] == 4 - t, (t, scal[4].tolist())           # busy with the FIRST Restore: its ticks run down
        assert words[0] == 1 and words[4] == -2 and words[11] == -1 and words[15] == -1 and not words[12:15].any() and words[3] + words[4] == rew[0], t
    ora.close()
