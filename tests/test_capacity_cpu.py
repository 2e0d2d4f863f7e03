"""CPU: the engine's bounded containers one below, at and past their capacity, on the oracle (the host build of csrc/cc4_engine.h).
tests/capacity_util.py crafts the states; here

* after each fill the session and process lists of the true-state document equal a plain list model of the adds performed (idents max + 1, pids
  as returned, insertion order), and a container that is exactly full has raised nothing;
* the operation that overflows a full container raises exactly its flag and leaves the container's listed content as it was, the same operation
  on the container one below its capacity fills it without a flag, and the full container left alone ('cap', the twin) stays clean;
* every flag of the table in DESIGN.md section 2 except E_OBS_OVERFLOW is raised in at least one episode while its twin shows err == 0 -- the
  condition that keeps tests/test_capacity.py (the same episodes on every kernel) from passing vacuously.  The seed is chosen here: a step of
  the default configuration has a phishing session in one episode out of six, which may land in a crafted agent;
* tests/cpp/capacity_check.cpp -- a stand-alone program, never loaded into Python -- runs the same fills through state_edit and 2 x steps steps
  in both RNG modes on back-to-back rows under the address and undefined-behaviour sanitizers.

E_OBS_OVERFLOW (RedAgent.obs, MAX_OBS) is not reached by any crafted state, and the table says so: an agent's observation list is cleared at the
start of every step (step_red_policy_tick), so a poked count does not survive to a writer; within a step an agent executes one action -- the
largest contribution is a DiscoverRemoteSystems sweep, one entry for each of a subnet's at most 16 non-router hosts -- and besides it receives
at most one handed-over entry for each session another agent's exploit created in its zone in that step (red_reassign: five other agents, one
exploit each): 16 + 5 < MAX_OBS.  test_obs_list_is_cleared_before_it_is_written pins the first half of that argument."""
import json
import os

import numpy as np
import pytest

import capacity_util as U
from oracle_binding import OracleVecEnv, random_actions
from cpp_check import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1030                # every scenario's first step does what its operation says, in both RNG modes (see the module docstring)
N = len(U.SCENARIOS)
FLAGS = ('E_PROC', 'E_RSESS', 'E_KS', 'E_SUS', 'E_PEND')


@pytest.fixture(scope='module', params=[0, 1], ids=['numpy_stream', 'counter_mode'])
def crafted(request):
    """Every scenario once, episode e = scenario e: the state after the fill, after the operation's edits, after the first step."""
    mode = request.param
    ora = OracleVecEnv(N, steps=U.STEPS, rng_mode=mode)
    ora.reset(seeds=SEED)
    out = {'mode': mode, 'built': {}, 'filled': {}, 'err_filled': {}, 'rcs': {}, 'hot_filled': {}}
    for e, sc in enumerate(U.SCENARIOS):
        out['built'][e] = U.build(ora, e, sc)
        out['filled'][e] = json.loads(ora.true_state_json(e))
        out['hot_filled'][e] = ora.get_state(e)
        out['err_filled'][e] = int(ora.lib.cc4o_err(ora._h, e))
    for e, b in out['built'].items():
        out['rcs'][e] = U.apply_edits(ora, e, b)
    out['err_edited'] = {e: int(ora.lib.cc4o_err(ora._h, e)) for e in range(N)}
    out['edited'] = {e: json.loads(ora.true_state_json(e)) for e in range(N)}
    (red, green), blue = U.submissions(ora, out['built'])
    _o, _r, _d, info = ora.step_ex(U.first_step_actions(random_actions(SEED, 0, N), blue), None, red, green)
    out['err_stepped'] = info['err'].astype(np.int64).copy()
    out['stepped'] = {e: json.loads(ora.true_state_json(e)) for e in range(N)}
    out['hot_stepped'] = {e: ora.get_state(e) for e in range(N)}
    yield out
    ora.close()


def test_layout_and_caps_describe_the_rows():
    cp, L = U.caps(), U.layout()
    ora = OracleVecEnv(1, steps=U.STEPS)
    assert cp['cold_bytes'] == ora.lib.cc4o_cold_bytes(ora._h) and L['sizeof.EnvState'] == ora.lib.cc4o_state_bytes()
    ora.close()
    hosts = (L['sizeof.EnvState'] - L['hd']) // L['sizeof.HostDyn']
    assert cp['povf_off'] == L['cold.sus'] + 4 * 5 * cp['sus'] and L['cold.sus'] == L['sizeof.EnvCold']
    assert cp['povf_off'] + 4 * hosts * cp['povf'] == cp['cold_bytes']            # the last host's overflow row ends the cold row
    assert L['blue'] + 4 * L['sizeof.BlueAgent'] + L['blue.nsus'] + 2 <= L['spool'] and cp['povf'] % 8 == 0 and cp['sus'] % 16 == 0 and cp['MAX_RS'] % 8 == 0
    assert len({cp[f] for f in FLAGS + ('E_OBS',)}) == 6 and all(cp[f] & (cp[f] - 1) == 0 for f in FLAGS)


def test_fills_match_the_list_model_and_raise_nothing(crafted):
    cp = U.caps()
    full = cp['PIN'] + cp['povf']
    for e, b in crafted['built'].items():
        U.check_model(crafted['filled'][e], b)
        assert crafted['err_filled'][e] == 0, (b.scenario, crafted['err_filled'][e])
    # the fills reached what they name
    by = {b.scenario: (e, b) for e, b in crafted['built'].items()}
    nsess = lambda sc, r: len(crafted['filled'][by[sc][0]]['red'][r]['sessions'])            # noqa: E731
    nproc = lambda sc, h: [len(x['procs']) for x in crafted['filled'][by[sc][0]]['hosts'] if x['h'] == h][0]      # noqa: E731
    assert (nsess('rs_add:m1', 1), nsess('rs_add:cap', 1), nsess('rs_add:over', 1)) == (cp['MAX_RS'] - 1, cp['MAX_RS'], cp['MAX_RS'])
    for k in range(4):
        assert sum(nsess(f'pool{k}:over', r) for r in range(6)) == cp['RS_POOL'] - k and sum(nsess(f'pool{k}:m1', r) for r in range(6)) == cp['RS_POOL'] - k - 1
    assert max(nsess('pool0:cap', r) for r in range(6)) <= cp['MAX_RS'] and sum(nsess('pool0:cap', r) for r in range(6)) == cp['RS_POOL']
    for sc in ('proc_decoy_edit', 'proc_decoy', 'proc_exploit', 'proc_phish'):
        for v, want in (('m1', full - 1), ('cap', full), ('over', full)):
            for key in by[f'{sc}:{v}'][1].watch:
                assert nproc(f'{sc}:{v}', key[1]) == want, (sc, v, key)
    assert 136 in [k[1] for k in by['proc_decoy_edit:cap'][1].watch]                       # the host whose overflow row closes the cold row
    for v, want in (('m1', cp['PIN'] - 1), ('cap', cp['PIN']), ('over', cp['PIN'] + 1)):
        e = by[f'proc_pin:{v}'][0]
        assert sum(len(x['procs']) == want for x in crafted['filled'][e]['hosts']) >= 20
    for bl in (0, 4):
        for v, d in (('m1', -1), ('cap', 0), ('over', 0)):
            assert len(crafted['filled'][by[f'sus{bl}_end:{v}'][0]]['blue'][bl]['sus']) == cp['sus'] + d
    for v, d in (('m1', -1), ('cap', 0), ('over', 0)):
        assert len(crafted['filled'][by[f'known:{v}'][0]]['red'][2]['known_sessions']) == cp['MAX_KS'] + d
        assert 300 in crafted['filled'][by[f'known256:{v}'][0]]['red'][2]['known_sessions']
        assert int(crafted['hot_filled'][by[f'pend:{v}'][0]][U.layout()['npend']]) == cp['MAX_PEND'] + d


def test_overflowing_operation_raises_exactly_its_flag_and_leaves_the_content(crafted):
    cp = U.caps()
    for e, b in crafted['built'].items():
        assert crafted['rcs'][e] == [x[4] for x in b.edits], (b.scenario, crafted['rcs'][e], b.edits)
        if b.edits:                                     # the operation is an edit: its flag is there before any step
            assert crafted['err_edited'][e] == b.expect, (b.scenario, crafted['err_edited'][e])
        assert int(crafted['err_stepped'][e]) == b.expect, (b.scenario, int(crafted['err_stepped'][e]), b.expect)
        before = U.listed(crafted['filled'][e], b, crafted['hot_filled'][e])
        after = U.listed(crafted['stepped'][e] if not b.edits else crafted['edited'][e], b, crafted['hot_stepped'][e])
        for key, was in before.items():
            now = after[key]
            if key[0] == 'pend':                        # (the end of the step hands the events over and empties the list: compared through the flag alone)
                continue
            if b.variant == 'over':
                if key[0] == 'proc':                    # a process list is compared by pid and kind (an exploit elsewhere on the host changes no record)
                    assert [p[:2] for p in now] == [p[:2] for p in was], (b.scenario, key)
                else:
                    assert now == was, (b.scenario, key, now[-3:], was[-3:])
            elif b.variant == 'm1':                     # the same operation one below the capacity: the container is exactly full now
                want = {'sess': cp['MAX_RS'], 'proc': cp['PIN'] + cp['povf'], 'known': cp['MAX_KS'], 'sus': cp['sus']}[key[0]]
                assert len(now) == want and now[:len(was)] == was, (b.scenario, key, len(now), want)
            else:
                assert len(now) == len(was), (b.scenario, key)
    # a refused SE_ADD_RED_SESSION leaves its process and its pid draw behind
    e = U.SCENARIOS.index('rs_add:over')
    h = crafted['built'][e].edits[0][2]
    n0, n1 = ([len(x['procs']) for x in crafted[k][e]['hosts'] if x['h'] == h][0] for k in ('filled', 'edited'))
    assert n1 == n0 + 1
    # the refused reassignment drops the session and frees its record: the source agent lost it, the pool holds exactly the listed sessions
    e = U.SCENARIOS.index('rs_reassign:over')
    used = lambda hot: int(np.unpackbits(hot[U.layout()['spool_used']:U.layout()['spool_used'] + cp['RS_POOL'] // 8]).sum())      # noqa: E731
    held = lambda ts: [len(a['sessions']) for a in ts['red']]                                                                      # noqa: E731
    assert used(crafted['hot_filled'][e]) == sum(held(crafted['filled'][e])) and used(crafted['hot_stepped'][e]) == sum(held(crafted['stepped'][e]))
    assert held(crafted['stepped'][e])[:2] == [held(crafted['filled'][e])[0] - 1, cp['MAX_RS']]
    # pool: with k free records and k + 1 exploiting agents exactly the last agent goes without
    for k in range(4):
        e = U.SCENARIOS.index(f'pool{k}:over')
        b = crafted['built'][e]
        got = [len(crafted['stepped'][e]['red'][r]['sessions']) - len(crafted['filled'][e]['red'][r]['sessions']) for r, *_ in b.red]
        assert got == [1] * k + [0], (k, got)
        assert used(crafted['hot_stepped'][e]) == cp['RS_POOL']


def test_every_flag_is_raised_and_its_twin_is_clean(crafted, capsys):
    cp = U.caps()
    raised = {f: [] for f in FLAGS}
    for e, b in crafted['built'].items():
        if b.variant != 'over' or not b.flag:
            continue
        twin = U.SCENARIOS.index(b.container + ':cap')
        name = [f for f in FLAGS if cp[f] == b.flag][0]
        if int(crafted['err_stepped'][e]) & b.flag and int(crafted['err_stepped'][twin]) == 0:
            raised[name].append((e, b.scenario, 0 if b.edits else 1))
    with capsys.disabled():
        for f, where in raised.items():
            print(f'\n  {f} (RNG mode {crafted["mode"]}): ' + ', '.join(f'episode {e} ({sc}) at step {t}' for e, sc, t in where), end='')
    assert all(raised[f] for f in FLAGS), {f: len(v) for f, v in raised.items()}
    both = {b.container for b in crafted['built'].values() if b.container.startswith('sus')}
    assert {'sus0_end', 'sus4_end', 'sus0_monitor', 'sus4_monitor'} <= both          # both raise sites, blue agents 0 and 4
    assert cp['E_OBS'] not in {b.flag for b in crafted['built'].values()}              # not reachable: the module docstring says why


def test_obs_list_is_cleared_before_it_is_written():
    """A poked RedAgent.nobs at MAX_OBS does not survive to a writer: the step's policy tick starts the observation empty."""
    cp, L = U.caps(), U.layout()
    for mode in (0, 1):
        ora = OracleVecEnv(1, steps=U.STEPS, rng_mode=mode)
        ora.reset(seeds=SEED)
        hot, cold = ora.snapshot(0)
        hot[L['red'] + L['red.nobs']] = cp['MAX_OBS']                 # red_agent_0: active, acts in this step
        ora.restore(0, (hot, cold))
        for t in range(12):
            _o, _r, _d, info = ora.step(random_actions(SEED, t, 1))
            assert not int(info['err'][0]) & cp['E_OBS'], (mode, t)
        assert json.loads(ora.true_state_json(0))['red'][0]['obs'] is not None
        ora.close()


def test_long_runs_of_every_scenario_report_where_flags_come_up(crafted, capsys):
    """2 x steps steps of seeded random blue actions behind the first step (what the sanitised program does, here for the record): per flag, the
    episodes and steps at which the oracle raised it.  Nothing of the run is asserted beyond its end: natural play may fill any container."""
    cp = U.caps()
    mode = crafted['mode']
    ora = OracleVecEnv(N, steps=U.STEPS, rng_mode=mode, autoreset=True)
    ora.reset(seeds=SEED)
    built = {e: U.build(ora, e, sc) for e, sc in enumerate(U.SCENARIOS)}
    for e, b in built.items():
        U.apply_edits(ora, e, b)
    (red, green), blue = U.submissions(ora, built)
    seen = {f: {} for f in FLAGS}
    prev = np.zeros(N, np.int64)
    for t in range(2 * U.STEPS):
        if t == 0:
            _o, _r, _d, info = ora.step_ex(U.first_step_actions(random_actions(SEED, 0, N), blue), None, red, green)
        else:
            _o, _r, _d, info = ora.step(random_actions(SEED, t, N))
        err = info['err'].astype(np.int64)
        for f in FLAGS:
            for e in np.nonzero(err & ~prev & cp[f])[0]:
                seen[f].setdefault(int(e), t + 1)
        prev = err.copy()
    with capsys.disabled():
        for f in FLAGS:
            print(f'\n  {f} over {2 * U.STEPS} steps (RNG mode {mode}): ' + ', '.join(f'{e}@{t}' for e, t in sorted(seen[f].items())), end='')
    assert all(seen[f] for f in FLAGS)
    ora.close()


def test_capacity_states_under_sanitizers(tmp_path, capsys):
    run = build_and_run(os.path.join(ROOT, 'tests', 'cpp', 'capacity_check.cpp'), tmp_path, required=False, timeout=600, flags=['-ffp-contract=off'])
    assert ' 0 failures' in run.stdout and 'E_PROC ' in run.stdout, run.stdout
    with capsys.disabled():
        print(f'\n  {run.stdout.strip().splitlines()[-1]} ({run.seconds:.1f} s)', end='')
