"""GPU: the one-wave step body's red FSM option table (fsm_pk) and its wave-asked single-lane sections -- the phishing / slot-reservation
section in front of the red actions (skipped by ballot, the reservation on the agents' lanes: rs_reserve_lane), the merge of the agents'
pid-carrying events (step_red_merge only when some agent's slot is set) and the Impact term of the reward on the agents' lanes
(step_impact_term, step_end without its loop) -- against the CPU oracle, whose serial walk keeps the serial forms.

Random play reaches the usual branches; the rest is made by hand the way the scripted tests do (cc4_edit_state on the oracle, the episode
restored into the device batch), and every state is asserted from the oracle's true state to have been reached: session pools with 31, 32,
63 and 64 used records in front of a step on which two or more agents' Exploits resolve (the reserved records straddle a word of spool_used),
steps with phishing and an Exploit, phishing only, neither; two agents' Impact on one step in each mission phase; pid-carrying events of two
agents on one step.  Red and green actions of a chosen step go in through cc4_step_ex (the full build of the same body), so the fast build
also plays 64 episodes x 150 steps at random, with the oracle's trace showing that both sides of each of the three questions occurred.  The
persistent kernel runs the scripted pools at 8192 episodes under the library's self-check."""
import json
import numpy as np
import pytest
from oracle_binding import OracleVecEnv, random_actions

pytestmark = pytest.mark.gpu

SE_SET_PHASE, SE_ADD_RED_SESSION = 0, 5
RA_AGGR, RA_EXPLOIT, RA_IMPACT, RA_SLEEP = 1, 4, 6, 9
XG_LOCAL, XG_SLEEP = 1, 2
XF_RATE0, XF_RATE1, XF_SKIP_VALID = 1, 2, 4
SLOTS = 17
RED_ZONE = ((4,), (0,), (1,), (2,), (3,), (5, 6, 7))       # red agent r's subnets (EnterpriseScenarioGenerator.py:769-776)
POOLS = (31, 32, 63, 64)
N = 16


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, **kw)


def _doc(ora, e):
    return json.loads(ora.true_state_json(e))


def _zone_hosts(d, r):
    """The hosts (no routers) of red agent r's own subnets, in host order."""
    return [h['h'] for h in d['hosts'] if h['h'] % SLOTS and h['h'] // SLOTS in RED_ZONE[r]]


def _used(d):
    return sum(len(a['sessions']) for a in d['red'])


def _fill_pool(ora, e, target):
    """Red sessions (RedAbstractSession shells on the first half of the hosts of the agents' own zones -- the rest stays free to be exploited --
    agents in turn, so that every agent holds some) until `target` records of the episode's pool are used.  The pool hands out its lowest free record, so records 0 .. target - 1 are the used ones."""
    d = _doc(ora, e)
    k = 0
    while _used(d) + k < target:
        r = k % 6
        zone = _zone_hosts(d, r)
        assert ora.edit_state(e, SE_ADD_RED_SESSION, r, zone[(k // 6) % max(1, len(zone) // 2)], 4 | ((k // 6) & 1)) >= 0
        k += 1
    d = _doc(ora, e)
    assert _used(d) == target and all(a['sessions'] for a in d['red']), (e, target, _used(d))
    return d


def _pair(monkeypatch, n, seed, steps=100):
    monkeypatch.setenv('CC4_PHILOX_LEAN', '1')
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    assert dev.step_kernel == 'k_step_philox1'
    ora = OracleVecEnv(n, steps=steps, rng_mode=1)
    assert np.array_equal(dev.reset(seeds=seed), ora.reset(seeds=seed))
    return dev, ora


def _same(dev, ora, d, o, t):
    bad = np.nonzero((d[0] != o[0]).any(axis=1) | (d[1] != o[1]) | (d[2] != o[2]) | (d[3]['err'] != o[3]['err']))[0]
    assert bad.size == 0, (t, bad[:10].tolist())
    rows = dev.get_states()
    bad = [e for e in range(dev.num_envs) if not np.array_equal(rows[e], ora.get_state(e))]
    assert not bad, (t, bad[:10])


def _sleep_all(red, green, e, d):
    for r in range(6):
        rec = red[e, r]
        rec['type'] = RA_SLEEP; rec['host'] = rec['arg'] = rec['ticks'] = rec['flags'] = 0; rec['session'] = 0
    for g in range(d['n_green']):
        rec = green[e, g]
        rec['type'] = XG_SLEEP; rec['host'] = d['green_hosts'][g]; rec['session'] = 0; rec['flags'] = 0


def _exploit(red, e, d, r, k, ty=RA_EXPLOIT):
    """Agent r's Exploit of the k-th host of its zone it holds no session on, from its first session, resolving on this step (an Exploit needs the
    session to know the host's ports: the same call with ty = RA_AGGR, an AggressiveServiceDiscovery of that host, a step earlier)."""
    held = {s[1] for s in d['red'][r]['sessions']}
    free = [h for h in _zone_hosts(d, r) if h not in held]
    rec = red[e, r]
    rec['type'] = ty; rec['host'] = free[k % len(free)]; rec['arg'] = 0; rec['ticks'] = 1
    rec['session'] = d['red'][r]['sessions'][0][0]; rec['flags'] = XF_SKIP_VALID


def _phish(green, e, d):
    """Every green agent: GreenLocalWork whose PhishingEmail always follows (when the work itself succeeds) and never a false positive."""
    for g in range(d['n_green']):
        rec = green[e, g]
        rec['type'] = XG_LOCAL; rec['host'] = d['green_hosts'][g]; rec['session'] = 0
        rec['flags'] = XF_RATE0 | XF_RATE1; rec['rate0'] = 0.0; rec['rate1'] = 1.0


def _step_facts(before, after):
    """What the oracle's true state says happened on a step: Exploits that resolved (agents), sessions they created, sessions a PhishingEmail
    created (on a green agent's host that held no red session), pid-carrying events handed to the blue agents, executed Impacts."""
    exploits = [r for r in range(6) if after['last_red'][r][0] == RA_EXPLOIT and after['last_red'][r][3]]
    created = [r for r in range(6) if after['red'][r]['new_session'][0] != 255]
    red_hosts = lambda d: {s[1] for a in d['red'] for s in a['sessions']}          # noqa: E731
    greens = set(after['green_hosts'][:after['n_green']])
    phished = (red_hosts(after) - red_hosts(before)) & greens - {after['red'][r]['new_session'][0] for r in created}
    sus = sum(len(b['sus']) for b in after['blue']) - sum(len(b['sus']) for b in before['blue'])
    impacts = [r for r in range(6) if after['last_red'][r][0] == RA_IMPACT and after['red'][r]['sessions']]
    # the agents whose own event slot (StepWork.pend_r) was merged: the new sus entries that are [host, pid] of the session an agent's Exploit created
    old_sus = {tuple(x) for b in before['blue'] for x in b['sus']}
    new_sus = {tuple(x) for b in after['blue'] for x in b['sus']} - old_sus
    sus_agents = [r for r in created if any(s[1] == after['red'][r]['new_session'][0] and s[0] == after['red'][r]['new_session'][1] and (s[1], s[2]) in new_sus
                                            for s in after['red'][r]['sessions'])]
    return {'exploits': exploits, 'created': created, 'phished': sorted(phished), 'sus': sus, 'impacts': impacts, 'sus_agents': sus_agents}


def test_scripted_pools_exploits_phishing_and_impact_on_the_full_build(monkeypatch):
    """cc4_step_ex (the full build of the one-wave body) from scripted states, hot rows and outputs after every step.  Episode e starts with
    POOLS[e % 4] used pool records.  Step 0: every agent scans the host it will exploit; step 1: all six agents' Exploits resolve (episodes 0-7
    with phishing requests from every green agent, 8-15 without); step 2: phishing only; step 3: neither (everyone sleeps); step 4: two agents
    scan another host; step 5: Impact by agents e % 6 and (e + 1 + e // 6) % 6 in mission phase e % 3; step 6: those two agents' Exploits
    (the pools have moved on)."""
    dev, ora = _pair(monkeypatch, N, 8100)
    for e in range(N):
        _fill_pool(ora, e, POOLS[e % 4])
        dev.restore(e, ora.snapshot(e))
    red, green = dev.agent_actions('red'), dev.agent_actions('green')
    facts = {}
    for t in range(7):
        before = [_doc(ora, e) for e in range(N)]
        red['type'] = -1; green['type'] = -1
        for e in range(N):
            d = before[e]
            if t == 5:
                ora.edit_state(e, SE_SET_PHASE, e % 3)
                dev.restore(e, ora.snapshot(e))
                before[e] = d = _doc(ora, e)
            _sleep_all(red, green, e, d)
            if t in (0, 1):
                for r in range(6):
                    _exploit(red, e, d, r, e, RA_AGGR if t == 0 else RA_EXPLOIT)
                if t == 1 and e < 8:
                    _phish(green, e, d)
            elif t == 2:
                _phish(green, e, d)
            elif t == 4:
                for r in (e % 6, (e + 2) % 6):
                    _exploit(red, e, d, r, e + 3, RA_AGGR)
            elif t == 5:
                for r in (e % 6, (e + 1 + e // 6) % 6):
                    rec = red[e, r]
                    rec['type'] = RA_IMPACT; rec['host'] = d['red'][r]['sessions'][-1][1]; rec['ticks'] = 1
                    rec['session'] = d['red'][r]['sessions'][0][0]; rec['flags'] = XF_SKIP_VALID
            elif t == 6:
                for r in (e % 6, (e + 2) % 6):
                    _exploit(red, e, d, r, e + 3)
            if t == 4:
                facts['targets', e] = {r: int(red[e, r]['host']) for r in (e % 6, (e + 2) % 6)}
            if t == 6:      # (sessions came and went since the scan: the scanned host, not the k-th free one of now)
                for r, h in facts['targets', e].items():
                    red[e, r]['host'] = h
        a = random_actions(8100, t, N)
        _same(dev, ora, dev.step_ex(a, None, red, green), ora.step_ex(a, None, red, green), t)
        for e in range(N):
            facts[t, e] = _step_facts(before[e], _doc(ora, e))
            facts[t, e]['used'] = _used(before[e])
            facts[t, e]['phase'] = before[e]['phase']
    # ---- the states were reached (all from the oracle's true state)
    for e in range(N):
        f = facts[1, e]
        assert f['used'] == POOLS[e % 4] and len(f['exploits']) == 6, (e, f)           # six askers in front of / on a word boundary of spool_used
        assert len(f['created']) >= 2, (e, f)                                          # ... and two or more of them took their record
        f = facts[2, e]
        assert not f['exploits'] and not f['created'], (e, f)                          # phishing only
        f = facts[3, e]
        assert not f['exploits'] and not f['phished'] and not f['impacts'] and not f['sus'], (e, f)      # neither
        f = facts[5, e]
        assert f['phase'] == e % 3 and len(f['impacts']) == 2, (e, f)                   # two agents' Impact in each mission phase
        assert len(facts[6, e]['exploits']) == 2, (e, facts[6, e])
    assert sum(bool(facts[1, e]['phished']) for e in range(8)) >= 4, [facts[1, e]['phished'] for e in range(8)]        # phishing and Exploits
    assert not any(facts[1, e]['phished'] for e in range(8, N))
    assert sum(bool(facts[2, e]['phished']) for e in range(N)) >= 8, [facts[2, e]['phished'] for e in range(N)]        # phishing only
    assert sum(len(facts[1, e]['sus_agents']) >= 2 for e in range(N)) >= 4, [facts[1, e]['sus_agents'] for e in range(N)]   # pend_r of two agents or more
    assert sum(len(facts[6, e]['created']) == 2 for e in range(N)) >= 2, [facts[6, e]['created'] for e in range(N)]
    assert {facts[5, e]['phase'] for e in range(N)} == {0, 1, 2}
    for e in range(N):
        assert np.array_equal(dev.snapshot(e)[1], ora.snapshot(e)[1]), f'cold row differs env {e}'
    dev.close(); ora.close()


def test_random_play_on_the_fast_build_takes_both_sides_of_every_question(monkeypatch):
    """64 episodes x 150 steps of random play on the fast build of k_step_philox1, hot rows and outputs after every step; the oracle's trace of
    the first eight episodes shows steps with and without a resolving Exploit, a phishing session, a pid-carrying red event and an Impact."""
    n, seed, traced = 64, 8200, 8
    dev, ora = _pair(monkeypatch, n, seed, steps=500)
    seen = {k: [0, 0] for k in ('exploits', 'phished', 'sus', 'impacts')}
    before = [_doc(ora, e) for e in range(traced)]
    for t in range(150):
        a = random_actions(seed, t, n)
        _same(dev, ora, dev.step(a), ora.step(a), t)
        for e in range(traced):
            after = _doc(ora, e)
            f = _step_facts(before[e], after)
            for k in seen:
                seen[k][1 if f[k] else 0] += 1
            before[e] = after
    assert all(v[0] > 0 and v[1] > 0 for v in seen.values()), seen
    dev.close(); ora.close()


def test_persistent_kernel_with_the_scripted_pools(monkeypatch):
    """One 20-step call of k_run_philox1 at 8192 episodes with the scripted pools (31 / 32 / 63 / 64 used records, two mission phases set by hand)
    in its first sixteen episodes, the agents' own policies acting.  Two checks: the library's self-check (CC4_PERSIST_VERIFY=1) repeats the call with
    per-step launches of the same body -- that covers the persistent loop's hand-over only, a mistake both forms share passes it -- and the CPU
    oracle walks the sixteen scripted episodes through the same twenty steps (the call draws random_actions' blue actions in the kernel): their hot
    rows must be the oracle's, and the oracle's trace must show that Exploits resolved and created sessions on the way."""
    monkeypatch.delenv('CC4_PERSIST_MIN_K', raising=False)
    monkeypatch.delenv('CC4_PHILOX_LEAN', raising=False)
    monkeypatch.setenv('CC4_PERSIST_VERIFY', '1')
    n, K, seed = 8192, 20, 8300
    dev = _dev(n, steps=100, rng_mode=1, autoreset=True, strict=False)
    assert dev.run_kernel_for(K) == 'k_run_philox1'
    ora = OracleVecEnv(N, steps=100, rng_mode=1, autoreset=True)
    dev.reset(seeds=seed); ora.reset(seeds=seed)
    for e in range(N):
        _fill_pool(ora, e, POOLS[e % 4])
        if e >= 8:
            ora.edit_state(e, SE_SET_PHASE, 1 + (e & 1))
        dev.restore(e, ora.snapshot(e))
    dev.run_random_steps(seed, 0, K, timed=False)
    assert dev.verify_stats() == (1, 0)
    resolved = created = 0
    before = [_doc(ora, e) for e in range(N)]
    for t in range(K):
        ora.step(random_actions(seed, t, N))
        for e in range(N):
            after = _doc(ora, e)
            f = _step_facts(before[e], after)
            resolved += len(f['exploits']); created += len(f['created'])
            before[e] = after
    assert resolved >= 6 and created >= 2, (resolved, created)      # (the reservation's lane form ran with askers, and records were taken)
    bad = [e for e in range(N) if not np.array_equal(dev.get_state(e), ora.get_state(e))]
    assert not bad, bad
    dev.close(); ora.close()
