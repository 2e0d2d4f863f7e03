"""CPU: the blue view against the REFERENCE, not against the row.  The CPU oracle replays traj_seed123_random_ctor_500 with the event log on; for
each of the 120 steps blueobs_seed123_random.json records in full, the view the host function makes of the oracle's rows
(blue_view.from_row: cc4_blue_view_from_row, the kernel's definition compiled for the host) must equal, in columns 3..7 and words 0, 4, 5, 7, the
view tests/blue_util.py derives from the reference's own dict observation of that step.  A view that merely agrees with the packed row fails here
if the row's reading of the reference is wrong."""
import json
import os

import numpy as np

import blue_util as BU
import golden_util
from cage_challenge_4_amd import blue_view as BV
from oracle_binding import OracleVecEnv

GOLD = os.path.join(golden_util.GOLDEN_DIR, 'blueobs_seed123_random.json')


def test_host_view_matches_the_reference_dict_observation(oracle_lib):
    gold = json.load(open(GOLD))
    fix = golden_util.load(os.path.join(golden_util.GOLDEN_DIR, gold['fixture']))
    env = OracleVecEnv(1, steps=fix['steps'])
    env.reset(seeds=fix['seed'])
    env.reset(seeds=None)
    env.enable_event_log(True)
    stats = BU.new_stats()
    assert len(gold['steps']) == 120
    for t, want in enumerate(gold['steps']):
        env.step(fix['actions'][t][None, :])
        doc = json.loads(env.true_state_json(0))
        hosts, scal = BV.from_row(env.get_state(0), env.get_cold(0), fix['steps'])
        assert (scal[:, 10] == 1).all() and (scal[:, 13] == t + 1).all(), t
        BU.compare(hosts, scal, want, doc, t, stats)
    env.close()
    # the fixture exercises what the comparison is about
    assert stats['pairs'] >= 550 and stats['files'] >= 10 and stats['decoys'] >= 30, stats
    assert stats['success'] == {BV.T_TRUE, BV.T_UNKNOWN, BV.T_FALSE, BV.T_IN_PROGRESS} and stats['conn'] > 300 and stats['proc'] > 20, stats


def test_reference_helper_reads_entry_classes_doubling_and_own_entries():
    """The helper on a hand-made observation: halved counts, a pid entry counted once, ports, remote hosts, Files order, a decoy."""
    doc = {'cidr': [10, 11, 12, 13, 14, 15, 16, 17, 18], 'hosts': [{'h': 1, 'ip': 5}, {'h': 2, 'ip': 6}, {'h': 70, 'ip': 9}, {'h': 18, 'ip': 7}]}
    n1, n2, n18 = BU.T.hostname_of(1), BU.T.hostname_of(2), BU.T.hostname_of(18)
    conn = {'Connections': [{'local_address': '10.0.10.5', 'local_port': 22, 'remote_address': '10.0.14.9', 'remote_port': 50000}]}
    local = {'Connections': [{'local_address': '10.0.10.5', 'local_port': 51000}]}
    files = [{'File Name': 'cmd.sh'}, {'File Name': 'escalate.sh'}]
    obs = {f'blue_agent_{b}': {'success': 'UNKNOWN', 'action': 'Sleep'} for b in range(5)}
    obs['blue_agent_0'] = {'success': 'TRUE', 'action': f'Analyse {n2}', n1: {'Processes': [conn, conn, conn, conn, local, local, {'PID': 77}]}, n2: {'Files': files}}
    obs['blue_agent_1'] = {'success': 'TRUE', 'action': f'DeployDecoy {n18}',
                           n18: {'Processes': [{'PID': 4, 'PPID': 1, 'service_name': 'tomcat', 'username': 'ubuntu'}]}}
    obs['blue_agent_2'] = {'success': 'IN_PROGRESS', 'action': None}
    hosts, own_mask, words, known = BU.reference_view(obs, doc)
    assert hosts[0, 1].tolist() == [0, 0, 0, 2, 2, 0, 1 | BV.PORT_PID, 0] and hosts[0, 70, 5] == 2 and hosts[0, 2, 7] == 7 and own_mask[0, 2] == 0xFF
    assert hosts[1, 18, 7] == (BV.OWN_DECOY | 6) and words[0, [0, 4, 5, 7]].tolist() == [0, 2, 2, 1] and words[2, [0, 4, 7]].tolist() == [1, 0, 4]
    assert known.tolist() == [True, True, False, False, False]
    obs['blue_agent_0'][n2] = {'Files': files[1:]}
    hosts, own_mask, _w, _k = BU.reference_view(obs, doc)
    assert hosts[0, 2, 7] == 2 and own_mask[0, 2] == 0xFB
    obs['blue_agent_0'][n1]['Processes'].append(conn)
    try:
        BU.reference_view(obs, doc)
    except AssertionError:
        pass
    else:
        raise AssertionError('an odd count of an entry without a pid must be refused')
