"""CPU: the Monitor's connection edges against the REFERENCE, not against the row.  The CPU oracle replays traj_seed123_random_ctor_500 with the event
log on; for each of the 120 steps blueobs_seed123_random.json records in full, the edge list the host function makes of the oracle's rows
(blue_edges.from_row: cc4_blue_edges_from_row, the kernel's definition compiled for the host) must equal the list tests/blue_edges_util.py derives
from the 'Connections' of the reference's own dict observation of that step; and the NumPy restatement from the true-state document must equal it
too.  A list that merely agrees with the packed row fails here if the row's reading of the reference is wrong."""
import json
import os

import numpy as np

import blue_edges_util as EU
import golden_util
from cage_challenge_4_amd import blue_edges as BE
from oracle_binding import OracleVecEnv

GOLD = os.path.join(golden_util.GOLDEN_DIR, 'blueobs_seed123_random.json')


def test_host_edges_match_the_reference_dict_observation(oracle_lib):
    gold = json.load(open(GOLD))
    fix = golden_util.load(os.path.join(golden_util.GOLDEN_DIR, gold['fixture']))
    env = OracleVecEnv(1, steps=fix['steps'])
    env.reset(seeds=fix['seed'])
    env.reset(seeds=None)
    env.enable_event_log(True)
    stats = EU.new_stats()
    assert len(gold['steps']) == 120
    for t, want in enumerate(gold['steps']):
        env.step(fix['actions'][t][None, :])
        doc = json.loads(env.true_state_json(0))
        hot, cold = env.get_state(0), env.get_cold(0)
        edges, counts = BE.from_row(hot, cold, fix['steps'])
        assert edges.shape == (160, 8) and edges.dtype == np.int32 and counts[6] == 1 and counts[7] == t + 1, t
        EU.compare(edges, counts, want, doc, t, stats)
        d_edges, d_counts = BE.from_true_state(doc)
        assert np.array_equal(d_edges, edges) and np.array_equal(d_counts, counts), t
        total = int(counts[5])
        for cap in {1, max(total - 1, 1), max(total, 1), 7}:          # a shorter list is a prefix; the counts stay the untruncated numbers
            e2, c2 = BE.from_row(hot, cold, fix['steps'], cap)
            assert np.array_equal(e2, edges[:cap]) and np.array_equal(c2, counts), (t, cap)
            e3, c3 = BE.from_true_state(doc, cap)
            assert np.array_equal(e3, e2) and np.array_equal(c3, c2), (t, cap)
    env.close()
    # the fixture exercises what the comparison is about (the reference alone gives 686, 19, 18, 328)
    assert stats['entries'] >= 600 and stats['merged'] >= 10 and stats['third_party'] >= 10 and stats['remote_outside'] >= 200, stats


def test_reference_helper_reads_connections_doubling_ports_and_order():
    """The helper on a hand-made observation: only items with a remote address, halved counts, absent ports 0, the sort, slots per agent."""
    doc = {'cidr': [10, 11, 12, 13, 14, 15, 16, 17, 18], 'hosts': [{'h': 1, 'ip': 5}, {'h': 2, 'ip': 6}, {'h': 70, 'ip': 9}, {'h': 18, 'ip': 7}]}
    n1, n2, n18 = EU.BU.T.hostname_of(1), EU.BU.T.hostname_of(2), EU.BU.T.hostname_of(18)
    ssh = {'local_address': '10.0.10.5', 'local_port': 22, 'remote_address': '10.0.14.9', 'remote_port': 50000}
    scan = {'local_address': '10.0.10.6', 'local_port': 80, 'remote_address': '10.0.10.5'}                 # no remote port
    third = {'local_address': '10.0.11.7', 'remote_address': '10.0.14.9', 'remote_port': 4444}             # no local port
    local = {'local_address': '10.0.10.5', 'local_port': 51000}                                            # no remote address: not an edge
    obs = {f'blue_agent_{b}': {'success': 'UNKNOWN', 'action': 'Sleep'} for b in range(5)}
    obs['blue_agent_0'] = {'success': 'TRUE', 'action': 'Monitor',
                           n2: {'Processes': [{'Connections': [scan]}, {'Connections': [scan]}, {'Connections': [third, third]}]},
                           n1: {'Processes': [{'Connections': [ssh]}] * 4 + [{'Connections': [local]}] * 2 + [{'PID': 77}]}}
    obs['blue_agent_1'] = {'success': 'TRUE', 'action': 'Monitor', n18: {'Processes': [{'Connections': [third]}, {'Connections': [third]}]}}
    stats = EU.new_stats()
    edges, counts = EU.reference_edges(obs, doc, 6, stats)
    assert edges.tolist() == [[0, 1, 1, 70, 22, 50000, 2, 0], [0, 2, 2, 1, 80, 0, 1, 1], [0, 2, 18, 70, 0, 4444, 1, 2], [1, 18, 18, 70, 0, 4444, 1, 0],
                              [-1] * 8, [-1] * 8]
    assert counts.tolist() == [3, 1, 0, 0, 0, 4, 1, 0]
    assert stats == dict(entries=5, merged=1, third_party=1, remote_outside=3, max_edges=4)
    edges, counts = EU.reference_edges(obs, doc, 2)
    assert edges[:, 7].tolist() == [0, 1] and counts.tolist() == [3, 1, 0, 0, 0, 4, 1, 0]
    obs['blue_agent_0'][n1]['Processes'].append({'Connections': [ssh]})
    try:
        EU.reference_edges(obs, doc)
    except AssertionError:
        pass
    else:
        raise AssertionError('an odd count of a connection entry must be refused')
