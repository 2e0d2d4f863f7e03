"""The Monitor's connection edges derived from the REFERENCE's dict observation (TEST INFRASTRUCTURE): what cc4_blue_edges_device must report for
a step, computed from CybORG.get_observation(agent) as tests/golden/blueobs_seed123_random.json records it -- not from the packed rows and not from
the engine's event log.  The true-state document supplies only the address plan (ip -> host id, blue_util.host_of_ip); hostnames map to host ids
by inverting true_state.hostname_of.

An edge is a 'Connections' item that has a 'remote_address' (blue_util: exactly the connection entries); an absent port is 0, an absent local
address is "no host".  The fixture is get_observation's doubled form (blue_util's docstring): such items are there an even number of times, which
is asserted, and the counts are halved.  Then the items are sorted by (agent, host, remote, local, local_port, remote_port)."""
import numpy as np

import blue_util as BU

NO_HOST = 255            # the byte the log carries for "no address"
ZONE_OF_SUBNET = (0, 1, 2, 3, -1, 4, 4, 4, -1)


def reference_multiset(step_obs, doc):
    """{(agent, host, remote, local byte, local_port, remote_port): count} of one recorded step, counts already halved."""
    ip2h = BU.host_of_ip(doc)
    raw = {}
    for b in range(5):
        for key, v in step_obs[f'blue_agent_{b}'].items():
            if key in ('success', 'action') or not isinstance(v, dict):
                continue
            h = BU.HOST_OF_NAME[key]
            for p in v.get('Processes', []):
                for c in p.get('Connections', []):
                    if 'remote_address' not in c:
                        continue
                    local = ip2h[c['local_address']] if 'local_address' in c else NO_HOST
                    k = (b, h, ip2h[c['remote_address']], local, c.get('local_port', 0), c.get('remote_port', 0))
                    raw[k] = raw.get(k, 0) + 1
    assert all(v % 2 == 0 for v in raw.values()), 'a connection entry is in the doubled observation an even number of times'
    return {k: v // 2 for k, v in raw.items()}


def edges_of_multiset(ms, max_edges=160, valid=1, step=0):
    """(edges [max_edges, 8] int32, counts [8] int32) of a {key: count} dictionary: the definition restated with a Python sort."""
    edges = np.full((max_edges, 8), -1, np.int32)
    counts = np.zeros(8, np.int32)
    slot = [0] * 5
    for i, k in enumerate(sorted(ms)):
        b, h, remote, local, lport, rport = k
        if i < max_edges:
            edges[i] = (b, h, local if local < 137 else -1, remote, lport, rport, ms[k], slot[b])
        slot[b] += 1
    counts[:5], counts[5], counts[6], counts[7] = slot, len(ms), valid, step
    return edges, counts


def reference_edges(step_obs, doc, max_edges=160, stats=None):
    ms = reference_multiset(step_obs, doc)
    if stats is not None:
        stats['entries'] += sum(ms.values())
        stats['merged'] += sum(1 for v in ms.values() if v > 1)
        stats['third_party'] += sum(1 for (b, h, remote, local, _lp, _rp) in ms if h != local and h != remote)
        stats['remote_outside'] += sum(1 for (b, _h, remote, _l, _lp, _rp) in ms if ZONE_OF_SUBNET[remote // 17] != b)
        stats['max_edges'] = max(stats['max_edges'], len(ms))
    return edges_of_multiset(ms, max_edges)


def new_stats():
    return dict(entries=0, merged=0, third_party=0, remote_outside=0, max_edges=0)


def edge_stats(edges, stats):
    """The same figures from an edge array [..., E, 8] (device tests: what a batch exercised)."""
    e = edges.reshape(-1, 8)
    e = e[e[:, 0] >= 0]
    stats['entries'] += int(e[:, 6].sum())
    stats['merged'] += int((e[:, 6] > 1).sum())
    stats['third_party'] += int(((e[:, 1] != e[:, 2]) & (e[:, 1] != e[:, 3])).sum())
    stats['remote_outside'] += int((np.asarray(ZONE_OF_SUBNET)[e[:, 3] // 17] != e[:, 0]).sum())


def compare(got_edges, got_counts, step_obs, doc, what, stats=None):
    """Edges and counts words 0..5 of one episode against the reference-derived ones."""
    edges, counts = reference_edges(step_obs, doc, got_edges.shape[0], stats)
    assert np.array_equal(got_counts[:6], counts[:6]), (what, got_counts.tolist(), counts.tolist())
    bad = np.argwhere((got_edges != edges).any(axis=1))
    assert bad.size == 0, (what, [(int(i), got_edges[i].tolist(), edges[i].tolist()) for i in bad[:6, 0]])
