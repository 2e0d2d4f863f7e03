"""What the tests of "log-probabilities of stored blue actions" (test_logp_cpu.py, test_logp_device.py, test_logp_torch.py) share: real mask rows
from the CPU oracle, stored actions drawn on valid slots, the crafted rows, and the comparisons with the float64 restatement
(cage_challenge_4_amd.action_logp.reference) under the tolerances below.

The tolerances follow from float32 rounding, not from the code under test.  logp and entropy: |v - ref| <= 2^-12 max(1, |ref|), the bound of the
sampling tests.  A gradient value is about 30 float32 operations -- a depth-10 sum of at most 242 terms among them -- on magnitudes up to
max(1, |ref|), scaled by 1 / T: |v - ref| <= 2^-12 max(1, 1 / T) max(1, |ref|), a margin of about 130; a bfloat16 output adds half an ulp,
2^-8 |ref|, a float16 output 2^-11 |ref| + 2^-25.  No case is left out."""
import numpy as np

import sample_util as U
from cage_challenge_4_amd import action_logp as AL

SEG = AL.SEGMENTS
TEMPERATURES = (0.5, 1.0, 2.0)


def oracle_masks(n=4, steps=30):
    """Mask rows of n oracle episodes (counter mode); episode 0 has the segment-edge slots 0 / 81 / 241 (sample_util.edge_seed)."""
    from oracle_binding import OracleVecEnv
    ora = OracleVecEnv(n, steps=steps, rng_mode=1)
    ora.reset(seeds=U.edge_seed(1, steps))
    mask = ora.mask().astype(bool).copy()
    ora.close()
    assert U.has_edge_slots(mask[0])
    return mask


def stored_actions(rng, mask, skip=0.2):
    """[B, 5] int32: a valid slot of every agent, drawn at random; a share `skip` of them -1."""
    out = np.zeros((mask.shape[0], 5), np.int32)
    for e in range(mask.shape[0]):
        for b in range(5):
            out[e, b] = -1 if rng.random() < skip else rng.choice(U.valid_slots(mask[e], b))
    if skip > 0:
        out[0, 2] = -1           # (at least one, whatever the draws)
    return out


def edge_actions(mask_row):
    """Stored actions on the segment-edge slots of a topology that has them: [(actions [5], agent, slot)]."""
    b82 = [b for b in range(4) if mask_row[SEG[b]] and mask_row[SEG[b] + 81]][0]
    base = np.array(U.SLEEP, np.int32)
    out = []
    for b, k in ((b82, 0), (b82, 81), (4, 0), (4, 241), (4, U.SLEEP[4])):
        a = base.copy()
        a[b] = k
        out.append((a, b, k))
    return out


def crafted_rows(mask_row, rng):
    """[(name, logits [570] float32, mask [570] bool, actions [5] int32, refused agents as a tuple)]: the crafted rows of the issue's item 3.
    mask_row: a topology with the segment-edge slots."""
    base = U.random_logits(rng)
    sleep = np.array(U.SLEEP, np.int32)
    act = np.array([U.valid_slots(mask_row, b)[-1] for b in range(5)], np.int32)
    rows = [('random logits, the last valid slots', base, mask_row, act, ())]      # (what the refusal rows below depart from)
    only = np.zeros(570, bool)
    only[np.array(SEG[:5]) + sleep] = True
    rows.append(('only the Sleep slot valid', base, only, sleep, ()))
    full = mask_row.copy()
    full[SEG[4]:] = True
    rows.append(('all 242 slots valid', base, full, np.array([act[0], act[1], act[2], act[3], 241], np.int32), ()))
    lg = base.copy()
    for b in range(5):
        lg[SEG[b] + U.valid_slots(mask_row, b)[0]] = -np.inf
    rows.append(('-inf among the valid logits', lg, mask_row, act, ()))
    rows.append(('the action on a valid -inf slot', lg, mask_row, np.array([U.valid_slots(mask_row, b)[0] for b in range(5)], np.int32), ()))
    rows.append(('every action -1', base, mask_row, np.full(5, -1, np.int32), ()))
    for a, b, k in edge_actions(mask_row):
        rows.append((f'the action on slot {k} of agent {b}', base, mask_row, a, ()))
    lg = base.copy()
    inv = np.nonzero(~mask_row)[0]
    lg[inv[::3]], lg[inv[1::3]], lg[inv[2::3]] = np.nan, np.inf, 3e38
    rows.append(('NaN, +inf and 3e38 on invalid slots', lg, mask_row, act, ()))
    # each refusal cause in turn, on agent b; the other four agents are unaffected
    for b, cause in ((0, 'nan'), (4, 'nan'), (2, '+inf'), (3, 'all -inf'), (1, 'no valid slot'), (4, 'action -2'), (0, 'action 82'), (4, 'action 242'),
                     (2, 'action 2^31 - 1'), (3, 'action on an invalid slot'), (4, 'action on an invalid slot')):
        lg, mk, a = base.copy(), mask_row.copy(), act.copy()
        v = U.valid_slots(mask_row, b)
        if cause == 'nan':
            lg[SEG[b] + v[len(v) // 2]] = np.nan
        elif cause == '+inf':
            lg[SEG[b] + v[-1]] = np.inf
        elif cause == 'all -inf':
            lg[SEG[b] + v] = -np.inf
        elif cause == 'no valid slot':
            mk[SEG[b]:SEG[b + 1]] = False
        elif cause == 'action on an invalid slot':
            a[b] = np.nonzero(~mask_row[SEG[b]:SEG[b + 1]])[0][-1]
        else:
            a[b] = {'action -2': -2, 'action 82': 82, 'action 242': 242, 'action 2^31 - 1': 2 ** 31 - 1}[cause]
        rows.append((f'agent {b} refused: {cause}', lg, mk, a, (b,)))
    return rows


def out_tolerance(ref, code):
    """What the rounding of a 16-bit output adds: half an ulp of ref."""
    return {3: 0.0, 2: 2.0 ** -8 * np.abs(ref), 1: 2.0 ** -11 * np.abs(ref) + 2.0 ** -25}[code]


def check_stats(logp, ent, ref_logp, ref_ent, what):
    """logp / entropy [.., 5] against the restatement's: |v - ref| <= 2^-12 max(1, |ref|); -inf must be -inf.  Returns the largest differences."""
    worst = []
    for v, r, name in ((logp, ref_logp, 'logp'), (ent, ref_ent, 'entropy')):
        v, r = np.asarray(v, np.float64), np.asarray(r, np.float64)
        inf = np.isinf(r)
        assert np.array_equal(v[inf], r[inf]), f'{what}: {name} where the reference is infinite'
        d = np.abs(v[~inf] - r[~inf])
        bad = d > 2.0 ** -12 * np.maximum(1.0, np.abs(r[~inf]))
        assert not bad.any(), f'{what}: {name} {v[~inf][bad][:4]}, reference {r[~inf][bad][:4]}'
        worst.append(float(d.max(initial=0.0)))
    return worst


def check_grad(grad, ref, temperature, code, what):
    """A gradient [.., 570] against the restatement's: 2^-12 max(1, 1 / T) max(1, |ref|) plus the output dtype's rounding.  Returns max |v - ref|."""
    v, ref = np.asarray(grad, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(v).all(), f'{what}: a gradient value that is not finite'
    d = np.abs(v - ref)
    bad = d > 2.0 ** -12 * max(1.0, 1.0 / temperature) * np.maximum(1.0, np.abs(ref)) + out_tolerance(ref, code)
    assert not bad.any(), f'{what}: gradient {v[bad][:4]}, reference {ref[bad][:4]} at {np.argwhere(bad)[:4].tolist()}'
    return float(d.max(initial=0.0))
