"""What the tests of the masked action sampling (test_sample_cpu.py, test_sample_device.py, test_sample_torch.py) share: the value sets a 16-bit
logits dtype can carry, the crafted logits rows, and the comparison of a float32 result with the float64 restatement
(cage_challenge_4_amd.action_sampling.reference) under the two tolerances.

The tolerances follow from float32 rounding, not from the code under test.  A score z = l / T + g is about ten float32 operations on magnitudes up to
max(1, max |z|): an error of about 10 * 2^-24 * max(1, max |z|), plus a few ulp per log.  tau = 2^-12 * max(1, max |z|) leaves a margin of about
400 over that.  An agent whose float64 winning margin is at least tau must get exactly the reference's action; below tau one of its top two.  logp
and entropy: |value - reference| <= 2^-12 * max(1, |reference|)."""
import numpy as np

from bf16_util import to_bits, upcast
from cage_challenge_4_amd import action_sampling as AS
from cage_challenge_4_amd import blue_view as BV

SEG = AS.SEGMENTS
SLEEP = (49, 49, 49, 49, 145)          # the agents' Sleep slots (3 * hosts + 1): always valid


def value_sets(lg):
    """lg float32 [.., 570] -> {dtype code: (the float32 values that dtype carries, the array to hand the device)}: 3 float32, 2 bfloat16 (uint16
    bit patterns), 1 float16."""
    bits = to_bits(lg)
    with np.errstate(over='ignore'):
        h = lg.astype(np.float16)
    return {3: (lg, lg), 2: (upcast(bits), bits), 1: (h.astype(np.float32), h)}


def busy_of(hot, steps=0):
    return BV.from_row(hot, None, steps)[1][:, 0] != 0


def random_logits(rng, shape=(570,), scale=4.0):
    """|l| <= 20 (with T >= 0.25 and |g| < 17: |z| <= 100)."""
    return np.clip(rng.standard_normal(shape) * scale, -20, 20).astype(np.float32)


class Tally:
    """Collects a test's (entry, agent) cases: how many fell below tau, and the largest float differences."""

    def __init__(self):
        self.cases = self.below = 0
        self.dlogp = self.dent = 0.0

    def check(self, actions, stats, ref, what=''):
        """actions [5], stats [5, 2] or None of an implementation; ref: reference(..., details=True)."""
        ra, rl, rn, margin, d = ref
        for b in range(5):
            self.cases += 1
            tau = 2.0 ** -12 * d['zmax'][b]
            lp = rl[b]
            if margin[b] >= tau:
                assert actions[b] == ra[b], f'{what} agent {b}: action {actions[b]}, reference {ra[b]} (margin {margin[b]:.3g} >= tau {tau:.3g})'
            else:
                self.below += 1
                assert actions[b] in (ra[b], d['second'][b]), f'{what} agent {b}: action {actions[b]}, reference {ra[b]} or {d["second"][b]}'
                if actions[b] != ra[b]:
                    lp = d['logp_second'][b]
            if stats is not None:
                dl, de = abs(float(stats[b, 0]) - lp), abs(float(stats[b, 1]) - rn[b])
                self.dlogp, self.dent = max(self.dlogp, dl), max(self.dent, de)
                assert dl <= 2.0 ** -12 * max(1.0, abs(lp)), f'{what} agent {b}: logp {stats[b, 0]!r}, reference {lp!r}'
                assert de <= 2.0 ** -12 * max(1.0, abs(rn[b])), f'{what} agent {b}: entropy {stats[b, 1]!r}, reference {rn[b]!r}'

    def close(self, what):
        print(f'{what}: {self.cases} cases, {self.below} below tau, max |logp - ref| {self.dlogp:.3g}, max |entropy - ref| {self.dent:.3g}')
        assert self.below * 100 <= self.cases, f'{what}: {self.below} of {self.cases} cases below tau (at most 1 %: choose other seeds)'


def valid_slots(mask, b):
    return np.nonzero(np.asarray(mask[SEG[b]:SEG[b + 1]]))[0]


def has_edge_slots(mask):
    """The topology has slots 0 and 81 of some agent with 82 slots, and slots 0 and 241 of agent 4 (its first server and its last user)."""
    return any(mask[SEG[b]] and mask[SEG[b] + 81] for b in range(4)) and bool(mask[SEG[4]] and mask[SEG[4] + 241])


def edge_seed(rng_mode=1, steps=30):
    """The first reset seed (both RNG modes generate the scenario from it) whose topology has the segment-edge slots: found on the CPU oracle."""
    from oracle_binding import OracleVecEnv
    for base in range(0, 4096, 64):
        ora = OracleVecEnv(64, steps=steps, rng_mode=rng_mode)
        ora.reset(seeds=base)
        hit = [k for k, m in enumerate(ora.mask()) if has_edge_slots(m)]
        ora.close()
        if hit:
            return base + hit[0]
    raise AssertionError('no topology with the segment-edge slots among 4096 seeds')


def crafted_edge_rows(mask):
    """[(name, logits [570], agent, slot)]: +20 on one valid slot and -20 elsewhere, at slots 0 and 81 of an agent with 82 slots and at slots 0,
    241 and the Sleep slot of agent 4 (a topology that has them: has_edge_slots): that slot is drawn, whatever the noise (|g| < 17 < 40)."""
    assert has_edge_slots(mask)
    b82 = [b for b in range(4) if mask[SEG[b]] and mask[SEG[b] + 81]][0]
    rows = []
    for b, k in ((b82, 0), (b82, 81), (4, 0), (4, 241), (4, SLEEP[4])):
        lg = np.full(570, -20.0, np.float32)
        lg[SEG[b] + k] = 20.0
        rows.append((f'+20 on slot {k} of agent {b}', lg, b, k))
    return rows


def four_slot_logits(mask):
    """log(0.4, 0.3, 0.2, 0.1) on four valid slots of every agent (the first, the last, the Sleep slot and the one before it), -inf elsewhere.
    Returns (logits [570], slots [5, 4])."""
    lg = np.full(570, -np.inf, np.float32)
    slots = np.zeros((5, 4), np.int64)
    for b in range(5):
        v = valid_slots(mask, b)
        pick = [v[0], v[-1], SLEEP[b], SLEEP[b] - 1]      # Restore of the zone's last host slot ... Sleep - 1 is a host slot: valid or not
        pick = list(dict.fromkeys(int(k) for k in pick if k in v))
        for k in v:
            if len(pick) == 4:
                break
            if int(k) not in pick:
                pick.append(int(k))
        slots[b] = pick
        lg[SEG[b] + slots[b]] = np.log(np.array([0.4, 0.3, 0.2, 0.1], np.float32))
    return lg, slots


def chi2_bound(df):
    """The upper 1e-6 quantile of chi-square with df degrees of freedom: 30.7 for df = 3 (tabulated); beyond, Wilson-Hilferty
    df (1 - 2 / (9 df) + z sqrt(2 / (9 df)))^3 with z = 4.7534 the normal quantile, which for df >= 10 is within 1 % of the exact value."""
    if df == 3:
        return 30.7
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + 4.7534 * np.sqrt(a)) ** 3 * 1.01
