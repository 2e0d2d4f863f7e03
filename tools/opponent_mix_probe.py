#!/usr/bin/env python
"""What a mix of red classes costs in ONE handle against the only way to run it before cc4_set_policies: a handle per class.

  mixed     one handle of 8192 episodes, red classes 0..3 (FiniteStateRedAgent, SleepAgent, DiscoveryFSRed, RandomSelectRedAgent) assigned to 2048
            episodes each (episode e: class e % 4)
  uniform   four handles of 2048 episodes created with red_policy = 0..3, run one after the other

Both step cc4_run_random_steps at K = 20 and K = 500 steps per call, counter mode, 500-step episodes with autoreset, the same seeds.  A region is
several calls back to back between two device synchronisations, timed with the host clock (a region of the uniform side is the four handles' calls in
turn); every shape is warmed up; mixed and uniform regions alternate, and the median region is reported with the extremes.  Rates are agent-env steps
per second: 5 blue agents x 8192 episodes x steps / region time on both sides.

  python tools/opponent_mix_probe.py [--rounds 3] [--out profiles/r17_opponent_mix.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, CLASSES = 8192, 500, 4
KS = (20, 500)
REGION_STEPS = 4000        # steps per timed region


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from cage_challenge_4_amd import CC4VecEnv
    cls = (np.arange(N) % CLASSES).astype(np.int8)
    mixed = CC4VecEnv(N, steps=STEPS, rng_mode=1, autoreset=True, strict=False, red_policy=cls)
    mixed.reset(seeds=0)
    uniform = []
    for c in range(CLASSES):
        e = CC4VecEnv(N // CLASSES, steps=STEPS, rng_mode=1, autoreset=True, strict=False, red_policy=c)
        e.reset(seeds=np.arange(N, dtype=np.uint64)[c::CLASSES])          # the seeds of the mixed handle's episodes of this class
        uniform.append(e)
    t = {'mixed': 0, 'uniform': 0}

    def region(side, K, calls):
        envs = [mixed] if side == 'mixed' else uniform
        for e in envs:
            e.synchronize()
        t0 = time.perf_counter()
        for e in envs:
            for i in range(calls):
                e.run_random_steps(1, t[side] + i * K, K, timed=False)
        for e in envs:
            e.synchronize()
        dt = time.perf_counter() - t0
        t[side] += calls * K
        return 5.0 * N * calls * K / dt / 1e6

    lines = [f'# opponent-mix probe: {N} episodes, counter mode, {STEPS}-step episodes with autoreset, red classes 0..3 on {N // CLASSES} episodes each; M agent-env steps/s',
             f'# (5 blue agents x {N} episodes x steps / host time of a region of ~{REGION_STEPS} steps between device synchronisations); median of',
             f'# {args.rounds} regions [min .. max]; mixed and uniform regions alternate in one process.',
             '# mixed: ONE handle with the classes assigned per episode (cc4_set_policies).  uniform: four handles of 2048 episodes, red_policy = 0..3, one after the other.', '']
    for K in KS:
        calls = max(1, REGION_STEPS // K)
        kern = (mixed.run_kernel_for(K), uniform[0].run_kernel_for(K))
        for side in ('mixed', 'uniform'):                                # warm-up of the shape
            region(side, K, max(1, calls // 4))
        got = {'mixed': [], 'uniform': []}
        for _ in range(args.rounds):
            for side in ('mixed', 'uniform'):
                got[side].append(region(side, K, calls))
        med = {s: statistics.median(v) for s, v in got.items()}
        lines.append(f'K = {K}')
        for side, k in zip(('mixed', 'uniform'), kern):
            v = got[side]
            lines.append(f'  {side:8s} {k:16s} {med[side]:8.1f}  [{min(v):8.1f} .. {max(v):8.1f}]  ({calls} calls per handle and region)')
        lines.append(f'  uniform / mixed = {med["uniform"] / med["mixed"]:.3f}')
        lines.append('')
    mixed._fetch()
    live = mixed.policies()[0][:, 0]
    lines.append(f'# live red classes of the mixed handle after {t["mixed"]} steps per episode (every episode regenerated {t["mixed"] // STEPS} times): '
                 f'{[int((live == c).sum()) for c in range(CLASSES)]} episodes of class 0..3; error words raised: {int(np.count_nonzero(mixed.err))}')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    for e in [mixed] + uniform:
        e.close()


if __name__ == '__main__':
    main()
