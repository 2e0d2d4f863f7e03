"""k_reward_terms timed on one GPU beside k_blue_view and k_red_view, and what recording the reward terms costs a blue learner's loop.  8192
episodes, counter mode, 500-step episodes with autoreset, 100 steps in.

  python tools/reward_terms_probe.py run --json CALLS.json
        (a) K steps of [stand-in blue policy on the device, cc4_step_device] with the switch off (the fast build of the step kernel), K steps
            of [the same + cc4_reward_terms_device] with the switch on (the full build, a launch more per step), and K steps with the switch
            on and no view: enqueued with no host wait, one synchronise at the end; wall clock; twice each, alternating.
        (b) switch on: --reps calls each of cc4_reward_terms_device, cc4_blue_view_device and cc4_red_view_device on the same rows, for the
            profiler to time.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/reward_terms_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler (no counters): the kernels' own durations per dispatch
  python tools/reward_terms_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_reward_terms.txt

Bytes k_reward_terms must move per episode, from the shapes: the parts of the hot row it reads (READ_FIELDS), the 64-byte record of the cold row,
and the 9 x 4 x 4 + 16 x 4 output bytes."""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, WARM = 8192, 3
VP = ctypes.c_void_p
# csrc/cc4_state.h: what rt_valid / rt_green / rt_impact / rt_word (csrc/cc4_reward_terms.h) read of the hot row
READ_FIELDS = {'phase, step_count': 8, 'n_green': 1, 'green_host': 80, 'the six red headers: the exec word and nsess': 6 * 8}
RECORD, OUT_BYTES = 64, 9 * 4 * 4 + 16 * 4
BLUE_BYTES, RED_BYTES = 6378, 8181          # profiles/r22_blue_view.txt (log off), profiles/r21_red_learner.txt: bytes per episode


class Dev:
    def __init__(self, hip, nbytes):
        self.hip, self.p = hip, VP()
        assert hip.hipMalloc(ctypes.byref(self.p), nbytes) == 0

    def down(self, dtype, shape, off=0):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(VP), VP(self.p.value + off), out.nbytes, 2) == 0
        return out


def run(a):
    from cage_challenge_4_amd import CC4VecEnv
    from cage_challenge_4_amd.vec_env import _hip
    hip = _hip()
    res = {'n': N, 'steps': a.steps, 'reps': a.reps}
    env = CC4VecEnv(N, steps=500, rng_mode=1, autoreset=True, strict=False)
    env.reset(seeds=1)
    env.run_random_steps(7, 0, 100, timed=False)
    env.synchronize()
    res['step_kernel'] = env.step_kernel
    lib, h = env.lib, env._h
    acts = VP()
    env._chk(lib.cc4_actions_device(h, ctypes.byref(acts)), 'cc4_actions_device')
    b_terms = N * 9 * 4 * 4
    d_rt, d_blue, d_red = Dev(hip, N * OUT_BYTES), Dev(hip, N * (5 * 137 * 8 + 5 * 16 * 4)), Dev(hip, N * (6 * 137 * 8 + 6 * 16 * 4))
    p_w, p_bs, p_rs = VP(d_rt.p.value + b_terms), VP(d_blue.p.value + N * 5 * 137 * 8), VP(d_red.p.value + N * 6 * 137 * 8)

    def loop(t0, k, view):
        rc = 0
        for t in range(t0, t0 + k):
            rc = rc or lib.cc4_random_actions_device(h, 7, t) or lib.cc4_step_device(h, acts, None)
            if view:
                rc = rc or lib.cc4_reward_terms_device(h, None, 0, None, N, d_rt.p, p_w)
        env._chk(rc, 'device loop')
        env.synchronize()

    # ---- (a) the loop: switch off / switch on with the view / switch on without it; twice each, alternating
    t, walls = 100, {'off': [], 'on_view': [], 'on': []}
    for _ in range(2):
        for key, on, view in (('off', False, False), ('on_view', True, True), ('on', True, False)):
            env.enable_reward_terms(on)
            loop(t, 10, view)                       # warm: the build of the step kernel this setting launches
            t += 10
            t0 = time.perf_counter()
            loop(t, a.steps, view)
            walls[key].append(time.perf_counter() - t0)
            t += a.steps
    res['loop_s'] = walls
    # ---- (b) the three kernels on the same rows, switch on (the last step recorded)
    env.enable_reward_terms(True)
    loop(t, 3, False)
    for _ in range(WARM + a.reps):
        env._chk(lib.cc4_reward_terms_device(h, None, 0, None, N, d_rt.p, p_w), 'cc4_reward_terms_device')
        env._chk(lib.cc4_blue_view_device(h, None, 0, None, N, d_blue.p, p_bs), 'cc4_blue_view_device')
        env._chk(lib.cc4_red_view_device(h, None, 0, None, N, d_red.p, p_rs), 'cc4_red_view_device')
        env.synchronize()
    terms, words = d_rt.down(np.int32, (N, 9, 4)), d_rt.down(np.int32, (N, 16), b_terms)
    res['rows'] = {'valid': float(words[:, 0].mean()), 'events_per_episode': float(terms[..., 3].sum()) / N,
                   'restore_per_episode': float(-words[:, 4].sum()) / N, 'brm_mean': float(words[:, 3].mean())}
    faults = ctypes.c_uint32(0)
    env._chk(lib.cc4_copy_faults(h, ctypes.byref(faults)), 'cc4_copy_faults')
    res['faults'] = faults.value
    env.close()
    with open(a.json, 'w') as f:
        json.dump(res, f, indent=1)
    print(res)


def kernel_times(trace_dir, name):
    files = sorted(glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True))
    if len(files) != 1:
        raise SystemExit(f'expected one *kernel_trace.csv under {trace_dir}, found {files}')
    rows = [r for r in csv.DictReader(open(files[0])) if name in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    return [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1000.0 for r in rows]


def report(a):
    c = json.load(open(a.calls))
    n, k, per = c['n'], c['steps'], WARM + c['reps']
    rt, blue, red = (kernel_times(a.trace, s) for s in ('k_reward_terms', 'k_blue_view', 'k_red_view'))
    if len(blue) != per or len(red) != per or len(rt) < per:
        raise SystemExit(f'{len(rt)} k_reward_terms, {len(blue)} k_blue_view, {len(red)} k_red_view dispatches in the trace, expected at least {per}, {per}, {per}')
    med = lambda x: float(np.median(x[WARM:]))          # noqa: E731
    t_rt, t_b, t_r = med(rt[-per:]), med(blue), med(red)
    in_loop = float(np.median(rt[:-per]))
    bytes_rt = sum(READ_FIELDS.values()) + RECORD + OUT_BYTES
    tbs = lambda b, us: b * n / (us * 1e-6) / 1e12      # noqa: E731
    w = {key: min(v) for key, v in c['loop_s'].items()}
    us = lambda s: 1e6 * s / k                          # noqa: E731
    runs = lambda key: ', '.join(f'{us(x):.1f}' for x in c['loop_s'][key])      # noqa: E731
    r = c['rows']
    lines = [f'# tools/reward_terms_probe.py: k_reward_terms on one GPU; {n} episodes, counter mode, 500-step episodes with autoreset, 100 steps in',
             f'# kernel us: rocprofv3 --kernel-trace --stats in a run of its own (no counters), median of {c["reps"]} dispatches on the same rows',
             f'  k_reward_terms  {t_rt:7.1f} us   {bytes_rt:5d} B per episode from the shapes ({OUT_BYTES} B out)   {tbs(bytes_rt, t_rt):5.2f} TB/s   '
             f'(valid {r["valid"]:.3f}, {r["events_per_episode"]:.2f} charged events and {r["restore_per_episode"]:.2f} Restore costs per episode, mean brm {r["brm_mean"]:.2f})',
             f'  k_blue_view     {t_b:7.1f} us   {BLUE_BYTES:5d} B per episode (profiles/r22_blue_view.txt, log off)   {tbs(BLUE_BYTES, t_b):5.2f} TB/s',
             f'  k_red_view      {t_r:7.1f} us   {RED_BYTES:5d} B per episode (profiles/r21_red_learner.txt)   {tbs(RED_BYTES, t_r):5.2f} TB/s',
             f'  k_reward_terms inside the loop (behind a step): median of {len(rt) - per} dispatches {in_loop:7.1f} us',
             f'# the loop ({c["step_kernel"]}): wall clock of {k} steps, enqueued without a host wait, one synchronise at the end; two runs each, alternating; the faster one.',
             '#   Episode steps/s (x 5 = agent-env steps/s); outside the profiler',
             f'  switch off: k_random_actions + cc4_step_device (fast build)                   {n * k / w["off"]:12.4g} steps/s   {us(w["off"]):8.1f} us per step   (runs: {runs("off")})',
             f'  switch on:  the same on the full build, records written                       {n * k / w["on"]:12.4g} steps/s   {us(w["on"]):8.1f} us per step   (runs: {runs("on")})',
             f'  switch on:  the same + cc4_reward_terms_device                                {n * k / w["on_view"]:12.4g} steps/s   {us(w["on_view"]):8.1f} us per step   (runs: {runs("on_view")})',
             f'  the switch costs {us(w["on"] - w["off"]):.1f} us per step = {100 * (w["on"] - w["off"]) / w["off"]:.1f} % (the full build of the step kernel); '
             f'the view adds {us(w["on_view"] - w["on"]):.1f} us per step; together {100 * (w["on_view"] - w["off"]) / w["off"]:.1f} %',
             f'  fault bits after the run: {c["faults"]}']
    txt = '\n'.join(lines) + '\n'
    print(txt, end='')
    with open(a.out, 'w') as fo:
        fo.write(txt)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--reps', type=int, default=20)
    r.add_argument('--steps', type=int, default=200)
    r.add_argument('--json', required=True)
    p = sub.add_parser('report')
    p.add_argument('--calls', required=True)
    p.add_argument('--trace', required=True)
    p.add_argument('--out', required=True)
    a = ap.parse_args()
    (run if a.cmd == 'run' else report)(a)


if __name__ == '__main__':
    main()
