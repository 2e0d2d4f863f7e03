"""k_blue_view timed on one GPU beside k_red_view and k_state_features, and what the view adds to a blue learner's loop.  8192 episodes, counter
mode, 500-step episodes with autoreset, 100 steps in.

  python tools/blue_view_probe.py run --json CALLS.json
        (a) event log off: K steps of [stand-in blue policy on the device, cc4_step_device, cc4_blue_view_device], enqueued with no host wait, one
            synchronise at the end -- and K steps of the same loop without the view; wall clock.
        (b) event log off: --reps calls each of cc4_blue_view_device, cc4_red_view_device and cc4_state_features_device on the same rows, for the
            profiler to time.
        (c) event log on (a few steps with it first, so that the log describes the last step): --reps calls of cc4_blue_view_device.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/blue_view_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler (no counters): the kernels' own durations per dispatch
  python tools/blue_view_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_blue_view.txt

Bytes k_blue_view must move per episode, from the shapes: the parts of the hot row it reads (READ_FIELDS), with the log on its header and its
entries (12 bytes each), the sus entries (4 bytes each), and the 5 x 137 x 8 + 5 x 16 x 4 output bytes."""
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

N, WARM, LOG_STEPS = 8192, 3, 5
VP = ctypes.c_void_p
# csrc/cc4_state.h: what bv_host_row / bv_scalar / bv_events_valid (csrc/cc4_blue_view.h) read of the hot row
READ_FIELDS = {'step_count, steps, phase': 12, 'exists': 20, 'bexec': 40, 'blue[5]': 200, 'hev': 137, 'nsf of the analysed hosts': 5}
LOG_HEADER, LOG_ENTRY, SUS_ENTRY = 16, 12, 4
OUT_BYTES = 5 * 137 * 8 + 5 * 16 * 4
RED_BYTES, FEAT_BYTES = 8181, 7600          # profiles/r21_red_learner.txt, profiles/r13_state_features.txt: bytes per episode
RED_US, FEAT_US = 20.0, 23.9                # profiles/r21_red_learner.txt: the committed figures


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
    b_hosts = N * 5 * 137 * 8
    d_blue, d_red, d_feat = Dev(hip, N * OUT_BYTES), Dev(hip, N * (6 * 137 * 8 + 6 * 16 * 4)), Dev(hip, N * (137 * 16 + 32 * 4))
    p_bs, p_rs, p_glob = VP(d_blue.p.value + b_hosts), VP(d_red.p.value + N * 6 * 137 * 8), VP(d_feat.p.value + N * 137 * 16)

    def loop(t0, k, view):
        rc = 0
        for t in range(t0, t0 + k):
            rc = rc or lib.cc4_random_actions_device(h, 7, t) or lib.cc4_step_device(h, acts, None)
            if view:
                rc = rc or lib.cc4_blue_view_device(h, None, 0, None, N, d_blue.p, p_bs)
        env._chk(rc, 'device loop')
        env.synchronize()

    # ---- (a) the loop with and without the view, event log off; twice each, alternating
    loop(100, 10, True)
    t, walls = 110, {True: [], False: []}
    for view in (True, False, True, False):
        t0 = time.perf_counter()
        loop(t, a.steps, view)
        walls[view].append(time.perf_counter() - t0)
        t += a.steps
    res['loop_view_s'], res['loop_no_view_s'] = walls[True], walls[False]
    # ---- (b) the three kernels on the same rows, log off
    for _ in range(WARM + a.reps):
        env._chk(lib.cc4_blue_view_device(h, None, 0, None, N, d_blue.p, p_bs), 'cc4_blue_view_device')
        env._chk(lib.cc4_red_view_device(h, None, 0, None, N, d_red.p, p_rs), 'cc4_red_view_device')
        env._chk(lib.cc4_state_features_device(h, None, 0, None, N, d_feat.p, p_glob), 'cc4_state_features_device')
        env.synchronize()
    scal = d_blue.down(np.int32, (N, 5, 16), b_hosts)
    res['off'] = {'events_valid': float(scal[..., 10].mean()), 'sus_per_episode': float(scal[..., 8].sum()) / N}
    # ---- (c) log on
    env.enable_event_log(True)
    res['step_kernel_log'] = env.step_kernel
    loop(t, LOG_STEPS, False)
    for _ in range(WARM + a.reps):
        env._chk(lib.cc4_blue_view_device(h, None, 0, None, N, d_blue.p, p_bs), 'cc4_blue_view_device')
        env.synchronize()
    hosts, scal = d_blue.down(np.uint8, (N, 5, 137, 8)), d_blue.down(np.int32, (N, 5, 16), b_hosts)
    res['on'] = {'events_valid': float(scal[..., 10].mean()), 'sus_per_episode': float(scal[..., 8].sum()) / N,
                 'entries_per_episode': float(scal[..., 11].sum()) / N, 'nonzero_rows_per_episode': float(hosts.any(axis=3).sum()) / N}
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
    blue, red, feat = (kernel_times(a.trace, s) for s in ('k_blue_view', 'k_red_view', 'k_state_features'))
    if len(red) != per or len(feat) != per or len(blue) < 2 * per:
        raise SystemExit(f'{len(blue)} k_blue_view, {len(red)} k_red_view, {len(feat)} k_state_features dispatches in the trace, expected at least {2 * per}, {per}, {per}')
    med = lambda x: float(np.median(x[WARM:]))          # noqa: E731
    b_on, b_off, r, f = med(blue[-per:]), med(blue[-2 * per:-per]), med(red), med(feat)
    in_loop = float(np.median(blue[:-2 * per]))
    hot = sum(READ_FIELDS.values())
    bytes_off = hot + LOG_HEADER + SUS_ENTRY * c['off']['sus_per_episode'] + OUT_BYTES
    bytes_on = hot + LOG_HEADER + LOG_ENTRY * c['on']['entries_per_episode'] + SUS_ENTRY * c['on']['sus_per_episode'] + OUT_BYTES
    tbs = lambda b, us: b * n / (us * 1e-6) / 1e12      # noqa: E731
    wv, wn = min(c['loop_view_s']), min(c['loop_no_view_s'])
    lines = [f'# tools/blue_view_probe.py: k_blue_view on one GPU; {n} episodes, counter mode, 500-step episodes with autoreset, 100 steps in',
             f'# kernel us: rocprofv3 --kernel-trace --stats in a run of its own (no counters), median of {c["reps"]} dispatches on the same rows',
             f'  k_blue_view, log off  {b_off:7.1f} us   {bytes_off:6.0f} B per episode from the shapes ({c["off"]["sus_per_episode"]:.1f} sus entries; {OUT_BYTES} B out)   {tbs(bytes_off, b_off):5.2f} TB/s',
             f'  k_blue_view, log on   {b_on:7.1f} us   {bytes_on:6.0f} B per episode ({c["on"]["entries_per_episode"]:.1f} log entries counted with rep -- an upper bound of the 12-byte records --, '
             f'{c["on"]["sus_per_episode"]:.1f} sus entries, {c["on"]["nonzero_rows_per_episode"]:.1f} non-zero rows of 685; events_valid {c["on"]["events_valid"]:.3f})   {tbs(bytes_on, b_on):5.2f} TB/s',
             f'  k_red_view            {r:7.1f} us   {RED_BYTES:6d} B per episode (profiles/r21_red_learner.txt: {RED_US} us)   {tbs(RED_BYTES, r):5.2f} TB/s',
             f'  k_state_features      {f:7.1f} us   {FEAT_BYTES:6d} B per episode (profiles/r21_red_learner.txt: {FEAT_US} us)   {tbs(FEAT_BYTES, f):5.2f} TB/s',
             f'  k_blue_view inside the loop (log off, behind a step): median of {len(blue) - 2 * per} dispatches {in_loop:7.1f} us',
             f'# the loop, log off ({c["step_kernel"]}): wall clock of {k} steps, enqueued without a host wait, one synchronise at the end; two runs each, alternating; the faster one.',
             '#   Episode steps/s (x 5 = agent-env steps/s); outside the profiler',
             f'  k_random_actions + cc4_step_device + cc4_blue_view_device   {n * k / wv:12.4g} steps/s   {1e6 * wv / k:8.1f} us per step   (runs: {", ".join(f"{1e6 * x / k:.1f}" for x in c["loop_view_s"])})',
             f'  the same without the view                                   {n * k / wn:12.4g} steps/s   {1e6 * wn / k:8.1f} us per step   (runs: {", ".join(f"{1e6 * x / k:.1f}" for x in c["loop_no_view_s"])})',
             f'  the view adds {1e6 * (wv - wn) / k:.1f} us per step = {100 * (wv - wn) / wn:.1f} %',
             f'  step kernel with the log on: {c["step_kernel_log"]}; fault bits after the run: {c["faults"]}']
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
