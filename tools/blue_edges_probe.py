"""k_blue_edges timed on one GPU beside k_blue_view and k_red_view, and what the edge lists add to a blue learner's loop.  8192 episodes, counter
mode, 500-step episodes with autoreset, 100 steps in, the per-step event log ON throughout (the lists are made of it).

  python tools/blue_edges_probe.py run --json CALLS.json
        (a) K steps of [stand-in blue policy on the device, cc4_step_device, cc4_blue_edges_device at max_edges 160], enqueued with no host wait,
            one synchronise at the end -- and K steps of the same loop without the lists; wall clock, twice each, alternating.
        (b) --reps calls each of cc4_blue_view_device and cc4_red_view_device, then of cc4_blue_edges_device at max_edges 160, then at 32, on the
            same rows, for the profiler to time.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/blue_edges_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler (no counters): the kernels' own durations per dispatch
  python tools/blue_edges_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_blue_edges.txt

Bytes k_blue_edges must move per episode, from the shapes: of the hot row exists and step_count, the log's header and its entries (12 bytes each),
and the max_edges x 32 + 32 output bytes."""
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
HOT_BYTES, LOG_HEADER, LOG_ENTRY = 20 + 4, 16, 12          # exists, step_count
VIEW_OUT = 5 * 137 * 8 + 5 * 16 * 4


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
    env.enable_event_log(True)
    res['step_kernel'] = env.step_kernel
    lib, h = env.lib, env._h
    acts = VP()
    env._chk(lib.cc4_actions_device(h, ctypes.byref(acts)), 'cc4_actions_device')
    d_edges, d_blue, d_red = Dev(hip, N * (160 * 32 + 32)), Dev(hip, N * VIEW_OUT), Dev(hip, N * (6 * 137 * 8 + 6 * 16 * 4))
    p_cnt, p_bs, p_rs = VP(d_edges.p.value + N * 160 * 32), VP(d_blue.p.value + N * 5 * 137 * 8), VP(d_red.p.value + N * 6 * 137 * 8)

    def loop(t0, k, lists):
        rc = 0
        for t in range(t0, t0 + k):
            rc = rc or lib.cc4_random_actions_device(h, 7, t) or lib.cc4_step_device(h, acts, None)
            if lists:
                rc = rc or lib.cc4_blue_edges_device(h, None, 0, None, N, 160, d_edges.p, p_cnt)
        env._chk(rc, 'device loop')
        env.synchronize()

    # ---- (a) the loop with and without the lists; twice each, alternating.  Distinct edges per episode over the steps of the first runs
    loop(100, 10, True)
    t, walls = 110, {True: [], False: []}
    per_step = []
    for lists in (True, False, True, False):
        t0 = time.perf_counter()
        loop(t, a.steps, lists)
        walls[lists].append(time.perf_counter() - t0)
        t += a.steps
        if lists:
            per_step.append(d_edges.down(np.int32, (N, 8), N * 160 * 32))
    res['loop_lists_s'], res['loop_no_lists_s'] = walls[True], walls[False]
    loop(t, LOG_STEPS, False)
    # ---- (b) the kernels on the same rows
    for _ in range(WARM + a.reps):
        env._chk(lib.cc4_blue_view_device(h, None, 0, None, N, d_blue.p, p_bs), 'cc4_blue_view_device')
        env._chk(lib.cc4_red_view_device(h, None, 0, None, N, d_red.p, p_rs), 'cc4_red_view_device')
        env.synchronize()
    for E in (160, 32):
        for _ in range(WARM + a.reps):
            env._chk(lib.cc4_blue_edges_device(h, None, 0, None, N, E, d_edges.p, VP(d_edges.p.value + N * E * 32)), 'cc4_blue_edges_device')
            env.synchronize()
    cnt = d_edges.down(np.int32, (N, 8), N * 32 * 32)
    scal = d_blue.down(np.int32, (N, 5, 16), N * 5 * 137 * 8)
    seen = np.concatenate(per_step + [cnt])
    res['events_valid'] = float(cnt[:, 6].mean())
    res['edges_mean'], res['edges_max'], res['edges_samples'] = float(seen[:, 5].mean()), int(seen[:, 5].max()), int(seen.shape[0])
    res['edges_mean_last'], res['edges_max_last'] = float(cnt[:, 5].mean()), int(cnt[:, 5].max())
    res['entries_per_episode'] = float(scal[..., 11].sum()) / N
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
    edges, blue, red = (kernel_times(a.trace, s) for s in ('k_blue_edges', 'k_blue_view', 'k_red_view'))
    if len(red) != per or len(blue) != per or len(edges) < 2 * per:
        raise SystemExit(f'{len(edges)} k_blue_edges, {len(blue)} k_blue_view, {len(red)} k_red_view dispatches in the trace, expected at least {2 * per}, {per}, {per}')
    med = lambda x: float(np.median(x[WARM:]))          # noqa: E731
    spread = lambda x: float(max(x[WARM:]) - min(x[WARM:]))          # noqa: E731
    e160, e32, in_loop = edges[-2 * per:-per], edges[-per:], edges[:-2 * per]
    log_bytes = HOT_BYTES + LOG_HEADER + LOG_ENTRY * c['entries_per_episode']
    tbs = lambda b, us: b * n / (us * 1e-6) / 1e12      # noqa: E731
    wl, wn = min(c['loop_lists_s']), min(c['loop_no_lists_s'])
    over = med(e160) - med(blue)
    lines = [f'# tools/blue_edges_probe.py: k_blue_edges on one GPU; {n} episodes, counter mode, 500-step episodes with autoreset, 100 steps in, event log on',
             f'# kernel us: rocprofv3 --kernel-trace --stats in a run of its own (no counters), median of {c["reps"]} dispatches on the same rows; (min .. max)',
             f'  k_blue_edges, max_edges 160  {med(e160):7.1f} us  ({min(e160[WARM:]):.1f} .. {max(e160[WARM:]):.1f})   {log_bytes + 160 * 32 + 32:6.0f} B per episode from the shapes '
             f'({160 * 32 + 32} B out)   {tbs(log_bytes + 160 * 32 + 32, med(e160)):5.2f} TB/s',
             f'  k_blue_edges, max_edges 32   {med(e32):7.1f} us  ({min(e32[WARM:]):.1f} .. {max(e32[WARM:]):.1f})   {log_bytes + 32 * 32 + 32:6.0f} B per episode ({32 * 32 + 32} B out)'
             f'   {tbs(log_bytes + 32 * 32 + 32, med(e32)):5.2f} TB/s',
             f'  k_blue_view, log on          {med(blue):7.1f} us  ({min(blue[WARM:]):.1f} .. {max(blue[WARM:]):.1f})   {VIEW_OUT} B out per episode; dispatch-to-dispatch spread {spread(blue):.1f} us',
             f'  k_red_view                   {med(red):7.1f} us  ({min(red[WARM:]):.1f} .. {max(red[WARM:]):.1f})',
             f'  k_blue_edges at 160 minus k_blue_view: {over:+.1f} us: ' + ('below k_blue_view' if over <= 0 else ('inside' if over <= spread(blue) else 'beyond') + ' the spread of k_blue_view in this job'),
             f'  k_blue_edges inside the loop (max_edges 160, behind a step): median of {len(in_loop)} dispatches {float(np.median(in_loop)):7.1f} us',
             f'# the log: {c["entries_per_episode"]:.1f} entries per episode counted with rep (an upper bound of the 12-byte records); events_valid {c["events_valid"]:.3f}',
             f'# distinct edges per episode: mean {c["edges_mean"]:.2f}, maximum {c["edges_max"]} over {c["edges_samples"]} (episode, step) samples; '
             f'on the rows the kernels were timed on: mean {c["edges_mean_last"]:.2f}, maximum {c["edges_max_last"]}',
             f'# the loop, log on ({c["step_kernel"]}): wall clock of {k} steps, enqueued without a host wait, one synchronise at the end; two runs each, alternating; the faster one.',
             '#   Episode steps/s (x 5 = agent-env steps/s); outside the profiler',
             f'  k_random_actions + cc4_step_device + cc4_blue_edges_device   {n * k / wl:12.4g} steps/s   {1e6 * wl / k:8.1f} us per step   (runs: {", ".join(f"{1e6 * x / k:.1f}" for x in c["loop_lists_s"])})',
             f'  the same without the lists                                   {n * k / wn:12.4g} steps/s   {1e6 * wn / k:8.1f} us per step   (runs: {", ".join(f"{1e6 * x / k:.1f}" for x in c["loop_no_lists_s"])})',
             f'  the lists add {1e6 * (wl - wn) / k:.1f} us per step = {100 * (wl - wn) / wn:.1f} %',
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
