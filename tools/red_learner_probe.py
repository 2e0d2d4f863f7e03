"""A red learner's loop timed on one GPU: cc4_step_red_device + cc4_red_view_device per step against the only way to submit red actions without
them, cc4_step_ex from host arrays; and k_red_view beside k_state_features.  8192 episodes, counter mode, 500-step episodes with autoreset, 100
steps in.

  python tools/red_learner_probe.py run --json CALLS.json
        (a) K steps of [stand-in blue policy on the device, cc4_step_red_device, cc4_red_view_device], enqueued with no host wait, one
            synchronise at the end -- and K steps of cc4_step_ex with the same red records as host arrays (every call ends in
            a host wait; the red agents' knowledge is not fetched at all on that path: cc4_get_true_state serves one episode per call).  Both
            start from the same state and submit the same red records (explicit session ids: the host path has no SID_AUTO) beside random blue
            indices -- drawn on the device on one side, a host array on the other; wall clock.
        (b) --reps calls each of cc4_red_view_device and cc4_state_features_device on the same rows, for the profiler to time.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/red_learner_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler: the kernels' own durations per dispatch
  python tools/red_learner_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_red_learner.txt

Bytes k_red_view must move per episode, from the shapes: the six agents' part of the row it reads (READ_FIELDS), the session records their lists
name, and the 6 x 137 x 8 + 6 x 16 x 4 output bytes."""
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
# csrc/cc4_state.h: what rv_sess_item / rv_obs_item / rv_host_row / rv_scalar (csrc/cc4_red_view.h) read of each of the six agents
READ_FIELDS = {'sord': 64, 'as_ip, as_hn': 40, 'obs': 64, 'the 32-byte header': 32}
OUT_BYTES = 6 * 137 * 8 + 6 * 16 * 4
FEAT_BYTES = 7600           # profiles/r13_state_features.txt: k_state_features, bytes per episode


class Dev:
    def __init__(self, hip, nbytes):
        self.hip, self.p = hip, VP()
        assert hip.hipMalloc(ctypes.byref(self.p), nbytes) == 0

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        assert self.hip.hipMemcpy(self.p, arr.ctypes.data_as(VP), arr.nbytes, 1) == 0

    def down(self, dtype, shape):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(VP), self.p, out.nbytes, 2) == 0
        return out


def red_arrays(rng):
    """The same red actions for both paths: words [N, 6, 4] for the device, cc4_agent_action records [N, 6] for the host.  Every type -1..10, hosts
    and subnets in range, session id 0 (an explicit id: the host path has no way to SID_AUTO)."""
    from cage_challenge_4_amd import _lib as L
    w = np.zeros((N, 6, 4), np.int32)
    w[..., 0] = rng.integers(-1, 11, (N, 6))
    w[..., 1] = rng.integers(0, 137, (N, 6))
    w[..., 2] = np.where(w[..., 0] == 0, rng.integers(0, 9, (N, 6)), np.where(w[..., 0] == 8, w[..., 1], 0))
    rec = np.zeros((N, 6), dtype=L.AGENT_ACTION_DTYPE)
    rec['type'], rec['host'], rec['arg'] = w[..., 0], w[..., 1], w[..., 2]
    return w, rec


def run(a):
    from cage_challenge_4_amd import CC4VecEnv
    from cage_challenge_4_amd.vec_env import _hip
    hip = _hip()
    rng = np.random.default_rng(11)
    words, recs = red_arrays(rng)
    res = {'n': N, 'steps': a.steps, 'reps': a.reps}

    def fresh():
        env = CC4VecEnv(N, steps=500, rng_mode=1, autoreset=True, strict=False)
        env.reset(seeds=1)
        env.run_random_steps(7, 0, 100, timed=False)
        env.synchronize()
        return env

    # ---- (a) the device path
    env = fresh()
    res['step_kernel'] = env.step_kernel
    lib, h = env.lib, env._h
    acts = VP()
    env._chk(lib.cc4_actions_device(h, ctypes.byref(acts)), 'cc4_actions_device')
    d_red, d_view = Dev(hip, words.nbytes), Dev(hip, N * OUT_BYTES)
    d_feat = Dev(hip, N * (137 * 16 + 32 * 4))
    d_red.up(words)
    p_scal, p_glob = VP(d_view.p.value + N * 6 * 137 * 8), VP(d_feat.p.value + N * 137 * 16)

    def device_steps(t0, k):
        rc = 0
        for t in range(t0, t0 + k):
            rc = rc or lib.cc4_random_actions_device(h, 7, t) or lib.cc4_step_red_device(h, acts, None, d_red.p)
            rc = rc or lib.cc4_red_view_device(h, None, 0, None, N, d_view.p, p_scal)
        env._chk(rc, 'device loop')
        env.synchronize()

    device_steps(100, 10)
    t0 = time.perf_counter()
    device_steps(110, a.steps)
    res['device_s'] = time.perf_counter() - t0
    # the same without the view: what the view adds to a step
    t0 = time.perf_counter()
    rc = 0
    for t in range(110 + a.steps, 110 + 2 * a.steps):
        rc = rc or lib.cc4_random_actions_device(h, 7, t) or lib.cc4_step_red_device(h, acts, None, d_red.p)
    env._chk(rc, 'device loop')
    env.synchronize()
    res['device_no_view_s'] = time.perf_counter() - t0
    # ---- (b) the two feature kernels on the same rows
    for _ in range(WARM + a.reps):
        env._chk(lib.cc4_red_view_device(h, None, 0, None, N, d_view.p, p_scal), 'cc4_red_view_device')
        env._chk(lib.cc4_state_features_device(h, None, 0, None, N, d_feat.p, p_glob), 'cc4_state_features_device')
        env.synchronize()
    view = d_view.down(np.uint8, (N, 6, 137, 8))
    res['sessions_per_episode'] = float(view[..., 3].sum()) / N
    res['nonzero_rows_per_episode'] = float(view.any(axis=3).sum()) / N
    faults = ctypes.c_uint32(0)
    env._chk(lib.cc4_copy_faults(h, ctypes.byref(faults)), 'cc4_copy_faults')
    res['faults'] = faults.value
    env.close()

    # ---- (a) the host path: the same records, and random blue indices, as host arrays
    env = fresh()
    blue = np.ascontiguousarray(np.random.default_rng(12).integers(-1, 83, (N, 5)), np.int32)
    for _ in range(10):
        env._chk(env.lib.cc4_step_ex(env._h, blue.ctypes.data_as(VP), None, recs.ctypes.data_as(VP), None), 'cc4_step_ex')
    t0 = time.perf_counter()
    for _ in range(a.steps):
        env._chk(env.lib.cc4_step_ex(env._h, blue.ctypes.data_as(VP), None, recs.ctypes.data_as(VP), None), 'cc4_step_ex')
    res['host_s'] = time.perf_counter() - t0
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
    n, k = c['n'], c['steps']
    view, feat, submit = (kernel_times(a.trace, s) for s in ('k_red_view', 'k_state_features', 'k_red_submit'))
    per = WARM + c['reps']
    if len(feat) != per or len(view) < per:
        raise SystemExit(f'{len(view)} k_red_view and {len(feat)} k_state_features dispatches in the trace, expected at least {per} and {per}')
    v, f, s = float(np.median(view[-per:][WARM:])), float(np.median(feat[WARM:])), float(np.median(submit))
    b = 6 * sum(READ_FIELDS.values()) + 8.0 * c['sessions_per_episode'] + OUT_BYTES
    dev, nov, host = n * k / c['device_s'], n * k / c['device_no_view_s'], n * k / c['host_s']
    lines = [f'# tools/red_learner_probe.py: a red learner\'s loop on one GPU; {n} episodes, counter mode ({c["step_kernel"]}, full build), 500-step episodes with autoreset, 100 steps in',
             f'# (a) wall clock of {k} steps, one synchronise at the end of the device loops; the host path waits in every call.  Episode steps/s (x 5 = agent-env steps/s)',
             '#     not like for like in two respects: the device loop draws new blue indices every step (k_random_actions), the host loop submits one constant blue array;',
             '#     and both submit session id 0 in every red record, so most red actions fail the validity check.  The ratio is the per-call upload and host wait.',
             f'  device: k_random_actions + cc4_step_red_device + cc4_red_view_device   {dev:12.4g} steps/s   {1e6 * c["device_s"] / k:8.1f} us per step',
             f'  device: the same without the view                                   {nov:12.4g} steps/s   {1e6 * c["device_no_view_s"] / k:8.1f} us per step',
             f'  host:   cc4_step_ex from host arrays (no red knowledge fetched)      {host:12.4g} steps/s   {1e6 * c["host_s"] / k:8.1f} us per step',
             f'  device / host = {dev / host:.2f}',
             f'# (b) kernel us: rocprofv3 --kernel-trace --stats in a run of its own, median of {c["reps"]} dispatches on the same rows',
             f'  k_red_view        {v:7.1f} us   {b:6.0f} B per episode from the shapes ({c["sessions_per_episode"]:.1f} sessions, {c["nonzero_rows_per_episode"]:.1f} non-zero rows of 822)   {b * n / (v * 1e-6) / 1e12:5.2f} TB/s',
             f'  k_state_features  {f:7.1f} us   {FEAT_BYTES:6d} B per episode (profiles/r13_state_features.txt: 24.6 us)   {FEAT_BYTES * n / (f * 1e-6) / 1e12:5.2f} TB/s',
             f'  k_red_submit      {s:7.1f} us   (median of {len(submit)} dispatches inside the loops)',
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
