#!/usr/bin/env python
"""What a device-resident action plan costs (cc4_run_plan_device), against what it replaces -- 8192 episodes, counter mode, 500-step episodes with
autoreset, K = 20 and K = 500 steps per call:
  (a) cc4_run_random_steps                                   the headline path (actions drawn in the kernel; only the last step's outputs survive)
  (b) K x cc4_step_device over the rows of a plan            the only way to run a plan without this call
  (c) cc4_run_plan_device, rewards and dones recorded
  (d) the same with the packed observations of every step
Timed with HIP events on a stream of the probe's around the enqueued work of a REGION (several calls back to back, so that a region is a good
fraction of a second); every shape is warmed up first; the median region is reported with the extremes.  One process per library (CC4_LIB is read
when the package loads): with --parent-lib the parent commit's build runs (a) and (b) in the same job, the two processes alternating round by round.

  python tools/plan_probe.py [--parent-lib PATH --parent-commit HASH] [--rounds 3] [--out profiles/r10_plan_probe.txt]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS = 8192, 500
KS = (20, 500)
REGION_STEPS = 6000        # steps per timed region (~0.25-0.5 s)
REGIONS = 3                # regions per variant, K and round


def child(variants):
    sys.path.insert(0, ROOT)
    import torch
    from cage_challenge_4_amd import CC4VecEnv, _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    for s in ('cc4_run_plan_device', 'cc4_plan_kernel_for', 'cc4_unpack_rows_device'):     # (a library older than the plan call: bound without it)
        if not hasattr(raw, s):
            L.SIGNATURES.pop(s, None)
    env = CC4VecEnv(N, steps=STEPS, rng_mode=1, autoreset=True, strict=False)
    env.reset(seeds=0)
    lib, h, vp = env.lib, env._h, ctypes.c_void_p
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    sp = vp(stream.cuda_stream)
    has_plan = 'cc4_run_plan_device' in L.SIGNATURES
    out = []
    with torch.cuda.stream(stream):
        for K in KS:
            plan = torch.cat([torch.randint(0, 82, (K, N, 4), device=dev, dtype=torch.int32),
                              torch.randint(0, 242, (K, N, 1), device=dev, dtype=torch.int32)], 2).contiguous()
            rew = torch.empty((K, N), dtype=torch.float32, device=dev)
            done = torch.empty((K, N), dtype=torch.uint8, device=dev)
            packed = torch.empty((K, N, 148), dtype=torch.uint8, device=dev)
            calls = max(1, REGION_STEPS // K)

            def one(v, i):
                if v == 'a':
                    return lib.cc4_run_random_steps(h, ctypes.c_uint64(1), ctypes.c_uint32(i * K), K, None)
                if v == 'b':
                    rc = 0
                    for j in range(K):
                        rc = rc or lib.cc4_step_device(h, vp(plan.data_ptr() + j * N * 20), None)
                    return rc
                return lib.cc4_run_plan_device(h, K, vp(plan.data_ptr()), None, vp(rew.data_ptr()), vp(done.data_ptr()),
                                               vp(packed.data_ptr()) if v == 'd' else None)
            for v in variants:
                if v in 'cd' and not has_plan:
                    continue
                ms = []
                for r in range(REGIONS + 1):                    # region 0 warms the shape up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    env._chk(lib.cc4_stream_wait(h, sp), 'cc4_stream_wait')
                    for i in range(calls if r else max(1, calls // 4)):
                        env._chk(one(v, i), 'variant ' + v)
                    env._chk(lib.cc4_stream_signal(h, sp), 'cc4_stream_signal')
                    e1.record(stream)
                    stream.synchronize()
                    if r:
                        ms.append(e0.elapsed_time(e1))
                kern = ''
                if v == 'a':
                    kern = lib.cc4_run_kernel_for(h, K).decode()
                elif v == 'b':
                    kern = lib.cc4_step_kernel(h).decode()
                else:
                    kern = lib.cc4_plan_kernel_for(h, K).decode()
                out.append({'variant': v, 'K': K, 'kernel': kern, 'calls': calls, 'rates': [N * 5 * K * calls / (m * 1e-3) for m in ms]})
    env.close()
    print('PROBE ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--parent-commit', default='?')
    ap.add_argument('--commit', default='working tree')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child)
    libs = [('this', None, 'abcd')] + ([('parent', a.parent_lib, 'ab')] if a.parent_lib else [])
    got = {}
    for rnd in range(a.rounds):
        for name, path, variants in (libs if rnd % 2 == 0 else libs[::-1]):
            env = dict(os.environ, CC4_PERSIST_VERIFY_EVERY='0')      # (no sampled self-check inside a timed region)
            if path:
                env['CC4_LIB'] = path
            # (a fresh child process per library and round: no process keeps the GPU open beside it)
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', variants], env=env, capture_output=True, text=True, timeout=900)
            if pr.returncode != 0:
                sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
                raise SystemExit(f'the {name} library\'s probe process failed (exit code {pr.returncode})')
            for ln in pr.stdout.splitlines():
                if ln.startswith('PROBE '):
                    for row in json.loads(ln[6:]):
                        e = got.setdefault((name, row['variant'], row['K']), {'kernel': row['kernel'], 'calls': row['calls'], 'rates': []})
                        e['rates'] += row['rates']
    what = {'a': 'cc4_run_random_steps', 'b': 'K x cc4_step_device over a plan', 'c': 'cc4_run_plan_device, rewards + dones',
            'd': 'cc4_run_plan_device, + packed observations'}
    lines = [f'# plan probe: {N} episodes, counter mode, {STEPS}-step episodes with autoreset; M agent-env steps/s (5 blue agents x episodes x steps / HIP-event time of a',
             f'# region of ~{REGION_STEPS} steps); median of {a.rounds} rounds x {REGIONS} regions [min .. max]; libraries alternate round by round in one job.',
             f'# this library: {a.commit}; parent library: {a.parent_commit if a.parent_lib else "(not run)"}', '']
    for K in KS:
        lines.append(f'K = {K}')
        for name, _, variants in libs:
            for v in variants:
                e = got.get((name, v, K))
                if not e:
                    continue
                r = sorted(e['rates'])
                lines.append(f"  ({v}) {what[v]:44s} {name:6s} {e['kernel']:16s} {statistics.median(r) / 1e6:8.1f}  [{r[0] / 1e6:7.1f} .. {r[-1] / 1e6:7.1f}]  ({e['calls']} calls per region)")
        lines.append('')
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        open(a.out, 'w').write(txt + '\n')


if __name__ == '__main__':
    main()
