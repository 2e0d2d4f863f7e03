"""cc4_state_features_device (k_state_features) timed on one GPU: the whole batch, a 1/8 subset of ids and a read from a snapshot bank, at 1024 and
8192 episodes (counter mode, 500-step episodes with autoreset, 100 steps in).

  python tools/state_features_probe.py run --json CALLS.json
        the call on the caller's stream (torch events around cc4_stream_wait + the kernel + cc4_stream_signal; median of --reps)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/state_features_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler: the kernel's own duration per dispatch
  python tools/state_features_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_state_features.txt
        both together: bytes the kernel must move (from the shapes) / kernel time, and that as a share of 8 TB/s

Bytes per episode, from the shapes: the fields of the agent part the kernel reads (READ_FIELDS), 32 B per existing host (the second half of its
HostDyn row), and the 137 x 16 + 32 x 4 output bytes."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 3
HBM_PEAK = 8.0e12
# csrc/cc4_state.h: what feat_sess_item / feat_green_item / feat_host_row / feat_global_word (csrc/cc4_features.h) read in front of the host table
READ_FIELDS = {'step_count, steps, phase, err, done, n_green': 4 * 4 + 2, 'blocks': 2 * 9, 'exists': 20, 'spool_used': 24, 'spool (192 records)': 192 * 8,
               'green_host': 80, 'red[6]: live_hosts, as_ip, the 32-byte header': 6 * (20 + 20 + 32), 'blue[5]: sus_hosts, queue': 5 * (20 + 8), 'hev': 137}
OUT_BYTES = 137 * 16 + 32 * 4


def run(a):
    import torch
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    res = {'device': torch.cuda.get_device_name(dev), 'cus': torch.cuda.get_device_properties(dev).multi_processor_count, 'reps': a.reps, 'configs': []}
    for n in (1024, 8192):
        env = CC4TorchVecEnv(n, steps=500, rng_mode=1, autoreset=True, strict=False)
        env.reset(seeds=1)
        env.venv.run_random_steps(7, 0, 100, timed=False)
        env.venv.synchronize()
        ids = torch.randperm(n, device=dev)[:n // 8].contiguous()
        bank = env.new_bank(n)
        every = torch.arange(n, device=dev)
        env.save_episodes(every, bank, every)
        for name, kw, m in (('all episodes', {}, n), ('1/8 of the ids, shuffled', {'ids': ids}, n // 8), ('bank, all slots', {'bank': bank}, n)):
            out = (torch.empty((m, 137, 16), dtype=torch.uint8, device=dev), torch.empty((m, 32), dtype=torch.int32, device=dev))
            ts = []
            for i in range(WARM + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                env.state_features(out=out, **kw)
                e1.record()
                torch.cuda.synchronize(dev)
                if i >= WARM:
                    ts.append(e0.elapsed_time(e1) * 1000.0)
            hosts = float(out[0][:, :, 0].sum().item()) / m
            res['configs'].append({'n': n, 'what': name, 'entries': m, 'call_us': float(np.median(ts)), 'hosts_per_episode': hosts})
        env.check_errors()
        del bank
        env.close()
        torch.cuda.empty_cache()
    with open(a.json, 'w') as f:
        json.dump(res, f, indent=1)
    for c in res['configs']:
        print(c)


def kernel_times(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True))
    if len(files) != 1:
        raise SystemExit(f'expected one *kernel_trace.csv under {trace_dir}, found {files}')
    rows = [r for r in csv.DictReader(open(files[0])) if 'k_state_features' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    return [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1000.0 for r in rows]


def report(a):
    calls = json.load(open(a.calls))
    us = kernel_times(a.trace)
    per = WARM + calls['reps']
    if len(us) != per * len(calls['configs']):
        raise SystemExit(f'{len(us)} k_state_features dispatches in the trace, expected {per} x {len(calls["configs"])}')
    fixed = sum(READ_FIELDS.values())
    lines = [f'# tools/state_features_probe.py: cc4_state_features_device (k_state_features) on one GPU ({calls["device"]}, {calls["cus"]} CUs); counter mode, '
             '500-step episodes with autoreset, 100 steps in',
             f'# call us: torch events on the caller\'s stream around cc4_stream_wait + k_state_features + cc4_stream_signal, median of {calls["reps"]};  kernel us: '
             'rocprofv3 --kernel-trace --stats in a run of its own, median of the same dispatches',
             f'# bytes per episode from the shapes: {fixed} B of the agent part (' + ', '.join(f'{k} {v}' for k, v in READ_FIELDS.items()) + '), 32 B per existing host, '
             f'{OUT_BYTES} B of output;  share = of {HBM_PEAK / 1e12:.0f} TB/s',
             f'  {"episodes":>8s}  {"what":26s} {"entries":>7s} {"hosts/ep":>8s} {"B/entry":>7s} {"call us":>8s} {"kernel us":>9s} {"TB/s":>6s} {"share":>6s}']
    for i, c in enumerate(calls['configs']):
        k = float(np.median(us[i * per + WARM:(i + 1) * per]))
        b = fixed + 32.0 * c['hosts_per_episode'] + OUT_BYTES
        rate = b * c['entries'] / (k * 1e-6)
        lines.append(f'  {c["n"]:8d}  {c["what"]:26s} {c["entries"]:7d} {c["hosts_per_episode"]:8.1f} {b:7.0f} {c["call_us"]:8.1f} {k:9.1f} {rate / 1e12:6.2f} {100 * rate / HBM_PEAK:5.1f}%')
    lines += ['# for scale, figures the project already has: k_policy_outputs moves its rows at 4.0 TB/s (profiles/r07_torch_env.txt), and one step of 8192 episodes',
              '# takes 30 us (profiles/r08_bench_full.json: 1382 M agent-env steps/s); the step path is not touched by this call.']
    txt = '\n'.join(lines) + '\n'
    print(txt, end='')
    with open(a.out, 'w') as f:
        f.write(txt)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--reps', type=int, default=20)
    r.add_argument('--json', required=True)
    p = sub.add_parser('report')
    p.add_argument('--calls', required=True)
    p.add_argument('--trace', required=True)
    p.add_argument('--out', required=True)
    a = ap.parse_args()
    (run if a.cmd == 'run' else report)(a)


if __name__ == '__main__':
    main()
