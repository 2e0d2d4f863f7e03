"""Episode copies on the device (cc4_copy_episodes_device) timed on one GPU: writes profiles/r09_episode_copy.txt.

Episodes of 500 steps, 250 steps in (run_random_steps), both RNG modes.  A clone needs destinations that are not sources, so the handle holds
2 x 8192 episodes: clones go from the first half to the second.  Timed on the stream of the caller (torch events around cc4_stream_wait,
the two copy kernels and cc4_stream_signal; median of --reps), for clones of 64 / 1024 / 8192 episodes and a save and a load of 8192.
Bytes moved per episode: the hot row, the packed outputs, and the live cold bytes, counted on a sample of destinations whose cold rows were
filled with two different patterns before a clone (a byte the copy wrote carries the source's value under both).  Baseline: torch's
device-to-device copy of the same number of episodes' full rows (hot + cold, equal bytes)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps, dev):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ts.append(e0.elapsed_time(e1) * 1000.0)
    return float(np.median(ts))


def live_cold_bytes(venv, src, dst):
    lib, h = venv.lib, venv._h
    nc = lib.cc4_cold_bytes(h)
    got = []
    for fill in (0xA5, 0x5A):
        pat = np.full(nc, fill, np.uint8)
        for d in dst:
            venv._chk(lib.cc4_set_cold(h, int(d), pat.ctypes.data_as(ctypes.c_void_p)), 'cc4_set_cold')
        venv._chk(lib.cc4_clone_episodes(h, len(src), np.asarray(src, np.int32).ctypes.data_as(ctypes.c_void_p),
                                         np.asarray(dst, np.int32).ctypes.data_as(ctypes.c_void_p), None), 'cc4_clone_episodes')
        got.append(np.stack([venv.get_cold(int(d)) for d in dst]))
    written = (got[0] != 0xA5) | (got[1] != 0x5A)
    return written.sum(axis=1)


def probe(rng_mode, n, steps, at, reps, dev):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    env = CC4TorchVecEnv(2 * n, steps=steps, rng_mode=rng_mode, autoreset=True, strict=False)
    venv, lib, h = env.venv, env.lib, env._h
    env.reset(seeds=1)
    venv.run_random_steps(7, 0, at, timed=False)
    venv.synchronize()
    hot, slot = lib.cc4_state_bytes(), env.snapshot_bytes
    cold = lib.cc4_cold_bytes(h)
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    bank = env.new_bank(n)
    rows = {}

    def copy(m, src_bank=None, dst_bank=None):
        src = torch.arange(m, dtype=torch.int32, device=dev)
        dst = src + (n if src_bank is None and dst_bank is None else 0)
        sb = ctypes.c_void_p(src_bank.data_ptr()) if src_bank is not None else None
        db = ctypes.c_void_p(dst_bank.data_ptr()) if dst_bank is not None else None

        def run():
            rc = lib.cc4_stream_wait(h, s) or lib.cc4_copy_episodes_device(h, m, sb, n, ctypes.c_void_p(src.data_ptr()), db, n,
                                                                              ctypes.c_void_p(dst.data_ptr()), None) or lib.cc4_stream_signal(h, s)
            assert rc == 0, lib.cc4_last_error(h)
        return run

    for m in (64, 1024, n):
        rows[f'clone {m}'] = (m, _time(copy(m), reps, dev))
    rows[f'save {n}'] = (n, _time(copy(n, dst_bank=bank), reps, dev))
    rows[f'load {n}'] = (n, _time(copy(n, src_bank=bank), reps, dev))
    f = ctypes.c_uint32()
    venv._chk(lib.cc4_copy_faults(h, ctypes.byref(f)), 'cc4_copy_faults')
    assert f.value == 0, f.value
    # live bytes of a sample of episodes (sources in the first half, destinations in the second)
    sample = np.arange(0, n, max(1, n // 64))[:64]
    lc = live_cold_bytes(venv, sample, sample + n)
    per_ep = hot + float(lc.mean()) + 2312 + 9          # hot row, live cold bytes, observation row (int32) + reward / done / err
    full = hot + cold
    base = {}
    for m in (64, 1024, n):
        a = torch.empty(m * full, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        base[m] = _time(lambda: b.copy_(a), reps, dev)
        del a, b
    torch.cuda.empty_cache()
    out = [f'rng_mode {rng_mode} ({"numpy stream" if rng_mode == 0 else "counter"}): {2 * n} episodes of {steps} steps, {at} steps in; '
           f'hot row {hot} B, cold row {cold} B, snapshot slot {slot} B',
           f'  live cold bytes per episode (sample of {len(lc)}): mean {lc.mean():.0f}, min {lc.min()}, max {lc.max()};  bytes moved per episode '
           f'(hot + live cold + outputs) {per_ep:.0f} = {full / per_ep:.1f}x fewer than the full rows ({full} B)',
           f'  {"call":12s} {"episodes":>8s} {"us":>9s} {"us/ep":>7s} {"TB/s eff":>8s} | full-row torch copy: {"us":>9s} {"TB/s":>6s} {"speed-up":>8s}']
    for k, (m, us) in rows.items():
        bus = base.get(m, base[n])
        eff = 2 * per_ep * m / (us * 1e-6) / 1e12
        out.append(f'  {k:12s} {m:8d} {us:9.1f} {us / m:7.3f} {eff:8.2f} | {"":19s} {bus:9.1f} {2 * full * m / (bus * 1e-6) / 1e12:6.2f} {bus / us:7.1f}x')
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--at', type=int, default=250)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09_episode_copy.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = [f'# tools/episode_copy_probe.py: device episode copies (cc4_copy_episodes_device) on one GPU ({torch.cuda.get_device_name(dev)}, '
             f'{torch.cuda.get_device_properties(dev).multi_processor_count} CUs)',
             '# on-stream time (torch events around cc4_stream_wait + k_copy_claim + k_copy_episodes + cc4_stream_signal, median of '
             f'{a.reps}); TB/s eff = 2 x bytes moved / time (read + write); baseline: torch copy of the same episodes\' full rows']
    for mode in (1, 0):
        lines += probe(mode, a.n, a.steps, a.at, a.reps, dev)
    txt = '\n'.join(lines) + '\n'
    print(txt, end='')
    with open(a.out, 'w') as f:
        f.write(txt)


if __name__ == '__main__':
    main()
