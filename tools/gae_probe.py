"""k_gae timed on one GPU against the same definition as a learner writes it in PyTorch (a reverse loop over T with torch.where), on the same
tensors in the same job; the builds of the kernel (wavefronts per workgroup, rows loaded ahead) side by side.

  python tools/gae_probe.py --out profiles/rNN_gae.txt [--json RAW.json] [--lib NAME=PATH ...] [--trace DIR]
        T in {20, 128, 500} x N in {1024, 8192}, A = 5, bfloat16 values, actions given, the autoreset layout with bootstrap.
        kernel   device events around K back-to-back calls of cc4_gae_device on the current stream, the calls rotating over SETS copies of the
                 tensors (so that a large shape is not served from the last call's lines in the 256 MB last-level cache; SETS is capped, so the
                 small shapes are), five rounds alternating over the builds, the median round.  The first --lib-less build is the package's own
                 library; --lib NAME=PATH adds another build of libcc4.so (make EXTRA="-DCC4_GAE_WAVES=w -DCC4_GAE_ROWS=r" OUT=PATH), loaded
                 beside it: the call is a pure function and needs no handle
        PyTorch  wall clock around the loop and a synchronise, three runs, the fastest; float32 values (the upcast is outside the timed part)
        bytes    per call from the shapes, over the kernel time, as a fraction of 8 TB/s
        --trace  a directory written by `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gae_probe.py --trace-run`: the
                 kernel's own duration per dispatch (package build only), quoted beside the event times
A run needs a GPU; without one it fails."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cage_challenge_4_amd._tensors import ELEM_BYTES      # noqa: E402
from trace_util import kernel_times      # noqa: E402

TS, NS, A = (20, 128, 500), (1024, 8192), 5
GAMMA, LAM, FLAGS = 0.99, 0.95, 3
ROUNDS, WARM, TRACE_REPS = 5, 3, 10
PEAK = 8.0e12
VP = ctypes.c_void_p


def bytes_per_call(T, N, a=A, elt=ELEM_BYTES['bfloat16']):
    """What one call must move: values, actions in; adv, ret, weight out; rewards and dones per episode; last and done0 once."""
    return T * N * a * (elt + 4 + 4 + 4 + 1) + T * N * (4 + 1) + N * a * elt + N


def torch_loop(torch, rewards, values, last, dones, done0, actions, gamma, lam, bootstrap=True):
    """The autoreset layout as a learner writes it in PyTorch: (adv, ret, weight)."""
    T = values.shape[0]
    skip = torch.cat((done0[None], dones[:-1]), dim=0)[..., None]
    d = dones[..., None]
    r = rewards[..., None]
    adv = torch.empty_like(values)
    zero = torch.zeros_like(last)
    a_next, v_next = zero, last
    gl = gamma * lam
    for t in range(T - 1, -1, -1):
        vb = torch.where(d[t], v_next if bootstrap else zero, v_next)
        an = torch.where(d[t], zero, a_next)
        delta = r[t] + gamma * vb - values[t]
        a_next = torch.where(skip[t], zero, delta + gl * an)
        adv[t] = a_next
        v_next = values[t]
    ret = torch.where(skip, values, adv + values)
    return adv, ret, ~skip & (actions != -1)


def make_set(torch, gen, dev, T, N):
    dones = torch.zeros((T, N), dtype=torch.bool, device=dev)
    dones[torch.randint(0, T, (N,), generator=gen, device=dev), torch.arange(N, device=dev)] = True      # one done per episode somewhere
    done0 = torch.zeros(N, dtype=torch.bool, device=dev)
    skip = torch.cat((done0[None], dones[:-1]), dim=0)
    rewards = -torch.randint(0, 21, (T, N), generator=gen, device=dev).float()
    rewards[skip] = 0.0
    values = (torch.randn((T, N, A), generator=gen, device=dev) * 50).to(torch.bfloat16)
    last = (torch.randn((N, A), generator=gen, device=dev) * 50).to(torch.bfloat16)
    actions = torch.randint(-1, 50, (T, N, A), generator=gen, device=dev, dtype=torch.int32)
    out = (torch.empty((T, N, A), device=dev), torch.empty((T, N, A), device=dev), torch.empty((T, N, A), dtype=torch.bool, device=dev))
    return dict(rewards=rewards, values=values, last=last, dones=dones, done0=done0, actions=actions, out=out)


def load_libs(specs):
    from cage_challenge_4_amd import _lib as L
    libs = [('package', L.load())]
    for spec in specs:
        name, path = spec.split('=', 1)
        lib = ctypes.CDLL(os.path.abspath(path))
        for sym in ('cc4_gae_device', 'cc4_gae_rows'):
            getattr(lib, sym).restype, getattr(lib, sym).argtypes = L.SIGNATURES[sym]
        libs.append((name, lib))
    return libs


def call(torch, lib, s, T, N, stream):
    p = lambda x: VP(x.data_ptr())      # noqa: E731
    rc = lib.cc4_gae_device(VP(stream), p(s['rewards']), 1, p(s['values']), 2, p(s['last']), p(s['dones']), p(s['done0']), p(s['actions']), T, N, A,
                            GAMMA, LAM, FLAGS, p(s['out'][0]), p(s['out'][1]), p(s['out'][2]))
    if rc != 0:
        raise SystemExit(f'cc4_gae_device failed (rc={rc})')


def run(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/gae_probe.py needs a GPU')
    dev = torch.device('cuda', 0)
    libs = load_libs(a.lib)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    res = {'libs': {name: int(lib.cc4_gae_rows()) for name, lib in libs}, 'cases': {}}
    stream = torch.cuda.current_stream(dev).cuda_stream
    for N in NS:
        for T in TS:
            nb = bytes_per_call(T, N)
            nsets = int(min(8, max(1, -(-600_000_000 // nb))))
            sets = [make_set(torch, gen, dev, T, N) for _ in range(nsets)]
            k = max(2 * nsets, min(200, int(40e-3 / (nb / 4e12 + 5e-6))))          # calls per timed window: about 40 ms of work
            k -= k % nsets
            if a.trace_run:
                for j in range(WARM + TRACE_REPS):
                    call(torch, libs[0][1], sets[j % nsets], T, N, stream)
                torch.cuda.synchronize(dev)
                continue
            times = {name: [] for name, _ in libs}
            for name, lib in libs:
                for j in range(WARM * nsets):
                    call(torch, lib, sets[j % nsets], T, N, stream)
            torch.cuda.synchronize(dev)
            for _ in range(ROUNDS):
                for name, lib in libs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for j in range(k):
                        call(torch, lib, sets[j % nsets], T, N, stream)
                    e1.record()
                    e1.synchronize()
                    times[name].append(1e3 * e0.elapsed_time(e1) / k)
            # the PyTorch loop on set 0, float32 values; and what the two disagree by
            s = sets[0]
            v32, l32 = s['values'].float(), s['last'].float()
            walls = []
            for _ in range(4):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                ref = torch_loop(torch, s['rewards'], v32, l32, s['dones'], s['done0'], s['actions'], GAMMA, LAM)
                torch.cuda.synchronize(dev)
                walls.append(1e6 * (time.perf_counter() - t0))
            call(torch, libs[0][1], s, T, N, stream)
            torch.cuda.synchronize(dev)
            diff = [float((s['out'][0] - ref[0]).abs().max()), float((s['out'][1] - ref[1]).abs().max()), int((s['out'][2] != ref[2]).sum())]
            res['cases'][f'{T} {N}'] = {'bytes': nb, 'sets': nsets, 'calls': k, 'us': times, 'torch_us': walls[1:], 'diff': diff}
            print(T, N, {n_: round(float(np.median(v)), 2) for n_, v in times.items()}, 'torch', round(min(walls[1:]), 1), diff, flush=True)
            del sets, ref, v32, l32
            torch.cuda.empty_cache()
    if a.trace_run:
        return
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    report(res, a)


def report(res, a):
    names = list(res['libs'])
    lines = ['# tools/gae_probe.py: cc4_gae_device (k_gae) on one MI355X against the same definition as a PyTorch loop (reverse over T, torch.where); A = 5 heads, '
             'bfloat16 values, int32 actions given, autoreset layout with bootstrap, gamma 0.99, lam 0.95',
             f'# kernel: device events around K back-to-back calls rotating over SETS copies of the tensors, {ROUNDS} rounds alternating over the builds: '
             'median (min .. max) us per call.  PyTorch: wall clock of the loop + one synchronise, fastest of three, float32 values',
             '# bytes per call from the shapes (values, actions in; adv, ret, weight out; rewards, dones per episode); fraction of 8 TB/s at the median',
             '# builds: ' + ', '.join(f'{n} (GAE_ROWS {r})' for n, r in res['libs'].items())]
    trace = kernel_times(a.trace, 'k_gae') if a.trace else None
    per = WARM + TRACE_REPS
    for j, (key, c) in enumerate(res['cases'].items()):
        T, N = (int(x) for x in key.split())
        lines.append(f'  T {T:3d} N {N:4d}   {c["bytes"] / 1e6:8.2f} MB per call, SETS {c["sets"]}, K {c["calls"]}   PyTorch loop {min(c["torch_us"]):9.1f} us '
                     f'(runs: {", ".join(f"{x:.0f}" for x in c["torch_us"])})   max |kernel - PyTorch|: adv {c["diff"][0]:.3g}, ret {c["diff"][1]:.3g}, '
                     f'weights that differ {c["diff"][2]}')
        for n in names:
            t = c['us'][n]
            m = float(np.median(t))
            lines.append(f'      {n:14s} {m:8.2f} us  ({min(t):.2f} .. {max(t):.2f})   {c["bytes"] / (m * 1e-6) / 1e12:5.2f} TB/s = {c["bytes"] / (m * 1e-6) / PEAK:5.1%} of 8 TB/s'
                         f'   PyTorch / kernel {min(c["torch_us"]) / m:7.1f}x')
        if trace:
            t = trace[j * per + WARM:(j + 1) * per]
            lines.append(f'      package, rocprofv3 --kernel-trace in a run of its own, {len(t)} dispatches: median {float(np.median(t)):.2f} us ({min(t):.2f} .. {max(t):.2f})')
    txt = '\n'.join(lines) + '\n'
    print(txt, end='')
    with open(a.out, 'w') as f:
        f.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--json', default=None)
    ap.add_argument('--lib', action='append', default=[], help='NAME=PATH of another build of libcc4.so')
    ap.add_argument('--trace', default=None)
    ap.add_argument('--trace-run', action='store_true', help='only the dispatches for the profiler: the package build, WARM + TRACE_REPS per shape')
    ap.add_argument('--from-json', default=None, help='write the report from a saved run (with --trace)')
    a = ap.parse_args()
    if a.from_json:
        report(json.load(open(a.from_json)), a)
    else:
        if not a.trace_run and not a.out:
            ap.error('--out is required')
        run(a)


if __name__ == '__main__':
    main()
