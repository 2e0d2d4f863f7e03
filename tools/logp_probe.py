"""k_logp_fwd and k_logp_bwd timed on one GPU beside k_sample_actions, and a learner's minibatch of [logits -> logp, entropy of the stored actions
-> loss -> backward to the logits] through action_logp.evaluate_actions against the same minibatch written in PyTorch.  8192 and 32768 rows,
bfloat16 and float32 logits; the masks and the stored actions come from a counter-mode env 20 steps in (busy agents: -1).

  python tools/logp_probe.py run --json CALLS.json
        (a) per (rows, dtype) K minibatches each, enqueued with no host wait, one synchronise at the end, wall clock, twice each, alternating:
              fused   evaluate_actions(logits, mask, actions) -> (w0 logp + w1 entropy).sum().backward()
              torch   the same loss through torch_chain below (masked_fill, per-segment log_softmax, gather of the stored actions, entropy,
                      the -1 rule) and its autograd backward
        (b) --reps times per (rows, dtype): sample_actions on an env of that many episodes, evaluate_actions and its backward, for the profiler.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/logp_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler (no counters): the kernels' own durations per dispatch
  python tools/logp_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_logp.txt [--tests LOG]
        LOG: the output of pytest -s on the logp GPU tests, whose lines with the observed differences are quoted

Bytes the kernels must move per row, from the shapes: forward 570 logits in their dtype, 570 mask bytes, 5 x 4 action bytes in, 20 x 4 aux bytes
out; backward the same inputs, the aux and 10 x 4 g bytes in, 570 gradient values in the logits' dtype out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cage_challenge_4_amd._tensors import ELEM_BYTES      # noqa: E402
from cage_challenge_4_amd.action_sampling import SEGMENTS as SEG      # noqa: E402
from trace_util import kernel_times      # noqa: E402

ROWS, DTYPES, WARM = (8192, 32768), ('bfloat16', 'float32'), 3


def torch_chain(torch, logits, mask, actions):
    """logp and entropy of stored actions as a learner writes them in PyTorch: (logp [B, 5], entropy [B, 5]), zero where the action is -1."""
    x = logits.float().masked_fill(~mask, float('-inf'))
    logps, ents = [], []
    for b in range(5):
        lp = torch.log_softmax(x[:, SEG[b]:SEG[b + 1]], dim=1)
        logps.append(lp.gather(1, actions[:, b:b + 1].long().clamp(min=0)))
        ents.append(-(lp.exp() * lp.masked_fill(lp == float('-inf'), 0.0)).sum(dim=1, keepdim=True))
    on = actions >= 0
    return torch.cat(logps, 1).masked_fill(~on, 0.0), torch.cat(ents, 1).masked_fill(~on, 0.0)


def run(a):
    import torch
    from cage_challenge_4_amd import action_logp as AL
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    res = {'steps': a.steps, 'reps': a.reps, 'loop_s': {}, 'agree': {}, 'skipped_share': {}}
    envs, data = {}, {}
    for n in ROWS:
        env = envs[n] = CC4TorchVecEnv(n, steps=500, rng_mode=1, autoreset=True, strict=False)
        dev = env.device
        env.reset(seeds=1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        base = torch.randn((n, 570), generator=gen, device=dev) * 3
        for _ in range(20):                                      # 20 steps in, with sampled actions: busy agents exist
            env.step(env.sample_actions(base, seed=7)[0])
        out = env.sample_actions(base, seed=7)
        actions = out[0].clone()
        w = torch.rand((n, 5, 2), generator=gen, device=dev) * 2 - 1
        data[n] = (base, env.action_mask.clone(), actions, w, out)
        res['skipped_share'][str(n)] = float((actions < 0).float().mean())
    torch.cuda.synchronize(dev)

    def minibatch(kind, lg, mask, actions, w, k):
        for _ in range(k):
            lg.grad = None
            logp, ent = AL.evaluate_actions(lg, mask, actions) if kind == 'fused' else torch_chain(torch, lg, mask, actions)
            (w[..., 0] * logp + w[..., 1] * ent).sum().backward()
        torch.cuda.synchronize(dev)

    # ---- (a) the minibatches, twice each, alternating
    for n in ROWS:
        base, mask, actions, w, _out = data[n]
        for dt in DTYPES:
            lg = base.to(getattr(torch, dt)).clone().requires_grad_(True)
            walls = {'fused': [], 'torch': []}
            for _ in range(2):
                for kind in walls:
                    minibatch(kind, lg, mask, actions, w, 5)
                    t0 = time.perf_counter()
                    minibatch(kind, lg, mask, actions, w, a.steps)
                    walls[kind].append(time.perf_counter() - t0)
            res['loop_s'][f'{n} {dt}'] = walls
            minibatch('fused', lg, mask, actions, w, 1)
            gf, (lf, ef) = lg.grad.float().clone(), AL.evaluate_actions(lg.detach(), mask, actions)
            minibatch('torch', lg, mask, actions, w, 1)
            lt, et = torch_chain(torch, lg.detach(), mask, actions)
            res['agree'][f'{n} {dt}'] = {'logp': float((lf - lt).abs().max()), 'entropy': float((ef - et).abs().max()),
                                         'grad': float((gf - lg.grad.float()).abs().max())}
    # ---- (b) the kernels, for the profiler
    for n in ROWS:
        base, mask, actions, w, out = data[n]
        for dt in DTYPES:
            lg = base.to(getattr(torch, dt)).clone().requires_grad_(True)
            for _ in range(WARM + a.reps):
                envs[n].sample_actions(lg.detach(), seed=7, t=3, out=out)
                minibatch('fused', lg, mask, actions, w, 1)
    AL.check_errors(dev)
    for env in envs.values():
        env.check_errors()
        env.close()
    with open(a.json, 'w') as f:
        json.dump(res, f, indent=1)
    print(res)


def report(a):
    c = json.load(open(a.calls))
    k, per = c['steps'], WARM + c['reps']
    cases = [(n, dt) for n in ROWS for dt in DTYPES]
    times = {}
    for kern in ('k_logp_fwd', 'k_logp_bwd', 'k_sample_actions'):
        t = kernel_times(a.trace, kern)
        if len(t) < len(cases) * per:
            raise SystemExit(f'{len(t)} {kern} dispatches in the trace, expected at least {len(cases) * per}')
        times[kern] = t[-len(cases) * per:]              # part (b) is the end of the run: `per` dispatches per case, in the order of cases
    stat = lambda x: (float(np.median(x[WARM:])), float(np.min(x[WARM:])), float(np.max(x[WARM:])))      # noqa: E731
    lines = ['# tools/logp_probe.py: k_logp_fwd and k_logp_bwd on one GPU beside k_sample_actions; masks and stored actions of a counter-mode env 20 steps in; '
             + ', '.join(f'{100 * v:.1f} % of the (row, agent) pairs -1 at {n} rows' for n, v in c['skipped_share'].items()),
             f'# kernel us: rocprofv3 --kernel-trace --stats in a run of its own (no counters), median of {c["reps"]} dispatches on the same rows; (min .. max); '
             'bytes per row from the shapes']
    for j, (n, dt) in enumerate(cases):
        e = ELEM_BYTES[dt]
        for kern, b in (('k_logp_fwd', 570 * e + 570 + 20 + 80), ('k_logp_bwd', 2 * 570 * e + 570 + 20 + 80 + 40), ('k_sample_actions', None)):
            m, lo, hi = stat(times[kern][j * per:(j + 1) * per])
            tail = f'   {b:5d} B per row   {b * n / (m * 1e-6) / 1e12:5.2f} TB/s' if b else ''
            lines.append(f'  {n:6d} rows {dt:9s} {kern:17s} {m:7.1f} us  ({lo:.1f} .. {hi:.1f}){tail}')
    lines += [f'# the minibatch: wall clock of {k} x [forward, loss, backward to the logits], enqueued without a host wait, one synchronise at the end; two runs '
              'each, alternating; the faster one; outside the profiler',
              '#   fused: evaluate_actions (k_logp_fwd; backward: one stack of the two incoming gradients + k_logp_bwd); PyTorch: torch_chain and its autograd backward']
    us = lambda s: 1e6 * s / k                          # noqa: E731
    for n, dt in cases:
        w = c['loop_s'][f'{n} {dt}']
        f_, t_ = min(w['fused']), min(w['torch'])
        runs = lambda key: ', '.join(f'{us(x):.1f}' for x in w[key])      # noqa: E731
        g = c['agree'][f'{n} {dt}']
        lines.append(f'  {n:6d} rows {dt:9s} fused {us(f_):8.1f} us per minibatch (runs: {runs("fused")})   PyTorch {us(t_):8.1f} us (runs: {runs("torch")})   '
                     f'{t_ / f_:.2f}x   max |fused - PyTorch|: logp {g["logp"]:.3g}, entropy {g["entropy"]:.3g}, grad {g["grad"]:.3g}')
    if a.tests:
        lines.append('# float32 on the device against the float64 restatement, and against the sampler (the logp GPU tests, pytest -s): largest differences')
        lines += ['  ' + ln.strip().lstrip('.') for ln in open(a.tests) if 'max |' in ln or 'bit-equal' in ln]
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
    p.add_argument('--tests', default=None)
    a = ap.parse_args()
    (run if a.cmd == 'run' else report)(a)


if __name__ == '__main__':
    main()
