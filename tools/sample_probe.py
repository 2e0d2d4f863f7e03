"""k_sample_actions timed on one GPU beside k_reward_terms and k_blue_view, and a learner's loop of [fixed bf16 logits -> sample_actions -> step]
against the same loop with the sampling written in PyTorch.  8192 episodes, counter mode, 500-step episodes with autoreset, 100 steps in.

  python tools/sample_probe.py run --json CALLS.json
        (a) K steps each, enqueued with no host wait, one synchronise at the end, wall clock, twice each, alternating:
              fused     env.sample_actions(logits) + env.step(actions)
              torch     the same sampling as a chain of PyTorch operations (torch_chain below: masked_fill, per-segment log_softmax, Gumbel
                        arg-max, gather, entropy, and the busy rule from blue_view()) + env.step(actions)
              torch_nb  that chain without the busy rule (no blue_view call): what a learner that ignores busy agents pays
              step      env.step(fixed actions) alone
        (b) --reps calls each of sample_actions with float32 / bfloat16 / float16 logits and without logits, reward_terms() and blue_view() on
            the same rows, for the profiler to time.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sample_probe.py run --json TRACED.json
        the same sequence in a run of its own under the profiler (no counters): the kernels' own durations per dispatch
  python tools/sample_probe.py report --calls CALLS.json --trace DIR --out profiles/rNN_sample.txt [--tests LOG]
        LOG: the output of pytest -s on tests/test_sample_device.py, whose lines with the observed float differences are quoted

Bytes k_sample_actions must move per entry, from the shapes: 570 logits in their dtype, of the hot row the 20 bytes of exists and the five busy
bytes, and 5 x 4 + 10 x 4 output bytes."""
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

N, WARM = 8192, 3
VARIANTS = ('float32', 'bfloat16', 'float16', 'none')
ROW_READ, OUT_BYTES = 20 + 5, 5 * 4 + 10 * 4


def torch_chain(torch, env, logits, views, busy_rule=True):
    """The sampling of sample_actions() as a learner writes it in PyTorch: (actions [N, 5] int32, logp [N, 5], entropy [N, 5])."""
    x = logits.float().masked_fill(~env.action_mask, float('-inf'))
    u = torch.rand_like(x).clamp_(2.0 ** -24, 1.0 - 2.0 ** -24)
    z = x - torch.log(-torch.log(u))
    acts, logps, ents = [], [], []
    for b in range(5):
        lp = torch.log_softmax(x[:, SEG[b]:SEG[b + 1]], dim=1)
        a = z[:, SEG[b]:SEG[b + 1]].argmax(dim=1, keepdim=True)
        acts.append(a)
        logps.append(lp.gather(1, a))
        ents.append(-(lp.exp() * lp.masked_fill(lp == float('-inf'), 0.0)).sum(dim=1, keepdim=True))
    act, logp, ent = torch.cat(acts, 1).to(torch.int32), torch.cat(logps, 1), torch.cat(ents, 1)
    if busy_rule:
        env.blue_view(out=views)
        busy = views[1][..., 0] != 0
        act, logp, ent = torch.where(busy, -1, act), logp.masked_fill(busy, 0.0), ent.masked_fill(busy, 0.0)
    return act, logp, ent


def run(a):
    import torch
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    res = {'n': N, 'steps': a.steps, 'reps': a.reps}
    env = CC4TorchVecEnv(N, steps=500, rng_mode=1, autoreset=True, strict=False)
    dev = env.device
    env.reset(seeds=1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    base = torch.randn((N, 570), generator=gen, device=dev) * 3
    logits = {'float32': base, 'bfloat16': base.to(torch.bfloat16), 'float16': base.to(torch.float16), 'none': None}
    bf = logits['bfloat16']
    for t in range(100):                                        # 100 steps in, with sampled actions: busy agents exist
        env.step(env.sample_actions(bf, seed=7)[0])
    torch.cuda.synchronize(dev)
    res['step_kernel'] = env.venv.step_kernel
    views = env.blue_view()
    res['busy_share'] = float((views[1][..., 0] != 0).float().mean())
    fixed = env.sample_actions(bf, seed=7)[0].clone()
    out = env.sample_actions(bf, seed=7)

    def loop(kind, k):
        for _ in range(k):
            if kind == 'fused':
                act = env.sample_actions(bf, seed=7, out=out)[0]
            elif kind == 'torch':
                act = torch_chain(torch, env, bf, views)[0]
            elif kind == 'torch_nb':
                act = torch_chain(torch, env, bf, views, busy_rule=False)[0]
            else:
                act = fixed
            env.step(act)
        torch.cuda.synchronize(dev)

    # ---- (a) the loops, twice each, alternating
    walls = {k: [] for k in ('fused', 'torch', 'torch_nb', 'step')}
    for _ in range(2):
        for kind in walls:
            loop(kind, 10)
            t0 = time.perf_counter()
            loop(kind, a.steps)
            walls[kind].append(time.perf_counter() - t0)
    res['loop_s'] = walls
    # the two samplers agree on what they draw from: mean logp and entropy over the batch (different noise, the same distribution)
    f_act, f_st = env.sample_actions(bf, seed=7, t=12345)
    t_act, t_lp, t_en = torch_chain(torch, env, bf, views)
    live = f_act >= 0
    res['agree'] = {'busy_equal': bool(torch.equal(f_act < 0, t_act < 0)), 'entropy_max_diff': float((f_st[..., 1] - t_en).abs().max()),
                    'mean_logp_fused': float(f_st[..., 0][live].mean()), 'mean_logp_torch': float(t_lp[live].mean())}
    # ---- (b) the kernels on the same rows
    rt = env.reward_terms()
    for _ in range(WARM + a.reps):
        for name in VARIANTS:
            env.sample_actions(logits[name], seed=7, t=3, out=out)
        env.reward_terms(out=rt)
        env.blue_view(out=views)
        torch.cuda.synchronize(dev)
    env.check_errors()
    env.close()
    with open(a.json, 'w') as f:
        json.dump(res, f, indent=1)
    print(res)


def report(a):
    c = json.load(open(a.calls))
    n, k, per = c['n'], c['steps'], WARM + c['reps']
    sa, rt, blue = (kernel_times(a.trace, s) for s in ('k_sample_actions', 'k_reward_terms', 'k_blue_view'))
    if len(sa) < 4 * per or len(rt) < per or len(blue) < per:
        raise SystemExit(f'{len(sa)} k_sample_actions, {len(rt)} k_reward_terms, {len(blue)} k_blue_view dispatches in the trace, expected at least {4 * per}, {per}, {per}')
    tail = sa[-4 * per:]
    stat = lambda x: (float(np.median(x[WARM:])), float(np.min(x[WARM:])), float(np.max(x[WARM:])))      # noqa: E731
    in_loop = float(np.median(sa[100:-4 * per])) if len(sa) > 4 * per + 100 else float('nan')
    w = {key: min(v) for key, v in c['loop_s'].items()}
    us = lambda s: 1e6 * s / k                          # noqa: E731
    runs = lambda key: ', '.join(f'{us(x):.1f}' for x in c['loop_s'][key])      # noqa: E731
    lines = [f'# tools/sample_probe.py: k_sample_actions on one GPU; {n} episodes, counter mode, 500-step episodes with autoreset, 100 steps in; '
             f'{100 * c["busy_share"]:.1f} % of the (episode, agent) pairs busy',
             f'# kernel us: rocprofv3 --kernel-trace --stats in a run of its own (no counters), median of {c["reps"]} dispatches on the same rows; (min .. max)']
    for j, name in enumerate(VARIANTS):
        m, lo, hi = stat(tail[j::4])
        elt = ELEM_BYTES.get(name, 0)      # (none: no logits)
        b = 570 * elt + ROW_READ + OUT_BYTES
        lines.append(f'  k_sample_actions, logits {name:9s} {m:7.1f} us  ({lo:.1f} .. {hi:.1f})   {b:5d} B per episode from the shapes ({OUT_BYTES} B out)   '
                     f'{b * n / (m * 1e-6) / 1e12:5.2f} TB/s')
    for name, x in (('k_reward_terms (switch off: no record)', rt[-per:]), ('k_blue_view, log off', blue[-per:])):
        m, lo, hi = stat(x)
        lines.append(f'  {name:41s} {m:7.1f} us  ({lo:.1f} .. {hi:.1f})')
    lines += [f'  k_sample_actions inside the loop (bfloat16, behind a step): median {in_loop:7.1f} us',
              f'# the loop ({c["step_kernel"]}): wall clock of {k} steps, enqueued without a host wait, one synchronise at the end; two runs each, alternating; the faster one.',
              '#   Episode steps/s (x 5 = agent-env steps/s); outside the profiler; the logits are a fixed bfloat16 tensor',
              f'  sample_actions + step                                       {n * k / w["fused"]:12.4g} steps/s   {us(w["fused"]):8.1f} us per step   (runs: {runs("fused")})',
              f'  the sampling in PyTorch, busy rule from blue_view() + step  {n * k / w["torch"]:12.4g} steps/s   {us(w["torch"]):8.1f} us per step   (runs: {runs("torch")})',
              f'  the sampling in PyTorch without the busy rule + step        {n * k / w["torch_nb"]:12.4g} steps/s   {us(w["torch_nb"]):8.1f} us per step   (runs: {runs("torch_nb")})',
              f'  step alone (fixed actions)                                  {n * k / w["step"]:12.4g} steps/s   {us(w["step"]):8.1f} us per step   (runs: {runs("step")})',
              f'  the sampling adds: fused {us(w["fused"] - w["step"]):.1f} us per step, PyTorch {us(w["torch"] - w["step"]):.1f} us, PyTorch without the busy rule '
              f'{us(w["torch_nb"] - w["step"]):.1f} us; the loop with the fused call is {w["torch"] / w["fused"]:.2f}x / {w["torch_nb"] / w["fused"]:.2f}x as fast',
              f'  the two samplers on the same rows: the same agents at -1: {c["agree"]["busy_equal"]}; max |entropy fused - entropy PyTorch| {c["agree"]["entropy_max_diff"]:.3g}; '
              f'mean logp of the draws {c["agree"]["mean_logp_fused"]:.4f} (fused) / {c["agree"]["mean_logp_torch"]:.4f} (PyTorch, other noise)']
    if a.tests:
        lines.append('# float32 on the device against the float64 restatement (tests/test_sample_device.py, pytest -s): cases, cases below tau, largest differences')
        lines += ['  ' + ln.strip().lstrip('.') for ln in open(a.tests) if 'below tau' in ln]
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
