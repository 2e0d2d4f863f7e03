#!/usr/bin/env python
"""A PyTorch learner's step loop on the same GPU, four ways, in one process (counter mode, autoreset; profiles/r07_torch_env.txt):
  (a) CC4VecEnv.step             host actions in, host observations out (cc4_step_fetch: one copy each way, one host wait per step)
  (b) CC4VecEnv.run_policy_steps the stand-in policy kernel writes the handle's device action buffer, cc4_step_device (no outputs for torch)
  (c) CC4TorchVecEnv.step        a trivial torch policy (torch.randint modulo each agent's range: two torch kernels) -> step -> uint8 observations
  (d) CC4TorchVecEnv.step        a small masked-categorical MLP in torch.nn (578 -> 256 -> 570 logits, bfloat16, masked, sampled per agent)
Every form is timed with device events on the torch stream after a warm-up; (a) and (b) run on the handle's streams, which the torch stream
waits for (cc4_stream_wait before the region, cc4_stream_signal after it).  Rates are agent-env steps/s (episode steps x 5 agents).

Usage: torch_env_probe.py [--envs 1024,8192] [--steps 200] [--warmup 20] [--forms abcd]"""
import argparse
import ctypes
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cage_challenge_4_amd import CC4VecEnv
from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
from cage_challenge_4_amd import _lib as L

RANGES = torch.tensor(L.ACT_LEN, dtype=torch.int32)


class MaskedPolicy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(L.OBS_PER_ENV, 256), torch.nn.ReLU(), torch.nn.Linear(256, L.MASK_PER_ENV))

    def forward(self, obs, mask):
        logits = self.net(obs).float().masked_fill(~mask, float('-inf'))
        g = -torch.log(-torch.log(torch.rand_like(logits).clamp_(1e-20, 1.0)))     # Gumbel-max: one sample per agent segment
        z = logits + g
        short = z[:, :4 * 82].view(-1, 4, 82).argmax(-1)
        long_ = z[:, 4 * 82:].argmax(-1, keepdim=True)
        return torch.cat([short, long_], 1)


def timed(fn, k, warmup, s):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(k):
        fn(warmup + i)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='1024,8192')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--forms', default='abcd')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    s = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(s.cuda_stream)
    K, W = args.steps, args.warmup
    print(f'# torch {torch.__version__}, HIP {torch.version.hip}, {torch.cuda.get_device_name(dev)}; {K} timed steps after {W} warm-up steps per form')
    for n in (int(x) for x in args.envs.split(',')):
        kw = dict(steps=500, rng_mode=1, autoreset=True, strict=False)
        res = {}
        if 'a' in args.forms or 'b' in args.forms:
            env = CC4VecEnv(n, **kw)
            env.reset(seeds=1000)
            rng = np.random.default_rng(0)
            acts = [np.stack([rng.integers(0, r, n) for r in L.ACT_LEN], 1).astype(np.int32) for _ in range(8)]

            def around_handle(body):            # the handle's streams inside the torch stream's timed region
                def f(i):
                    env.lib.cc4_stream_wait(env._h, sp)
                    body(i)
                    env.lib.cc4_stream_signal(env._h, sp)
                return f
            if 'a' in args.forms:
                res['a'] = timed(around_handle(lambda i: env.step(acts[i % 8])), K, W, s)
            if 'b' in args.forms:
                # one call of K steps (as bench.py's policy_in_loop): the region's stream operations are enqueued back to back
                for _ in range(2):
                    env.run_policy_steps(1000, 0, W)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                env.lib.cc4_synchronize(env._h)
                e0.record(s)
                env.lib.cc4_stream_wait(env._h, sp)
                env.run_policy_steps(1000, W, K)
                env.lib.cc4_stream_signal(env._h, sp)
                e1.record(s)
                e1.synchronize()
                res['b'] = e0.elapsed_time(e1) * 1e-3
            env.close()
        if 'c' in args.forms:
            tenv = CC4TorchVecEnv(n, obs_dtype=torch.uint8, **kw)
            tenv.reset(seeds=1000)
            ranges = RANGES.to(dev)

            def trivial(i):
                a = torch.randint(0, 1 << 30, (n, 5), dtype=torch.int32, device=dev) % ranges     # two torch kernels
                tenv.step(a)
            res['c'] = timed(trivial, K, W, s)
            tenv.close()
        if 'd' in args.forms:
            tenv = CC4TorchVecEnv(n, obs_dtype=torch.bfloat16, **kw)
            obs, info = tenv.reset(seeds=1000)
            pol = MaskedPolicy().to(dev, torch.bfloat16)

            def mlp(i):
                with torch.no_grad():
                    tenv.step(pol(tenv.obs, tenv.action_mask))
            res['d'] = timed(mlp, K, W, s)
            tenv.close()
        names = {'a': 'CC4VecEnv.step (host actions, host outputs)', 'b': 'CC4VecEnv.run_policy_steps (stand-in policy kernel)',
                 'c': 'CC4TorchVecEnv, trivial torch policy', 'd': 'CC4TorchVecEnv, masked MLP 578-256-570 (bf16)'}
        for f, sec in res.items():
            rate = n * 5 * K / sec
            print(f'envs {n:5d}  ({f}) {names[f]:52s} {sec / K * 1e6:9.1f} us/step  {rate / 1e6:8.1f} M agent-env steps/s')
        if 'b' in res and 'c' in res:
            print(f'envs {n:5d}  (c)/(b) = {res["b"] / res["c"]:.3f}' + (f'   (c)/(a) = {res["a"] / res["c"]:.2f}' if 'a' in res else ''))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
