"""What a wave of k_run_philox1 pays between two items, measured in the kernel.

Needs a library built with -DCC4_BOUNDARY_PROF (make -C cage_challenge_4_amd/csrc BUILD=<dir> OUT=<lib> EXTRA=-DCC4_BOUNDARY_PROF), named by CC4_LIB: its
headline kernel sums, per wave and in registers, the wall-clock ticks between the end of an item's last step and the first step_phase of the wave's next
item, split into stage-out drain + publish / pick / progress wait + acquire / stage-in, and writes them once at exit; the library prints one
`[cc4 boundary]` line per call on stderr.  The shipped library has none of this code.

    CC4_LIB=<lib> python tools/persist_boundary.py [episodes] [k ...]          (default 8192 episodes, calls of 500 500 20 20 steps)
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ['CC4_PERSIST_TIMELINE'] = '1'
from cage_challenge_4_amd import CC4VecEnv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
ks = [int(v) for v in sys.argv[2:]] or [500, 500, 20, 20]
env = CC4VecEnv(n, steps=500, autoreset=True, rng_mode=1, strict=False)
env.reset(seeds=1000)
env.run_random_steps(1000, 0, 50, timed=False)
t = 50
for k in ks:
    env.run_random_steps(1000, t, k, timed=True)
    t += k
print('kernel', env.run_kernel_for(ks[0]) if hasattr(env, 'run_kernel_for') else '?', 'runs', os.environ.get('CC4_PERSIST_RUNS', 'default'))
