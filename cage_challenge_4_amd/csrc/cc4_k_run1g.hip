// cc4_k_run1g.hip -- k_run_philox1g: the persistent counter-mode kernel with every run-time flag (host actions, messages, system-scope action loads), on
// the register budget of k_run_philox1.  persist_launch sends it whatever call of a handle without a communicator does not have the headline
// kernel's shape (cc4_k_run1.hip); the exchange and the rollout protocol are not in this build either (k_run_philox1x / k_run_philox1r).
#include "cc4_philox1_body.h"
#include "cc4_persist.h"

__global__ __launch_bounds__(WAVE, CC4_PERSIST_MINW) void k_run_philox1g(StepArgs a, RunArgs ra, XchgArgs x) { persist_loop<false, false, false>(a, ra, x); }
