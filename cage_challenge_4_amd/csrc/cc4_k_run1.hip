// cc4_k_run1.hip -- the persistent kernel of large counter-mode batches: k_run_philox1 (six waves per SIMD) and k_run_philox1x (five: beside RCCL).
#include "cc4_philox1_body.h"
#include "cc4_persist.h"

// register budget of the persistent counter-mode kernel in waves per SIMD: 6 (80 VGPRs, eight spilled: 24 waves per CU -- by registers and,
// since r06's 5952-byte agent part made a wave FIVE 1280-byte LDS granules, by LDS as well: 25) or 5 (93 VGPRs, nothing spilled: 20 per CU).
// Measured, 8192 episodes, one box (profiles/r06_layout_ab.txt): K = 500: 989-990 vs 914-915 M, K = 20: 831-846 vs 797-807 M.  (r05, when LDS
// capped a CU at 21 waves: 952 vs 939-948 M -- inside the box-to-box spread.)
// The headline build (HEAD): no exchange, no rollout protocol, no plan, and the blue actions always drawn in the kernel -- persist_launch sends it only
// calls of that shape (anything else takes k_run_philox1g, cc4_k_run1g.hip, which keeps every run-time flag), so it has no XchgArgs and neither loads nor tests the
// action / message arguments.
__global__ __launch_bounds__(WAVE, CC4_PERSIST_MINW) void k_run_philox1(StepArgs a, RunArgs ra) { persist_loop<false, false, false, false, true>(a, ra, XchgArgs{}); }
