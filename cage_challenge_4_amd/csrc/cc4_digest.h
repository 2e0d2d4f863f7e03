// cc4_digest.h -- the self-check's digest of one episode (CC4_PERSIST_VERIFY), stated once for the device (cc4_k_misc.hip: k_digest, one
// wavefront per episode, lane = threadIdx.x) and the host (cc4_debug_digest_rows: the 64 lanes in a loop).  Three 64-bit words per episode -- hot row,
// cold row, outputs -- so that a mismatch says where.  The words are defined in prose in include/cc4_debug.h; tests/digest_util.py restates that prose.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "cc4_rng.h"      // CC4_HD

namespace cc4 {

constexpr int DIGEST_LANES = 64, DIGEST_OBS = 578, DIGEST_ACTIONS = 5, DIGEST_SCALAR_LANE = 8;
constexpr uint64_t DIGEST_ROW_SEED = 0x1234567ull, DIGEST_OUT_SEED = 0x89ABCDEFull;

CC4_HD uint64_t digest_mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  return h * 0xD6E8FEB86659FD93ull;
}

// Every lane closes its chain with one more round on its own number.  Without it the LAST value a lane takes reaches the lane's h through one XOR and one
// multiplication only: bit b of that value flipped moves h by +-2^b M (carries aside) whatever the lane, so the same flip in two lanes' last vectors gave
// the same word, and opposite flips in two lanes cancelled in the sum (tests/test_digest_cpu.py found 55 equal words among the 1840 single-bit flips of
// a hot row).  Behind the closing round a difference in h has gone through the lane's own h << 6, h >> 2 and carries.
CC4_HD uint64_t digest_close(uint64_t h, int lane) { return digest_mix(h, (uint64_t)lane); }

// one 16-byte vector of a row as four little-endian words (the device rows are 16-byte aligned: one load; a host row need not be)
struct alignas(16) DigestVec { uint32_t x, y, z, w; };
CC4_HD DigestVec digest_load(const void* row, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<const DigestVec*>(row)[i];
#else
  DigestVec v;
  __builtin_memcpy(&v, static_cast<const char*>(row) + 16 * i, 16);
  return v;
#endif
}

// a lane's chain over the vectors lane, lane + 64, .. of a row of nv vectors: position-dependent within the lane
CC4_HD uint64_t digest_row_lane(const void* row, size_t nv, int lane) {
  uint64_t h = DIGEST_ROW_SEED + (uint64_t)lane;
  for (size_t i = (size_t)lane; i < nv; i += DIGEST_LANES) {
    const DigestVec v = digest_load(row, i);
    h = digest_mix(h, ((uint64_t)v.x << 32) | v.y);
    h = digest_mix(h, ((uint64_t)v.z << 32) | v.w);
  }
  return digest_close(h, lane);
}

// a lane's share of the outputs word: the observation values lane, lane + 64, ..; lanes 0..4 the drawn actions; lane 8 reward, then done << 32 | err
CC4_HD uint64_t digest_out_lane(const int32_t* obs, const int32_t* actions, uint32_t reward_bits, uint8_t done, uint32_t err, int lane) {
  uint64_t h = DIGEST_OUT_SEED + (uint64_t)lane;
  for (int i = lane; i < DIGEST_OBS; i += DIGEST_LANES) h = digest_mix(h, (uint64_t)(uint32_t)obs[i]);
  if (lane < DIGEST_ACTIONS) h = digest_mix(h, (uint64_t)(uint32_t)actions[lane]);
  if (lane == DIGEST_SCALAR_LANE) { h = digest_mix(h, (uint64_t)reward_bits); h = digest_mix(h, ((uint64_t)done << 32) | err); }
  return digest_close(h, lane);
}

// the cross-lane sum (mod 2^64): order-independent across lanes
#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t digest_wave_sum(uint64_t h) {
  for (int off = DIGEST_LANES / 2; off >= 1; off >>= 1) h += __shfl_xor(h, off);
  return h;
}
#endif
inline uint64_t digest_row_word(const void* row, size_t nv) {
  uint64_t s = 0;
  for (int lane = 0; lane < DIGEST_LANES; ++lane) s += digest_row_lane(row, nv, lane);
  return s;
}
inline uint64_t digest_out_word(const int32_t* obs, const int32_t* actions, uint32_t reward_bits, uint8_t done, uint32_t err) {
  uint64_t s = 0;
  for (int lane = 0; lane < DIGEST_LANES; ++lane) s += digest_out_lane(obs, actions, reward_bits, done, err, lane);
  return s;
}

// the compare of two sides' digests of episode e ([N][3] words each): bit 0 the hot rows differ, bit 1 the cold rows, bit 2 the outputs
inline int digest_differs(const uint64_t* a, const uint64_t* b, size_t e) {
  return (a[3 * e] != b[3 * e] ? 1 : 0) | (a[3 * e + 1] != b[3 * e + 1] ? 2 : 0) | (a[3 * e + 2] != b[3 * e + 2] ? 4 : 0);
}

}  // namespace cc4
