// gs_trial_plan.h -- what the LDS plans of the trial-resident kernels share
// (gs_ppt_plan.h, gs_rmt_plan.h, gs_mdt_plan.h).  Pure
// host arithmetic and no HIP header, so a host compiler takes it alone.
//
// One workgroup runs one trial with the trial's state in LDS: so many bytes
// per 64-node word of the trial (the engine's own layout) and the block
// reduction's scratch, a u32 per counter and wave of the largest block.  A
// trial fits when that is within what the device grants one workgroup.
#ifndef GS_TRIAL_PLAN_H
#define GS_TRIAL_PLAN_H

#include <cstdint>

namespace gs {

constexpr uint32_t kTrialMaxBlock = 1024;  // threads: 16 waves

constexpr uint64_t trial_scratch_bytes(uint32_t counters) { return counters * (kTrialMaxBlock / 64) * 4; }

// Smaller blocks for small n: the smallest of 64 .. 1024 threads (powers of
// two) that leaves a lane at most 16 nodes per round.
inline uint32_t trial_block(uint64_t n) {
  uint32_t block = 64;
  while (block < kTrialMaxBlock && (uint64_t)block * 16 < n) block *= 2;
  return block;
}

inline bool trial_fits(uint64_t n, uint64_t lds_bytes, uint64_t lds_limit_bytes) {
  return n >= 1 && lds_bytes <= lds_limit_bytes;
}

// The largest n that fits (0: not even one word does).
inline uint64_t trial_max_n(uint64_t lds_limit_bytes, uint64_t scratch_bytes, uint64_t word_bytes) {
  if (lds_limit_bytes < scratch_bytes + word_bytes) return 0;
  return (lds_limit_bytes - scratch_bytes) / word_bytes * 64;
}

}  // namespace gs

#endif
