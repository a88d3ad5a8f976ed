// gs_ppt_plan.h -- the LDS plan of the trial-resident push-pull kernel
// (k_ppt_rounds, gs_pushpull_trials.hip).  Pure host arithmetic and no HIP
// header, so a host compiler takes it alone (tests/test_pushpull_trials.py).
//
// One workgroup runs one trial with the trial's informed set in LDS: two
// bitsets (the round's `cur` and the `next` being built) of ceil(n / 64)
// 8-byte words, then the block reduction's scratch (four u32 counters per
// wave of the largest block).  A trial fits when that is within what the
// device grants one workgroup.
//
// With per-trial failure masks (gs_set_failed on a batch) a third, read-only
// bitset `F` of the trial's failed nodes sits beside them: three bitsets and
// the same scratch, so the masked limit is two thirds of the unmasked one.
#ifndef GS_PPT_PLAN_H
#define GS_PPT_PLAN_H

#include <cstdint>

namespace gs {

constexpr uint32_t kPptMaxBlock = 1024;                           // threads: 16 waves
constexpr uint32_t kPptCounters = 4;                              // fired, sent, messages, received
constexpr uint64_t kPptScratchBytes = kPptCounters * (kPptMaxBlock / 64) * 4;  // 256 B

struct PptPlan {
  uint64_t words = 0;      // ceil(n / 64): words per bitset
  uint64_t lds_bytes = 0;  // dynamic LDS of one workgroup
  uint32_t block = 0;      // threads per workgroup (a multiple of 64)
  bool fits = false;       // lds_bytes <= the limit
};

// Smaller blocks for small n: the smallest of 64 .. 1024 threads (powers of
// two) that leaves a lane at most 16 nodes per round.
inline PptPlan ppt_plan(uint64_t n, uint64_t lds_limit_bytes) {
  PptPlan p;
  p.words = (n + 63) / 64;
  p.lds_bytes = 2 * p.words * 8 + kPptScratchBytes;
  p.block = 64;
  while (p.block < kPptMaxBlock && (uint64_t)p.block * 16 < n) p.block *= 2;
  p.fits = n >= 1 && p.lds_bytes <= lds_limit_bytes;
  return p;
}

// The largest n that fits (0: not even one word does).
inline uint64_t ppt_max_n(uint64_t lds_limit_bytes) {
  if (lds_limit_bytes < kPptScratchBytes + 16) return 0;
  return (lds_limit_bytes - kPptScratchBytes) / 16 * 64;
}

// The masked layout: cur, next and the failed set F, then the scratch.  Same
// block rule.
inline PptPlan ppt_plan_masked(uint64_t n, uint64_t lds_limit_bytes) {
  PptPlan p = ppt_plan(n, lds_limit_bytes);
  p.lds_bytes = 3 * p.words * 8 + kPptScratchBytes;
  p.fits = n >= 1 && p.lds_bytes <= lds_limit_bytes;
  return p;
}

// The largest n the masked layout fits (0: not even one word does).
inline uint64_t ppt_max_n_masked(uint64_t lds_limit_bytes) {
  if (lds_limit_bytes < kPptScratchBytes + 24) return 0;
  return (lds_limit_bytes - kPptScratchBytes) / 24 * 64;
}

}  // namespace gs

#endif
