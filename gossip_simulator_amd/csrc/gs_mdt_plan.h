// gs_mdt_plan.h -- the LDS plan of the trial-resident median-counter kernel
// (k_mdt_rounds, gs_median_trials.hip).  Pure host arithmetic and no HIP
// header, so a host compiler takes it alone (tests/test_median_trials.py).
//
// One workgroup runs one trial with the trial's state in LDS, in this order
// (W = ceil(n / 64) words of 64 nodes):
//   diff     i32[64 W]  ge - lt of a B node's partners this round (one signed
//                       word: only its sign is read, and |ge - lt| <= n + 1)
//   gotb     u64[W]     A nodes with a B partner this round
//   gotc     u64[W]     A and B nodes with a C partner this round
//   scratch  u32[5][16] the block reduction's: five counters per wave of the
//                       largest block
//   st       u8[64 W]   the state bytes every decision of the round reads (a
//                       lane owns its node's byte)
// 336 B per word and 320 B of scratch.  Block rule, fit and limit:
// gs_trial_plan.h.  A failure mask is read from global memory: it is no part
// of the plan.
#ifndef GS_MDT_PLAN_H
#define GS_MDT_PLAN_H

#include <cstdint>
#include "gs_trial_plan.h"

namespace gs {

constexpr uint32_t kMdtMaxBlock = kTrialMaxBlock;
constexpr uint32_t kMdtCounters = 5;  // fired, sent, messages, newly informed, active
constexpr uint64_t kMdtScratchBytes = trial_scratch_bytes(kMdtCounters);  // 320 B
constexpr uint64_t kMdtWordBytes = 64 * 4 + 8 + 8 + 64;                   // 336 B per 64 nodes

struct MdtPlan {
  uint64_t words = 0;  // ceil(n / 64)
  // byte offsets of the arrays in the workgroup's dynamic LDS
  uint64_t off_diff = 0, off_gotb = 0, off_gotc = 0, off_scratch = 0, off_st = 0;
  uint64_t lds_bytes = 0;  // dynamic LDS of one workgroup
  uint32_t block = 0;      // threads per workgroup (a multiple of 64)
  bool fits = false;       // lds_bytes <= the limit
};

inline MdtPlan mdt_plan(uint64_t n, uint64_t lds_limit_bytes) {
  MdtPlan p;
  p.words = (n + 63) / 64;
  p.off_diff = 0;
  p.off_gotb = p.off_diff + 64 * 4 * p.words;
  p.off_gotc = p.off_gotb + 8 * p.words;
  p.off_scratch = p.off_gotc + 8 * p.words;
  p.off_st = p.off_scratch + kMdtScratchBytes;
  p.lds_bytes = p.off_st + 64 * p.words;
  p.block = trial_block(n);
  p.fits = trial_fits(n, p.lds_bytes, lds_limit_bytes);
  return p;
}

inline uint64_t mdt_max_n(uint64_t lds_limit_bytes) {
  return trial_max_n(lds_limit_bytes, kMdtScratchBytes, kMdtWordBytes);
}

}  // namespace gs

#endif
