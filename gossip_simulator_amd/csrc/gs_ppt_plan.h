// gs_ppt_plan.h -- the LDS plan of the trial-resident push-pull kernel
// (k_ppt_rounds, gs_pushpull_trials.hip).  Pure host arithmetic and no HIP
// header, so a host compiler takes it alone (tests/test_pushpull_trials.py).
//
// One workgroup runs one trial with the trial's informed set in LDS: two
// bitsets (the round's `cur` and the `next` being built) of ceil(n / 64)
// 8-byte words, then the block reduction's scratch (four u32 counters per
// wave of the largest block).  Block rule, fit and limit: gs_trial_plan.h.
//
// With per-trial failure masks (gs_set_failed on a batch) a third, read-only
// bitset `F` of the trial's failed nodes sits beside them: three bitsets and
// the same scratch, so the masked limit is two thirds of the unmasked one.
#ifndef GS_PPT_PLAN_H
#define GS_PPT_PLAN_H

#include <cstdint>
#include "gs_trial_plan.h"

namespace gs {

constexpr uint32_t kPptMaxBlock = kTrialMaxBlock;
constexpr uint32_t kPptCounters = 4;                                        // fired, sent, messages, received
constexpr uint64_t kPptScratchBytes = trial_scratch_bytes(kPptCounters);    // 256 B

struct PptPlan {
  uint64_t words = 0;      // ceil(n / 64): words per bitset
  uint64_t lds_bytes = 0;  // dynamic LDS of one workgroup
  uint32_t block = 0;      // threads per workgroup (a multiple of 64)
  bool fits = false;       // lds_bytes <= the limit
};

// `bitsets` bitsets (cur, next; masked: and F), then the scratch.
inline PptPlan ppt_plan_of(uint64_t n, uint32_t bitsets, uint64_t lds_limit_bytes) {
  PptPlan p;
  p.words = (n + 63) / 64;
  p.lds_bytes = bitsets * p.words * 8 + kPptScratchBytes;
  p.block = trial_block(n);
  p.fits = trial_fits(n, p.lds_bytes, lds_limit_bytes);
  return p;
}

inline PptPlan ppt_plan(uint64_t n, uint64_t lds_limit_bytes) { return ppt_plan_of(n, 2, lds_limit_bytes); }
inline uint64_t ppt_max_n(uint64_t lds_limit_bytes) { return trial_max_n(lds_limit_bytes, kPptScratchBytes, 2 * 8); }

// The masked layout.
inline PptPlan ppt_plan_masked(uint64_t n, uint64_t lds_limit_bytes) { return ppt_plan_of(n, 3, lds_limit_bytes); }
inline uint64_t ppt_max_n_masked(uint64_t lds_limit_bytes) {
  return trial_max_n(lds_limit_bytes, kPptScratchBytes, 3 * 8);
}

}  // namespace gs

#endif
