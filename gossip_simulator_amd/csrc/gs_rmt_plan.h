// gs_rmt_plan.h -- the LDS plan of the trial-resident rumor kernel
// (k_rmt_rounds, gs_rumor_trials.hip).  Pure host arithmetic and no HIP
// header, so a host compiler takes it alone (tests/test_rumor_trials.py).
//
// One workgroup runs one trial with the trial's state in LDS: bitsets of
// ceil(n / 64) 8-byte words -- `cur` (the informed set every decision of the
// round reads), `next` (the set being built) and `hot`; with GS_RUMOR_PULL and
// feedback also `served` and `vain` -- then the block reduction's scratch (five
// u32 counters per wave of the largest block), then, unless GS_RUMOR_COIN, the
// miss counts: one byte per node of the trial's words (64 per word, so a lane
// owns its node's byte and the bytes of a word are the wave's own).  Block rule,
// fit and limit: gs_trial_plan.h.  A failure mask is read from global memory:
// it is no part of the plan.
#ifndef GS_RMT_PLAN_H
#define GS_RMT_PLAN_H

#include <cstdint>
#include "gs_trial_plan.h"

namespace gs {

constexpr uint32_t kRmtMaxBlock = kTrialMaxBlock;
constexpr uint32_t kRmtCounters = 5;  // fired, sent, messages, newly informed, hot
constexpr uint64_t kRmtScratchBytes = trial_scratch_bytes(kRmtCounters);  // 320 B
constexpr uint32_t kRmtBlind = 1, kRmtCoin = 2, kRmtPull = 4;  // gossip.h's GS_RUMOR_* bits

struct RmtPlan {
  uint64_t words = 0;       // ceil(n / 64): words per bitset
  uint32_t bitsets = 0;     // 3, or 5 in feedback pull
  uint64_t miss_bytes = 0;  // 64 * words, or 0 with a coin
  uint64_t lds_bytes = 0;   // dynamic LDS of one workgroup
  uint32_t block = 0;       // threads per workgroup (a multiple of 64)
  bool fits = false;        // lds_bytes <= the limit
};

inline uint32_t rmt_bitsets(uint32_t mode) { return (mode & kRmtPull) && !(mode & kRmtBlind) ? 5u : 3u; }
inline bool rmt_has_miss(uint32_t mode) { return !(mode & kRmtCoin); }
// LDS bytes per 64-node word of the trial.
inline uint64_t rmt_word_bytes(uint32_t mode) { return rmt_bitsets(mode) * 8ull + (rmt_has_miss(mode) ? 64ull : 0ull); }

inline RmtPlan rmt_plan(uint64_t n, uint32_t mode, uint64_t lds_limit_bytes) {
  RmtPlan p;
  p.words = (n + 63) / 64;
  p.bitsets = rmt_bitsets(mode);
  p.miss_bytes = rmt_has_miss(mode) ? 64 * p.words : 0;
  p.lds_bytes = p.bitsets * p.words * 8 + kRmtScratchBytes + p.miss_bytes;
  p.block = trial_block(n);
  p.fits = trial_fits(n, p.lds_bytes, lds_limit_bytes);
  return p;
}

inline uint64_t rmt_max_n(uint32_t mode, uint64_t lds_limit_bytes) {
  return trial_max_n(lds_limit_bytes, kRmtScratchBytes, rmt_word_bytes(mode));
}

}  // namespace gs

#endif
