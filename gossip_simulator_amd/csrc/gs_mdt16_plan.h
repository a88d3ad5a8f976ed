// gs_mdt16_plan.h -- the packed LDS plan of the trial-resident median-counter
// kernel (k_mdt16_rounds, gs_median_trials.hip; GS_FLAG_MEDIAN_PACKED;
// DESIGN.md section 4.8.2) and the arithmetic of its 16-bit tallies.  Pure
// arithmetic and no HIP header, so a host compiler takes it alone
// (tests/test_median_packed.py); the kernel compiles the same functions.
//
// gs_mdt_plan.h with the signed word of a node cut to a 16-bit field, two
// nodes per 32-bit word (W = ceil(n / 64) words of 64 nodes):
//   diff16   u16[64 W]  0x8000 + (ge - lt) of a B node's partners this round
//   gotb     u64[W]     as in gs_mdt_plan.h
//   gotc     u64[W]
//   scratch  u32[5][16]
//   st       u8[64 W]
// 208 B per word and 320 B of scratch.  Block rule, fit and limit:
// gs_trial_plan.h.
//
// The fields.  Node v's field is half v & 1 of 32-bit word v >> 1 (the low
// half first: the u16 at index v of the same bytes, little-endian).  A field
// holds 0x8000 + d, d = ge - lt.  A +-1 on node v is one 32-bit add of
// +-1 << 16 (v & 1) to its word, in any order with the adds to the other
// half: while every partial sum of a field's adds stays within +-32,767 the
// field stays in 1 .. 0xFFFF, so the add of 1 carries nothing out of it and
// the add of -1 (all ones from the field's lowest bit up) carries exactly the
// one that turns the ones above the field back into zero.  A node has at most
// one partner per used slot that names it and one for its own call (two for a
// self-call, which is a slot that names it), so |d| <= 32,767 whenever no
// node is named by more than kMdt16MaxNamed slots of its trial's table --
// which holds for every table of n <= kMdt16MaxNamed nodes, where the callers
// themselves are that few.  The commit reads its own half as a u16 and
// stores 0x8000 to that half alone.
#ifndef GS_MDT16_PLAN_H
#define GS_MDT16_PLAN_H

#include <cstdint>
#include "gs_mdt_plan.h"

#if defined(__HIPCC__)
#define GS_MDT16_FN __host__ __device__ inline
#else
#define GS_MDT16_FN inline
#endif

namespace gs {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "node v's field is the u16 at index v of the tally words");

constexpr uint64_t kMdt16WordBytes = 64 * 2 + 8 + 8 + 64;  // 208 B per 64 nodes
constexpr uint32_t kMdt16Bias = 0x8000;                    // a field of d = 0
constexpr uint32_t kMdt16Init = 0x80008000u;               // a word of two such fields
constexpr uint32_t kMdt16MaxDiff = 32767;                  // |ge - lt| a field holds
constexpr uint32_t kMdt16MaxNamed = 32766;                 // used slots that may name one node (and its own call)
constexpr uint64_t kMdt16MaxN = 50304;                     // mdt16_max_n at the 163,840 B an MI355X grants a workgroup

// The same struct as the unpacked plan's: off_diff is diff16's.
inline MdtPlan mdt16_plan(uint64_t n, uint64_t lds_limit_bytes) {
  MdtPlan p;
  p.words = (n + 63) / 64;
  p.off_diff = 0;
  p.off_gotb = p.off_diff + 64 * 2 * p.words;
  p.off_gotc = p.off_gotb + 8 * p.words;
  p.off_scratch = p.off_gotc + 8 * p.words;
  p.off_st = p.off_scratch + kMdtScratchBytes;
  p.lds_bytes = p.off_st + 64 * p.words;
  p.block = trial_block(n);
  p.fits = trial_fits(n, p.lds_bytes, lds_limit_bytes);
  return p;
}

inline uint64_t mdt16_max_n(uint64_t lds_limit_bytes) {
  return trial_max_n(lds_limit_bytes, kMdtScratchBytes, kMdt16WordBytes);
}

static_assert((163840 - kMdtScratchBytes) / kMdt16WordBytes * 64 == kMdt16MaxN, "786 words of 208 B and 320 B");

// A field seen through its own 16 bits (the commit's view of the words the
// round half adds to).
typedef uint16_t __attribute__((may_alias)) mdt16_half_t;

GS_MDT16_FN uint32_t mdt16_word(uint32_t v) { return v >> 1; }

// What a +1 (up) or a -1 on node v adds to word mdt16_word(v).
GS_MDT16_FN uint32_t mdt16_delta(uint32_t v, bool up) { return (up ? 1u : ~0u) << (16 * (v & 1)); }

// ge - lt of node v from its word.
GS_MDT16_FN int32_t mdt16_diff(uint32_t word, uint32_t v) {
  return (int32_t)((word >> (16 * (v & 1))) & 0xFFFFu) - (int32_t)kMdt16Bias;
}

// The commit's read-and-clear: ge - lt of node v from its own half of
// `words`, and that half alone back to d = 0.
GS_MDT16_FN int32_t mdt16_take(uint32_t* words, uint32_t v) {
  mdt16_half_t* h = (mdt16_half_t*)words + v;
  const int32_t d = (int32_t)*h - (int32_t)kMdt16Bias;
  if (d) *h = (mdt16_half_t)kMdt16Bias;
  return d;
}

}  // namespace gs

#endif
