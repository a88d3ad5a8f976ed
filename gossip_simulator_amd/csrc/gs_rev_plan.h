// gs_rev_plan.h -- the pass plan of the partitioned reverse-table build
// (pp_rev_build_part, gs_pp_rev.hip).  Pure host arithmetic and no HIP
// header, so a host compiler takes it alone (tests/devmem_harness.cpp).
//
// The coarse bins are taken in passes of consecutive bins.  A pass holds two
// copies of its records in one temporary: the coarse copy (h[c] records of bin
// c) at the block's start and the fine regions (need[c] - h[c] records) right
// behind it, so a pass takes the sum of need[c] over its bins and the block is
// as large as the largest pass.  Unforced, a pass takes bins while that sum
// stays within `cap` records: the block then fits the extent the plan was made
// for.  (Sizing the block as the largest coarse copy plus the largest fine
// copy, with one split for all passes, does not: the two maxima may come from
// different passes.)
#ifndef GS_REV_PLAN_H
#define GS_REV_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

namespace gs {

struct RevPlan {
  bool ok = false;             // false: not even one bin fits `cap`
  std::vector<uint32_t> cut;   // pass p = bins [cut[p], cut[p+1]); cut[0] = 0, cut.back() = nbins
  std::vector<uint64_t> rec;   // pass p's coarse records: its fine copy starts that far into the block
  uint64_t tmp_records = 0;    // the temporary, in 8-byte records (at least 1)
};

// h[c]: bin c's records; need[c] >= h[c]: its records in both copies; forced:
// 0, or the pass count to plan whatever `cap` is (passes of ceil(nbins/forced)
// bins).
inline RevPlan pp_rev_plan(const unsigned long long* h, const unsigned long long* need, uint64_t nbins, uint64_t cap,
                           uint64_t forced) {
  RevPlan pl;
  pl.cut.push_back(0);
  if (forced) {
    const uint64_t per = (nbins + forced - 1) / forced;
    for (uint64_t c = per; c < nbins; c += per) pl.cut.push_back((uint32_t)c);
  } else {
    uint64_t acc = 0;
    for (uint64_t c = 0; c < nbins; ++c) {
      if (need[c] > cap) return pl;
      if (acc + need[c] > cap) {
        pl.cut.push_back((uint32_t)c);
        acc = 0;
      }
      acc += need[c];
    }
  }
  pl.cut.push_back((uint32_t)nbins);
  pl.tmp_records = 1;
  for (size_t p = 0; p + 1 < pl.cut.size(); ++p) {
    uint64_t sum = 0, r = 0;
    for (uint32_t c = pl.cut[p]; c < pl.cut[p + 1]; ++c) {
      sum += need[c];
      r += h[c];
    }
    pl.rec.push_back(r);
    pl.tmp_records = std::max(pl.tmp_records, sum);
  }
  pl.ok = true;
  return pl;
}

}  // namespace gs

#endif
