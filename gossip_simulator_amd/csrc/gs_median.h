// gs_median.h -- the median-counter push-pull engine (GS_MODEL_MEDIAN,
// DESIGN.md section 4.8): the device state gs_median.hip's kernels work on and
// the launchers gs_median_host.cpp calls.
#pragma once
#include "gs_internal.h"

namespace gs {

// st[v]: 0 = A (uninformed), m in 1..k = B-m, k + c with c in 1..k = C-c,
// kMedianDone = D.  k <= 127, so C-k <= 254.
constexpr uint8_t kMedianDone = 255;
// own[v]: what v's own call met, written by v's lane only and merged by the
// commit.  For a caller in A, kOwnGe says "a B partner" (b(v) > 0).
constexpr uint8_t kOwnNone = 0, kOwnC = 1, kOwnGe = 2, kOwnLt = 3;
// tally[u]: the callers' ends of a B node's connections, ge in the low word
// and lt in the high one.  A round has at most n < 2^31 callers, so neither
// field reaches bit 31 and the low one never carries into the high one.
constexpr unsigned long long kTallyGe = 1ull, kTallyLt = 1ull << 32;

// The round control is the rumor engine's block (RumorCtl): acc = the round's
// fired / sent / messages / newly informed, wlen = the active nodes after the
// round, rlen = before it, stop = gs_run's rule.
struct MedianState {
  RumorCtl* ctl;
  uint8_t* st;                  // [n] the state bytes
  uint8_t* own;                 // [n] v's own end of its connection (zero between rounds)
  unsigned long long* tally;    // [n] the callers' ends at a B node (zero between rounds)
  unsigned long long* gotb;     // [W] A nodes a B caller reached this round (zero between rounds)
  unsigned long long* gotc;     // [W] A and B nodes a C caller reached this round (zero between rounds)
  uint32_t k;                   // gs_params.rumor_k, 1..127
};

// The persistent round grid for n nodes: `want` blocks (0: 256 CUs x 8), at most one lane per node.
uint32_t median_grid(uint64_t n, uint32_t want);
// ctl, st and the round buffers zeroed by the caller; a live sender becomes B-1.
hipError_t median_seed(const DevState& s, const MedianState& m, uint32_t node, unsigned long long cover,
                       hipStream_t st);
// Round t: every live node with a friend that is not done calls; own, tally, gotb and gotc are built from st.
hipError_t median_round(const DevState& s, const MedianState& m, uint32_t t, uint32_t grid, hipStream_t st);
// The end of round t: the new states, recv rebuilt, the round buffers cleared, then the stats row and the stop word.
hipError_t median_commit(const DevState& s, const MedianState& m, uint32_t t, hipStream_t st);
// out = the D set.
hipError_t median_done_set(const DevState& s, const MedianState& m, unsigned long long* out, hipStream_t st);

}  // namespace gs
