// gs_rumorset.h -- concurrent rumors for push-pull (gs_create_rumorset,
// DESIGN.md section 4.9): the device state gs_rumorset.hip's kernels work on
// and the launchers gs_rumorset_host.cpp calls.
#pragma once
#include "gs_internal.h"

namespace gs {

constexpr uint32_t kRsMax = 64;  // GS_RUMORSET_MAX: a bit per rumor in a u64 per node

// Round control.  The words many workgroups add to sit on 256-byte blocks of
// their own (counter layout): the round's three counters,
// then the round's newly informed nodes per rumor; the rest is written by one
// wave per round (k_rs_seed, k_rs_publish) and read by the next kernels.
enum RsAcc : uint32_t { RS_FIRED = 0, RS_SENT = 1, RS_MSGS = 2 };
enum RsTraffic : uint32_t { RS_WANTED = 0, RS_CARRIED = 1, RS_BOUND = 2 };
struct RsCtl {
  unsigned long long acc[3];    // the round's fired / sent / messages (RsAcc)
  unsigned long long traffic[3];  // the broadcast's wanted / carried / bound (RsTraffic; k_rsc_round, section 4.9.1)
  unsigned long long pad0_[26];
  unsigned long long newc[kRsMax];  // the round's newly informed nodes per rumor (two blocks)
  unsigned long long cnt[kRsMax];   // nodes that hold rumor j, cumulative
  unsigned long long cover;     // smallest count the float32 coverage rule accepts
  unsigned long long live;      // bit j: rumor j started (its sender was not failed)
  unsigned long long received;  // (node, rumor) pairs so far
  unsigned long long pending;   // started rumors below `cover`
  uint32_t stop, pad1_;         // 0 while a started rumor is uncovered; else kRumorCovered / kRumorQuiescent
  unsigned long long pad2_[27];
};
static_assert(sizeof(RsCtl) == 6 * 256, "RsCtl: six 256-byte blocks");

struct RsState {
  RsCtl* ctl;
  unsigned long long* have;   // [n] bit j: the node holds rumor j (bits >= R are 0)
  unsigned long long* next;   // [n] what the round's callers gave the node (zero between rounds)
  unsigned long long* own;    // [n] what the node's own call took; v's lane only (zero between rounds)
  unsigned long long* ring;   // [kStatSlots][kRsMax] the per-rumor counts after round t, slot t % kStatSlots
  uint32_t R;                 // rumors, 1..kRsMax
};

struct RsSenders {
  uint32_t node[kRsMax];  // rumor j starts at node[j] (j < R)
};

// The persistent grid of the round and the commit for n nodes: `want` blocks
// (0: 256 CUs x 8), at most one lane per node.
uint32_t rs_grid(uint64_t n, uint32_t want);
// ctl, have, next, own and recv zeroed by the caller: the live senders' bits, the counts, the live mask, the stop word.
hipError_t rs_seed(const DevState& s, const RsState& r, const RsSenders& snd, unsigned long long cover, hipStream_t st);
// Round t: every live node with a friend calls; next and own are built from have.
hipError_t rs_round(const DevState& s, const RsState& r, uint32_t t, uint32_t grid, hipStream_t st);
// The end of round t: have |= next | own, the round buffers cleared, the per-rumor new counts and the
// holds-every-rumor set (recv); then the stats row, the count ring's slot and the stop word.
hipError_t rs_commit(const DevState& s, const RsState& r, uint32_t t, uint32_t grid, hipStream_t st);
// out[W] = bit `rumor` of every word of have.
hipError_t rs_column(const DevState& s, const RsState& r, uint32_t rumor, unsigned long long* out, hipStream_t st);

// gs_rumorset_cap.hip: a payload cap per message and late starts.
// rs_seed with starts: `now` has bit j where rumor j enters at begin; the others are live but not yet held by anyone.
hipError_t rsc_seed(const DevState& s, const RsState& r, const RsSenders& snd, unsigned long long now,
                    unsigned long long cover, hipStream_t st);
// Between a round's kernel and its commit: the rumors of `mask` enter at their senders (bits of next).
hipError_t rsc_inject(const RsState& r, const RsSenders& snd, unsigned long long mask, hipStream_t st);
// rs_round under a cap of `payload` rumors (1..64) per message, `pick` one of GS_PICK_*; adds to ctl->traffic.
hipError_t rsc_round(const DevState& s, const RsState& r, uint32_t t, uint32_t payload, uint32_t pick, uint32_t grid,
                     hipStream_t st);

}  // namespace gs
