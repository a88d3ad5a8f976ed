// gs_win_dev.h -- device helpers shared by the window engine's stages: the
// broadcast round loop as a window pipeline without global random atomics.
//
// Why windows: a Broadcast() fires off = max(delaylow,1)..delayhigh-1 ticks
// after the receipt that triggered it (simulator.go:122,142,167), so every
// broadcast firing in ticks [t0, t0+L), L <= max(delaylow,1), is already
// scheduled when tick t0 starts.  The L ticks are processed together; the
// receipts of each tick are still resolved in tick order per node.
//
// Pipeline of one window, one translation unit per stage:
//   units, groupmap, close   gs_win_units.hip
//   expand                   gs_win_expand.hip
//   plan, part2              gs_win_part.hip
//   resolve                  gs_win_resolve.hip
//   the device-driven shard layer (pack, receive layout, close)
//                            gs_win_shard.hip
// A region that overflows its estimated size is detected and the window's
// partition is redone with exact counts (expand and part2 are idempotent).
// Fire lists: fcount[R][nfine] + flist[R][nfine][16384] (u16 local ids).
#pragma once
#include <cstdlib>

#include "gossip.h"
#include "gs_internal.h"
#include "gs_wave.h"

namespace gs {
namespace {

constexpr uint32_t kExpandBlock = 256;
constexpr uint32_t kExpandBlock6 = 512;   // k_expand's workgroup for rows <= 6 slots
constexpr uint32_t kExpandNpt = 4;        // firing nodes per thread per round (rows <= 8)
constexpr uint32_t kResolveBlock = 512;
#ifndef GS_RESOLVE_WAVES
#define GS_RESOLVE_WAVES 4  // min waves per SIMD: two 512-thread workgroups per CU
#endif
// Messages: coarse = u_in_coarse | k << 22 | roll0 << 26; fine = loc | k << 14 |
// roll0 << 18, where roll0 is the receiver's crash roll for ordinal 0.
constexpr uint32_t kRoll0Coarse = kCoarseShift + 4;
constexpr uint32_t kRoll0Fine = kFineLog + 4;

// Compute units of the current device, for the persistent grids (256 if the
// query fails).  A thread-safe one-time query: contexts may run in threads.
inline uint32_t device_cus() {
  static const uint32_t cus = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      return (uint32_t)v;
    return 256u;
  }();
  return cus;
}

// Device-driven windows (w.ctl set): the window being opened starts at
// ctl->tnext and may hold up to Lw ticks (none once the run has stopped, a
// partition overflowed -- the host then redoes that window -- or tend is
// reached; never past the next poll).  0 = nothing to do.
// Error bits that stop a window: an overflow (the host redoes the window), or
// in device-driven shard windows only kErrAbort (k_rtab: some shard's window
// overflowed; a fine overflow is re-partitioned in the window itself) --
// except a single in-process shard (w.solo), which stops on any overflow as
// the unsharded engine does.
__device__ __forceinline__ uint32_t stop_bits(const WinState& w) {
  return w.dd && !w.solo ? kErrAbort : (kErrCoarse | kErrFine | kErrAbort);
}
__device__ __forceinline__ bool win_abort(const WinState& w) {
  return (*w.err & stop_bits(w)) != 0;
}
// The window control block's first 32 bytes (t, L, tnext, tend, poll, pbase,
// stop, lmax) and the error word, all loaded before any is tested: a kernel
// of a window pays one load latency for them, not a chain of dependent ones.
struct CtlView {
  uint32_t t, L, tnext, tend, poll, pbase, stop, lmax, err;
};
__device__ __forceinline__ CtlView ctl_view(const WinState& w) {
  static_assert(offsetof(WinCtl, t) == 0 && offsetof(WinCtl, lmax) == 28, "WinCtl's first 32 bytes");
  const uint4* p = reinterpret_cast<const uint4*>(w.ctl);
  const uint4 a = p[0], b = p[1];
  const uint32_t e = *w.err;
  return CtlView{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, e};
}
// (The tests are selects, not early returns: a branch on the error word would
// let the compiler sink the control-block load behind it, two latencies.)
__device__ __forceinline__ uint32_t win_open(const WinState& w, uint32_t& t) {
  const CtlView c = ctl_view(w);
  t = c.tnext;
  const bool dead = (c.err & stop_bits(w)) || c.stop || t >= c.tend;
  uint32_t Lw = min(c.lmax, c.tend - t);
  if (c.poll) {
    const uint32_t P = c.pbase + c.poll * ((t - c.pbase + c.poll - 1) / c.poll);  // next poll tick
    Lw = min(Lw, P - t + 1);
  }
  return dead ? 0u : Lw;
}
// A kernel of an opened window: its start and length (0: skip the window).
__device__ __forceinline__ uint32_t win_live(const WinState& w, uint32_t& t0, uint32_t L) {
  if (!w.ctl) return w.abort_on_err && win_abort(w) ? 0u : L;  // shards: a window that overflowed is redone
  const CtlView c = ctl_view(w);
  t0 = c.t;
  // a guarded launch (the exact fine re-partition) runs only after an overflow
  const bool off = (c.err & stop_bits(w)) || (w.guard && !(c.err & kErrFine));
  return off ? 0u : c.L;
}

// Per-tick counters are added into one of kStatShards copies (by workgroup)
// and summed into the stats ring by k_stats_reduce / k_close: thousands of
// workgroups adding into the same few lines would serialise at the
// memory-side atomic unit (32 copies take a dense window's few hundred
// thousand adds at well under one per microsecond per address).
__device__ __forceinline__ unsigned long long* shard_row(const WinState& w, uint32_t k) {
  return w.sstats + ((size_t)(blockIdx.x & (kStatShards - 1)) * kMaxWindow + k) * kStatFields;
}

// Sum of stat shard field `i` (= tick * kStatFields + field) over the
// kStatShards copies, leaving them zeroed: lane group of kCloseLanes lanes
// per field, each lane kStatShards / kCloseLanes shards with all its loads
// in flight together.
constexpr uint32_t kCloseLanes = 8;
__device__ __forceinline__ unsigned long long stat_shard_sum(const WinState& w, uint32_t i, uint32_t part) {
  constexpr uint32_t kPer = kStatShards / kCloseLanes;
  unsigned long long x[kPer], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) x[j] = w.sstats[(size_t)(j * kCloseLanes + part) * kMaxWindow * kStatFields + i];
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) {
    sum += x[j];
    if (x[j]) w.sstats[(size_t)(j * kCloseLanes + part) * kMaxWindow * kStatFields + i] = 0;
  }
#pragma unroll
  for (uint32_t o = 1; o < kCloseLanes; o <<= 1) sum += __shfl_xor(sum, o, 64);
  return sum;
}

// The counting sorts of k_expand and k_part2: off[0..256] = exclusive scan of
// the 256 bin counters, by the first wave (4 per lane).
__device__ __forceinline__ void block_scan256(uint32_t* cnt, uint32_t* off) {
  if (threadIdx.x < 64) {
    const uint32_t l = threadIdx.x;
    const uint32_t a = cnt[4 * l], b = cnt[4 * l + 1], c = cnt[4 * l + 2], d = cnt[4 * l + 3];
    const uint32_t sum = a + b + c + d;
    const uint32_t x = wave_inscan(sum);
    const uint32_t ex = x - sum;
    off[4 * l] = ex;
    off[4 * l + 1] = ex + a;
    off[4 * l + 2] = ex + a + b;
    off[4 * l + 3] = ex + a + b + c;
    if (l == 63) off[256] = x;
  }
}

// End of coarse region r, and its messages (the fill capped at its size).
__device__ __forceinline__ unsigned long long region_end(const WinState& w, uint32_t r) {
  return w.ccap_end ? w.ccap_end[r] : w.ccap[r + 1];
}
__device__ __forceinline__ unsigned long long region_fill(const WinState& w, uint32_t r) {
  const unsigned long long room = region_end(w, r) - w.ccap[r];
  return w.cfill[r] < room ? w.cfill[r] : room;
}

// Unsharded layouts deal k_part2's tiles by XCD: all tiles of coarse bin c
// go to XCD c & 7, so each fine region is written from one XCD's L2 (the
// runs of different tiles meet in whole lines there instead of in partial
// lines from eight L2s).  xcd_bin_pos(c) = the bin's place in that order.
__device__ __forceinline__ bool tiles_by_xcd(const WinState& w) {
  return w.csub == kCoarseSub && !w.csrc && !w.noxcd;
}
__device__ __forceinline__ uint32_t xcd_bin_pos(uint32_t c) { return (c & 7) * 32 + (c >> 3); }
__device__ __forceinline__ uint32_t xcd_bin_of(uint32_t pc) { return (pc & 31) * 8 + (pc >> 5); }

// receipt (fine message): loc | k << 14 | roll0 << 18
__device__ __forceinline__ uint32_t msg_loc(uint32_t m) { return m & (kFineNodes - 1); }
__device__ __forceinline__ uint32_t msg_tick(uint32_t m) { return (m >> kFineLog) & (kMaxWindow - 1); }

}  // namespace
}  // namespace gs
