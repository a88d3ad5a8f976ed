// gs_win_shard.hip -- the window engine's shard layer.
//
// Node-range shards (config C4):
// Shard r of G owns nodes [r * seg_per, min((r+1) * seg_per, N)) and their
// friend rows.  Every window it expands its OWN firing nodes with k_expand in
// owner mode: a kept message is binned by the shard that owns its target
// (bin = owner * obins + 2^22-node chunk of the owner's range), so the
// coarse regions of owner d are one contiguous block of the message buffer.
// k_pack moves the filled prefixes of each block that leaves the device or
// rank back to back; the blocks go to their owners (all-to-all); each shard
// then partitions (k_plan / k_part2 over the receive layout: G senders x 8
// sub-regions per bin, each region in its sender's buffer read in place or in
// the received blocks) and resolves its own buckets with the resolve stage's
// kernels.  Keys are global ids, so the union over shards equals the
// unsharded run bit for bit.
#include "gs_win_dev.h"

namespace gs {
namespace {

// out[poff[r] ..] = the filled prefix of region r (< nreg), one region per
// blockIdx.x, blockIdx.y strided over it.
__global__ void k_pack(const WinState w, const unsigned long long* poff, uint32_t nreg, uint32_t* out) {
  const uint32_t r = blockIdx.x;
  if (r >= nreg || poff[r] == ~0ull) return;
  if (w.dd && (*w.err & kErrAbort)) return;  // device-driven shard window that some shard overflowed
  const unsigned long long f = region_fill(w, r);
  const uint32_t* src = w.cmsg + w.ccap[r];
  uint32_t* dst = out + poff[r];
  for (unsigned long long i = (unsigned long long)blockIdx.y * blockDim.x + threadIdx.x; i < f;
       i += (unsigned long long)gridDim.y * blockDim.x)
    dst[i] = src[i];
}

// Shards: the window's fire lists are consumed right after the expand (and
// its exact sender redo, which clears the coarse flag first); nothing later
// reads them -- a receive-side redo (receiver_redo) re-partitions and
// resolves the received messages only -- so the consume is unconditional.
__global__ void k_consume_sh(const WinState w, uint32_t t0, uint32_t L) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < L * w.nfine; i += gridDim.x * blockDim.x) {
    const uint32_t k = i / w.nfine, f = i - k * w.nfine;
    w.fcount[(size_t)((t0 + k) % w.R) * w.nfine + f] = 0;
  }
}

// ---- device-driven shard windows ------------------
// The host-driven shard window (gs_shards.cpp shard_windows) reads every shard's
// fire counts and region fills on the host to cut the window and lay out the
// receive side.  Here the counts and fills are gathered into device buffers
// (RCCL all-gathers between ranks; the shards of one device share them), every
// shard cuts the same window (k_cut over the gathered counts) and computes its
// own receive layout (k_rtab), so a window needs no host round trip unless
// its blocks travel between ranks (the host then reads the block sizes for
// the grouped send / receive).

// Shard w.rank's receive layout from the gathered fills: the region starts,
// ends and fills of (bin c, sender s, sub-region x) at (c * G + s) * 8 + x, its
// own pack offsets, the source buffers and the window's received messages --
// what shard_exchange lays out on the host.  Every shard's row also carries
// its overflow flag and fine-buffer capacity: if any shard's expand overflowed
// a region estimate, or any shard would receive more messages than its fine
// buffer holds, every shard sets kErrAbort (the same decision everywhere,
// from the same gathered rows) and the host redoes the window host-driven.
// One block of 256 threads.
__device__ __forceinline__ void rtab_body(const WinState& w, unsigned long long* rtab,
                                          const unsigned long long* const* ccaps, const uint32_t* const* src,
                                          uint32_t nsrc, uint32_t travels) {
  __shared__ unsigned long long s_x[4];
  __shared__ unsigned long long s_R[256];
  __shared__ uint32_t s_abort;
  const uint32_t tid = threadIdx.x;
  uint32_t t0;
  if (!win_live(w, t0, 0)) return;
  const uint32_t G = w.G, me = w.rank, B8 = w.obins * kCoarseSub, nreg = G * B8;
  constexpr size_t K1 = kRegions + 1;
  // the f[8] staging below covers 8 regions per thread: nreg <= 8 * 256 =
  // kRegions, which ctx_setup's shard check (G * bins <= 256) guarantees; a
  // wider layout stops the window instead of dropping regions
  static_assert(kRegions == 8 * 256, "eight regions per thread");
  if (nreg > kRegions) {
    if (tid == 0) atomicOr(w.err, kErrAbort);
    return;
  }
  unsigned long long *rcap = rtab, *rend = rtab + K1, *rfill = rtab + 2 * K1, *mypoff = rtab + 3 * K1;
  s_R[tid] = 0;
  if (tid == 0) s_abort = 0;
  __syncthreads();
  uint32_t fl = 0;
  for (uint32_t s = tid; s < G; s += 256) fl |= (uint32_t)w.glay[(size_t)s * kDDRow + kRegions];
  if (fl & (kErrCoarse | kErrAbort)) atomicOr(&s_abort, 1u);
  for (uint32_t s = 0; s < G; ++s) {
    const unsigned long long* row = w.glay + (size_t)s * kDDRow;
    for (uint32_t r = tid; r < nreg; r += 256) {
      const unsigned long long f = row[r];
      if (f) atomicAdd(&s_R[r / B8], f);
    }
  }
  __syncthreads();
  for (uint32_t d = tid; d < G; d += 256) {  // shard d's fine plan bound (shard_receive's fcap) vs its buffer
    const unsigned long long lo = (unsigned long long)d * w.seg_per;
    const unsigned long long nd = min((unsigned long long)w.seg_per, (unsigned long long)w.nglob - lo);
    const unsigned long long ncd = (((nd + kFineNodes - 1) >> kFineLog) + 255) / 256;
    const unsigned long long R = s_R[d];
    if (R + R / 8 + ncd * 256 * 513 + 16 > w.glay[(size_t)d * kDDRow + kRegions + 1]) atomicOr(&s_abort, 2u);
  }
  __syncthreads();
  if (s_abort) {
    if (tid == 0) atomicOr(w.err, kErrAbort);
    return;
  }
  for (uint32_t rr = tid; rr < K1; rr += 256) {
    rcap[rr] = rend[rr] = rfill[rr] = 0;
    mypoff[rr] = ~0ull;
  }
  __syncthreads();
  // region (c, s, x) of the blocks for this shard: in place in sender s's
  // buffer (its region start), or in the received blocks at the sender's
  // block offset plus the fills before it inside the block
  const uint32_t in_src = travels ? 0u : G;
  const uint32_t per = (B8 + 255) / 256;  // <= 8 (B8 <= kRegions)
  unsigned long long in_s = 0, tot = 0;
  for (uint32_t s = 0; s < G; ++s) {
    const bool tr = travels && s != me;
    const unsigned long long* row = w.glay + (size_t)s * kDDRow + (size_t)me * B8;
    const unsigned long long* cc = ccaps[travels ? 0u : s] + (size_t)me * B8;
    unsigned long long f[8], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t i = tid * per + j;
      f[j] = j < per && i < B8 ? row[i] : 0ull;
      sum += f[j];
    }
    unsigned long long btot;
    unsigned long long off = block_exscan_u64<4>(sum, s_x, &btot);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t i = tid * per + j;
      if (j >= per || i >= B8) continue;
      const uint32_t c = i / kCoarseSub, x = i % kCoarseSub;
      const size_t rr = ((size_t)c * G + s) * kCoarseSub + x;
      const unsigned long long at = tr ? ((unsigned long long)in_src << kSrcShift) | (in_s + off)
                                       : ((unsigned long long)(travels ? 1u : s) << kSrcShift) | cc[i];
      rcap[rr] = at;
      rend[rr] = at + f[j];
      rfill[rr] = f[j];
      off += f[j];
    }
    if (tr) in_s += btot;
    tot += btot;
  }
  if (travels) {  // this shard's own blocks that leave, back to back in region order (k_pack)
    const unsigned long long* row = w.glay + (size_t)me * kDDRow;
    const uint32_t per2 = (nreg + 255) / 256;
    unsigned long long f[8], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t r = tid * per2 + j;
      f[j] = j < per2 && r < nreg && r / B8 != me ? row[r] : 0ull;
      sum += f[j];
    }
    unsigned long long btot;
    unsigned long long off = block_exscan_u64<4>(sum, s_x, &btot);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t r = tid * per2 + j;
      if (j >= per2 || r >= nreg || r / B8 == me) continue;
      mypoff[r] = off;
      off += f[j];
    }
  }
  if (tid < nsrc) rtab[4 * K1 + tid] = (unsigned long long)(uintptr_t)src[tid];
  if (tid == 0) rtab[kRtabTotal] = tot;
}
__global__ __launch_bounds__(256) void k_rtab(const WinState w, unsigned long long* rtab,
                                              const unsigned long long* const* ccaps, const uint32_t* const* src,
                                              uint32_t nsrc, uint32_t travels) {
  rtab_body(w, rtab, ccaps, src, nsrc, travels);
}
// shard blockIdx.x's layout goes to its receive state's region table (wr.ccap)
__global__ __launch_bounds__(256) void k_rtab_m(const WinState* __restrict__ ws, const WinState* __restrict__ wr,
                                                const unsigned long long* const* ccaps, const uint32_t* const* src,
                                                uint32_t nsrc) {
  rtab_body(ws[blockIdx.x], const_cast<unsigned long long*>(wr[blockIdx.x].ccap), ccaps, src, nsrc, 0u);
}

// The close of a device-driven shard window from its summed counter rows
// (F = kMaxWindow * kStatFields counters, then the flags): gs_run's poll rule
// (simulator.go:243-248, as k_close) on every shard's control block, and
// staging slot `slot` for the host.  Block-wide (tid 0 applies the rule).
__device__ void close_rows(const WinState& w, const unsigned long long* rows, WinCtl* const* ctls, uint32_t n,
                           uint32_t slot) {
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t F = kMaxWindow * kStatFields;
  const WinCtl* c0 = ctls[0];
  const bool dead = rows[F + 2] != 0;
  const uint32_t t0 = c0->t, L = dead || c0->stop ? 0u : c0->L;
  unsigned long long* st = w.stage + (size_t)slot * kStageWords;
  for (uint32_t i = tid; i < F; i += blockDim.x) st[8 + i] = i / kStatFields < L ? rows[i] : 0ull;
  if (tid != 0) return;
  uint32_t stop = c0->stop;
  if (L) {
    unsigned long long recv = c0->recv, crashed = c0->crashed, pending = c0->pending;
    for (uint32_t j = 0; j < L; ++j) {
      recv += rows[j * kStatFields + ST_RECV];
      crashed += rows[j * kStatFields + ST_CRASH];
      pending += rows[j * kStatFields + ST_SCHED] - rows[j * kStatFields + ST_FIRED];
    }
    const uint32_t tl = t0 + L - 1;  // windows never cross a poll tick
    if (c0->poll && (tl - c0->pbase) % c0->poll == 0 && !stop) {
      if (recv >= c0->cover) stop = 1 + GS_RUN_COVERED;
      else if (pending == 0) stop = 1 + GS_RUN_QUIESCENT;
      else if (tl >= c0->max_ticks) stop = 1 + GS_RUN_MAX_TICKS;
    }
    for (uint32_t q = 0; q < n; ++q) {
      WinCtl* c = ctls[q];
      c->recv = recv;
      c->crashed = crashed;
      c->pending = pending;
      c->stop = stop;
    }
  }
  st[0] = t0;
  st[1] = L;
  st[2] = stop;
  st[3] = (dead ? kErrAbort : 0u) | (rows[F] ? kErrArrivals : 0u);
  st[4] = rows[F + 1];  // exact fine re-partitions in the window
}

// The window's counters of this shard (its stat shards summed into w.wstat,
// zero rows past the window or in a stopped one) and its flags: kErrArrivals,
// an exact fine re-partition (kErrFine, cleared here), kErrAbort.  A single
// in-process shard (w.solo) closes its window here too (close_rows), one
// launch instead of two.
// kMaxWindow * kStatFields * kCloseLanes threads.
__device__ __forceinline__ void stats_dd_body(const WinState& w, uint32_t slot) {
  __shared__ unsigned long long rows[kDDWStat];  // w.solo: closed here (no k_close_dd)
  const uint32_t tid = threadIdx.x;
  const CtlView c = ctl_view(w);
  const bool dead = (c.err & stop_bits(w)) != 0;
  const uint32_t L = dead || c.stop ? 0u : c.L;
  const uint32_t i = tid / kCloseLanes, part = tid % kCloseLanes, k = i / kStatFields;
  unsigned long long sum = 0;
  if (k < L) sum = stat_shard_sum(w, i, part);  // k is uniform over each lane group
  if (part == 0) {
    w.wstat[i] = sum;
    rows[i] = sum;
  }
  if (tid < 8) {
    constexpr uint32_t F = kMaxWindow * kStatFields;
    unsigned long long v = 0;
    if (tid == 0) v = (c.err & kErrArrivals) ? 1 : 0;
    if (tid == 1) v = !w.solo && (c.err & kErrFine) ? 1 : 0;
    if (tid == 2) v = dead ? 1 : 0;
    w.wstat[F + tid] = v;
    rows[F + tid] = v;
  }
  if (tid == 0 && !w.solo && (c.err & kErrFine)) atomicAnd(w.err, ~kErrFine);
  if (!w.solo) return;
  __syncthreads();
  WinCtl* const one[1] = {w.ctl};
  close_rows(w, rows, one, 1, slot);
}
__global__ void k_stats_dd(const WinState w, uint32_t slot) { stats_dd_body(w, slot); }
__global__ void k_stats_dd_m(const WinState* __restrict__ ws, uint32_t slot) { stats_dd_body(ws[blockIdx.x], slot); }

// The close of a device-driven shard window: the window's global counters
// (the sum of the n shards' wstat: the group's shards, or this rank's own
// after the all-reduce), then close_rows.  One block of 128 threads.
__global__ __launch_bounds__(128) void k_close_dd(const WinState w, const unsigned long long* const* wstats,
                                                  WinCtl* const* ctls, uint32_t n, uint32_t slot) {
  __shared__ unsigned long long rows[kDDWStat];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kDDWStat; i += blockDim.x) {
    unsigned long long v = 0;
    for (uint32_t q = 0; q < n; ++q) v += wstats[q][i];
    rows[i] = v;
  }
  __syncthreads();
  close_rows(w, rows, ctls, n, slot);
}

}  // namespace

hipError_t win_rtab(const WinState& w, unsigned long long* rtab, const unsigned long long* const* ccaps,
                    const uint32_t* const* src, uint32_t nsrc, uint32_t travels, hipStream_t s) {
  hipLaunchKernelGGL(k_rtab, dim3(1), dim3(256), 0, s, w, rtab, ccaps, src, nsrc, travels);
  return hipGetLastError();
}

hipError_t win_stats_dd(const WinState& w, uint32_t slot, hipStream_t s) {
  hipLaunchKernelGGL(k_stats_dd, dim3(1), dim3(kMaxWindow * kStatFields * kCloseLanes), 0, s, w, slot);
  return hipGetLastError();
}

hipError_t win_close_dd(const WinState& w, const unsigned long long* const* wstats, WinCtl* const* ctls,
                        uint32_t n, uint32_t slot, hipStream_t s) {
  hipLaunchKernelGGL(k_close_dd, dim3(1), dim3(128), 0, s, w, wstats, ctls, n, slot);
  return hipGetLastError();
}

hipError_t win_rtab_g(const WinGroup& g, const unsigned long long* const* ccaps, const uint32_t* const* src,
                      uint32_t nsrc, hipStream_t s) {
  hipLaunchKernelGGL(k_rtab_m, dim3(g.M), dim3(256), 0, s, g.ws, g.wr, ccaps, src, nsrc);
  return hipGetLastError();
}

hipError_t win_stats_dd_g(const WinGroup& g, uint32_t slot, hipStream_t s) {
  hipLaunchKernelGGL(k_stats_dd_m, dim3(g.M), dim3(kMaxWindow * kStatFields * kCloseLanes), 0, s, g.ws, slot);
  return hipGetLastError();
}

hipError_t win_consume_sh(const WinState& w, uint32_t t0, uint32_t L, hipStream_t s) {
  const uint32_t blocks = std::min<uint32_t>((L * w.nfine + 255) / 256, 2048);
  hipLaunchKernelGGL(k_consume_sh, dim3(blocks ? blocks : 1), dim3(256), 0, s, w, t0, L);
  return hipGetLastError();
}

hipError_t win_pack(const WinState& w, const unsigned long long* poff, uint32_t nreg, uint32_t* out, hipStream_t s) {
  if (!nreg) return hipSuccess;
  hipLaunchKernelGGL(k_pack, dim3(nreg, 8), dim3(256), 0, s, w, poff, nreg, out);
  return hipGetLastError();
}

}  // namespace gs
