// gs_win_part.hip -- the window engine's partition stage (gs_win_dev.h has the
// pipeline):
//   plan      fine-bucket regions (16384 nodes) inside each coarse region,
//             sized from the coarse count (+ margin)
//   part2     one pass per coarse tile: LDS counting sort by fine digit,
//             coalesced runs into fine regions; message = u_in_fine | k << 14
// and the exact fine re-partition of a window whose estimates overflowed.
#include <hipcub/hipcub.hpp>

#include "gs_win_dev.h"

namespace gs {
namespace {

// Fine regions inside each coarse region: capacity per fine bucket of coarse
// c = cfill[c]*1.15/256 + 512 (fast path), or exact counts (fhist != null).
__device__ __forceinline__ void plan_body(const WinState& w, bool exact) {
  __shared__ unsigned long long s_base[257];
  __shared__ unsigned long long s_cap[256];
  __shared__ uint32_t s_tp[257];
  const uint32_t tid = threadIdx.x;  // 256 threads per block: thread c plans coarse bucket c
  if (w.ctl) {
    uint32_t t0;
    if (!win_live(w, t0, 0)) return;
  }
  // messages of bucket c = the fills of its csub sub-regions (capped at their
  // size); part2 tiles never cross a sub-region
  const uint32_t csub = w.csub;
  unsigned long long cnt = 0;
  uint32_t ntile = 0;
  unsigned long long fl[kCoarseSub];  // unsharded layout (csub = 8): the fills' loads in flight together
  if (csub == kCoarseSub) {
#pragma unroll
    for (uint32_t x = 0; x < kCoarseSub; ++x) fl[x] = region_fill(w, tid * kCoarseSub + x);
#pragma unroll
    for (uint32_t x = 0; x < kCoarseSub; ++x) {
      cnt += fl[x];
      ntile += (uint32_t)((fl[x] + kPartTile - 1) / kPartTile);
    }
  } else {
    for (uint32_t x = 0; x < csub && tid * csub + x < kRegions; ++x) {
      const unsigned long long f = region_fill(w, tid * csub + x);
      cnt += f;
      ntile += (uint32_t)((f + kPartTile - 1) / kPartTile);
    }
  }
  const bool live = tid < w.ncoarse;
  // the last coarse bucket may hold fewer than 256 fine buckets
  const uint32_t nf = live ? min(256u, w.nfine - tid * 256) : 1u;
  __shared__ unsigned long long s_x[4];
  s_cap[tid] = live ? (cnt + cnt / 8 + nf - 1) / nf + 512 : 0;
  unsigned long long tb, tt;
  // the bucket's nf fine regions (a partial last bucket's were counted as
  // 256 before: its plan outgrew the host's bound R + R/8 + 513 * 256 per
  // coarse bucket, and a shard window whose fine buffer was sized by that
  // bound overflowed every time -- r04aj)
  s_base[tid] = block_exscan_u64<4>(s_cap[tid] * nf, s_x, &tb);
  s_tp[tid] = (uint32_t)block_exscan_u64<4>(live ? ntile : 0u, s_x, &tt);
  if (tid == 0) { s_base[256] = tb; s_tp[256] = (uint32_t)tt; }
  __syncthreads();
  if (blockIdx.x == 0) {  // every region < kRegions is written (256 * csub >= kRegions)
    uint32_t a = s_tp[tid];
    if (tiles_by_xcd(w)) {
      // k_part2 deals the tiles of bin c to XCD c & 7: tprefix is in the
      // order (c & 7, c >> 3, sub-region), so XCD x's tiles are one run
      __shared__ uint32_t s_pt[256];
      const uint32_t pc = xcd_bin_pos(tid);
      s_pt[pc] = live ? ntile : 0u;
      __syncthreads();
      const uint32_t mine = s_pt[tid];
      unsigned long long tot;
      const uint32_t pre = (uint32_t)block_exscan_u64<4>(mine, s_x, &tot);
      s_pt[tid] = pre;
      __syncthreads();
      a = s_pt[pc];
#pragma unroll
      for (uint32_t x = 0; x < kCoarseSub; ++x) {
        w.tprefix[pc * kCoarseSub + x] = a;
        a += live ? (uint32_t)((fl[x] + kPartTile - 1) / kPartTile) : 0u;
      }
    } else if (csub == kCoarseSub) {
#pragma unroll
      for (uint32_t x = 0; x < kCoarseSub; ++x) {
        w.tprefix[tid * kCoarseSub + x] = a;
        a += live ? (uint32_t)((fl[x] + kPartTile - 1) / kPartTile) : 0u;
      }
    } else {
      for (uint32_t x = 0; x < csub && tid * csub + x < kRegions; ++x) {
        const uint32_t r = tid * csub + x;
        w.tprefix[r] = a;
        a += live ? (uint32_t)((region_fill(w, r) + kPartTile - 1) / kPartTile) : 0u;
      }
    }
    if (tid == 255) w.tprefix[kRegions] = s_tp[256];
  }
  if (exact) return;  // fstart comes from the exact count + scan instead
  // device-driven windows: regions past the buffer are empty, and the window
  // is flagged for the host to grow the buffer and redo it
  const unsigned long long cap = w.ctl ? w.ctl->fmsg_cap : ~0ull;
  if (w.tnodes) {
    // batched trials: a coarse bucket is whole trials of bpt fine buckets, the
    // first `full` of them full, one partial (rem nodes), the rest empty (ids
    // past the trial's n); a message stays in its trial, so a fine bucket's
    // share of the coarse count is its share of the nodes, not 1/256 (the
    // uniform share under-planned every full bucket by n / 2^tlog and sent most
    // dense windows of a C3 batch to the exact redo)
    const uint32_t bpt = 1u << (w.tlog - kFineLog);
    const uint32_t full = w.tnodes >> kFineLog, rem = w.tnodes & (kFineNodes - 1);
    __syncthreads();
    if (tid < w.ncoarse) {  // s_cap[c] = one trial's capacity in bucket c
      const uint32_t nf = min(256u, w.nfine - tid * 256);
      const unsigned long long nodes = (unsigned long long)(nf / bpt) * w.tnodes;
      const unsigned long long cf = (cnt * 9 * kFineNodes + 8 * nodes - 1) / (8 * nodes) + 512;
      const unsigned long long cr = rem ? (cnt * 9 * rem + 8 * nodes - 1) / (8 * nodes) + 512 : 0;
      s_cap[tid] = full * cf + cr;
      s_tp[tid] = (uint32_t)(nf / bpt);
      s_base[tid] = cf;  // (s_base is rebuilt below)
      fl[0] = cr;
    }
    __syncthreads();
    __shared__ unsigned long long s_cf[256], s_cr[256];
    if (tid < w.ncoarse) { s_cf[tid] = s_base[tid]; s_cr[tid] = fl[0]; }
    unsigned long long tb2;
    const unsigned long long btot = tid < w.ncoarse ? s_tp[tid] * s_cap[tid] : 0ull;
    __syncthreads();
    s_base[tid] = block_exscan_u64<4>(btot, s_x, &tb2);
    if (tid == 0) s_base[256] = tb2;
    __syncthreads();
    if (w.ctl && blockIdx.x == 0 && tid == 0 && s_base[w.ncoarse] > cap) atomicOr(w.err, kErrFine);
    for (uint32_t f = blockIdx.x * blockDim.x + tid; f <= w.nfine; f += gridDim.x * blockDim.x) {
      const uint32_t c = f >> 8, d = f & 255, q = d / bpt, j = d % bpt;
      const unsigned long long x =
          f == w.nfine ? s_base[w.ncoarse]
                       : s_base[c] + q * s_cap[c] + min(j, full) * s_cf[c] + (j > full ? s_cr[c] : 0ull);
      w.fstart[f] = x < cap ? x : cap;
    }
    return;
  }
  if (w.ctl && blockIdx.x == 0 && tid == 0 && s_base[w.ncoarse] > cap) atomicOr(w.err, kErrFine);
  for (uint32_t f = blockIdx.x * blockDim.x + tid; f <= w.nfine; f += gridDim.x * blockDim.x) {
    const uint32_t c = f >> 8, d = f & 255;
    const unsigned long long x = f == w.nfine ? s_base[w.ncoarse] : s_base[c] + d * s_cap[c];
    w.fstart[f] = x < cap ? x : cap;
  }
}
__global__ void k_plan(const WinState w, bool exact) { plan_body(w, exact); }
__global__ void k_plan_m(const WinState* __restrict__ ws, bool exact) { plan_body(ws[blockIdx.y], exact); }

// LDS counting sort of one tile by an 8-bit digit, then coalesced runs out.
#ifndef GS_PART_BLOCK
#define GS_PART_BLOCK 1024
#endif
constexpr uint32_t kPartBlock = GS_PART_BLOCK;  // threads per partition tile (16 messages each)
static_assert(kPartTile % kPartBlock == 0, "whole messages per thread");

// The tile holds coarse messages as they came: the fine digit (bits 14..21) is
// re-read at write-out, so there is no per-slot bin byte (64 KB: two tiles/CU).
struct TileSort {
  uint32_t buf[kPartTile];
  uint32_t cnt[256];
  uint32_t off[257];
  unsigned long long gbase[256];  // digit b's message p goes to gbase[b] + p
  unsigned long long gend[256];  // end of fine region b (fstart[c*256 + b + 1])
  uint32_t ovf;                  // a fine region of this tile overflowed
};

// part2: coarse tiles -> fine regions; message = u_in_fine | k << 14.
// SCATTER=false counts per fine bucket (exact fallback).
template <bool SCATTER>
__device__ __forceinline__ void part2_body(const WinState& w) {
  __shared__ TileSort ts;
  __shared__ uint32_t s_tp[kRegions + 1];
  const uint32_t tid = threadIdx.x;
  if (w.ctl) {
    uint32_t t0;
    if (!win_live(w, t0, 0)) return;
  }
  // a sparse window has few tiles: the workgroups past them leave before
  // staging the 8-KB tile prefix (the grid is sized for the densest window)
  const bool perm = tiles_by_xcd(w);
  uint32_t g0 = blockIdx.x, g1 = w.tprefix[kRegions], gstep = gridDim.x;
  if (perm && (gridDim.x & 7) == 0) {  // XCD x = blockIdx & 7 takes its bins' tiles
    const uint32_t x = blockIdx.x & 7;
    g0 = w.tprefix[x * 256] + (blockIdx.x >> 3);
    g1 = w.tprefix[(x + 1) * 256];
    gstep = gridDim.x >> 3;
  }
  if (g0 >= g1) return;
  for (uint32_t i = tid; i <= kRegions; i += kPartBlock) s_tp[i] = w.tprefix[i];
  __syncthreads();
  for (uint32_t g = g0; g < g1; g += gstep) {
    uint32_t lo = 0, hi = kRegions - 1;  // tile-order position rho: s_tp[rho] <= g < s_tp[rho+1]
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (s_tp[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const uint32_t rho = lo;
    const uint32_t r = perm ? xcd_bin_of(rho / kCoarseSub) * kCoarseSub + rho % kCoarseSub : rho;
    const uint32_t c = r / w.csub;
    unsigned long long cb = w.ccap[r];
    const uint32_t* msrc = w.cmsg;  // the region's messages (a receive layout names their buffer)
    if (w.csrc) {
      msrc = w.csrc[cb >> kSrcShift];
      cb &= kSrcMask;
    }
    const unsigned long long ce = cb + region_fill(w, r);
    const unsigned long long base = cb + (unsigned long long)(g - s_tp[rho]) * kPartTile;
    if (tid < 256) ts.cnt[tid] = 0;
    __syncthreads();
    if (tid == 0) ts.ovf = 0;
    constexpr uint32_t kPer = kPartTile / kPartBlock;
    static_assert(kPartTile <= 65536 && kPer % 2 == 0, "two 16-bit ranks per register");
    uint32_t m[kPer], rank[kPer / 2] = {};
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
      const unsigned long long x = base + r * kPartBlock + tid;
      // branch-free load (index clamped into the tile's region: base < ce)
      const uint32_t m1 = msrc[x < ce ? x : ce - 1];
      m[r] = x < ce ? m1 : kEmptyMsg;
    }
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r)
      if (m[r] != kEmptyMsg) rank[r / 2] |= atomicAdd(&ts.cnt[(m[r] >> kFineLog) & 255], 1u) << (16 * (r & 1));
    __syncthreads();
    if (!SCATTER) {
      if (tid < 256 && ts.cnt[tid]) atomicAdd(&w.fhist[c * 256 + tid], (unsigned long long)ts.cnt[tid]);
      __syncthreads();
      continue;
    }
    block_scan256(ts.cnt, ts.off);
    // thread b < 256 reserves fine bucket c*256+b's run; the atomic's return
    // latency overlaps the LDS scatter (which needs only off[] from the scan)
    const uint32_t mycnt = tid < 256 ? ts.cnt[tid] : 0u;
    const uint32_t myf = c * 256 + (tid & 255);
    unsigned long long at = 0, fb = 0, fe = 0;
    if (mycnt) {
      at = atomicAdd(&w.ffill[myf], (unsigned long long)mycnt);
      fb = w.fstart[myf];
      fe = w.fstart[myf + 1];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r)
      if (m[r] != kEmptyMsg) {
        ts.buf[ts.off[(m[r] >> kFineLog) & 255] + ((rank[r / 2] >> (16 * (r & 1))) & 0xFFFFu)] = m[r];
        if ((m[r] >> kRoll0Coarse) & 1u) {  // a crash roll: its node is special in k_resolve
          const uint32_t v = (c << kCoarseShift) | (m[r] & ((1u << kCoarseShift) - 1));
          atomicOr(&w.rollw[v >> 5], 1u << (v & 31));
        }
      }
    if (mycnt) {
      if (at + mycnt > fe - fb) {
        atomicOr(w.err, kErrFine);
        ts.ovf = 1;
      }
      ts.gbase[tid] = fb + at - ts.off[tid];
      ts.gend[tid] = fe;
    }
    __syncthreads();
    const uint32_t total = ts.off[256];
    // two LDS reads per message; the region bound is checked only in a tile
    // whose reservation overflowed (the window is then redone exactly)
    if (!ts.ovf) {
      for (uint32_t p = tid; p < total; p += kPartBlock) {
        const uint32_t m1 = ts.buf[p];
        w.fmsg[ts.gbase[(m1 >> kFineLog) & 255] + p] = (m1 & (kFineNodes - 1)) | ((m1 >> kCoarseShift) << kFineLog);
      }
    } else {
      for (uint32_t p = tid; p < total; p += kPartBlock) {
        const uint32_t m1 = ts.buf[p], b = (m1 >> kFineLog) & 255;
        const unsigned long long pos = ts.gbase[b] + p;
        if (pos < ts.gend[b]) w.fmsg[pos] = (m1 & (kFineNodes - 1)) | ((m1 >> kCoarseShift) << kFineLog);
      }
    }
    __syncthreads();
  }
}
template <bool SCATTER>
__global__ __launch_bounds__(kPartBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part2(const WinState w) {
  part2_body<SCATTER>(w);
}
template <bool SCATTER>
__global__ __launch_bounds__(kPartBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part2_m(
    const WinState* __restrict__ ws) {
  part2_body<SCATTER>(ws[blockIdx.y]);
}

// The exact fine re-partition of a device-driven shard window whose fine
// regions overflowed their estimates (kErrFine): the counts cleared (here),
// k_plan's tile prefix, k_part2's counting pass, the scan into fstart
// (k_fine_scan), k_part2's scatter.  Guarded launches (w.guard): they do
// nothing unless the shard's kErrFine is set; k_stats_dd clears it.
__device__ __forceinline__ void fine_zero_body(const WinState& w) {
  uint32_t t0;
  if (!win_live(w, t0, 0)) return;
  const uint32_t nh = w.ncoarse * 256 + 1;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nh; i += gridDim.x * blockDim.x) {
    w.fhist[i] = 0;
    if (i < w.nfine) w.ffill[i] = 0;
  }
}
__global__ void k_fine_zero(const WinState w) { fine_zero_body(w); }
__global__ void k_fine_zero_m(const WinState* __restrict__ ws) { fine_zero_body(ws[blockIdx.y]); }

__device__ __forceinline__ void fine_scan_body(const WinState& w) {
  __shared__ unsigned long long s_x[16];
  uint32_t t0;
  if (!win_live(w, t0, 0)) return;
  const uint32_t n = w.nfine + 1, per = (n + 1023) / 1024, tid = threadIdx.x;
  unsigned long long sum = 0;
  for (uint32_t j = 0; j < per; ++j) {
    const uint32_t i = tid * per + j;
    if (i < n) sum += w.fhist[i];
  }
  unsigned long long tot;
  unsigned long long a = block_exscan_u64<16>(sum, s_x, &tot);
  for (uint32_t j = 0; j < per; ++j) {
    const uint32_t i = tid * per + j;
    if (i >= n) break;
    w.fstart[i] = a;
    a += w.fhist[i];
    if (i < w.nfine) w.ffill[i] = 0;
  }
}
__global__ __launch_bounds__(1024) void k_fine_scan(const WinState w) { fine_scan_body(w); }
__global__ __launch_bounds__(1024) void k_fine_scan_m(const WinState* __restrict__ ws) {
  fine_scan_body(ws[blockIdx.x]);
}

}  // namespace

hipError_t win_plan(const WinState& w, bool exact, hipStream_t s) {
  const uint32_t blocks = std::min<uint32_t>((w.nfine + 1 + 255) / 256, 1024);
  hipLaunchKernelGGL(k_plan, dim3(blocks), dim3(256), 0, s, w, exact);
  return hipGetLastError();
}

// GS_PART2_GRID=<workgroups> (read once per process; 0 = unset): the grid of
// every k_part2 launch, the guarded redo's count and scatter included, so
// tests can make a workgroup take several tiles of a small window.  A multiple
// of 8 keeps the tiles dealt by XCD; any other value strides the whole list.
static uint32_t part2_grid_env() {
  static const uint32_t g = [] { const char* e = getenv("GS_PART2_GRID"); return e ? (uint32_t)std::max(atoi(e), 1) : 0u; }();
  return g;
}
// the guarded redo's count and scatter grids
static uint32_t redo_grid() { return part2_grid_env() ? part2_grid_env() : 512u; }

hipError_t win_part2(const WinState& w, uint64_t T, bool scatter, hipStream_t s) {
  const uint64_t tiles = (T + kPartTile - 1) / kPartTile + 256;
  uint32_t blocks = (uint32_t)(std::min<uint64_t>(tiles, 8192) + 7) & ~7u;  // a multiple of 8: tiles by XCD
  if (part2_grid_env()) blocks = part2_grid_env();
  if (scatter) hipLaunchKernelGGL(k_part2<true>, dim3(blocks), dim3(kPartBlock), 0, s, w);
  else hipLaunchKernelGGL(k_part2<false>, dim3(blocks), dim3(kPartBlock), 0, s, w);
  return hipGetLastError();
}

hipError_t win_scan_fine(const WinState& w, void* tmp, size_t& tmp_bytes, hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, (const unsigned long long*)w.fhist,
                                          w.fstart, (int)(w.nfine + 1), s);
}

hipError_t win_fine_redo(const WinState& w, uint64_t /*T*/, hipStream_t s) {  // (fixed grids: T is not used)
  WinState g = w;
  g.guard = 1;
  // small persistent grids: when nothing overflowed (nearly always) each launch
  // only reads the control block and leaves
  hipLaunchKernelGGL(k_fine_zero, dim3(64), dim3(256), 0, s, g);
  hipLaunchKernelGGL(k_plan, dim3(1), dim3(256), 0, s, g, true);
  hipLaunchKernelGGL(k_part2<false>, dim3(redo_grid()), dim3(kPartBlock), 0, s, g);
  hipLaunchKernelGGL(k_fine_scan, dim3(1), dim3(1024), 0, s, g);
  hipLaunchKernelGGL(k_part2<true>, dim3(redo_grid()), dim3(kPartBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t win_recv_g(const WinGroup& g, uint64_t T, hipStream_t s) {
  const uint32_t pblocks = std::min<uint32_t>((g.nfine_max + 1 + 255) / 256, 1024);
  hipLaunchKernelGGL(k_plan_m, dim3(pblocks, g.M), dim3(256), 0, s, g.wr, false);
  const uint64_t tiles = (T + kPartTile - 1) / kPartTile + 256;
  uint32_t blocks = (uint32_t)(std::min<uint64_t>(tiles, 8192) + 7) & ~7u;
  if (part2_grid_env()) blocks = part2_grid_env();
  hipLaunchKernelGGL(k_part2_m<true>, dim3(blocks, g.M), dim3(kPartBlock), 0, s, g.wr);
  // the guarded exact redo (win_fine_redo): each launch leaves at once unless
  // its shard's fine regions overflowed
  hipLaunchKernelGGL(k_fine_zero_m, dim3(64, g.M), dim3(256), 0, s, g.wg);
  hipLaunchKernelGGL(k_plan_m, dim3(1, g.M), dim3(256), 0, s, g.wg, true);
  hipLaunchKernelGGL(k_part2_m<false>, dim3(redo_grid(), g.M), dim3(kPartBlock), 0, s, g.wg);
  hipLaunchKernelGGL(k_fine_scan_m, dim3(g.M), dim3(1024), 0, s, g.wg);
  hipLaunchKernelGGL(k_part2_m<true>, dim3(redo_grid(), g.M), dim3(kPartBlock), 0, s, g.wg);
  return hipGetLastError();
}

}  // namespace gs
