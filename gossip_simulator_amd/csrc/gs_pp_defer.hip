// gs_pp_defer.hip -- push-pull: the pull-answer rounds' deferred sets
// (PPSparse::dset, gs_internal.h).  k_ppa_round (gs_pp_round.hip) appends the
// nodes it informs to per-workgroup lists; here they are partitioned twice in
// LDS and ORed into `next` a 16384-node bucket at a time.
#include "gs_pp_dev.h"

namespace gs {
namespace {

// ---- deferred sets: coarse and fine LDS partitions, then the bitmap OR ----
constexpr uint32_t kPPDTile = 16384;   // set targets per partition tile
constexpr uint32_t kPPDBlock = 1024;   // 16 per thread

// Exclusive scan of cnt[0..256) into off[0..257) by the first 256 threads
// (block-uniform call; every thread passes the barriers).
__device__ __forceinline__ void ppd_scan256(const uint32_t* cnt, uint32_t* off, uint32_t* s_w) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t v = tid < 256 ? cnt[tid] : 0u, x = wave_inscan(v);
  if (tid < 256 && lane == 63) s_w[wv] = x;
  __syncthreads();
  if (tid < 256) {
    uint32_t pre = 0;
    for (uint32_t q = 0; q < wv; ++q) pre += s_w[q];
    off[tid] = pre + x - v;
    if (tid == 255) off[256] = pre + x;
  }
  __syncthreads();
}

// One partition pass: tiles of the `nsrc` input lists (list L holds
// min(fill[L], cap_in) targets at in + L * cap_in) are counting-sorted in LDS
// by the 8-bit digit (x >> shift) & 255 and leave as runs: coarse pass (shift
// 22) into region digit * 8 + (blockIdx & 7) of `out`, fine pass (shift 14)
// into fine bucket (region's bin) * 256 + digit; one reservation per (tile,
// digit); what does not fit its region is an atomicOr into next.
template <bool FINE>
__global__ __launch_bounds__(kPPDBlock) void k_ppd_part(const PPSparse sp, unsigned long long* __restrict__ next,
                                                        const uint32_t* in, const unsigned long long* fill,
                                                        uint32_t nsrc, uint64_t cap_in, uint32_t* out,
                                                        unsigned long long* ofill, uint64_t cap_out) {
  if (sp.ctl->mode != PP_ANSWER) return;
  __shared__ uint32_t buf[kPPDTile];
  __shared__ uint32_t cnt[256], off[257], s_w[4];
  __shared__ unsigned long long gb[256], ge[256];
  constexpr uint32_t kPer = kPPDTile / kPPDBlock;
  constexpr uint32_t shift = FINE ? 14 : 22;
  const uint32_t tid = threadIdx.x;
  const uint64_t nch = (cap_in + kPPDTile - 1) / kPPDTile;
  for (uint64_t tt = blockIdx.x; tt < nsrc * nch; tt += gridDim.x) {
    const uint32_t L = (uint32_t)(tt % nsrc);
    const uint64_t ch = tt / nsrc;
    const unsigned long long fl = fill[L];
    const uint64_t n = fl < cap_in ? fl : cap_in, b0 = ch * kPPDTile;
    if (b0 >= n) continue;  // block-uniform
    const uint32_t m = (uint32_t)min((uint64_t)kPPDTile, n - b0);
    if (tid < 256) cnt[tid] = 0;
    __syncthreads();
    uint32_t x[kPer], rk[kPer];
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
      const uint32_t i = r * kPPDBlock + tid;
      x[r] = i < m ? in[L * cap_in + b0 + i] : ~0u;
      rk[r] = x[r] != ~0u ? atomicAdd(&cnt[(x[r] >> shift) & 255], 1u) : 0u;
    }
    __syncthreads();
    ppd_scan256(cnt, off, s_w);
    if (tid < 256 && cnt[tid]) {
      const uint64_t reg = FINE ? (uint64_t)(L / 8) * 256 + tid : (uint64_t)tid * 8 + (blockIdx.x & 7);
      const unsigned long long at = atomicAdd(&ofill[reg], (unsigned long long)cnt[tid]);
      gb[tid] = reg * cap_out + at - off[tid];
      ge[tid] = reg * cap_out + cap_out;
    }
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r)
      if (x[r] != ~0u) buf[off[(x[r] >> shift) & 255] + rk[r]] = x[r];
    __syncthreads();
    for (uint32_t p = tid; p < m; p += kPPDBlock) {
      const uint32_t v = buf[p], dg = (v >> shift) & 255;
      const unsigned long long pos = gb[dg] + p;
      if (pos < ge[dg]) out[pos] = FINE ? (v & ((1u << 14) - 1)) : v;
      else atomicOr(&next[v >> 6], 1ull << (v & 63));
    }
    __syncthreads();
  }
}

// One workgroup per 16384-node bucket f: its fine region's targets into an
// LDS bitmap, ORed into its 256 words of next (this workgroup alone writes
// them; the fallback atomics ran in the kernels before).
__global__ __launch_bounds__(256) void k_ppd_apply(const PPSparse sp, unsigned long long* __restrict__ next,
                                                   uint64_t W, uint32_t nfine) {
  if (sp.ctl->mode != PP_ANSWER) return;
  __shared__ uint32_t bm[512];
  const unsigned long long* ffill = sp.dcnt + kPPDLists + kPPDRegions;
  const uint32_t* fine = sp.dset + (size_t)kPPDLists * sp.dcap + (size_t)kPPDRegions * sp.ccap;
  for (uint32_t f = blockIdx.x; f < nfine; f += gridDim.x) {
    const unsigned long long fl = ffill[f];
    const uint32_t n = (uint32_t)(fl < sp.fcap ? fl : sp.fcap);
    if (!n) continue;  // block-uniform
    bm[threadIdx.x] = 0;
    bm[threadIdx.x + 256] = 0;
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < n; p += 256) {
      const uint32_t loc = fine[(size_t)f * sp.fcap + p];
      atomicOr(&bm[loc >> 5], 1u << (loc & 31));
    }
    __syncthreads();
    const uint64_t w = (uint64_t)f * 256 + threadIdx.x;
    const unsigned long long v = (unsigned long long)bm[2 * threadIdx.x] |
                                 ((unsigned long long)bm[2 * threadIdx.x + 1] << 32);
    if (v && w < W) next[w] |= v;
    __syncthreads();
  }
}
}  // namespace

void pp_launch_deferred(const DevState& s, unsigned long long* next, const PPSparse& sp, uint32_t nlists,
                        hipStream_t st) {
  if (sp.dset) {  // no-ops unless the round is pull-answer
    const uint32_t nfine = (uint32_t)((s.n + 16383) >> 14);
    uint32_t* coarse = sp.dset + (size_t)kPPDLists * sp.dcap;
    uint32_t* fine = coarse + (size_t)kPPDRegions * sp.ccap;
    unsigned long long* cfill = sp.dcnt + kPPDLists;
    hipLaunchKernelGGL(k_ppd_part<false>, dim3(1024), dim3(kPPDBlock), 0, st, sp, next, sp.dset, sp.dcnt,
                       nlists, sp.dcap, coarse, cfill, sp.ccap);
    hipLaunchKernelGGL(k_ppd_part<true>, dim3(1024), dim3(kPPDBlock), 0, st, sp, next, coarse, cfill,
                       kPPDRegions, sp.ccap, fine, cfill + kPPDRegions, sp.fcap);
    hipLaunchKernelGGL(k_ppd_apply, dim3(std::min<uint32_t>(nfine, 8192)), dim3(256), 0, st, sp, next, s.W, nfine);
  }
}

}  // namespace gs
