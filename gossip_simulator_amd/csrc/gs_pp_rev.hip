// gs_pp_rev.hip -- push-pull: the reverse table (in-edges (v, j) of every
// node u: PPSparse::rend / rsrc / rslot, gs_internal.h), built with an atomic
// per edge around a hipcub scan (pp_rev_build, and the _range pair for
// shards) or by partitioning the edges (pp_rev_build_part), and its compact
// view.  The only push-pull file that needs hipcub.
#include <vector>

#include <hipcub/hipcub.hpp>

#include "gs_pp_dev.h"
#include "gs_rev_plan.h"

namespace gs {
namespace {

// ---- reverse table ------------------------------------------------------------
__global__ __launch_bounds__(kPPBlock) void k_rev_count(const DevState s, unsigned long long* cnt) {
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < s.n; v += (uint64_t)gridDim.x * kPPBlock) {
    const uint32_t d = s.deg[v];
    for (uint32_t j = 0; j < d; ++j) atomicAdd(&cnt[s.ids[v * s.stride + j]], 1ull);
  }
}

// After the exclusive scan rend[u] = start of u's in-edges; each fill bumps
// it, so it ends as the end of u's in-edges (= the start of u + 1's).
__global__ __launch_bounds__(kPPBlock) void k_rev_fill(const DevState s, unsigned long long* rend, uint32_t* rsrc,
                                                       uint8_t* rslot) {
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < s.n; v += (uint64_t)gridDim.x * kPPBlock) {
    const uint32_t d = s.deg[v];
    for (uint32_t j = 0; j < d; ++j) {
      const unsigned long long at = atomicAdd(&rend[s.ids[v * s.stride + j]], 1ull);
      rsrc[at] = (uint32_t)v;
      rslot[at] = (uint8_t)(pp_rslot_packed(s.stride) ? j | (d - 1) << 4 : j);
    }
  }
}

// ---- node-range shards ----------------------------------------------------------
// In-edge counts of the targets in [lo, hi) over the full table (cnt indexed
// by target - lo), then the fill (rend ends as the end of each target's edges).
__global__ __launch_bounds__(kPPBlock) void k_rev_count_range(const uint8_t* deg, const uint32_t* ids, uint64_t n,
                                                              uint32_t stride, uint64_t lo, uint64_t hi,
                                                              unsigned long long* cnt) {
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kPPBlock) {
    const uint32_t d = deg[v];
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t u = ids[v * stride + j];
      if (u >= lo && u < hi) atomicAdd(&cnt[u - lo], 1ull);
    }
  }
}

__global__ __launch_bounds__(kPPBlock) void k_rev_fill_range(const uint8_t* deg, const uint32_t* ids, uint64_t n,
                                                             uint32_t stride, uint64_t lo, uint64_t hi,
                                                             unsigned long long* rend, uint32_t* rsrc,
                                                             uint8_t* rslot) {
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kPPBlock) {
    const uint32_t d = deg[v];
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t u = ids[v * stride + j];
      if (u < lo || u >= hi) continue;
      const unsigned long long at = atomicAdd(&rend[u - lo], 1ull);
      rsrc[at] = (uint32_t)v;
      rslot[at] = (uint8_t)(pp_rslot_packed(stride) ? j | (d - 1) << 4 : j);
    }
  }
}

// ---- reverse table by partitioning (pp_rev_build_part) ----------------------
// The in-edges (v, j) -> u of the whole table, without a random atomic per
// edge (k_rev_count + k_rev_fill make two, 0.85 s at N = 1e9): a histogram of
// the targets' 2^22-node coarse bins (exact coarse regions), a coarse
// partition of the edges as 8-byte records (u mod 2^22 | v << 22 | slot byte
// << 53), a fine partition of each coarse region by the 16384-node bucket,
// and one workgroup per bucket that counts its targets' in-edges in LDS, writes
// their rend and places rsrc / rslot.  The order of a node's in-list is free
// (every use of the reverse table is order-independent, as with the atomic
// fill).
constexpr uint32_t kRvShift = 22;            // coarse bin = u >> 22
constexpr uint32_t kRvBins = 512;            // n < 2^31
constexpr uint32_t kRvBlock = 1024;
constexpr uint32_t kRvRows = 2 * kRvBlock;   // rows per coarse-pass round
constexpr uint32_t kRvTile = 16 * kRvBlock;  // records per fine-pass tile

__device__ __forceinline__ uint8_t rv_slot_byte(uint32_t stride, uint32_t j, uint32_t d) {
  return (uint8_t)(pp_rslot_packed(stride) ? j | (d - 1) << 4 : j);
}

// The compact view of rend (PPSparse::rend16 / rbase): one thread per node.
__global__ __launch_bounds__(kPPBlock) void k_rv_compact(const unsigned long long* __restrict__ rend, uint64_t n,
                                                         uint16_t* __restrict__ rend16,
                                                         unsigned long long* __restrict__ rbase, uint32_t* ovf) {
  for (uint64_t u = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; u < n; u += (uint64_t)gridDim.x * kPPBlock) {
    const uint64_t w = u >> 6;
    const unsigned long long b = w ? rend[(w << 6) - 1] : 0ull;
    if ((u & 63) == 0) rbase[w] = b;
    const unsigned long long d = rend[u] - b;
    if (d > 0xFFFFull) atomicOr(ovf, 1u);
    rend16[u] = (uint16_t)d;
  }
}

__global__ __launch_bounds__(kRvBlock) void k_rv_hist(const DevState s, unsigned long long* chist) {
  __shared__ uint32_t h[kRvBins];
  for (uint32_t b = threadIdx.x; b < kRvBins; b += kRvBlock) h[b] = 0;
  __syncthreads();
  for (uint64_t v = (uint64_t)blockIdx.x * kRvBlock + threadIdx.x; v < s.n; v += (uint64_t)gridDim.x * kRvBlock) {
    const uint32_t d = s.deg[v];
    for (uint32_t j = 0; j < d; ++j) atomicAdd(&h[s.ids[v * s.stride + j] >> kRvShift], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kRvBins; b += kRvBlock)
    if (h[b]) atomicAdd(&chist[b], (unsigned long long)h[b]);
}

// Rounds of kRvRows rows: count per coarse bin in LDS, one reservation per
// (round, bin), then every record to its bin's run (the rows re-read from L2).
// One pass covers the coarse bins [blo, bhi) (edges to other bins are
// skipped; cstart / cfill are indexed by bin - blo): a build in several passes
// bounds the temporaries (pp_rev_build_part).
__global__ __launch_bounds__(kRvBlock) void k_rv_coarse(const DevState s, const unsigned long long* __restrict__ cstart,
                                                        unsigned long long* __restrict__ cfill,
                                                        unsigned long long* __restrict__ rec, uint32_t blo,
                                                        uint32_t bhi) {
  __shared__ uint32_t cnt[kRvBins], off[kRvBins];
  __shared__ unsigned long long gb[kRvBins];
  const uint32_t tid = threadIdx.x;
  const uint64_t rounds = (s.n + kRvRows - 1) / kRvRows;
  for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
    for (uint32_t b = tid; b < kRvBins; b += kRvBlock) { cnt[b] = 0; off[b] = 0; }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      const uint64_t v = r * kRvRows + k * kRvBlock + tid;
      if (v >= s.n) continue;
      const uint32_t d = s.deg[v];
      for (uint32_t j = 0; j < d; ++j) {
        const uint32_t b = s.ids[v * s.stride + j] >> kRvShift;
        if (b >= blo && b < bhi) atomicAdd(&cnt[b], 1u);
      }
    }
    __syncthreads();
    for (uint32_t b = tid; b < kRvBins; b += kRvBlock)
      if (cnt[b]) gb[b] = cstart[b - blo] + atomicAdd(&cfill[b - blo], (unsigned long long)cnt[b]);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      const uint64_t v = r * kRvRows + k * kRvBlock + tid;
      if (v >= s.n) continue;
      const uint32_t d = s.deg[v];
      for (uint32_t j = 0; j < d; ++j) {
        const uint32_t u = s.ids[v * s.stride + j], b = u >> kRvShift;
        if (b < blo || b >= bhi) continue;
        const unsigned long long pos = gb[b] + atomicAdd(&off[b], 1u);
        rec[pos] = (u & ((1u << kRvShift) - 1)) | (v << kRvShift) |
                   ((unsigned long long)rv_slot_byte(s.stride, j, d) << 53);
      }
    }
    __syncthreads();
  }
}

// Tiles of a coarse region -> its fine regions (bits 14..21 of u): LDS counts,
// one reservation per (tile, bucket), records placed by offset atomics.  A
// fine region past its planned capacity sets *ovf (the build falls back).
__global__ __launch_bounds__(kRvBlock) void k_rv_fine(const unsigned long long* __restrict__ rec,
                                                      const unsigned long long* __restrict__ cstart,
                                                      const unsigned long long* __restrict__ cend,
                                                      const uint32_t* __restrict__ tpre, uint32_t nbins,
                                                      const unsigned long long* __restrict__ fstart,
                                                      unsigned long long* __restrict__ ffill,
                                                      unsigned long long* __restrict__ frec, uint32_t* ovf) {
  __shared__ uint32_t cnt[256], off[256];
  __shared__ unsigned long long gb[256], ge[256];
  __shared__ uint32_t s_tp[kRvBins + 1];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i <= nbins; i += kRvBlock) s_tp[i] = tpre[i];
  __syncthreads();
  const uint32_t ntiles = s_tp[nbins];
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint32_t lo = 0, hi = nbins - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (s_tp[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const uint32_t c = lo;
    const unsigned long long b0 = cstart[c] + (unsigned long long)(t - s_tp[c]) * kRvTile, be = cend[c];
    if (tid < 256) { cnt[tid] = 0; off[tid] = 0; }
    __syncthreads();
    unsigned long long r[kRvTile / kRvBlock];
#pragma unroll
    for (uint32_t k = 0; k < kRvTile / kRvBlock; ++k) {
      const unsigned long long i = b0 + k * kRvBlock + tid;
      r[k] = i < be ? rec[i] : ~0ull;
      if (r[k] != ~0ull) atomicAdd(&cnt[(r[k] >> 14) & 255], 1u);
    }
    __syncthreads();
    if (tid < 256 && cnt[tid]) {
      const size_t fb = (size_t)c * 256 + tid;
      gb[tid] = fstart[fb] + atomicAdd(&ffill[fb], (unsigned long long)cnt[tid]);
      ge[tid] = fstart[fb + 1];
      if (gb[tid] + cnt[tid] > ge[tid]) atomicOr(ovf, 1u);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kRvTile / kRvBlock; ++k)
      if (r[k] != ~0ull) {
        const uint32_t d = (r[k] >> 14) & 255;
        const unsigned long long pos = gb[d] + atomicAdd(&off[d], 1u);
        if (pos < ge[d]) frec[pos] = r[k];
      }
    __syncthreads();
  }
}

// One workgroup per 16384-node bucket: in-degree counts in LDS, the bucket's
// rend (end of each node's in-edges), then rsrc / rslot in place.
__global__ __launch_bounds__(kRvBlock) void k_rv_final(const unsigned long long* __restrict__ frec,
                                                       const unsigned long long* __restrict__ fstart,
                                                       const unsigned long long* __restrict__ ffill,
                                                       const unsigned long long* __restrict__ bbase, uint64_t n,
                                                       unsigned long long* __restrict__ rend, uint32_t* __restrict__ rsrc,
                                                       uint8_t* __restrict__ rslot, uint32_t fb0) {
  __shared__ uint32_t cnt[16384];
  __shared__ unsigned long long s_x[kRvBlock / 64];
  // bucket b of the table = bucket blockIdx.x of this pass's arrays
  const uint32_t tid = threadIdx.x, b = fb0 + blockIdx.x;
  const unsigned long long M = ffill[blockIdx.x], f0 = fstart[blockIdx.x], ob = bbase[blockIdx.x];
  for (uint32_t i = tid; i < 16384; i += kRvBlock) cnt[i] = 0;
  __syncthreads();
  for (unsigned long long i = tid; i < M; i += kRvBlock) atomicAdd(&cnt[frec[f0 + i] & 16383], 1u);
  __syncthreads();
  // exclusive offsets: 16 consecutive counters per thread
  uint32_t loc[16], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) { loc[k] = cnt[tid * 16 + k]; sum += loc[k]; }
  const uint32_t lane = tid & 63, wv = tid >> 6;
  const uint32_t x = wave_inscan(sum);
  if (lane == 63) s_x[wv] = x;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t q = 0; q < wv; ++q) before += (uint32_t)s_x[q];
  uint32_t a = before + x - sum;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint64_t u = (uint64_t)b * 16384 + tid * 16 + k;
    cnt[tid * 16 + k] = a;
    a += loc[k];
    if (u < n) rend[u] = ob + a;  // the end of u's in-edges
  }
  __syncthreads();
  for (unsigned long long i = tid; i < M; i += kRvBlock) {
    const unsigned long long rc = frec[f0 + i];
    const unsigned long long at = ob + atomicAdd(&cnt[rc & 16383], 1u);
    rsrc[at] = (uint32_t)((rc >> kRvShift) & 0x7FFFFFFFull);
    rslot[at] = (uint8_t)(rc >> 53);
  }
}
}  // namespace

size_t pp_rev_scan_bytes(uint64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (unsigned long long*)nullptr,
                                         (unsigned long long*)nullptr, (int)(n + 1));
  return bytes;
}

hipError_t pp_rev_build(const DevState& s, unsigned long long* rend, uint32_t* rsrc, uint8_t* rslot, void* tmp,
                        size_t tmp_bytes, hipStream_t st) {
  hipError_t e = hipMemsetAsync(rend, 0, (s.n + 1) * 8, st);
  if (e != hipSuccess) return e;
  const uint32_t blocks = grid_for(s.n, kPPBlock, 8192);
  hipLaunchKernelGGL(k_rev_count, dim3(blocks), dim3(kPPBlock), 0, st, s, rend);
  e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, rend, rend, (int)(s.n + 1), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rev_fill, dim3(blocks), dim3(kPPBlock), 0, st, s, rend, rsrc, rslot);
  return hipGetLastError();
}

hipError_t pp_rev_compact(const unsigned long long* rend, uint64_t n, uint16_t* rend16, unsigned long long* rbase,
                          uint32_t* ovf, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t blocks = grid_for(n, kPPBlock, 8192);
  hipLaunchKernelGGL(k_rv_compact, dim3(blocks), dim3(kPPBlock), 0, st, rend, n, rend16, rbase, ovf);
  return hipGetLastError();
}

// The reverse table by partitioning (the k_rv_* kernels above): host-paced
// (a few small read-backs per pass).  The coarse bins are taken in passes of
// consecutive bins whose temporaries (8-B records: the coarse copy, then the
// fine regions, ~17 B per edge) fit the largest block the device allocator can
// give without returning cached memory to the driver (gs_devmem_largest): one
// pass when memory allows, more after other contexts left their blocks cached
// (every pass streams the table again, ~8 ms per pass at N = 1e9, where a
// hipMalloc right after large hipFrees stalled for seconds: DESIGN.md section
// 9).  GS_PP_REV_PASSES=k (read per call) forces k passes.  An error (no
// memory even for one bin, or a fine region past its planned size on a skewed
// table) leaves the outputs unspecified: the caller then builds with
// pp_rev_build.
hipError_t pp_rev_build_part(const DevState& s, unsigned long long* rend, uint32_t* rsrc, uint8_t* rslot,
                             hipStream_t st, uint32_t* passes_out) {
  if (!s.n || s.n >= (1ull << 31)) return hipErrorInvalidValue;
  const uint64_t n = s.n, nbins = (n + (1ull << kRvShift) - 1) >> kRvShift, nbf = (n + 16383) >> 14;
  // small device arrays: chist[512] | cstart[513] | cend[512] | fstart[nbf+1] | ffill[nbf] | bbase[nbf] | tpre[513] | ovf
  const size_t small = 8 * (512 + 513 + 512 + (nbf + 1) + nbf + nbf) + 4 * 513 + 64;
  char* sm = nullptr;
  hipError_t e = dev_malloc(&sm, small);
  if (e != hipSuccess) return e;
  unsigned long long* d_chist = (unsigned long long*)sm;
  unsigned long long* d_cstart = d_chist + 512;
  unsigned long long* d_cend = d_cstart + 513;
  unsigned long long* d_fstart = d_cend + 512;
  unsigned long long* d_ffill = d_fstart + nbf + 1;
  unsigned long long* d_bbase = d_ffill + nbf;
  uint32_t* d_tpre = (uint32_t*)(d_bbase + nbf);
  uint32_t* d_ovf = d_tpre + 513;
  unsigned long long* tmp = nullptr;
  std::vector<unsigned long long> h(512, 0), cs(513, 0), fsz(nbf, 0), need(nbins, 0);
  uint32_t ovf = 0;
  const uint32_t grid = 512;
  auto done = [&](hipError_t r) {
    (void)hipStreamSynchronize(st);
    if (tmp) (void)dev_free(tmp);
    (void)dev_free(sm);
    return r;
  };
#define RV(x)                          \
  do {                                 \
    hipError_t e_ = (x);               \
    if (e_ != hipSuccess) return done(e_); \
  } while (0)
  RV(hipMemsetAsync(sm, 0, small, st));
  hipLaunchKernelGGL(k_rv_hist, dim3(grid), dim3(kRvBlock), 0, st, s, d_chist);
  RV(hipGetLastError());
  RV(hipMemcpyAsync(h.data(), d_chist, 512 * 8, hipMemcpyDeviceToHost, st));
  RV(hipStreamSynchronize(st));
  // exact coarse regions; a fine region planned at 1.125 x its node share of
  // its coarse region + 1024; need[c] = bin c's records in both copies
  for (uint64_t c = 0; c < nbins; ++c) {
    cs[c + 1] = cs[c] + h[c];
    const uint64_t nf = std::min<uint64_t>(256, nbf - c * 256);
    const uint64_t nodes_c = std::min<uint64_t>(1ull << kRvShift, n - (c << kRvShift));
    need[c] = h[c];
    for (uint64_t d = 0; d < nf; ++d) {
      const uint64_t fb = c * 256 + d, nodes_b = std::min<uint64_t>(16384, n - fb * 16384);
      const unsigned long long share = (unsigned long long)((double)h[c] * nodes_b / nodes_c);
      fsz[fb] = share + share / 8 + 1024;
      need[c] += fsz[fb];
    }
  }
  const unsigned long long E = cs[nbins];
  // passes of consecutive bins (gs_rev_plan.h): a forced count, or as many
  // bins per pass as fit the largest block the allocator can give
  const char* fp = getenv("GS_PP_REV_PASSES");
  const uint64_t forced = fp ? (uint64_t)std::max(atoi(fp), 1) : 0;
  const RevPlan plan = pp_rev_plan(h.data(), need.data(), nbins, forced ? 0 : gs_devmem_largest() / 8, forced);
  if (!plan.ok) return done(hipErrorOutOfMemory);  // not even one bin: the atomic build
  const std::vector<uint32_t>& cut = plan.cut;
  const size_t P = cut.size() - 1;
  if (passes_out) *passes_out = (uint32_t)P;
  // one block for both copies of the largest pass: it fits the extent the plan
  // was made for; each pass puts its fine copy right behind its coarse copy
  RV(dev_malloc(&tmp, plan.tmp_records * 8));
  unsigned long long* rec = tmp;
  for (size_t p = 0; p < P; ++p) {
    const uint32_t blo = cut[p], bhi = cut[p + 1], nb = bhi - blo;
    const uint64_t fb0 = (uint64_t)blo * 256, fb1 = std::min<uint64_t>((uint64_t)bhi * 256, nbf), nfl = fb1 - fb0;
    unsigned long long* frec = tmp + plan.rec[p];
    std::vector<unsigned long long> csl(nb + 1, 0), cel(nb, 0), fsl(nfl + 1, 0), ffl(nfl, 0), bbl(nfl, 0);
    std::vector<uint32_t> tpl(nb + 1, 0);
    for (uint32_t c = 0; c < nb; ++c) {
      csl[c + 1] = csl[c] + h[blo + c];
      cel[c] = csl[c + 1];
      tpl[c + 1] = tpl[c] + (uint32_t)((h[blo + c] + kRvTile - 1) / kRvTile);
    }
    for (uint64_t i = 0; i < nfl; ++i) fsl[i + 1] = fsl[i] + fsz[fb0 + i];
    RV(hipMemcpyAsync(d_cstart, csl.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
    RV(hipMemcpyAsync(d_cend, cel.data(), nb * 8, hipMemcpyHostToDevice, st));
    RV(hipMemcpyAsync(d_fstart, fsl.data(), (nfl + 1) * 8, hipMemcpyHostToDevice, st));
    RV(hipMemcpyAsync(d_tpre, tpl.data(), (nb + 1) * 4, hipMemcpyHostToDevice, st));
    RV(hipMemsetAsync(d_ffill, 0, nfl * 8, st));
    unsigned long long* d_cfill = d_chist;  // reused: the fills of the coarse pass
    RV(hipMemsetAsync(d_cfill, 0, 512 * 8, st));
    hipLaunchKernelGGL(k_rv_coarse, dim3(grid_for(n, kRvRows, grid)), dim3(kRvBlock), 0, st, s, d_cstart, d_cfill,
                       rec, blo, bhi);
    RV(hipGetLastError());
    if (tpl[nb]) {
      hipLaunchKernelGGL(k_rv_fine, dim3(std::min<uint32_t>(tpl[nb], grid)), dim3(kRvBlock), 0, st, rec, d_cstart,
                         d_cend, d_tpre, nb, d_fstart, d_ffill, frec, d_ovf);
      RV(hipGetLastError());
    }
    RV(hipMemcpyAsync(ffl.data(), d_ffill, nfl * 8, hipMemcpyDeviceToHost, st));
    RV(hipMemcpyAsync(&ovf, d_ovf, 4, hipMemcpyDeviceToHost, st));
    RV(hipStreamSynchronize(st));
    if (ovf) return done(hipErrorInvalidValue);  // a skewed table: the atomic build
    bbl[0] = cs[blo];  // every in-edge of the earlier buckets lies in the earlier bins
    for (uint64_t b = 1; b < nfl; ++b) bbl[b] = bbl[b - 1] + ffl[b - 1];
    RV(hipMemcpyAsync(d_bbase, bbl.data(), nfl * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rv_final, dim3((uint32_t)nfl), dim3(kRvBlock), 0, st, frec, d_fstart, d_ffill, d_bbase, n,
                       rend, rsrc, rslot, (uint32_t)fb0);
    RV(hipGetLastError());
    RV(hipStreamSynchronize(st));  // this pass's host arrays and the temporaries are reused
  }
  RV(hipMemcpyAsync(rend + n, &E, 8, hipMemcpyHostToDevice, st));
#undef RV
  return done(hipSuccess);
}

size_t pp_rev_range_scan_bytes(uint64_t n) { return pp_rev_scan_bytes(n); }

hipError_t pp_rev_count_range(const uint8_t* deg, const uint32_t* ids, uint64_t nfull, uint32_t stride, uint64_t lo,
                              uint64_t hi, unsigned long long* rend, void* tmp, size_t tmp_bytes, hipStream_t st) {
  const uint64_t n = hi - lo;
  hipError_t e = hipMemsetAsync(rend, 0, (n + 1) * 8, st);
  if (e != hipSuccess) return e;
  const uint32_t blocks = grid_for(nfull, kPPBlock, 8192);
  hipLaunchKernelGGL(k_rev_count_range, dim3(blocks), dim3(kPPBlock), 0, st, deg, ids, nfull, stride, lo, hi, rend);
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, rend, rend, (int)(n + 1), st);
}

hipError_t pp_rev_fill_range(const uint8_t* deg, const uint32_t* ids, uint64_t nfull, uint32_t stride, uint64_t lo,
                             uint64_t hi, unsigned long long* rend, uint32_t* rsrc, uint8_t* rslot, hipStream_t st) {
  const uint32_t blocks = grid_for(nfull, kPPBlock, 8192);
  hipLaunchKernelGGL(k_rev_fill_range, dim3(blocks), dim3(kPPBlock), 0, st, deg, ids, nfull, stride, lo, hi, rend,
                     rsrc, rslot);
  return hipGetLastError();
}

}  // namespace gs
