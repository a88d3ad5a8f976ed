// gs_wave.h -- wave (64 lanes) and block primitives shared by the kernels:
// one copy of each, included by the .hip files that use them.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace gs {

// Sum over the wave's 64 lanes (xor butterfly): every lane gets the total.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (uint32_t o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (uint32_t o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ uint32_t lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// Lanes below this one whose bit is set in the ballot b.
__device__ __forceinline__ uint32_t lanes_below(unsigned long long b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// Wave-aggregated append: one LDS atomic per wave, lanes with `take` get
// consecutive slots of the list whose fill counter is *n (all lanes active).
__device__ __forceinline__ uint32_t wave_append(uint32_t* n, bool take) {
  const unsigned long long bal = __ballot(take);
  uint32_t base = 0;
  if (bal && lane_id() == 0) base = atomicAdd(n, (uint32_t)__popcll(bal));
  return __builtin_amdgcn_readfirstlane(base) + lanes_below(bal);
}

// LDS written by some lanes of a wave is read by others: release fence, wave
// barrier, acquire fence (no block barrier: the wave owns the data).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Inclusive scan over the wave's 64 lanes: lane l gets the sum of lanes 0..l.
template <class T>
__device__ __forceinline__ T wave_inscan(T x) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

// Exclusive scan of one u64 per thread over a block of NW waves (s: NW words
// of LDS); returns the thread's prefix, *total the block's sum.  Block-uniform.
template <uint32_t NW>
__device__ __forceinline__ unsigned long long block_exscan_u64(unsigned long long v, unsigned long long* s,
                                                               unsigned long long* total) {
  const unsigned long long x = wave_inscan(v);
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 63) s[wv] = x;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (uint32_t q = 0; q < NW; ++q) {
    const unsigned long long t = s[q];
    if (q < wv) before += t;
    all += t;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

}  // namespace gs
