// gs_pick.h -- which of the rumors an end wants a capped message carries
// (gs_rumorset_set_payload).  Plain C++ for both
// sides: gs_rumorset_cap.hip's round kernel calls rs_pick per lane, and a CPU
// test compiles this header alone with the host compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_PICK_HD __host__ __device__ inline
#else
#define GS_PICK_HD inline
#endif

namespace gs {

// (the values of GS_PICK_* in include/gossip.h)
constexpr uint32_t kPickLow = 0, kPickHigh = 1, kPickRotate = 2;

GS_PICK_HD uint32_t pick_popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

GS_PICK_HD uint64_t pick_reverse(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __brevll(x);
#else
  x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
  return __builtin_bswap64(x);
#endif
}

// Index of the set bit of x with k set bits below it (popcount(x) > k): six
// halvings, each a popcount of the window's low half and two selects.
GS_PICK_HD uint32_t pick_select(uint64_t x, uint32_t k) {
  const uint32_t lo = (uint32_t)x, c32 = (uint32_t)__builtin_popcount(lo);
  const bool up = k >= c32;
  uint32_t w = up ? (uint32_t)(x >> 32) : lo, pos = up ? 32u : 0u;
  k -= up ? c32 : 0u;
#if defined(__clang__)
#pragma unroll
#endif
  for (uint32_t h = 16; h >= 1; h >>= 1) {
    const uint32_t c = (uint32_t)__builtin_popcount(w & ((1u << h) - 1u));
    const bool hi = k >= c;
    w = hi ? w >> h : w;
    pos += hi ? h : 0u;
    k -= hi ? c : 0u;
  }
  return pos;
}

// The B set bits of x with the smallest indices (x itself if it has no more), B in 1..64.
GS_PICK_HD uint64_t pick_lowest(uint64_t x, uint32_t B) {
  const uint64_t cut = x & (~0ull >> (63u - pick_select(x, B - 1u)));  // (any index 0..63 if x has fewer)
  return pick_popc(x) <= B ? x : cut;
}

// x (bits below R only) turned down by o places in a ring of R bits, o < R <=
// 64; the second shift is split so that o = 0 with R = 64 shifts by 63 and 1.
GS_PICK_HD uint64_t pick_ring_down(uint64_t x, uint32_t o, uint32_t R) {
  return ((x >> o) | ((x << (R - 1u - o)) << 1)) & (~0ull >> (64u - R));
}
GS_PICK_HD uint64_t pick_ring_up(uint64_t x, uint32_t o, uint32_t R) {
  return ((x << o) | ((x >> (R - 1u - o)) >> 1)) & (~0ull >> (64u - R));
}

// What a message carries of the wanted rumors x (bits below R) under a cap of
// B rumors: x if it fits, else the B lowest (kPickLow), the B highest
// (kPickHigh) or the first B met going up from index o < R, wrapping from
// R - 1 to 0 (kPickRotate).
GS_PICK_HD uint64_t rs_pick(uint64_t x, uint32_t B, uint32_t pick, uint32_t o, uint32_t R) {
  if (pick == kPickHigh) return pick_reverse(pick_lowest(pick_reverse(x), B));
  if (pick == kPickRotate) return pick_ring_up(pick_lowest(pick_ring_down(x, o, R), B), o, R);
  return pick_lowest(x, B);
}

}  // namespace gs
