// gs_win_expand.hip -- the window engine's expand stage (gs_win_dev.h has the
// pipeline):
//   expand    one thread per firing node (Node.Broadcast, :141-147): row read
//             once, keyed RandomDrop per slot (one Philox per 4 slots), kept
//             targets counting-sorted in LDS by coarse bucket (target >> 22)
//             and written as coalesced runs into coarse regions sized from
//             the node share (+ margin); message = u_in_coarse | k << 22
// and the sealing and packing of the friends rows it reads.
#include <algorithm>

#include "gs_win_dev.h"

namespace gs {
namespace {

// Unit of firing index g (gmap[q] = unit holding firing index 64*q) for a
// wave whose 64 lanes hold the 64 consecutive firing indices of group g0 / 64
// (g0 wave-uniform): the group's unit bounds are two scalar loads, and only a
// group that spans several units searches [gmap[q], gmap[q + 1]] per lane.
__device__ __forceinline__ uint32_t unit_of_wave(const WinState& w, unsigned long long g0, unsigned long long g,
                                                 unsigned long long Tn, uint32_t units) {
  const unsigned long long q = g0 >> 6;
  uint32_t lo = w.gmap[q];
  uint32_t hi = ((q + 1) << 6) < Tn ? w.gmap[q + 1] : units - 1;
  if (lo == hi) return lo;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (w.unit_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// GS_XSTAMPS builds (diagnostics, GS_STAMPS=1 at run time): wave 0 of every
// k_expand workgroup waits for everything it issued and adds the cycles since
// its last stamp to phase i (w.dbg[kXStamp0 + i]; i = 0 counts rounds).
#ifdef GS_XSTAMPS
__device__ __forceinline__ void xstamp(const WinState& w, unsigned long long& last, uint32_t i) {
  if (w.dbg && threadIdx.x < 64) {
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0 && i) atomicAdd(&w.dbg[kXStamp0 + i], t - last);
    if (threadIdx.x == 0 && i == 1) atomicAdd(&w.dbg[kXStamp0], 1ull);
    last = t;
  }
}
#define XSTAMP(i) xstamp(w, xlast, i)
#else
#define XSTAMP(i) ((void)0)
#endif

template <uint32_t SLOTS>  // LDS message slots per round: block * nodes per thread * row length
struct ExpandLds {
  uint32_t sorted[SLOTS];
  uint8_t sbin[SLOTS];
  uint32_t cnt[256];
  uint32_t off[257];
  unsigned long long gbase[256];          // bin b's message p goes to gbase[b] + p
  unsigned long long cend[256];           // end of coarse region b (ccap[b + 1])
  uint32_t ovf;                           // a bin of this round overflowed its region
  unsigned long long acc[kMaxWindow][2];  // fired, sent per tick
};

// Batched trials: add (a, b) to fields (fa, fb) of row `key` of tstat
// (key = trial * kMaxWindow + tick, ~0u = nothing), one atomic pair per
// distinct key in the wave.  The wave's lanes usually share one key (firing
// indices are bucket-major, and a bucket belongs to one trial).
__device__ __forceinline__ void tstat_add(uint32_t* tstat, uint32_t key, uint32_t fa, uint32_t a,
                                          uint32_t fb, uint32_t b) {
  bool pend = key != ~0u;
  for (unsigned long long bal = __ballot(pend); bal; bal = __ballot(pend)) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(bal);
    const uint32_t k0 = __shfl(key, lead, 64);
    const bool mine = pend && key == k0;
    const uint32_t sa = wave_sum(mine ? a : 0u), sb = wave_sum(mine ? b : 0u);
    if ((threadIdx.x & 63) == lead) {
      if (sa) atomicAdd(&tstat[(size_t)k0 * kTStatFields + fa], sa);
      if (sb) atomicAdd(&tstat[(size_t)k0 * kTStatFields + fb], sb);
    }
    pend = pend && !mine;
  }
}

// Packed view (rows <= 6 slots, stride 8): row v is the 24 bytes at byte
// 24 * (v mod 5) of 128-B line v / 5 (8 bytes of each line unused), so a
// line holds five rows instead of four and no row straddles two lines.
__device__ __forceinline__ uint64_t pk_byte(uint32_t v) {
  const uint32_t line = (uint32_t)(((uint64_t)v * 0xCCCCCCCDull) >> 34);  // v / 5 for every 32-bit v
  return (uint64_t)line * 128 + (v - line * 5) * 24;
}

// The packed view's rows of NPT nodes per lane, fetched by LANE PAIRS: lanes
// 2p and 2p+1 load the 32 bytes from the 16-B aligned base of lane 2p's row
// (one uint4 each: both halves of one 128-B line in one instruction, so one
// L2 request per row instead of two), then those of lane 2p+1's row, and swap
// halves with a DPP move.  A random 24-B row costs two requests fetched per
// lane (uint4 + uint2); by pairs the gather ran 1.87x faster
// (scripts/micro/uncached_gather.hip: 4.84e10 vs 2.58e10 rows/s,
// profiles/r05p_gather_pairs.txt).  Every lane of a wave takes part (a lane
// without a node fetches line 0 and drops it), so the call must not sit in
// lane-divergent code; a wave with no node at all skips the fetch uniformly.
__device__ __forceinline__ uint32_t dpp_swap_pair(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
}
template <uint32_t MAXS>
__device__ __forceinline__ void decode_pk_row(uint4 x, uint4 y, bool o8, uint32_t (&mm)[MAXS]) {
  mm[0] = o8 ? x.z : x.x;
  mm[1] = o8 ? x.w : x.y;
  mm[2] = o8 ? y.x : x.z;
  mm[3] = o8 ? y.y : x.w;
  mm[4 % MAXS] = o8 ? y.z : y.x;
  if (MAXS > 5) mm[5 % MAXS] = o8 ? y.w : y.y;
}
template <uint32_t MAXS, uint32_t NPT>
__device__ __forceinline__ void load_rows_pk_pairs(const WinState& w, const uint32_t (&vv)[NPT], const bool (&wlive)[NPT],
                                                   uint32_t (&mm)[NPT][MAXS]) {
  const uint32_t odd = threadIdx.x & 1;
  const uint4* pk = reinterpret_cast<const uint4*>(w.pk);
  uint4 s0[NPT], s1[NPT];
  uint32_t o8[NPT];
#pragma unroll
  for (uint32_t q = 0; q < NPT; ++q) {
    if (!wlive[q]) continue;  // (wave-uniform)
    const uint64_t b = vv[q] != ~0u ? pk_byte(vv[q]) : 0ull;
    o8[q] = (uint32_t)b & 8u;
    const uint32_t mine = (uint32_t)(b >> 4), other = dpp_swap_pair(mine);  // uint4 index of the base
    const uint32_t ev = odd ? other : mine, od = odd ? mine : other;
    s0[q] = pk[(size_t)ev + odd];  // the pair's even row, half `odd`
    s1[q] = pk[(size_t)od + odd];  // the pair's odd row, half `odd`
  }
#pragma unroll
  for (uint32_t q = 0; q < NPT; ++q) {
    if (!wlive[q]) continue;
    // the even lane holds its half 0 (s0) and the odd lane's half 0 (s1); the
    // odd lane the even lane's half 1 (s0) and its own half 1 (s1)
    const uint4 send = odd ? s0[q] : s1[q];
    uint4 got;
    got.x = dpp_swap_pair(send.x);
    got.y = dpp_swap_pair(send.y);
    got.z = dpp_swap_pair(send.z);
    got.w = dpp_swap_pair(send.w);
    if (vv[q] != ~0u) decode_pk_row<MAXS>(odd ? got : s0[q], odd ? s1[q] : got, o8[q] != 0, mm[q]);
  }
}

// Friends row of v into registers; slots past the list hold kEmptyMsg (rows
// are sealed by k_seal_rows, so the length byte is not read).
template <uint32_t MAXS>
__device__ __forceinline__ void load_row(const WinState& w, uint32_t v, uint32_t (&mm)[MAXS]) {
  const uint32_t S = w.stride;
  if (MAXS >= 5 && MAXS <= 6 && w.pk) {  // two 16-B loads from the row's 16-B aligned base
    const uint64_t b = pk_byte(v);
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(w.pk) + (b & ~15ull));
    decode_pk_row<MAXS>(p[0], p[1], (b & 8) != 0, mm);  // (the row starts 8 bytes into the first load)
    return;
  }
  if ((S & 3) == 0 && S >= 8 && MAXS >= 5 && MAXS <= 8) {  // 16-B aligned rows: uint4 + uint2 / uint4
    const uint4 a = reinterpret_cast<const uint4*>(w.ids + (size_t)v * S)[0];
    mm[0] = a.x; mm[1] = a.y; mm[2] = a.z; mm[3] = a.w;
    if (MAXS > 4 && MAXS <= 6) {
      const uint2 b = reinterpret_cast<const uint2*>(w.ids + (size_t)v * S)[2];
      mm[4 % MAXS] = b.x;
      if (MAXS > 5) mm[5 % MAXS] = b.y;
    } else if (MAXS > 6) {
      const uint4 b = reinterpret_cast<const uint4*>(w.ids + (size_t)v * S)[1];
      mm[4 % MAXS] = b.x; mm[5 % MAXS] = b.y; mm[6 % MAXS] = b.z; mm[7 % MAXS] = b.w;
    }
  } else if ((S & 3) == 0 && MAXS > 8) {  // 16-B aligned longer rows: uint4 loads
    const uint4* row = reinterpret_cast<const uint4*>(w.ids + (size_t)v * S);
#pragma unroll
    for (uint32_t j = 0; j < MAXS; j += 4) {
      const uint4 x = j < S ? row[j / 4] : make_uint4(kEmptyMsg, kEmptyMsg, kEmptyMsg, kEmptyMsg);
      mm[j] = x.x;
      if (j + 1 < MAXS) mm[j + 1] = x.y;
      if (j + 2 < MAXS) mm[j + 2] = x.z;
      if (j + 3 < MAXS) mm[j + 3] = x.w;
    }
  } else if ((S & 1) == 0) {
    const uint2* row = reinterpret_cast<const uint2*>(w.ids + (size_t)v * S);
#pragma unroll
    for (uint32_t j = 0; j < MAXS; j += 2) {
      const uint2 x = 2 * j < 2 * S ? row[j / 2] : make_uint2(kEmptyMsg, kEmptyMsg);
      mm[j] = x.x;
      if (j + 1 < MAXS) mm[j + 1] = x.y;
    }
  } else {
    const uint32_t* row = w.ids + (size_t)v * S;
#pragma unroll
    for (uint32_t j = 0; j < MAXS; ++j) mm[j] = j < S ? row[j] : kEmptyMsg;
  }
}

// Coarse bin of target `t`; t becomes its index inside the bin.  Unsharded:
// bin = t >> 22.  Owner expand (node-range shards): the target's owner d (the
// shard whose range holds it: q = t >> 14 over seg_per >> 14, oseg_magic =
// floor((2^32 - 1) / oseg_q) never overestimates and is at most one below)
// and the 2^22-node chunk of d's range.
__device__ __forceinline__ uint32_t coarse_bin(const WinState& w, uint32_t& t) {
  if (!w.owner) {
    const uint32_t b = t >> kCoarseShift;
    t &= (1u << kCoarseShift) - 1;
    return b;
  }
  const uint32_t q = t >> kFineLog;
  uint32_t d = __umulhi(q, w.oseg_magic);
  if ((d + 1) * w.oseg_q <= q) ++d;
  const uint32_t off = t - d * w.seg_per;
  t = off & ((1u << kCoarseShift) - 1);
  return d * w.obins + (off >> kCoarseShift);
}

// Expand + coarse partition (Node.Broadcast, simulator.go:141-147).  Each
// thread takes NPT firing nodes per round; their rows are all in flight before
// any is used.  Kept targets are counting-sorted in LDS by coarse bucket and
// leave as coalesced runs, one global reservation per (round, bucket).
// WRITE=false only counts (exact fallback).
// XCD-aware round split: workgroups are dealt to the 8 XCDs round-robin
// (XCD = blockIdx & 7), so with a grid that is a multiple of 8 each XCD takes
// one contiguous eighth of the rounds, shared among its B/8 workgroups --
// fire lists of one bucket share friends-row lines in that XCD's L2, and the
// coarse sub-region (bin, blockIdx & 7) a workgroup writes receives an equal
// share of the window whatever the round count (a sparse window on a large
// fixed grid must not pile onto XCD 0).  Other grids: plain grid stride.
__device__ __forceinline__ void xcd_rounds(unsigned long long rounds, unsigned long long& beg,
                                           unsigned long long& end, unsigned long long& step) {
  const uint32_t B = gridDim.x;
  if ((B & 7) == 0) {
    const unsigned long long per = (rounds + 7) >> 3, x = blockIdx.x & 7;
    beg = x * per + (blockIdx.x >> 3);
    end = (x + 1) * per < rounds ? (x + 1) * per : rounds;
    step = B >> 3;
  } else {
    beg = blockIdx.x;
    end = rounds;
    step = B;
  }
}

template <bool WRITE, uint32_t MAXS, uint32_t NPT, uint32_t B>
__device__ __forceinline__ void expand_body(const WinState& w, uint32_t t0, uint32_t L, unsigned long long Tn,
                                            int add_stats) {
  __shared__ ExpandLds<B * NPT * MAXS> sm;
  const uint32_t tid = threadIdx.x;
  uint32_t Ls = L;  // unit layout stride
  if (w.ctl) {
    L = win_live(w, t0, 0);
    if (!L) return;
    Tn = w.ctl->Tn;
    Ls = w.lstride;
  }
  const uint32_t units = Ls * w.nfine;
  constexpr uint32_t per_round = B * NPT;
  if (tid < kMaxWindow * 2) (&sm.acc[0][0])[tid] = 0;
  static_assert(B % 256 == 0, "thread b < 256 owns coarse bin b");
  const bool binner = tid < 256;
  const uint32_t reg = (tid & 255) * kCoarseSub + (blockIdx.x & (kCoarseSub - 1));  // bin tid, this XCD's sub-region
  const unsigned long long cbase = w.ccap[reg], cend = w.ccap[reg + 1];
  if (binner) sm.cend[tid] = cend;
  const unsigned long long rounds = (Tn + per_round - 1) / per_round;
  unsigned long long rbeg, rend, rstep;
  xcd_rounds(rounds, rbeg, rend, rstep);
  // per-tick fired | sent << 16 of this thread's nodes (<= 1024 rounds per
  // workgroup, win_expand): registers, not same-address LDS atomics per node
  uint32_t accp[kBitTicks];
#pragma unroll
  for (uint32_t kx = 0; kx < kBitTicks; ++kx) accp[kx] = 0;
#ifdef GS_XSTAMPS
  unsigned long long xlast = 0;
  XSTAMP(0);
#endif
  for (unsigned long long rd = rbeg; rd < rend; rd += rstep) {
    if (binner) sm.cnt[tid] = 0;
    __syncthreads();
    if (tid == 0) sm.ovf = 0;
    XSTAMP(6);  // the previous round's write-out and this barrier
    uint32_t mm[NPT][MAXS], mt[NPT][MAXS];  // message, bin | rank << 8 (~0u = none)
    uint32_t vv[NPT], kk[NPT];
    bool wlive[NPT];  // the wave has a node in slot q (wave-uniform)
#pragma unroll
    for (uint32_t q = 0; q < NPT; ++q) {
      const unsigned long long g0 = rd * per_round + q * B + __builtin_amdgcn_readfirstlane(tid & ~63u);
      const unsigned long long g = g0 + (tid & 63);
      vv[q] = ~0u;
      kk[q] = 0;
      wlive[q] = g0 < Tn;
      if (g0 < Tn) {
        const uint32_t u = unit_of_wave(w, g0, g < Tn ? g : Tn - 1, Tn, units);
        if (g < Tn) {
        const uint32_t f = u / Ls, k = u - f * Ls;
        const uint32_t s = (t0 + k) % w.R;
        const uint32_t i = (uint32_t)(g - w.unit_off[u]);
        vv[q] = (f << kFineLog) + w.flist[((size_t)s * w.nfine + f) * kFineNodes + i];
        kk[q] = k;
        }
      }
    }
    XSTAMP(1);  // firing nodes looked up
#pragma unroll
    for (uint32_t q = 0; q < NPT; ++q) {
#pragma unroll
      for (uint32_t j = 0; j < MAXS; ++j) { mm[q][j] = kEmptyMsg; mt[q][j] = ~0u; }
    }
    if (MAXS >= 5 && MAXS <= 6 && w.pk && !w.nopair) {  // (uniform)
      load_rows_pk_pairs<MAXS, NPT>(w, vv, wlive, mm);  // all rows in flight
    } else {
#pragma unroll
      for (uint32_t q = 0; q < NPT; ++q)
        if (vv[q] != ~0u) load_row<MAXS>(w, vv[q], mm[q]);  // all rows in flight
    }
    XSTAMP(2);  // rows gathered
    uint32_t sentq[NPT];
#pragma unroll
    for (uint32_t q = 0; q < NPT; ++q) {
      sentq[q] = 0;
      if (vv[q] == ~0u) continue;
      const uint32_t v = vv[q], k = kk[q], t = t0 + k;
      uint32_t vn, c3drop;
      node_key(w.tlog, w.tmask, w.key, (uint64_t)w.base + v, K_DROP, vn, c3drop);
      uint32_t sent = 0;
#pragma unroll
      for (uint32_t jg = 0; jg < (MAXS + 3) / 4; ++jg) {
        if (mm[q][jg * 4] == kEmptyMsg) break;
        // :144, :172 and the messages' crash rolls (:180): one draw per slot
        const u32x4 r = philox(vn, t, jg, c3drop, w.key.k0, w.key.k1);
#pragma unroll
        for (uint32_t jj = 0; jj < 4; ++jj) {
          const uint32_t j = jg * 4 + jj;
          if (j >= MAXS) break;
          uint32_t dropd, crashd;
          drop_crash(lane_of(r, jj), dropd, crashd);
          if (mm[q][j] != kEmptyMsg && (int32_t)dropd >= w.kd) {  // kept: :145
            uint32_t loc = mm[q][j];
            const uint32_t bin = coarse_bin(w, loc);
            const uint32_t roll0 = (int32_t)crashd < w.kc;
            mt[q][j] = bin | (atomicAdd(&sm.cnt[bin], 1u) << 8);
            mm[q][j] = loc | (k << kCoarseShift) | (roll0 << kRoll0Coarse);
            ++sent;
          }
        }
      }
      sentq[q] = sent;
#pragma unroll
      for (uint32_t kx = 0; kx < kBitTicks; ++kx)
        if (kx == k) accp[kx] += 1u | (sent << 16);
    }
    if (WRITE && add_stats && w.tstat) {  // batched trials: fired/sent per (trial, tick)
#pragma unroll
      for (uint32_t q = 0; q < NPT; ++q) {
        const uint32_t key = vv[q] == ~0u ? ~0u : (uint32_t)((uint64_t)vv[q] >> w.tlog) * kMaxWindow + w.tofs + kk[q];
        tstat_add(w.tstat, key, TS_FIRED, 1u, TS_SENT, sentq[q]);
      }
    }
    XSTAMP(3);  // drop / crash draws and LDS ranks
    __syncthreads();
    if (!WRITE) {
      if (binner && sm.cnt[tid]) atomicAdd(&w.chist[reg], (unsigned long long)sm.cnt[tid]);
      continue;  // the next round's first barrier orders the reuse of sm.cnt
    }
    block_scan256(sm.cnt, sm.off);
    // thread b reserves bin b's run; the atomic's return latency overlaps the
    // LDS scatter below (which needs only off[] from the scan)
    const uint32_t mycnt = binner ? sm.cnt[tid] : 0u;
    unsigned long long at = 0;
    if (mycnt) at = atomicAdd(&w.cfill[reg], (unsigned long long)mycnt);
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < NPT; ++q)
#pragma unroll
      for (uint32_t j = 0; j < MAXS; ++j)
        if (mt[q][j] != ~0u) {
          const uint32_t bin = mt[q][j] & 255, p = sm.off[bin] + (mt[q][j] >> 8);
          sm.sorted[p] = mm[q][j];
          sm.sbin[p] = (uint8_t)bin;
        }
    if (mycnt) {
      if (at + mycnt > cend - cbase) {
        atomicOr(w.err, kErrCoarse);
        if (w.dd) atomicOr(reinterpret_cast<unsigned int*>(&w.cfill[kRegions]), kErrCoarse);  // every shard stops
        sm.ovf = 1;
      }
      sm.gbase[tid] = cbase + at - sm.off[tid];
    }
    XSTAMP(4);  // scan, reservation, LDS scatter (wave 0's part)
    __syncthreads();
    XSTAMP(5);  // waiting for the other waves
    const uint32_t total = sm.off[256];
    // two LDS reads per message; the region bound is checked only in a round
    // whose reservation overflowed (the window is then redone exactly)
    if (!sm.ovf) {
      for (uint32_t p = tid; p < total; p += B) w.cmsg[sm.gbase[sm.sbin[p]] + p] = sm.sorted[p];
    } else {
      for (uint32_t p = tid; p < total; p += B) {
        const uint32_t b = sm.sbin[p];
        const unsigned long long pos = sm.gbase[b] + p;
        if (pos < sm.cend[b]) w.cmsg[pos] = sm.sorted[p];
      }
    }
  }
  if (!WRITE || !add_stats) return;  // an exact redo must not count the window twice
#pragma unroll
  for (uint32_t kx = 0; kx < kBitTicks; ++kx) {
    if (kx >= L) continue;
    const uint32_t fired = wave_sum(accp[kx] & 0xFFFFu), sent = wave_sum(accp[kx] >> 16);
    if ((tid & 63) == 0) {
      if (fired) atomicAdd(&sm.acc[kx][0], (unsigned long long)fired);
      if (sent) atomicAdd(&sm.acc[kx][1], (unsigned long long)sent);
    }
  }
  __syncthreads();
  if (tid < L * 2) {
    const uint32_t k = tid >> 1, fld = tid & 1;
    const unsigned long long v = sm.acc[k][fld];
    unsigned long long* row = shard_row(w, k);
    if (v) atomicAdd(&row[fld ? ST_SENT : ST_FIRED], v);
    // every delivered send is a receipt; k_resolve subtracts the uncounted ones
    if (v && fld) atomicAdd(&row[ST_MSGS], v);
  }
}
template <bool WRITE, uint32_t MAXS, uint32_t NPT, uint32_t B = kExpandBlock>
__global__ __launch_bounds__(B) void k_expand(const WinState w, uint32_t t0, uint32_t L, unsigned long long Tn,
                                              int add_stats) {
  expand_body<WRITE, MAXS, NPT, B>(w, t0, L, Tn, add_stats);
}
// the shards of an in-process group (device-driven: each reads its Tn from its
// control block), a slice of the persistent grid each
template <bool WRITE, uint32_t MAXS, uint32_t NPT, uint32_t B = kExpandBlock>
__global__ __launch_bounds__(B) void k_expand_m(const WinState* __restrict__ ws, uint32_t L, int add_stats) {
  expand_body<WRITE, MAXS, NPT, B>(ws[blockIdx.y], 0u, L, 0ull, add_stats);
}

// The packed view of sealed stride-8 rows (pk_byte): slots 0..5 of row v.
__global__ void k_pack_rows(const uint32_t* ids, uint64_t n, uint32_t* pk) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n;
       v += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 a = reinterpret_cast<const uint4*>(ids + v * 8)[0];
    const uint2 b = reinterpret_cast<const uint2*>(ids + v * 8)[2];
    uint2* d = reinterpret_cast<uint2*>(reinterpret_cast<char*>(pk) + pk_byte((uint32_t)v));
    d[0] = make_uint2(a.x, a.y);
    d[1] = make_uint2(a.z, a.w);
    d[2] = b;
  }
}

// Slots past a node's friends list become kEmptyMsg (the window engine's
// expand reads rows without the length byte).
__global__ void k_seal_rows(const uint8_t* deg, uint32_t* ids, uint64_t n, uint32_t stride) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n;
       v += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = deg[v];
    for (uint32_t j = d; j < stride; ++j) ids[v * stride + j] = kEmptyMsg;
  }
}

}  // namespace

// k_expand's launch geometry for a window of Tn firing nodes: firing nodes per
// round, workgroup size, grid.  One source for win_expand and for the host's
// per-XCD region plan of batched trials (plan_coarse_trials, gs_windows.cpp),
// which must know which sub-region each round writes (xcd_rounds).
uint32_t win_expand_geometry(const WinState& w, uint64_t Tn, uint32_t* per_round_out, uint32_t* bsz_out,
                             uint32_t* npt_out) {
  // rows of <= 6 (C5's fanin 6) and <= 8 slots: 4 nodes per thread.  Rows
  // <= 6: 512-thread workgroups (2048 rows per round, two per CU by LDS): the
  // per-round scan, reservations and barriers cost half as much per message
  // and a bin's run per round doubles (~40 messages); 256 (four per CU) and
  // 1024 (one per CU) measured slower, as did two nodes per thread.
  const uint32_t rs = w.slots;  // rows may be padded past the longest one
  const uint32_t bsz = rs <= 6 ? kExpandBlock6 : kExpandBlock;
  const uint32_t per_round = rs <= 8 ? bsz * kExpandNpt : kExpandBlock;
  const uint64_t rounds = (Tn + per_round - 1) / per_round;
  // rows <= 8 slots: a persistent grid of four workgroups per CU (the LDS
  // holds four) whatever the window's size -- a sparse window then costs one
  // wave of workgroups, not several.  Longer rows (the 20- and 32-slot
  // instances fit more workgroups per CU): up to 8192.  GS_XGRID=<workgroups
  // of 256 threads> (A/B knob, at least 8; 0 = unset) replaces both caps, so
  // tests can make a workgroup run several rounds of a small window; it stays
  // in here, where plan_coarse_trials sees the same grid.
  static const uint64_t xgrid = [] {
    const char* e = getenv("GS_XGRID");
    return e ? (uint64_t)std::max(atoi(e), 8) : 0ull;
  }();
  const uint64_t cap = rs > 8 ? (xgrid ? xgrid : 8192) : (xgrid ? xgrid : (uint64_t)device_cus() * 4) * kExpandBlock / bsz;
  // (a thread counts fired | sent << 16 of its nodes in 16-bit halves: at most
  // 1024 rounds per workgroup, <= 4096 nodes and 32768 sends per thread)
  const uint64_t grid_cap = std::max<uint64_t>(cap, (rounds + 1023) / 1024);
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(rounds, grid_cap);
  if (per_round_out) *per_round_out = per_round;
  if (bsz_out) *bsz_out = bsz;
  if (npt_out) *npt_out = kExpandNpt;
  return blocks;
}

namespace {

// One row-width class of win_expand.  mode 0: count coarse buckets only;
// 1: write + per-tick stats; 2: write only.
template <uint32_t MAXS, uint32_t NPT, uint32_t B>
void launch_expand(const WinState& w, uint32_t t0, uint32_t L, unsigned long long Tn, int mode, dim3 grid,
                   hipStream_t s) {
  if (mode) hipLaunchKernelGGL((k_expand<true, MAXS, NPT, B>), grid, dim3(B), 0, s, w, t0, L, Tn, mode == 1 ? 1 : 0);
  else hipLaunchKernelGGL((k_expand<false, MAXS, NPT, B>), grid, dim3(B), 0, s, w, t0, L, Tn, 0);
}

}  // namespace

hipError_t win_expand(const WinState& w, uint32_t t0, uint32_t L, uint64_t Tn, int mode,
                      hipStream_t s) {
  const uint32_t blocks = win_expand_geometry(w, Tn, nullptr, nullptr, nullptr);
  const uint32_t rs = w.slots;
  const dim3 grid(blocks ? blocks : 1);
  if (rs <= 6) launch_expand<6, kExpandNpt, kExpandBlock6>(w, t0, L, Tn, mode, grid, s);
  else if (rs <= 8) launch_expand<8, kExpandNpt, kExpandBlock>(w, t0, L, Tn, mode, grid, s);
  // (20: C4's 19-slot rows, a 25-KB LDS stage, six workgroups per CU)
  else if (rs <= 20) launch_expand<20, 1, kExpandBlock>(w, t0, L, Tn, mode, grid, s);
  else launch_expand<kWinMaxStride, 1, kExpandBlock>(w, t0, L, Tn, mode, grid, s);
  return hipGetLastError();
}

hipError_t win_expand_g(const WinGroup& g, uint32_t L, hipStream_t s) {
  const uint32_t rs = g.slots_max;
  // win_expand's persistent grid (rows <= 8: four 256-thread workgroups per
  // CU, or two of 512 for rows <= 6) split over the shards, a multiple of 8
  // per shard (blockIdx.x & 7 is the XCD); longer rows: 8192 per shard
  const uint32_t bsz = rs <= 6 ? kExpandBlock6 : kExpandBlock;
  const uint32_t total = rs <= 8 ? device_cus() * 4 * kExpandBlock / bsz : 8192u * g.M;
  const uint32_t bx = std::max<uint32_t>(8, ((total + g.M - 1) / g.M + 7) & ~7u);
  const dim3 grid(bx, g.M);
  if (rs <= 6)
    hipLaunchKernelGGL((k_expand_m<true, 6, kExpandNpt, kExpandBlock6>), grid, dim3(kExpandBlock6), 0, s, g.ws, L, 1);
  else if (rs <= 8) hipLaunchKernelGGL((k_expand_m<true, 8, kExpandNpt>), grid, dim3(kExpandBlock), 0, s, g.ws, L, 1);
  else if (rs <= 20) hipLaunchKernelGGL((k_expand_m<true, 20, 1>), grid, dim3(kExpandBlock), 0, s, g.ws, L, 1);
  else hipLaunchKernelGGL((k_expand_m<true, kWinMaxStride, 1>), grid, dim3(kExpandBlock), 0, s, g.ws, L, 1);
  return hipGetLastError();
}

hipError_t win_pack_rows(const uint32_t* ids, uint64_t n, uint32_t* pk, hipStream_t s) {
  const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(k_pack_rows, dim3((uint32_t)(blocks ? blocks : 1)), dim3(256), 0, s, ids, n, pk);
  return hipGetLastError();
}

hipError_t win_seal_rows(const uint8_t* deg, uint32_t* ids, uint64_t n, uint32_t stride,
                         hipStream_t s) {
  const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(k_seal_rows, dim3((uint32_t)(blocks ? blocks : 1)), dim3(256), 0, s, deg, ids, n,
                     stride);
  return hipGetLastError();
}

}  // namespace gs
