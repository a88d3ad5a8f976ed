// gs_win_resolve.hip -- the window engine's resolve stage (gs_win_dev.h has
// the pipeline):
//   resolve   one workgroup per fine bucket: received/crashed bits and u16
//             arrival counters in LDS; per tick, count then let one owner lane
//             per node replay ordinals 0..count-1 of the receive case
//             (:107-123); infections append to the fire list (slot, f) that
//             only this workgroup writes
#include <algorithm>

#include "gs_win_dev.h"

namespace gs {
namespace {

constexpr uint32_t kResolveMaxBuckets = 256;  // buckets one persistent workgroup may own
constexpr uint32_t kSmallMax = 256;           // buckets with <= this many receipts: k_resolve_small
#ifndef GS_SMALL_BLOCK
#define GS_SMALL_BLOCK 512
#endif
constexpr uint32_t kSmallBlock = GS_SMALL_BLOCK;  // k_resolve_small: 8 waves, one bucket each
#ifndef GS_ROLLED_BLOCK
#define GS_ROLLED_BLOCK 256
#endif
constexpr uint32_t kRolledBlock = GS_ROLLED_BLOCK;  // the rolled replay: 4 waves, one bucket each

// Bit-parallel resolve (k_resolve).  Three kinds of node in a window:
//   crashed before it: every receipt is uncounted (simulator.go:108), by tick;
//   ROLLED: live, and a receipt in the window carries a crash roll (k_part2
//     marks those nodes in w.rollw): the receipts are written to the bucket's
//     rolled list (w.rlmsg, w.rlcnt) and replayed exactly (rule A6) by
//     k_resolve_rolled after this kernel, sorted per wave like k_resolve_small;
//   plain: every receipt is counted and the first one informs the node
//     (:111, :117-121), so a bit per (tick, node) is the whole state.
// Per receipt: b1[k] |= bit (no-return LDS atomic) and a read of the word's
// (crashed, rolled) pair.  A bucket whose rolled list overflows takes the
// per-tick large path (resolve_tick), which reuses the same LDS for per-node
// counters.
constexpr uint32_t kBitWords = kFineNodes / 32;
struct ResolveLds {
  union {
    struct {                            // b1 .. dlist, then the infection list
      uint32_t b1[kBitTicks][kBitWords];
      uint2 cr0[kBitWords];             // per word: crashed before the window, a crash-roll
                                        // receipt in the window (from w.rollw)
    };
    struct {                            // large path
      uint32_t cnt[kFineNodes];         // per node at the current tick: arrivals | crash rolls << 16
      uint32_t recv[kBitWords];
      uint32_t crash[kBitWords];
      uint32_t nrecv[kBitWords];
      uint32_t ncrash[kBitWords];
    };
  };
  uint32_t fc[kWinMaxRing];         // fire-list lengths of this bucket, per ring slot
  uint32_t st[kMaxWindow][4];       // dead (not counted), recv, crash per tick: whole launch
  uint32_t dead[kMaxWindow];        // this bucket's receipts at nodes crashed before the window
  uint32_t blist[kResolveMaxBuckets];  // this workgroup's non-empty buckets
  unsigned long long bstart[kResolveMaxBuckets];  // their message region starts (fstart)
  uint32_t bcnt[kResolveMaxBuckets];   // their message counts (ffill)
  uint32_t ndup;
  uint32_t ninf;
  uint32_t err;
  uint32_t nb;
  uint32_t cls;
  unsigned long long stamp[2][kStampPhases];  // GS_STAMPS: [M >= 1024][phase] cycles (thread 0)
  unsigned long long tlast;
};  // 78 KB: two workgroups per CU
static_assert(kBitTicks <= kMaxWindow, "window ticks fit the message format");
static_assert(sizeof(uint32_t) * kFineNodes <= sizeof(((ResolveLds*)0)->cnt), "the infection list fits");

// GS_STAMPS diagnostics: thread 0 adds the cycles since the last stamp to phase i.
template <class Lds>
__device__ __forceinline__ void stamp(const WinState& w, Lds& sm, uint32_t i) {
  if (w.dbg && threadIdx.x == 0) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    if (i) sm.stamp[sm.cls][i] += t - sm.tlast;
    sm.tlast = t;
  }
}

// GS_RESOLVE_PROBE=1 (timing probe builds only, results differ): k_resolve's
// receipts phase skips the per-receipt (crashed, rolled) read, every node is
// plain -- the floor of the b1 atomics alone
#if defined(GS_RESOLVE_PROBE) && GS_RESOLVE_PROBE == 1
#define GS_RESOLVE_CR0(loc) make_uint2(0u, 0u)
#else
#define GS_RESOLVE_CR0(loc) sm.cr0[(loc) >> 5]
#endif


// The receive case of Node.Start (simulator.go:107-123) for node `loc` of the
// bucket with kk arrivals at tick t, `ones` of them carrying a crash roll
// (rule A6, first_crash).  (Large-bucket path.)
__device__ __forceinline__ void resolve_node(const WinState& w, ResolveLds& sm, uint32_t f,
                                             uint32_t loc, uint32_t kk, uint32_t ones, uint32_t t,
                                             uint32_t& cm, uint32_t& cr, uint32_t& cc, uint32_t& cs) {
  const uint32_t bit = 1u << (loc & 31), wi = loc >> 5;
  if (sm.crash[wi] & bit) return;                                  // :108 (not counted)
  const uint64_t g = (uint64_t)w.base + (f << kFineLog) + loc;
  uint32_t u, c3order;
  node_key(w.tlog, w.tmask, w.key, g, K_ORDER, u, c3order);
  const uint32_t pos = ones ? first_crash(u, t, kk, ones, c3order, w.key.k0, w.key.k1) : kk + 1;
  cm += pos <= kk ? pos : kk;                                      // :111
  if (pos > 1 && !(sm.recv[wi] & bit)) {                           // :117
    atomicOr(&sm.recv[wi], bit);                                   // :120
    ++cr;                                                          // :121
    // Broadcast() (:122, :141-142): fire at t + off
    uint32_t c3delay;
    node_key(w.tlog, w.tmask, w.key, g, K_DELAY, u, c3delay);
    const uint32_t off = fire_offset(w.delay_low, w.delay_span,
                                     philox(u, t, 0, c3delay, w.key.k0, w.key.k1).x);
    const uint32_t s = (t + off) % w.R;
    const uint32_t at = atomicAdd(&sm.fc[s], 1u);
    w.flist[((size_t)s * w.nfine + f) * kFineNodes + at] = (uint16_t)loc;
    ++cs;
  }
  if (pos <= kk) {                                                 // :112-115
    atomicOr(&sm.crash[wi], bit);
    ++cc;
  }
}

// One tick's receipts over messages m[lo, hi) (large buckets, streamed from
// global memory): count arrivals per node, then the lane whose atomicAnd takes
// a node's nonzero count resolves that node.
template <class Src>
__device__ __forceinline__ void resolve_tick(const WinState& w, ResolveLds& sm, uint32_t f,
                                             const Src& src, uint32_t lo, uint32_t hi, uint32_t k,
                                             uint32_t t) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t p = lo + tid; p < hi; p += kResolveBlock) {
    const uint32_t m = src[p];
    if (msg_tick(m) != k) continue;
    const uint32_t old = atomicAdd(&sm.cnt[msg_loc(m)], 1u + (((m >> kRoll0Fine) & 1u) << 16));
    if ((old & 0xFFFFu) == 0xFFFFu) sm.err = 1;
  }
  __syncthreads();
  uint32_t arr = 0, cm = 0, cr = 0, cc = 0, cs = 0;
  for (uint32_t p = lo + tid; p < hi; p += kResolveBlock) {
    const uint32_t m = src[p];
    if (msg_tick(m) != k) continue;
    const uint32_t loc = msg_loc(m);
    const uint32_t kk = atomicExch(&sm.cnt[loc], 0u);
    arr += kk & 0xFFFFu;
    if (kk) resolve_node(w, sm, f, loc, kk & 0xFFFFu, kk >> 16, t, cm, cr, cc, cs);
  }
  if (arr != cm) atomicAdd(&sm.st[k][0], arr - cm);
  if (cr) atomicAdd(&sm.st[k][1], cr);
  if (cc) atomicAdd(&sm.st[k][2], cc);
  (void)cs;  // every infection schedules one Broadcast: ST_SCHED = ST_RECV
  __syncthreads();
}

// Adds the lanes' per-tick infection counts plus sm.st (dead, recv, crash) to
// the per-tick totals and, for a batched trial, to tstat[trial]; leaves them
// zeroed.  Block-uniform call.
// acc_ni[k / 2] holds tick k's count in bits 16 * (k & 1) (<= 32 per bucket,
// <= 256 buckets per lane).
template <class Lds>
__device__ __forceinline__ void flush_counts(const WinState& w, Lds& sm, uint32_t (&acc_ni)[kBitTicks / 2],
                                             uint32_t L, uint32_t trial) {
#pragma unroll
  for (uint32_t k = 0; k < kBitTicks; ++k) {
    if (k >= L) continue;
    const uint32_t sr = wave_sum((acc_ni[k / 2] >> (16 * (k & 1))) & 0xFFFFu);
    if (lane_id() == 0 && sr) atomicAdd(&sm.st[k][1], sr);
  }
#pragma unroll
  for (uint32_t k = 0; k < kBitTicks / 2; ++k) acc_ni[k] = 0;
  __syncthreads();
  const uint32_t tid = threadIdx.x;
  if (tid < L * 3) {
    const uint32_t k = tid / 3, fld = tid - k * 3;
    const uint32_t v = sm.st[k][fld];
    // field 0 counts receipts that were NOT counted (:108, after a crash):
    // the expand added every delivered send to ST_MSGS
    unsigned long long* row = shard_row(w, k);
    if (v && fld == 0) atomicAdd(&row[ST_MSGS], 0ull - (unsigned long long)v);
    if (v && fld == 1) {
      atomicAdd(&row[ST_RECV], (unsigned long long)v);
      atomicAdd(&row[ST_SCHED], (unsigned long long)v);  // every infection schedules one Broadcast
    }
    if (v && fld == 2) atomicAdd(&row[ST_CRASH], (unsigned long long)v);
    if (v && trial != ~0u) atomicAdd(&w.tstat[((size_t)trial * kMaxWindow + w.tofs + k) * kTStatFields + TS_DEAD + fld], v);
    sm.st[k][fld] = 0;
  }
  __syncthreads();
}

// Persistent: workgroup g owns buckets g, g + G, g + 2G, ... (G = gridDim.x),
// resolves its non-empty ones in turn, and adds its per-tick counters once at
// the end.  Per bucket:
//   stage    thread w owns bit word w (32 nodes): its recv/crash words in
//            registers, spec = crashed | marked in rollw (cleared here), its
//            b1 words and chain head zeroed
//   receipts every receipt sets its (tick, node) bit in b1; receipts at
//            special nodes are listed, then chained under their word
//   ticks    thread w resolves its plain nodes with bit ops, tick by tick
//            (informed at the first receipt), then replays its special nodes'
//            (node, tick) groups in order (rule A6, first_crash); the
//            infections are Broadcast() (:122, :141)
// A bucket with more rolled receipts than kRolledCap takes the per-tick large path.
__device__ __forceinline__ void resolve_body(const WinState& w, uint32_t t0, uint32_t L) {
  __shared__ ResolveLds sm;
  const uint32_t tid = threadIdx.x, G = gridDim.x;
  L = win_live(w, t0, L);
  if (!L) return;
  static_assert(kBitWords == kResolveBlock, "one bit word per thread");
  static_assert(kWinMaxRing <= kResolveBlock, "one ring slot per thread");
  if (tid < kMaxWindow * 4) (&sm.st[0][0])[tid] = 0;
  if (tid == 0) { sm.nb = 0; sm.cls = 0; }
  if (tid < 2 * kStampPhases) (&sm.stamp[0][0])[tid] = 0;
  __syncthreads();
  {
    const uint32_t f = blockIdx.x + tid * G;
    const unsigned long long fl = tid < kResolveMaxBuckets && f < w.nfine ? w.ffill[f] : 0ull;
    const bool ne = fl > kSmallMax;  // small: k_resolve_small
    const uint32_t at = wave_append(&sm.nb, ne);
    if (ne) {
      // the bucket descriptors come from LDS later: a wait for them never waits
      // for the vector loads in flight (the next bucket's prefetch)
      sm.blist[at] = f;
      sm.bstart[at] = w.fstart[f];
      sm.bcnt[at] = (uint32_t)fl;
    }
  }
  __syncthreads();
  const uint32_t nb = sm.nb;
  stamp(w, sm, 0);
  uint32_t fB = 0, MB = 0;
  unsigned long long mbB = 0;
  auto next_bucket = [&](uint32_t j) { fB = sm.blist[j]; mbB = sm.bstart[j]; MB = sm.bcnt[j]; };
  if (nb > 0) next_bucket(0);
  uint32_t* rwg = (uint32_t*)w.recv;
  uint32_t* cwg = (uint32_t*)w.crash;
  // this lane's infections per tick over all its buckets
  uint32_t acc_ni[kBitTicks / 2];
#pragma unroll
  for (uint32_t k = 0; k < kBitTicks / 2; ++k) acc_ni[k] = 0;
  static_assert(kBitTicks % 2 == 0 && 32 * kResolveMaxBuckets < 65536, "two 16-bit counts per register");
  constexpr uint32_t kU = 8;  // loads in flight per lane
  constexpr uint32_t kBatch = kResolveBlock * kU;
  // messages p0 + u * kResolveBlock + tid of a bucket (gm, M): raw loads, valid
  // iff the index is < M (M >= 1); 32-bit byte offsets from the uniform base
  // (M < 2^28)
  auto ld = [&](const uint32_t* gm, uint32_t M, uint32_t p0, uint32_t (&m)[kU]) {
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint32_t p = p0 + u * kResolveBlock + tid;
      m[u] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(gm) + ((p < M ? p : M - 1) << 2));
    }
  };
  // the next bucket's state words and first batch of messages are loaded
  // while this bucket finishes (from the end of its receipts)
  uint32_t pm[kU], p_recv0 = 0, p_crash0 = 0, p_roll0 = 0, p_fcv = 0;
  bool p_in = false;
  auto prefetch = [&](uint32_t f, uint32_t M, unsigned long long mb) {
    const uint64_t wi = ((uint64_t)(f << kFineLog) >> 5) + tid;
    const bool in = wi < w.W * 2;
    // branch-free (clamped) loads, masked where they are used: a load in a
    // branch, or a select right after it, makes the compiler wait for it at
    // once, which serialises the prefetch with the rest of this bucket
    const uint64_t wc = in ? wi : w.W * 2 - 1;
    p_in = in;
    p_recv0 = rwg[wc];
    p_crash0 = cwg[wc];
    p_roll0 = w.rollw[wc];
    p_fcv = w.fcount[(size_t)(tid < w.R ? tid : 0u) * w.nfine + f];
    ld(w.fmsg + mb, M, 0, pm);
  };
  if (nb > 0) prefetch(fB, MB, mbB);
  for (uint32_t i = 0; i < nb; ++i) {
    const uint32_t f = fB, M = MB;
    const unsigned long long mb = mbB;
    const uint32_t node0 = f << kFineLog;
    const uint64_t wi = ((uint64_t)node0 >> 5) + tid;
    // Philox keys of the bucket's nodes: key node knode0 + local offset (a
    // bucket lies inside one trial), counter words c3order / c3delay
    uint32_t knode0, c3order;
    node_key(w.tlog, w.tmask, w.key, (uint64_t)w.base + node0, K_ORDER, knode0, c3order);
    const uint32_t c3delay = (c3order & 0xFFFFFFu) | (K_DELAY << 24);
    const bool in = wi < w.W * 2;
    const uint32_t recv0 = p_in ? p_recv0 : 0u, crash0 = p_in ? p_crash0 : 0u, roll0 = p_in ? p_roll0 : 0u;
    const uint32_t fcv = tid < w.R ? p_fcv : 0u;
    if (i + 1 < nb) next_bucket(i + 1);
    if (roll0) w.rollw[wi] = 0u;  // consumed: the next window starts clear
    const uint32_t rollw = roll0 & ~crash0;
#pragma unroll
    for (uint32_t k = 0; k < kBitTicks; ++k)
      if (k < L) sm.b1[k][tid] = 0;
    sm.cr0[tid] = make_uint2(crash0, rollw);
    if (tid < w.R) sm.fc[tid] = fcv;
    if (tid < kMaxWindow) sm.dead[tid] = 0;
    if (tid == 0) { sm.ndup = 0; sm.ninf = 0; sm.err = M >= (1u << 28) ? 3 : 0; sm.cls = M >= 1024 ? 1 : 0; }
    __syncthreads();
    stamp(w, sm, 1);
    // receipts: (tick, node) bits; uncounted receipts at crashed nodes by
    // tick (8-bit fields per lane, flushed every 31 batches); receipts at
    // rolled nodes listed.  The next batch's loads are issued before this
    // batch's LDS work.
    const uint32_t* gm = w.fmsg + mb;
    unsigned long long dlo = 0, dhi = 0;  // uncounted receipts, ticks 0..7 / 8..15
    auto flush_dead = [&]() {
      while (dlo) {
        const uint32_t b = __builtin_ctzll(dlo) >> 3;
        atomicAdd(&sm.dead[b], (uint32_t)(dlo >> (8 * b)) & 255u);
        dlo &= ~(255ull << (8 * b));
      }
      while (dhi) {
        const uint32_t b = __builtin_ctzll(dhi) >> 3;
        atomicAdd(&sm.dead[8 + b], (uint32_t)(dhi >> (8 * b)) & 255u);
        dhi &= ~(255ull << (8 * b));
      }
    };
    // one batch: receipts m[u] where VALID (a macro body: a lambda spills)
#define GS_RESOLVE_BATCH(m, VALID)                                                                \
    {                                                                                             \
      uint2 sp[kU];                                                                               \
      _Pragma("unroll") for (uint32_t u = 0; u < kU; ++u) {                                       \
        sp[u] = make_uint2(0, 0);                                                                 \
        if (VALID) {                                                                              \
          const uint32_t loc = msg_loc(m[u]);                                                     \
          atomicOr(&sm.b1[msg_tick(m[u])][loc >> 5], 1u << (loc & 31)); /* no return */         \
          sp[u] = GS_RESOLVE_CR0(loc);                                                            \
        }                                                                                         \
      }                                                                                           \
      uint32_t dm = 0; /* bit u: receipt u is at a rolled node */                                 \
      _Pragma("unroll") for (uint32_t u = 0; u < kU; ++u) {                                       \
        const uint32_t sh = msg_loc(m[u]) & 31, k = msg_tick(m[u]);                               \
        if ((sp[u].x >> sh) & 1u) { /* crashed before the window: not counted (:108) */           \
          if (k < 8) dlo += 1ull << (8 * k);                                                      \
          else dhi += 1ull << (8 * (k - 8));                                                      \
        }                                                                                         \
        if ((sp[u].y >> sh) & 1u) dm |= 1u << u;                                                  \
      }                                                                                           \
      if (nbat % 31 == 30) flush_dead();                                                          \
      const uint32_t nd = __popc(dm);                                                             \
      if (__ballot(nd != 0)) {                                                                    \
        uint32_t pre = 0, tot = 0; /* wave prefix of nd (<= 8) */                                 \
        _Pragma("unroll") for (uint32_t bb = 0; bb < 4; ++bb) {                                   \
          const unsigned long long bal = __ballot((nd >> bb) & 1u);                               \
          pre += lanes_below(bal) << bb;                                                                \
          tot += (uint32_t)__popcll(bal) << bb;                                                   \
        }                                                                                         \
        uint32_t base = 0;                                                                        \
        if (lane_id() == 0) base = atomicAdd(&sm.ndup, tot);                                      \
        uint32_t at = __builtin_amdgcn_readfirstlane(base) + pre;                                 \
        _Pragma("unroll") for (uint32_t u = 0; u < kU; ++u) if ((dm >> u) & 1u) {                 \
          if (at < kRolledCap) w.rlmsg[(size_t)f * kRolledCap + at] = m[u] & ((1u << 19) - 1);    \
          else sm.err = 3;                                                                        \
          ++at;                                                                                   \
        }                                                                                         \
      }                                                                                           \
    }
    {
      uint32_t m[kU];
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) m[u] = pm[u];
      for (uint32_t p0 = 0, nbat = 0; p0 < (sm.err == 3 ? 0u : M); p0 += kBatch, ++nbat) {
        uint32_t mn[kU];
        if (p0 + kBatch < M) ld(gm, M, p0 + kBatch, mn);
        GS_RESOLVE_BATCH(m, p0 + u * kResolveBlock + tid < M)
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) m[u] = mn[u];
      }
    }
#undef GS_RESOLVE_BATCH
    flush_dead();
    stamp(w, sm, 2);
    __syncthreads();
    if (i + 1 < nb) prefetch(fB, MB, mbB);
    // the rolled list goes to k_resolve_rolled (none on the large path)
    if (tid == 0) w.rlcnt[f] = sm.err == 3 ? 0u : min(sm.ndup, kRolledCap);
    stamp(w, sm, 3);
    uint32_t rw = recv0, cw = crash0;
    if (sm.err != 3) {
      if (tid < L && sm.dead[tid]) atomicAdd(&sm.st[tid][0], sm.dead[tid]);
      // plain nodes: informed at their first receipt, tick by tick
      uint32_t infk[kBitTicks], ninf = 0;  // infections per tick of this word
      const uint32_t plain = ~(crash0 | rollw);
#pragma unroll
      for (uint32_t k = 0; k < kBitTicks; ++k) {
        infk[k] = 0;
        if (k >= L) continue;
        const uint32_t infS = sm.b1[k][tid] & plain & ~rw;  // :117-121
        rw |= infS;
        infk[k] = infS;
      }
      stamp(w, sm, 4);
#pragma unroll
      for (uint32_t k = 0; k < kBitTicks; ++k) {
        const uint32_t ni = __popc(infk[k]);
        acc_ni[k / 2] += ni << (16 * (k & 1));
        ninf += ni;
      }
      stamp(w, sm, 5);
      __syncthreads();
      stamp(w, sm, 6);
      // Broadcast() of an infected node x = loc | tick << 14 (:122, :141-142):
      // fire at t + off
      auto bcast = [&](uint32_t x) {
        const uint32_t loc = msg_loc(x), t = t0 + msg_tick(x);
        const uint32_t off = fire_offset(w.delay_low, w.delay_span,
                                         philox(knode0 + loc, t, 0, c3delay, w.key.k0, w.key.k1).x);
        const uint32_t slot = (t + off) % w.R;
        const uint32_t pos = atomicAdd(&sm.fc[slot], 1u);
        w.flist[((size_t)slot * w.nfine + f) * kFineNodes + pos] = (uint16_t)loc;
      };
      // infection list (loc | tick << 14) over the bitmaps, dead from here on
      uint32_t* inf = &sm.cnt[0];
      {
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (uint32_t b = 0; b < 9; ++b) {  // ninf <= 32 * kBitTicks < 512
          const unsigned long long bal = __ballot((ninf >> b) & 1u);
          pre += lanes_below(bal) << b;
          tot += (uint32_t)__popcll(bal) << b;
        }
        uint32_t base = 0;
        if (tot && lane_id() == 0) base = atomicAdd(&sm.ninf, tot);
        uint32_t at = __builtin_amdgcn_readfirstlane(base) + pre;
#pragma unroll
        for (uint32_t k = 0; k < kBitTicks; ++k)
          for (uint32_t x = k < L ? infk[k] : 0u; x; x &= x - 1)
            inf[at++] = (tid * 32 + __builtin_ctz(x)) | (k << kFineLog);
      }
      __syncthreads();
      stamp(w, sm, 7);
      // the listed infections, spread over the block
      const uint32_t ni_all = sm.ninf;
      for (uint32_t q = tid; q < ni_all; q += kResolveBlock) bcast(inf[q]);
    } else {
      // large path: per-node counters, the messages streamed once per tick
      __syncthreads();
      uint4* c4 = reinterpret_cast<uint4*>(sm.cnt);
      for (uint32_t q = tid; q < kFineNodes / 4; q += kResolveBlock) c4[q] = make_uint4(0, 0, 0, 0);
      sm.recv[tid] = recv0;
      sm.crash[tid] = crash0;
      sm.nrecv[tid] = 0;
      sm.ncrash[tid] = 0;
      __syncthreads();
      for (uint32_t k = 0; k < L; ++k) resolve_tick(w, sm, f, gm, 0, M, k, t0 + k);
      rw = sm.recv[tid] | sm.nrecv[tid];
      cw = sm.crash[tid] | sm.ncrash[tid];
      if (tid == 0 && sm.err == 1) atomicOr(w.err, kErrArrivals);
    }
    __syncthreads();
    stamp(w, sm, 8);
    if (in) {
      if (rw != recv0) rwg[wi] = rw;
      if (cw != crash0) cwg[wi] = cw;
    }
    if (tid < w.R) w.fcount[(size_t)tid * w.nfine + f] = sm.fc[tid];
    stamp(w, sm, 9);
    if (w.dbg && tid == 0) sm.stamp[sm.cls][0] += 1;
    // batched trials: the bucket's counters go to its trial's rows (a bucket
    // lies inside one trial) as well as to the per-tick totals
    if (w.tstat) flush_counts(w, sm, acc_ni, L, (uint32_t)(((uint64_t)w.base + node0) >> w.tlog));
  }
  if (w.dbg && tid < 2 * kStampPhases) atomicAdd(&w.dbg[tid], (&sm.stamp[0][0])[tid]);
  if (!w.tstat) flush_counts(w, sm, acc_ni, L, ~0u);
}
__global__ __launch_bounds__(kResolveBlock, GS_RESOLVE_WAVES) void k_resolve2(const WinState w, uint32_t t0, uint32_t L) {
  resolve_body(w, t0, L);
}
__global__ __launch_bounds__(kResolveBlock, GS_RESOLVE_WAVES) void k_resolve2_m(const WinState* __restrict__ ws,
                                                                                 uint32_t L) {
  resolve_body(ws[blockIdx.y], 0u, L);
}

// k_resolve: the bit path alone on a budget that lets three workgroups share a
// CU (six waves per SIMD to hide the dependent LDS round trips behind): at
// most 80 VGPRs and 53 KB of LDS.  Against resolve_body:
//   * a bucket whose rolled list overflows is appended to w.lgl and skipped
//     (k_resolve_large resolves it after this kernel), so the 64-KB counter
//     arm is gone;
//   * the infection list holds kInfCap entries in place of cr0 (dead after the
//     receipts), filled and drained in rounds when a bucket informs more;
//   * four loads in flight per lane (six waves x 4 per SIMD against four x 8);
//     the per-tick infection words are recomputed from b1 when they are
//     listed; the uncounted receipts are 6-bit fields of one register pair.
constexpr uint32_t kInfCap = 6656;  // C5's densest buckets inform ~5,700 nodes in a window: one round
constexpr uint32_t kResolveWaves3 = 6;  // min waves per SIMD: three 512-thread workgroups per CU
struct ResolveLds3 {
  uint32_t b1[kBitTicks][kBitWords];
  union {
    uint2 cr0[kBitWords];     // receipts phase (see ResolveLds)
    uint32_t inf[kInfCap];    // after it: infected nodes, loc | tick << 14
  };
  uint32_t fc[kWinMaxRing];
  uint32_t st[kMaxWindow][4];
  uint32_t dead[kMaxWindow];
  uint32_t blist[kResolveMaxBuckets];
  unsigned long long bstart[kResolveMaxBuckets];
  uint32_t bcnt[kResolveMaxBuckets];
  uint32_t ndup;
  uint32_t ninf;
  uint32_t err;
  uint32_t nb;
  uint32_t cls;
  unsigned long long stamp[2][kStampPhases];
  unsigned long long tlast;
};
static_assert(sizeof(ResolveLds3) <= 53 * 1024, "three workgroups per CU");
static_assert(kBitTicks * 6 <= 64, "6-bit dead counts per tick in one register pair");

__device__ __forceinline__ void resolve3_body(const WinState& w, uint32_t t0, uint32_t L) {
  __shared__ ResolveLds3 sm;
  const uint32_t tid = threadIdx.x, G = gridDim.x;
  L = win_live(w, t0, L);
  if (!L) return;
  if (tid < kMaxWindow * 4) (&sm.st[0][0])[tid] = 0;
  if (tid == 0) { sm.nb = 0; sm.cls = 0; }
  if (tid < 2 * kStampPhases) (&sm.stamp[0][0])[tid] = 0;
  __syncthreads();
  {
    const uint32_t f = blockIdx.x + tid * G;
    const unsigned long long fl = tid < kResolveMaxBuckets && f < w.nfine ? w.ffill[f] : 0ull;
    const bool ne = fl > kSmallMax;  // small: k_resolve_small
    const uint32_t at = wave_append(&sm.nb, ne);
    if (ne) {
      sm.blist[at] = f;
      sm.bstart[at] = w.fstart[f];
      sm.bcnt[at] = (uint32_t)fl;
    }
  }
  __syncthreads();
  const uint32_t nb = sm.nb;
  stamp(w, sm, 0);
  uint32_t* rwg = (uint32_t*)w.recv;
  uint32_t* cwg = (uint32_t*)w.crash;
  uint32_t acc_ni[kBitTicks / 2];  // this lane's infections per tick over all its buckets
#pragma unroll
  for (uint32_t k = 0; k < kBitTicks / 2; ++k) acc_ni[k] = 0;
  constexpr uint32_t kU = 4;  // loads in flight per lane
  constexpr uint32_t kBatch = kResolveBlock * kU;
  // messages p0 + u * kResolveBlock + tid of a bucket (gm, M >= 1): the index
  // clamped to M - 1, so a lane past the end holds a copy of the last receipt
  auto ld = [&](const uint32_t* gm, uint32_t M, uint32_t p0, uint32_t (&m)[kU]) {
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint32_t p = p0 + u * kResolveBlock + tid;
      m[u] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(gm) + ((p < M ? p : M - 1) << 2));
    }
  };
  // the next bucket's state words and first batch of messages are loaded
  // while this bucket finishes (branch-free, masked where they are used: see
  // resolve_body).  Without the batch, the windows of a few thousand receipts
  // per bucket pay a load latency per bucket: slower than resolve_body.
  uint32_t pm[kU], p_recv0 = 0, p_crash0 = 0, p_roll0 = 0, p_fcv = 0;
  bool p_in = false;
  auto prefetch = [&](uint32_t j) {
    const uint32_t f = sm.blist[j];
    const uint64_t wi = ((uint64_t)(f << kFineLog) >> 5) + tid;
    const bool in = wi < w.W * 2;
    const uint64_t wc = in ? wi : w.W * 2 - 1;
    p_in = in;
    p_recv0 = rwg[wc];
    p_crash0 = cwg[wc];
    p_roll0 = w.rollw[wc];
    p_fcv = w.fcount[(size_t)(tid < w.R ? tid : 0u) * w.nfine + f];
    ld(w.fmsg + sm.bstart[j], sm.bcnt[j], 0, pm);
  };
  if (nb > 0) prefetch(0);
  for (uint32_t i = 0; i < nb; ++i) {
    const uint32_t f = sm.blist[i], M = sm.bcnt[i];
    const uint32_t* gm = w.fmsg + sm.bstart[i];
    uint32_t m[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) m[u] = pm[u];
    const uint32_t node0 = f << kFineLog;
    const uint64_t wi = ((uint64_t)node0 >> 5) + tid;
    const bool in = p_in;
    const uint32_t recv0 = in ? p_recv0 : 0u, crash0 = in ? p_crash0 : 0u, roll0 = in ? p_roll0 : 0u;
    if (roll0) w.rollw[wi] = 0u;  // consumed: the next window starts clear
    const uint32_t rollw = roll0 & ~crash0;
#pragma unroll
    for (uint32_t k = 0; k < kBitTicks; ++k)
      if (k < L) sm.b1[k][tid] = 0;
    sm.cr0[tid] = make_uint2(crash0, rollw);
    if (tid < w.R) sm.fc[tid] = p_fcv;
    if (tid < kMaxWindow) sm.dead[tid] = 0;
    if (tid == 0) { sm.ndup = 0; sm.ninf = 0; sm.err = M >= (1u << 28) ? 3 : 0; sm.cls = M >= 1024 ? 1 : 0; }
    __syncthreads();
    stamp(w, sm, 1);
    // receipts: as resolve_body's, the uncounted ones in 6-bit fields per tick
    // (a lane adds <= kU per batch: flushed every 15 batches)
    unsigned long long dd = 0;
    auto flush_dead = [&]() {
      while (dd) {
        const uint32_t b = (uint32_t)__builtin_ctzll(dd) / 6;
        atomicAdd(&sm.dead[b], (uint32_t)(dd >> (6 * b)) & 63u);
        dd &= ~(63ull << (6 * b));
      }
    };
    for (uint32_t p0 = 0, nbat = 0; p0 < (sm.err == 3 ? 0u : M); p0 += kBatch, ++nbat) {
      uint32_t mn[kU];
      if (p0 + kBatch < M) ld(gm, M, p0 + kBatch, mn);
      uint2 sp[kU];
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        // (a lane past the end sets its copy's bit again: no change)
        const uint32_t loc = msg_loc(m[u]);
        atomicOr(&sm.b1[msg_tick(m[u])][loc >> 5], 1u << (loc & 31));  // no return
        sp[u] = GS_RESOLVE_CR0(loc);
      }
      uint32_t dm = 0;  // bit u: receipt u is at a rolled node
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        const uint32_t sh = msg_loc(m[u]) & 31, k = msg_tick(m[u]);
        const uint32_t valid = p0 + u * kResolveBlock + tid < M ? 1u : 0u;
        // crashed before the window: not counted (:108)
        dd += (unsigned long long)((sp[u].x >> sh) & valid) << (6 * k);
        dm |= ((sp[u].y >> sh) & valid) << u;
      }
      if (nbat % 15 == 14) flush_dead();
      if (__ballot(dm != 0)) {
        const uint32_t nd = __popc(dm);
        uint32_t pre = 0, tot = 0;  // wave prefix of nd (<= 4)
#pragma unroll
        for (uint32_t bb = 0; bb < 3; ++bb) {
          const unsigned long long bal = __ballot((nd >> bb) & 1u);
          pre += lanes_below(bal) << bb;
          tot += (uint32_t)__popcll(bal) << bb;
        }
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(&sm.ndup, tot);
        uint32_t at = __builtin_amdgcn_readfirstlane(base) + pre;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) if ((dm >> u) & 1u) {
          if (at < kRolledCap) w.rlmsg[(size_t)f * kRolledCap + at] = m[u] & ((1u << 19) - 1);
          else sm.err = 3;
          ++at;
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) m[u] = mn[u];
    }
    flush_dead();
    stamp(w, sm, 2);
    __syncthreads();
    if (i + 1 < nb) prefetch(i + 1);
    const bool large = sm.err == 3;  // its rolled list overflowed: k_resolve_large's
    if (tid == 0) {
      // the rolled list goes to k_resolve_rolled (none of a large bucket)
      w.rlcnt[f] = large ? 0u : sm.ndup;
      if (large) w.lgl[2 + atomicAdd(&w.lgl[0], 1u)] = f;
    }
    stamp(w, sm, 3);
    if (!large) {
      if (tid < L && sm.dead[tid]) atomicAdd(&sm.st[tid][0], sm.dead[tid]);
      // plain nodes: informed at their first receipt, tick by tick
      const uint32_t plain = ~(crash0 | rollw);
      uint32_t rw = recv0, ninf = 0;
#pragma unroll
      for (uint32_t k = 0; k < kBitTicks; ++k) {
        if (k >= L) continue;
        const uint32_t infS = sm.b1[k][tid] & plain & ~rw;  // :117-121
        rw |= infS;
        const uint32_t ni = __popc(infS);
        acc_ni[k / 2] += ni << (16 * (k & 1));
        ninf += ni;
      }
      stamp(w, sm, 4);
      stamp(w, sm, 5);
      stamp(w, sm, 6);
      if (in && rw != recv0) rwg[wi] = rw;
      // this lane's place in the bucket's infection list
      uint32_t at0;
      {
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (uint32_t b = 0; b < 9; ++b) {  // ninf <= 32 * kBitTicks < 512
          const unsigned long long bal = __ballot((ninf >> b) & 1u);
          pre += lanes_below(bal) << b;
          tot += (uint32_t)__popcll(bal) << b;
        }
        uint32_t base = 0;
        if (tot && lane_id() == 0) base = atomicAdd(&sm.ninf, tot);
        at0 = __builtin_amdgcn_readfirstlane(base) + pre;
      }
      // rounds of kInfCap: entries [r0, r0 + kInfCap) are listed (loc | tick
      // << 14, over cr0: the receipts are done), then Broadcast() by the whole
      // block.  Every consumer of the fire lists is order-free.
      for (uint32_t r0 = 0;; r0 += kInfCap) {
        uint32_t at = at0 - r0, r = recv0;
#pragma unroll
        for (uint32_t k = 0; k < kBitTicks; ++k) {
          if (k >= L) continue;
          uint32_t x = sm.b1[k][tid] & plain & ~r;
          r |= x;
          for (; x; x &= x - 1, ++at)
            if (at < kInfCap) sm.inf[at] = (tid * 32 + __builtin_ctz(x)) | (k << kFineLog);
        }
        __syncthreads();
        stamp(w, sm, 7);
        const uint32_t left = sm.ninf - r0;
        for (uint32_t q = tid; q < min(left, kInfCap); q += kResolveBlock) {
          // Broadcast() of an infected node x = loc | tick << 14 (:122,
          // :141-142): fire at t + off
          const uint32_t x = sm.inf[q];
          const uint32_t loc = msg_loc(x), t = t0 + msg_tick(x);
          uint32_t knode0, c3order;  // the bucket's Philox keys (a bucket lies inside one trial)
          node_key(w.tlog, w.tmask, w.key, (uint64_t)w.base + node0, K_ORDER, knode0, c3order);
          const uint32_t c3delay = (c3order & 0xFFFFFFu) | (K_DELAY << 24);
          const uint32_t off = fire_offset(w.delay_low, w.delay_span,
                                           philox(knode0 + loc, t, 0, c3delay, w.key.k0, w.key.k1).x);
          const uint32_t slot = (t + off) % w.R;
          const uint32_t pos = atomicAdd(&sm.fc[slot], 1u);
          w.flist[((size_t)slot * w.nfine + f) * kFineNodes + pos] = (uint16_t)loc;
        }
        if (left <= kInfCap) break;
        __syncthreads();  // drained before the next round lists
      }
    }
    __syncthreads();
    stamp(w, sm, 8);
    if (!large && tid < w.R) w.fcount[(size_t)tid * w.nfine + f] = sm.fc[tid];
    stamp(w, sm, 9);
    if (w.dbg && tid == 0) sm.stamp[sm.cls][0] += 1;
    // batched trials: the bucket's counters go to its trial's rows
    if (w.tstat) flush_counts(w, sm, acc_ni, L, (uint32_t)(((uint64_t)w.base + node0) >> w.tlog));
  }
  if (w.dbg && tid < 2 * kStampPhases) atomicAdd(&w.dbg[tid], (&sm.stamp[0][0])[tid]);
  if (!w.tstat) flush_counts(w, sm, acc_ni, L, ~0u);
}
__global__ __launch_bounds__(kResolveBlock, kResolveWaves3) void k_resolve(const WinState w, uint32_t t0, uint32_t L) {
  resolve3_body(w, t0, L);
}
__global__ __launch_bounds__(kResolveBlock, kResolveWaves3) void k_resolve_m(const WinState* __restrict__ ws,
                                                                             uint32_t L) {
  resolve3_body(ws[blockIdx.y], 0u, L);
}

// The buckets k_resolve listed in w.lgl (count, workgroups done, buckets):
// their rolled lists overflowed, so every node is replayed per tick from
// per-node counters (resolve_tick).  One workgroup per bucket; the last
// workgroup to finish clears the list for the next window.  No flood of the
// paper's configurations lists a bucket: the launch leaves at once.
__device__ __forceinline__ void resolve_large_body(const WinState& w, uint32_t t0, uint32_t L) {
  __shared__ ResolveLds sm;
  const uint32_t n = w.lgl[0];
  if (!n) return;
  const uint32_t tid = threadIdx.x;
  L = win_live(w, t0, L);
  if (L) {
    if (tid < kMaxWindow * 4) (&sm.st[0][0])[tid] = 0;
    uint32_t acc_ni[kBitTicks / 2];  // (the bit path's: none here)
#pragma unroll
    for (uint32_t k = 0; k < kBitTicks / 2; ++k) acc_ni[k] = 0;
    uint32_t* rwg = (uint32_t*)w.recv;
    uint32_t* cwg = (uint32_t*)w.crash;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
      const uint32_t f = w.lgl[2 + j], M = (uint32_t)w.ffill[f];
      const uint32_t* gm = w.fmsg + w.fstart[f];
      const uint32_t node0 = f << kFineLog;
      const uint64_t wi = ((uint64_t)node0 >> 5) + tid;
      const bool in = wi < w.W * 2;
      const uint32_t recv0 = in ? rwg[wi] : 0u, crash0 = in ? cwg[wi] : 0u;
      uint4* c4 = reinterpret_cast<uint4*>(sm.cnt);
      for (uint32_t q = tid; q < kFineNodes / 4; q += kResolveBlock) c4[q] = make_uint4(0, 0, 0, 0);
      sm.recv[tid] = recv0;
      sm.crash[tid] = crash0;
      if (tid < w.R) sm.fc[tid] = w.fcount[(size_t)tid * w.nfine + f];
      if (tid == 0) sm.err = 0;
      __syncthreads();
      for (uint32_t k = 0; k < L; ++k) resolve_tick(w, sm, f, gm, 0, M, k, t0 + k);
      const uint32_t rw = sm.recv[tid], cw = sm.crash[tid];
      if (in) {
        if (rw != recv0) rwg[wi] = rw;
        if (cw != crash0) cwg[wi] = cw;
      }
      if (tid < w.R) w.fcount[(size_t)tid * w.nfine + f] = sm.fc[tid];
      if (tid == 0 && sm.err == 1) atomicOr(w.err, kErrArrivals);
      if (w.tstat) flush_counts(w, sm, acc_ni, L, (uint32_t)(((uint64_t)w.base + node0) >> w.tlog));
      else __syncthreads();
    }
    if (!w.tstat) flush_counts(w, sm, acc_ni, L, ~0u);
  }
  __syncthreads();
  if (tid == 0 && atomicAdd(&w.lgl[1], 1u) == gridDim.x - 1) {
    w.lgl[0] = 0;
    w.lgl[1] = 0;
  }
}
__global__ __launch_bounds__(kResolveBlock) void k_resolve_large(const WinState w, uint32_t t0, uint32_t L) {
  resolve_large_body(w, t0, L);
}
__global__ __launch_bounds__(kResolveBlock) void k_resolve_large_m(const WinState* __restrict__ ws, uint32_t L) {
  resolve_large_body(ws[blockIdx.y], 0u, L);
}

// Small buckets (1..kSmallMax receipts in the window): one wave per bucket.
// In the sparse windows at the start and end of a broadcast nearly every
// bucket holds a few dozen or hundred receipts, and the bit-parallel
// k_resolve's fixed cost per bucket (512 bit words x L ticks, a chain of block
// barriers) is what the window pays.  Here a wave holds the bucket's
// receipts as E keys per lane (element lane*E + r in register r), sorts them
// by (node, tick, roll0) with a bitonic network (shuffles across lanes,
// swaps across registers), and the first element of every node's run replays
// the receive case (simulator.go:107-123, rule A6) along the run; infected
// nodes Broadcast() (:122, :141-142) into the bucket's fire lists.
// Instance E takes buckets with 64*(E/4) < M <= 64*E receipts (E = 1, 4);
// k_resolve takes the rest.  The launches touch disjoint buckets.
// The same body replays the rolled receipts k_resolve listed per bucket
// (k_resolve_rolled: the rolled nodes' receipts of a dense bucket, up to
// kRolledCap, E = 1, 4, 8 or 16); a rolled node is live when the window starts,
// and its recv/crash bits are untouched by k_resolve, so the replay is the
// same receive case from the same state.
template <uint32_t E, bool ROLLED>
__device__ __forceinline__ void resolve_small_bucket(const WinState& w, uint32_t t0, uint32_t L, uint32_t f,
                                                     const uint32_t* gm, unsigned long long M,
                                                     uint32_t (*st)[kMaxWindow][4], uint32_t* skw,
                                                     uint32_t* fcw) {
  constexpr uint32_t N = 64 * E;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    // the bucket's fire-list lengths, staged in this wave's LDS: infections
    // take their list positions with LDS atomics instead of same-address
    // global atomics (one wave owns the bucket)
    // device-driven windows: k_resolve_small, the first kernel to append to
    // the fire lists, consumes the window's (k_units counted them, k_expand
    // read them): ring slots t0 .. t0 + L - 1 restart at 0 in every bucket
    // before any infection of this window is appended (a short ring may
    // reuse them)
    const bool consume = !ROLLED && w.ctl;
    const uint32_t s0 = t0 % w.R;
    for (uint32_t s = lane; s < w.R; s += 64)
      fcw[s] = consume && (s + w.R - s0) % w.R < L ? 0u : w.fcount[(size_t)s * w.nfine + f];
    uint32_t knode0, c3order;  // keys of the bucket's nodes (one trial per bucket)
    node_key(w.tlog, w.tmask, w.key, (uint64_t)w.base + (f << kFineLog), K_ORDER, knode0, c3order);
    const uint32_t c3delay = (c3order & 0xFFFFFFu) | (K_DELAY << 24);
    // element i = lane * E + r in key[r] (lane-major: the bitonic stages with
    // j < E are register swaps, only those with j >= E shuffle across lanes)
    uint32_t key[E];  // loc << 5 | k << 1 | crash roll; ~0u sorts last
#pragma unroll
    for (uint32_t r = 0; r < E; ++r) {
      const uint32_t i = lane * E + r;
      key[r] = ~0u;
      if (i < M) {
        const uint32_t m = gm[i];
        key[r] = (msg_loc(m) << 5) | (msg_tick(m) << 1) | ((m >> kRoll0Fine) & 1u);
        // k_part2 marked the node of a crash roll for k_resolve: clear it here
        if (!ROLLED && ((m >> kRoll0Fine) & 1u)) w.rollw[((f << kFineLog) + msg_loc(m)) >> 5] = 0u;
      }
    }
#pragma unroll
    for (uint32_t k = 2; k <= N; k <<= 1)
#pragma unroll
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        if (j >= E) {  // partner in lane ^ (j / E), same register
#pragma unroll
          for (uint32_t r = 0; r < E; ++r) {
            const uint32_t i = lane * E + r;
            const uint32_t o = __shfl_xor(key[r], j / E, 64);
            const bool keep_min = ((i & j) == 0) == ((i & k) == 0);
            key[r] = keep_min ? min(key[r], o) : max(key[r], o);
          }
        } else {  // partner in register r ^ j of this lane
#pragma unroll
          for (uint32_t r = 0; r < E; ++r) {
            if (r & j) continue;
            const bool up = ((lane * E + r) & k) == 0;
            const uint32_t a = key[r], b = key[r | j];
            key[r] = up ? min(a, b) : max(a, b);
            key[r | j] = up ? max(a, b) : min(a, b);
          }
        }
      }
#pragma unroll
    for (uint32_t r = 0; r < E; ++r) skw[lane * E + r] = key[r];
    wave_lds_sync();
    uint32_t* rwg = (uint32_t*)w.recv;
    uint32_t* cwg = (uint32_t*)w.crash;
    bool any_inf = false;
    // run heads of this lane's elements
    uint32_t head = 0;
#pragma unroll
    for (uint32_t r = 0; r < E; ++r) {
      const uint32_t i = lane * E + r;
      if (key[r] != ~0u && !(i > 0 && (skw[i - 1] >> 5) == (key[r] >> 5))) head |= 1u << r;
    }
    // one run head at a time, keys re-read from LDS: the body (two Philox
    // draws) is emitted once, not E times (the E = 16 instance's unrolled
    // body outgrew the instruction cache)
#pragma unroll 1
    for (uint32_t r = 0; r < E; ++r) {
      if (!((head >> r) & 1u)) continue;
      const uint32_t i = lane * E + r;
      const uint32_t loc = skw[i] >> 5;
      const uint32_t wi = ((f << kFineLog) + loc) >> 5, bit = 1u << (loc & 31), u = knode0 + loc;
      const uint32_t cw = cwg[wi];
      bool rv = (rwg[wi] & bit) != 0, cr = (cw & bit) != 0, inf = false;
      uint32_t tinf = 0;
      for (uint32_t q = i; q < N;) {  // along the run, one (node, tick) group at a time
        const uint32_t e = skw[q];
        if ((e >> 5) != loc) break;  // (~0u never matches a loc)
        const uint32_t k = (e >> 1) & (kMaxWindow - 1), t = t0 + k;
        uint32_t c = 0, ones = 0;  // receipts, crash rolls among them
        for (; q < N && (skw[q] >> 1) == (e >> 1); ++q) {
          ++c;
          ones += skw[q] & 1u;
        }
        if (cr) {                                                   // :108 not counted
          atomicAdd(&st[wv][k][0], c);
          continue;
        }
        // rule A6: counted up to the first crash, informed if a receipt came first
        const uint32_t g = ones ? first_crash(u, t, c, ones, c3order, w.key.k0, w.key.k1) : c + 1;
        if (g > 1 && !rv) {                                         // :117-121
          rv = inf = true;
          tinf = t;
          atomicAdd(&st[wv][k][1], 1u);
        }
        if (g <= c) {                                               // :112-115
          cr = true;
          atomicAdd(&st[wv][k][2], 1u);
          if (c > g) atomicAdd(&st[wv][k][0], c - g);
        }
      }
      if (cr && !(cw & bit)) atomicOr(&cwg[wi], bit);
      if (inf) {  // Broadcast() (:122, :141-142): fire at tinf + off
        any_inf = true;
        atomicOr(&rwg[wi], bit);
        const uint32_t off = fire_offset(w.delay_low, w.delay_span,
                                         philox(u, tinf, 0, c3delay, w.key.k0, w.key.k1).x);
        const uint32_t slot = (tinf + off) % w.R;
        const uint32_t pos = atomicAdd(&fcw[slot], 1u);
        w.flist[((size_t)slot * w.nfine + f) * kFineNodes + pos] = (uint16_t)loc;
      }
    }
    wave_lds_sync();
    if (__ballot(any_inf)) {
      for (uint32_t s = lane; s < w.R; s += 64) w.fcount[(size_t)s * w.nfine + f] = fcw[s];
    } else if (consume && lane < L) {
      w.fcount[(size_t)((t0 + lane) % w.R) * w.nfine + f] = 0;
    }
    if (w.tstat) {  // batched trials: this bucket's counters go to its trial's rows
      wave_lds_sync();
      if (lane < L * 3) {
        const uint32_t k = lane / 3, fld = lane - k * 3;
        const uint32_t v = st[wv][k][fld];
        const uint32_t trial = (uint32_t)(((uint64_t)w.base + (f << kFineLog)) >> w.tlog);
        if (v) atomicAdd(&w.tstat[((size_t)trial * kMaxWindow + w.tofs + k) * kTStatFields + TS_DEAD + fld], v);
      }
    }
  }
}

// One launch for all sizes: each wave takes one bucket and the body by its
// receipt count (wave-uniform).
template <bool ROLLED>
__device__ __forceinline__ void resolve_small_body(const WinState& w, uint32_t t0, uint32_t L) {
  constexpr uint32_t kWaves = (ROLLED ? kRolledBlock : kSmallBlock) / 64;
  constexpr uint32_t kEmax = ROLLED ? 16 : 4;
  __shared__ uint32_t st[kWaves][kMaxWindow][4];  // per wave: dead (not counted), recv, crash per tick
  __shared__ uint32_t sk[kWaves][64 * kEmax];      // each wave's sorted keys
  __shared__ uint32_t fcw[kWaves][kWinMaxRing];    // each wave's bucket: fire-list lengths per ring slot
  const uint32_t tid = threadIdx.x, wv = tid >> 6;
  static_assert(kWaves * kMaxWindow * 4 == kWaves * 64, "one counter per thread");
  static_assert(kRolledCap == 64 * 16, "the rolled bodies cover 1..kRolledCap");
  const uint32_t f = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wv);
  // the bucket's size and start are loaded while the window check is in
  // flight (unused when the window is dead)
  unsigned long long M = 0;
  const uint32_t* gm = nullptr;
  if (f < w.nfine) {
    if (ROLLED) {
      M = w.rlcnt[f];
      gm = w.rlmsg + (size_t)f * kRolledCap;
    } else {
      M = w.ffill[f];
      gm = w.fmsg + w.fstart[f];
    }
  }
  L = win_live(w, t0, L);
  if (!L) return;
  (&st[0][0][0])[tid] = 0;
  __syncthreads();
  if (M > 0 && M <= 64) resolve_small_bucket<1, ROLLED>(w, t0, L, f, gm, M, st, sk[wv], fcw[wv]);
  else if (M > 64 && M <= 256) resolve_small_bucket<4, ROLLED>(w, t0, L, f, gm, M, st, sk[wv], fcw[wv]);
  else if (ROLLED && M > 256 && M <= 512)
    resolve_small_bucket<ROLLED ? 8 : 1, ROLLED>(w, t0, L, f, gm, M, st, sk[wv], fcw[wv]);
  else if (ROLLED && M > 512 && M <= kRolledCap)
    resolve_small_bucket<ROLLED ? 16 : 1, ROLLED>(w, t0, L, f, gm, M, st, sk[wv], fcw[wv]);
  if (ROLLED && M && (threadIdx.x & 63) == 0) w.rlcnt[f] = 0;  // consumed
  // device-driven windows: the window's fire lists of the buckets the body
  // did not take are consumed here (see resolve_small_bucket); k_resolve and
  // the rolled replay run after this kernel
  if (!ROLLED && w.ctl && !(M > 0 && M <= 256) && f < w.nfine && (threadIdx.x & 63) < L)
    w.fcount[(size_t)((t0 + (threadIdx.x & 63)) % w.R) * w.nfine + f] = 0;
  __syncthreads();
  if (tid < L * 3) {
    const uint32_t k = tid / 3, fld = tid - k * 3;
    uint32_t v = 0;
    for (uint32_t q = 0; q < kWaves; ++q) v += st[q][k][fld];
    unsigned long long* row = shard_row(w, k);
    if (v && fld == 0) atomicAdd(&row[ST_MSGS], 0ull - (unsigned long long)v);
    if (v && fld == 1) {
      atomicAdd(&row[ST_RECV], (unsigned long long)v);
      atomicAdd(&row[ST_SCHED], (unsigned long long)v);  // every infection schedules one Broadcast
    }
    if (v && fld == 2) atomicAdd(&row[ST_CRASH], (unsigned long long)v);
  }
}
template <bool ROLLED>
__global__ __launch_bounds__(ROLLED ? kRolledBlock : kSmallBlock) void k_resolve_small(const WinState w, uint32_t t0,
                                                                                       uint32_t L) {
  resolve_small_body<ROLLED>(w, t0, L);
}
template <bool ROLLED>
__global__ __launch_bounds__(ROLLED ? kRolledBlock : kSmallBlock) void k_resolve_small_m(
    const WinState* __restrict__ ws, uint32_t L) {
  resolve_small_body<ROLLED>(ws[blockIdx.y], 0u, L);
}

}  // namespace

// A/B switch GS_RESOLVE_OCC3=0: the two-per-CU k_resolve2 with its own large
// path; read once per process.
static bool resolve_occ3() {
  static const bool on = [] { const char* e = getenv("GS_RESOLVE_OCC3"); return !e || atoi(e) != 0; }();
  return on;
}

// GS_RESOLVE_GRID=<workgroups> (read once per process; 0 = unset): the
// persistent grid of k_resolve / k_resolve2 and their _m twins (per shard),
// so tests can make one workgroup own several buckets of a small table.  The
// kResolveMaxBuckets bound still holds.
static uint32_t resolve_grid_env() {
  static const uint32_t g = [] { const char* e = getenv("GS_RESOLVE_GRID"); return e ? (uint32_t)std::max(atoi(e), 1) : 0u; }();
  return g;
}

hipError_t win_resolve(const WinState& w, uint32_t t0, uint32_t L, hipStream_t s) {
  // persistent, each workgroup owning <= 256 buckets.  k_resolve: three
  // resident per CU, six queued (the second three even out the first three's
  // tails: 55.4 against 55.9 ms per C5 step; four, not a multiple of three,
  // 57.1).  k_resolve2: two, all resident.
  const uint32_t cus = device_cus();
  const bool occ3 = resolve_occ3();
  static const uint32_t per_cu_env = [] { const char* e = getenv("GS_RESOLVE_PER_CU"); return e ? (uint32_t)std::max(atoi(e), 1) : 0u; }();  // A/B knob
  const uint32_t per_cu = per_cu_env ? per_cu_env : occ3 ? 6u : 2u;
  uint32_t G = std::min<uint32_t>(w.nfine, resolve_grid_env() ? resolve_grid_env() : per_cu * cus);
  G = std::max<uint32_t>(G, (w.nfine + kResolveMaxBuckets - 1) / kResolveMaxBuckets);
  const uint32_t gs = (w.nfine + kSmallBlock / 64 - 1) / (kSmallBlock / 64);
  hipLaunchKernelGGL(k_resolve_small<false>, dim3(gs), dim3(kSmallBlock), 0, s, w, t0, L);
  static_assert(kSmallMax == 64 * 4, "the two bodies cover 1..kSmallMax");
  if (occ3) {
    hipLaunchKernelGGL(k_resolve, dim3(G), dim3(kResolveBlock), 0, s, w, t0, L);
    hipLaunchKernelGGL(k_resolve_large, dim3(std::min<uint32_t>(w.nfine, cus)), dim3(kResolveBlock), 0, s, w, t0, L);
  } else {
    hipLaunchKernelGGL(k_resolve2, dim3(G), dim3(kResolveBlock), 0, s, w, t0, L);
  }
  // k_resolve_rolled: small blocks (the E = 16 key arrays take 4 KB per wave; blocks finish independently)
  hipLaunchKernelGGL(k_resolve_small<true>, dim3((w.nfine + kRolledBlock / 64 - 1) / (kRolledBlock / 64)),
                     dim3(kRolledBlock), 0, s, w, t0, L);
  return hipGetLastError();
}

hipError_t win_resolve_g(const WinGroup& g, uint32_t L, hipStream_t s) {
  const uint32_t cus = device_cus();
  // k_resolve's resident workgroups per CU split over the shards (each still
  // owns <= kResolveMaxBuckets buckets of its shard)
  const bool occ3 = resolve_occ3();
  uint32_t G = std::min<uint32_t>(g.nfine_max,
                                  resolve_grid_env() ? resolve_grid_env() : ((occ3 ? 3 : 2) * cus + g.M - 1) / g.M);
  G = std::max<uint32_t>(G, (g.nfine_max + kResolveMaxBuckets - 1) / kResolveMaxBuckets);
  const uint32_t gs = (g.nfine_max + kSmallBlock / 64 - 1) / (kSmallBlock / 64);
  hipLaunchKernelGGL(k_resolve_small_m<false>, dim3(gs, g.M), dim3(kSmallBlock), 0, s, g.wr, L);
  if (occ3) {
    hipLaunchKernelGGL(k_resolve_m, dim3(G, g.M), dim3(kResolveBlock), 0, s, g.wr, L);
    hipLaunchKernelGGL(k_resolve_large_m, dim3(std::min<uint32_t>(g.nfine_max, (cus + g.M - 1) / g.M), g.M),
                       dim3(kResolveBlock), 0, s, g.wr, L);
  } else {
    hipLaunchKernelGGL(k_resolve2_m, dim3(G, g.M), dim3(kResolveBlock), 0, s, g.wr, L);
  }
  hipLaunchKernelGGL(k_resolve_small_m<true>, dim3((g.nfine_max + kRolledBlock / 64 - 1) / (kRolledBlock / 64), g.M),
                     dim3(kRolledBlock), 0, s, g.wr, L);
  return hipGetLastError();
}

}  // namespace gs
