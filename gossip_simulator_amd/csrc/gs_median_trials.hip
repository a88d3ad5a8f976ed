// gs_median_trials.hip -- batched Monte Carlo trials of the median-counter
// model (GS_MODEL_MEDIAN with trials > 1 through gs_create_batch; DESIGN.md
// section 4.8.1, "trial-resident rounds").
//
// One workgroup runs one trial, as in k_rmt_rounds (gs_rumor_trials.hip): the
// plan arithmetic, the launch plumbing and the host loops are shared with it
// and with push-pull (gs_trial_plan.h, gs_trials_host.cpp), the device code
// is this engine's own (DESIGN.md section 4.10 says why).  The kernel has the
// transition table of k_median_round and
// k_median_commit (gs_median.hip).  The trial's state lives in LDS (plan:
// gs_mdt_plan.h): the state bytes `st` every decision of the round reads, the
// signed word `diff` = ge - lt of a B node's partners this round, and the
// bitsets `gotb` and `gotc`.  A launch loads st from the trial's slot of
// global memory, runs up to kMaxWindow rounds between workgroup barriers with
// no global atomic, and stores st back with the informed words rebuilt from
// it; it writes one tstat row per round.
//
// A wave takes one 64-node word at a time, a lane per node.  A connection has
// two ends, and both are partners alike: the caller's lane adds +-1 to
// diff[v] (v in B), or sets v's bit of gotb (v in A, u in B) or gotc (u in C)
// -- the wave's own word, one OR per wave -- and it adds +-1 to diff[u] or ORs
// u's bit of gotb / gotc for the callee's end.  There is no own[] array.  A
// self-call is one connection with two ends: two adds to diff[v].  Only the
// sign of ge - lt is ever read and |ge - lt| <= n + 1, so one LDS atomicAdd of
// +-1 is exact for every table.  st changes only in the commit half, each lane
// its own byte, behind a barrier; the commit also zeroes the lane's diff and
// the wave's own flag words.  Nothing depends on wave or atomic order.
//
// GS_FLAG_MEDIAN_PACKED: k_mdt16_rounds is the same
// code on the plan of gs_mdt16_plan.h, where diff is a 16-bit field per node,
// two to a 32-bit word.  Only where a +-1 goes and how the commit reads and
// clears it differ (Tally32, Tally16); a table whose in-degrees could overflow
// a field is refused before the first round (k_mdt_count_named).
//
// Layout (the batched layout of gs_ctx.cpp): global node trial << tlog | v,
// deg, rows and state bytes at that index, the trial's words at word offset
// (trial << tlog) / 64 (tlog >= 14: whole words, disjoint per trial).  Padding
// nodes v >= n never call and are never counted; a target u >= n after masking
// never indexes LDS.  A failure mask is read from the trial's words of
// s.crash (read-only, L2-resident): the kMasked instantiation; the other has
// no trace of it.
#include "gs_internal.h"
#include "gs_mdt16_plan.h"
#include "gs_wave.h"

namespace gs {

namespace {

static_assert(kMdtCounters <= kTStatFields && TS_MSGS < kTStatFields && TS_HOT < kTStatFields,
              "a tstat row holds the round's counters");
static_assert(kMdtWordBytes == 336 && kMdtScratchBytes == 320, "the plan DESIGN.md section 4.8.1 states");
static_assert(kMdt16WordBytes == 208, "the plan DESIGN.md section 4.8.2 states");

constexpr uint32_t kDone = 255;  // gs_median.h's kMedianDone

// One trial's LDS (mdt_plan's layout) and its slot of the global arrays.
struct MdtTrial {
  int* diff;                       // [64 W]; packed: u16[64 W], seen as u32[32 W] (gs_mdt16_plan.h)
  unsigned long long *gotb, *gotc; // [W]
  uint32_t* scratch;               // [kMdtCounters][nwaves]
  uint8_t* st;                     // [64 W]
  const uint8_t* __restrict__ deg;
  const uint32_t* __restrict__ ids;
  const unsigned long long* __restrict__ fw;  // kMasked: the trial's failed words
  uint32_t W, tmask, c3;
};

__device__ __forceinline__ bool active(uint32_t s) { return s != 0 && s != kDone; }

// Where a +-1 on a node's tally goes and how the commit reads and clears it:
// all that the two plans' rounds differ in.  kDiff8: the tallies' 8-byte words
// per 64 nodes; kInit8: such a word with every tally at ge - lt = 0.
struct Tally32 {  // gs_mdt_plan.h: a signed word per node
  static constexpr uint32_t kDiff8 = 32;
  static constexpr unsigned long long kInit8 = 0;
  static __device__ __forceinline__ void add(const MdtTrial& T, uint32_t v, bool up) {
    atomicAdd(&T.diff[v], up ? 1 : -1);
  }
  static __device__ __forceinline__ int take(const MdtTrial& T, uint32_t v) {
    const int df = T.diff[v];
    if (df) T.diff[v] = 0;
    return df;
  }
};
// gs_mdt16_plan.h: a 16-bit field per node, two to a word.  The round half
// touches a word with 32-bit LDS atomics only, the commit half with 16-bit
// accesses to the lane's own half only, and a workgroup barrier is between
// the two: no access of one kind is ever concurrent with one of the other.
struct Tally16 {
  static constexpr uint32_t kDiff8 = 16;
  static constexpr unsigned long long kInit8 = ((unsigned long long)kMdt16Init << 32) | kMdt16Init;
  static __device__ __forceinline__ void add(const MdtTrial& T, uint32_t v, bool up) {
    atomicAdd((uint32_t*)T.diff + mdt16_word(v), mdt16_delta(v, up));
  }
  static __device__ __forceinline__ int take(const MdtTrial& T, uint32_t v) {
    return mdt16_take((uint32_t*)T.diff, v);
  }
};

// k_median_round on the trial's LDS: every live node with a friend that is not
// done calls; both ends of a connection go to diff, gotb and gotc.
template <bool kMasked, class Tally>
__device__ __forceinline__ void mdt_round(const MdtState& s, const MdtTrial& T, uint32_t t, uint32_t& fired,
                                          uint32_t& sent, uint32_t& msgs) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const uint32_t k = s.k;
  for (uint32_t w = wave; w < T.W; w += nwaves) {  // wave-uniform
    const uint32_t v = (w << 6) + lane;
    const uint32_t sv = T.st[v];  // (padding: 0)
    uint32_t d = v < s.n ? T.deg[v] : 0u;
    if (kMasked && ((T.fw[w] >> lane) & 1)) d = 0;  // failed: never calls
    bool ownb = false, ownc = false;
    if (d > 0 && sv != kDone) {  // a live node with a friend calls until it is done
      const u32x4 rr = philox(v, t, 0, T.c3, s.key.k0, s.key.k1);
      const uint32_t j = uniform(rr.x, d);
      ++fired;
      if ((int32_t)uniform(rr.y, 100u) >= s.kd) {  // the call is kept
        ++sent;
        const uint32_t u = T.ids[(size_t)v * s.stride + j] & T.tmask;
        const unsigned long long ubit = 1ull << (u & 63);
        if (u < s.n && !(kMasked && (T.fw[u >> 6] & ubit))) {  // a live callee: a connection
          const uint32_t su = T.st[u];  // (u == v: v is its own partner, once for each end)
          const bool av = active(sv), au = active(su);
          msgs += (uint32_t)av + (uint32_t)au;  // the caller pushes, the callee answers
          // v's end: its partner u
          if (au) {
            if (su > k) ownc = sv <= k;         // a C partner (only an A or B node keeps count)
            else if (sv == 0) ownb = true;      // an A caller: a B partner
            else if (sv <= k) Tally::add(T, v, su >= sv);
          } else if (su == 0 && av && sv <= k) {
            Tally::add(T, v, false);
          }
          // u's end: its partner v.  Only an A or B callee keeps count.
          if (su <= k) {
            if (sv > k) {  // a C caller (sv is not D here)
              unsigned long long* f = T.gotc + (u >> 6);
              if (!(*f & ubit)) atomicOr(f, ubit);  // thousands of callers may share one word
            } else if (su == 0) {
              if (sv) {  // a B caller informs an A callee
                unsigned long long* f = T.gotb + (u >> 6);
                if (!(*f & ubit)) atomicOr(f, ubit);
              }
            } else {  // u in B-su, v in A or B-sv
              Tally::add(T, u, sv >= su);
            }
          }
        }
      }
    }
    // the callers' own flags: the wave's own words, which other waves OR into too
    const unsigned long long bb = __ballot(ownb), bc = __ballot(ownc);
    if (lane == 0) {
      if (bb) atomicOr(&T.gotb[w], bb);
      if (bc) atomicOr(&T.gotc[w], bc);
    }
  }
}

// k_median_commit per word: the transition table, the lane's diff and the
// wave's flag words zeroed; newly = the nodes informed this round, nact = the
// active nodes after it.
template <class Tally>
__device__ __forceinline__ void mdt_commit(const MdtState& s, const MdtTrial& T, uint32_t& newly, uint32_t& nact) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const uint32_t k = s.k;
  for (uint32_t w = wave; w < T.W; w += nwaves) {
    const uint32_t v = (w << 6) + lane;
    const unsigned long long gb = T.gotb[w], gc = T.gotc[w];
    const uint32_t s0 = T.st[v];
    uint32_t s1 = s0;
    const bool c = (gc >> lane) & 1;
    if (s0 == 0) {
      if (c) s1 = k + 1;
      else if ((gb >> lane) & 1) s1 = 1;
    } else if (s0 <= k) {
      const int df = Tally::take(T, v);
      if (c) s1 = k + 1;
      else if (df > 0) s1 = s0 < k ? s0 + 1 : k + 1;
    } else if (s0 != kDone) {
      s1 = s0 == 2 * k ? kDone : s0 + 1;
    }
    if (s1 != s0) T.st[v] = (uint8_t)s1;
    const unsigned long long fresh = __ballot(s0 == 0 && s1 != 0), act = __ballot(active(s1));
    if (lane == 0) {  // the wave's own words
      if (gb) T.gotb[w] = 0;
      if (gc) T.gotc[w] = 0;
      newly += (uint32_t)__popcll(fresh);
      nact += (uint32_t)__popcll(act);
    }
  }
}

// Rounds t0 .. t0 + rounds - 1 (rounds <= kMaxWindow) of every trial; row k of
// a trial's tstat block gets round t0 + k's counters (TS_MSGS = the active
// ends of the round's connections, TS_HOT = the active nodes after the round).
//
// A round is two halves with a barrier after each.  The round half reads st as
// it was at the start of the round and builds diff, gotb and gotc; the commit
// half turns them into the new states, each node by its own lane, and leaves
// them zero for the next round.  The waves' counter sums go to scratch before
// the second barrier and one lane writes the row after it; scratch is not
// written again before the next round's first barrier.
//
// A trial is never skipped: after its own end its A nodes still call and are
// counted, as in the one-trial context.
template <bool kMasked, class Tally>
__device__ __forceinline__ void mdt_trial_rounds(const MdtState s, uint32_t t0, uint32_t rounds) {
  extern __shared__ unsigned long long mdt_lds[];
  constexpr uint32_t kD8 = Tally::kDiff8;
  const uint32_t trial = blockIdx.x;
  uint32_t* __restrict__ rows = s.tstat + (size_t)trial * kMaxWindow * kTStatFields;
  const uint32_t W = (s.n + 63) >> 6;
  const uint64_t base = (uint64_t)trial << s.tlog;
  MdtTrial T;
  T.W = W;
  T.diff = (int*)mdt_lds;                      // kD8 W words of 8 bytes
  T.gotb = mdt_lds + kD8 * (size_t)W;
  T.gotc = mdt_lds + (kD8 + 1) * (size_t)W;
  T.scratch = (uint32_t*)(mdt_lds + (kD8 + 2) * (size_t)W);
  T.st = (uint8_t*)(T.scratch + kMdtCounters * (kMdtMaxBlock / 64));
  T.deg = s.deg + base;
  T.ids = s.ids + base * s.stride;
  T.fw = kMasked ? s.crash + (base >> 6) : nullptr;
  T.tmask = (uint32_t)((1ull << s.tlog) - 1);
  T.c3 = ctr3(K_MEDIAN, s.key.trial + trial);
  unsigned long long* __restrict__ gw = s.recv + (base >> 6);
  unsigned long long* __restrict__ gs8 = (unsigned long long*)(s.st + base);  // 64 W bytes = 8 W words
  unsigned long long* ls8 = (unsigned long long*)T.st;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;

  for (uint32_t i = threadIdx.x; i < (kD8 + 2) * W; i += blockDim.x)  // diff, gotb, gotc
    mdt_lds[i] = i < kD8 * W ? Tally::kInit8 : 0ull;
  for (uint32_t i = threadIdx.x; i < 8 * W; i += blockDim.x) ls8[i] = gs8[i];
  __syncthreads();
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t t = t0 + r;
    uint32_t fired = 0, sent = 0, msgs = 0, newly = 0, nact = 0;
    mdt_round<kMasked, Tally>(s, T, t, fired, sent, msgs);
    __syncthreads();
    mdt_commit<Tally>(s, T, newly, nact);
    const uint32_t v5[kMdtCounters] = {fired, sent, msgs, newly, nact};
#pragma unroll
    for (uint32_t i = 0; i < kMdtCounters; ++i) {
      const uint32_t x = wave_sum(v5[i]);
      if (lane == 0) T.scratch[i * nwaves + wave] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one lane sums the waves' parts and writes the trial's row
      uint32_t tot[kMdtCounters];
      for (uint32_t i = 0; i < kMdtCounters; ++i) {
        tot[i] = 0;
        for (uint32_t q = 0; q < nwaves; ++q) tot[i] += T.scratch[i * nwaves + q];
      }
      uint32_t* row = rows + (size_t)r * kTStatFields;
      row[TS_FIRED] = tot[0];
      row[TS_SENT] = tot[1];
      row[TS_MSGS] = tot[2];
      row[TS_RECV] = tot[3];
      row[TS_DEAD] = row[TS_CRASH] = 0;
      row[TS_HOT] = tot[4];
    }
  }
  // (the last commit's writes to st are behind the round's second barrier)
  for (uint32_t i = threadIdx.x; i < 8 * W; i += blockDim.x) gs8[i] = ls8[i];
  for (uint32_t w = wave; w < W; w += nwaves) {  // the informed words, rebuilt from st
    const unsigned long long inf = __ballot(T.st[(w << 6) + lane] != 0);
    if (lane == 0) gw[w] = inf;
  }
}

}  // namespace

template <bool kMasked>
__global__ __launch_bounds__(kMdtMaxBlock) void k_mdt_rounds(const MdtState s, uint32_t t0, uint32_t rounds) {
  mdt_trial_rounds<kMasked, Tally32>(s, t0, rounds);
}

// k_mdt_rounds on the packed plan (gs_mdt16_plan.h):
// the same rounds with 16-bit tallies, exact for the tables mdt_count_named
// lets through.
template <bool kMasked>
__global__ __launch_bounds__(kMdtMaxBlock) void k_mdt16_rounds(const MdtState s, uint32_t t0, uint32_t rounds) {
  mdt_trial_rounds<kMasked, Tally16>(s, t0, rounds);
}

// The sender of every trial: `node` in each, or (~0u) the trial's own keyed
// sender (k_ppt_seed's rule).  A thread per trial; trials own disjoint words
// and bytes.  As k_median_seed leaves a one-trial context: a live sender is
// B-1, a failed one starts nothing.  st zeroed by the caller.
__global__ void k_mdt_seed(const MdtState s, uint32_t node, uint32_t* __restrict__ started) {
  const uint32_t trial = blockIdx.x * blockDim.x + threadIdx.x;
  if (trial >= s.trials) return;
  uint32_t v = node;
  if (node == ~0u)
    v = uniform(philox(0, 0, 0, ctr3(K_SENDER, s.key.trial + trial), s.key.k0, s.key.k1).x, s.n);
  const uint64_t g = ((uint64_t)trial << s.tlog) + v;
  const unsigned long long bit = 1ull << (g & 63);
  const bool ok = !s.crash || !(s.crash[g >> 6] & bit);
  if (ok) {
    s.recv[g >> 6] |= bit;
    s.st[g] = 1;
  }
  started[trial] = ok ? 1u : 0u;
}

// Tables back to back in device memory (deg [trials * n], ids [trials * n *
// stride], ids local to their trial) into the padded id space (zeroed by the
// caller): node trial << tlog | v, ids with the trial's bits.  err: bit 0 = a
// row longer than the stride, bit 1 = a friend id >= n (validate_table's).
__global__ void k_mdt_spread(const uint8_t* __restrict__ deg, const uint32_t* __restrict__ ids, uint32_t n,
                             uint32_t trials, uint32_t tlog, uint32_t stride, uint8_t* __restrict__ odeg,
                             uint32_t* __restrict__ oids, uint32_t* err) {
  const uint64_t total = (uint64_t)trials * n;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t trial = (uint32_t)(i / n), v = (uint32_t)(i % n);
    const uint32_t d = deg[i];
    if (d > stride) {
      atomicOr(err, 1u);
      continue;
    }
    const uint64_t g = ((uint64_t)trial << tlog) + v;
    odeg[g] = (uint8_t)d;
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t x = ids[i * stride + j];
      if (x >= n) atomicOr(err, 2u);
      else oids[g * stride + j] = (trial << tlog) | x;
    }
  }
}

// The packed tallies' in-degree guard, over the
// padded nodes of trials [t_lo, t_hi): cnt[g - (t_lo << tlog)] = the used slots
// of g's trial that name g.  Slots, not rows: a row that names a node twice
// calls it at most once a round, so the count is an upper bound on the callers.
__global__ void k_mdt_count_named(const MdtState s, uint32_t t_lo, uint32_t t_hi, uint32_t* __restrict__ cnt) {
  const uint64_t lo = (uint64_t)t_lo << s.tlog, total = ((uint64_t)t_hi << s.tlog) - lo;
  const uint32_t tmask = (uint32_t)((1ull << s.tlog) - 1);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = lo + i;
    if ((g & tmask) >= s.n) continue;  // padding
    const uint32_t d = s.deg[g];
    for (uint32_t j = 0; j < d && j < s.stride; ++j) {
      const uint32_t u = s.ids[g * s.stride + j] & tmask;
      if (u < s.n) atomicAdd(&cnt[(i & ~(uint64_t)tmask) + u], 1u);
    }
  }
}

// *worst = the lowest index into cnt whose count is above `bound` (~0: none).
__global__ void k_mdt_worst_named(const uint32_t* __restrict__ cnt, uint64_t total, uint32_t bound,
                                  unsigned long long* worst) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
    if (cnt[i] > bound) atomicMin(worst, (unsigned long long)i);
}

namespace {

const void* rounds_kernel(bool packed, bool masked) {
  if (packed) return masked ? (const void*)k_mdt16_rounds<true> : (const void*)k_mdt16_rounds<false>;
  return masked ? (const void*)k_mdt_rounds<true> : (const void*)k_mdt_rounds<false>;
}

}  // namespace

// What the device grants one workgroup of k_mdt_rounds or k_mdt16_rounds
// (trial_lds_limit, gs_trials_host.cpp).  (The masked instantiation has the
// same plan: the mask is not in LDS.)
hipError_t mdt_lds_limit(int device, bool packed, uint64_t* limit, const char** where) {
  return trial_lds_limit(device, rounds_kernel(packed, false), limit, where);
}

hipError_t mdt_prepare(int device, bool packed, uint32_t lds_bytes) {
  const void* f[] = {rounds_kernel(packed, false), rounds_kernel(packed, true)};
  return trial_raise_lds(device, f, 2, lds_bytes);
}

// s.crash set: the masked instantiation (the same LDS).  The plan checked is
// the one the context was made with.
hipError_t mdt_rounds(const MdtState& s, bool packed, uint32_t t0, uint32_t rounds, hipStream_t st) {
  if (rounds == 0) return hipSuccess;
  if (rounds > kMaxWindow || s.block == 0 || s.block > kMdtMaxBlock || s.lds_bytes == 0) return hipErrorInvalidValue;
  const MdtPlan plan = packed ? mdt16_plan(s.n, s.lds_bytes) : mdt_plan(s.n, s.lds_bytes);
  if (plan.lds_bytes != s.lds_bytes) return hipErrorInvalidValue;  // the kernel's own pointers
  MdtState arg = s;
  void* args[] = {&arg, &t0, &rounds};
  return hipLaunchKernel(rounds_kernel(packed, s.crash != nullptr), dim3(s.trials), dim3(s.block), args, s.lds_bytes,
                         st);
}

hipError_t mdt_count_named(const MdtState& s, uint32_t t_lo, uint32_t t_hi, uint32_t bound, uint32_t* cnt,
                           unsigned long long* worst, hipStream_t st) {
  if (t_lo >= t_hi || t_hi > s.trials) return hipErrorInvalidValue;
  const uint64_t total = (uint64_t)(t_hi - t_lo) << s.tlog;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_mdt_count_named, dim3(blocks), dim3(256), 0, st, s, t_lo, t_hi, cnt);
  hipLaunchKernelGGL(k_mdt_worst_named, dim3(blocks), dim3(256), 0, st, cnt, total, bound, worst);
  return hipGetLastError();
}

hipError_t mdt_seed(const MdtState& s, uint32_t node, uint32_t* started, hipStream_t st) {
  hipLaunchKernelGGL(k_mdt_seed, dim3((s.trials + 255) / 256), dim3(256), 0, st, s, node, started);
  return hipGetLastError();
}

hipError_t mdt_spread_table(const uint8_t* deg, const uint32_t* ids, uint32_t n, uint32_t trials, uint32_t tlog,
                            uint32_t stride, uint8_t* odeg, uint32_t* oids, uint32_t* err, hipStream_t st) {
  const uint64_t total = (uint64_t)trials * n;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_mdt_spread, dim3(blocks), dim3(256), 0, st, deg, ids, n, trials, tlog, stride, odeg, oids, err);
  return hipGetLastError();
}

}  // namespace gs
