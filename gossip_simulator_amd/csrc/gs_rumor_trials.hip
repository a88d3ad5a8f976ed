// gs_rumor_trials.hip -- batched Monte Carlo trials of the rumor model
// (GS_MODEL_RUMOR with trials > 1 through gs_create_trials; DESIGN.md section
// 4.7.2, "trial-resident rounds").
//
// One workgroup runs one trial, as in k_ppt_rounds (gs_pushpull_trials.hip).
// The plan arithmetic, the launch plumbing and the host loops are shared with
// it and with the median engine (gs_trial_plan.h, gs_trials_host.cpp); the
// device code is this engine's own (DESIGN.md section 4.10 says why).  The
// trial's state lives in LDS (plan:
// gs_rmt_plan.h): the bitsets `cur` (the informed set every decision of the
// round reads), `next` (the set being built) and `hot`, in feedback pull also
// `served` and `vain`, and unless GS_RUMOR_COIN a miss byte per node.  A launch
// loads them from the trial's slot of global memory, runs up to kMaxWindow
// rounds between workgroup barriers with no global atomic, and stores them
// back; it writes one tstat row per round.
//
// Every mode is dense over bitsets: a wave takes one 64-node word at a time, a
// lane per node; there are no lists.  A push round skips a word whose hot word
// is zero (one wave-uniform LDS read).  Draws, outcomes and counters are those
// of k_rumor_round, k_rumor_pull_round and k_rumor_pull_commit (gs_rumor.hip),
// keyed by the trial's own number, so trial i of the batch is a one-trial
// context with params.trial + i, trial i's table and trial i's mask.  Word w
// of every set is written by one wave only (the wave with w % nwaves), except
// the bits other waves OR into next, served and vain with LDS atomics; `cur`
// and `hot` change only in the commit half of a round, behind a barrier, so no
// outcome depends on wave or atomic order.
//
// Layout (the batched layout of gs_ctx.cpp): global node trial << tlog | v,
// deg, rows and miss bytes at that index, the trial's words at word offset
// (trial << tlog) / 64 (tlog >= 14: whole words, disjoint per trial).  Padding
// nodes v >= n never call and are never counted; a target u >= n after masking
// never indexes LDS.  A failure mask is read from the trial's words of
// s.crash (read-only, L2-resident): the kMasked instantiations; the others
// have no trace of it.
#include "gs_internal.h"
#include "gs_rmt_plan.h"
#include "gs_wave.h"

namespace gs {

namespace {

static_assert(kRmtBlind == kRumorBlind && kRmtCoin == kRumorCoin && kRmtPull == kRumorPull,
              "the plan's mode bits are the kernels'");
static_assert(kRmtCounters <= kTStatFields && TS_HOT < kTStatFields, "a tstat row holds the round's counters");

// One trial's LDS (rmt_plan's layout) and its slot of the global arrays.
struct RmtTrial {
  unsigned long long *cur, *next, *hot, *served, *vain;  // served, vain: feedback pull only
  uint32_t* scratch;                                     // [kRmtCounters][nwaves]
  uint8_t* miss;                                         // [64 W], unless a coin
  const uint8_t* __restrict__ deg;
  const uint32_t* __restrict__ ids;
  const unsigned long long* __restrict__ fw;             // kMasked: the trial's failed words
  uint32_t W, tmask, c3;
};

// One event of the lane's own hot node v: the coin, or the miss count.  True: v is removed.
template <uint32_t MODE>
__device__ __forceinline__ bool rmt_event(const RmtState& s, const RmtTrial& T, uint32_t v, uint32_t t) {
  if constexpr ((MODE & kRumorCoin) != 0) {
    return uniform(philox(v, t, 1, T.c3, s.key.k0, s.key.k1).x, s.k) == 0;
  } else {
    const uint32_t m = T.miss[v] + 1u;
    T.miss[v] = (uint8_t)m;
    return m >= s.k;
  }
}

// k_rumor_round on bitsets: every hot node calls; a kept call to a live u
// informs it (next) or, u informed at the start of the round, is a miss.  The
// removed leave the wave's own hot word here; the newly informed join it in
// rmt_push_commit.
template <uint32_t MODE, bool kMasked>
__device__ __forceinline__ void rmt_push_round(const RmtState& s, const RmtTrial& T, uint32_t t, uint32_t& fired,
                                               uint32_t& sent, uint32_t& msgs) {
  constexpr bool kBlind = (MODE & kRumorBlind) != 0;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (uint32_t w = wave; w < T.W; w += nwaves) {  // wave-uniform
    const unsigned long long Hw = T.hot[w];
    if (!Hw) continue;
    const uint32_t v = (w << 6) + lane;
    bool gone = false;
    if ((Hw >> lane) & 1) {  // hot: informed, live, v < n, a friend to call
      const u32x4 rr = philox(v, t, 0, T.c3, s.key.k0, s.key.k1);
      const uint32_t j = uniform(rr.x, T.deg[v]);
      ++fired;
      bool event = kBlind;  // blind: every round v is hot, reply or not
      if ((int32_t)uniform(rr.y, 100u) >= s.kd) {  // the call is kept
        ++sent;
        const uint32_t u = T.ids[(size_t)v * s.stride + j] & T.tmask;
        const unsigned long long ubit = 1ull << (u & 63);
        const bool in = u < s.n;
        if (!(kMasked && in && (T.fw[u >> 6] & ubit))) {  // u live: delivered, and u answers
          ++msgs;
          if (in) {
            if (T.cur[u >> 6] & ubit) event = true;  // u knew the rumor at the start of the round
            else atomicOr(&T.next[u >> 6], ubit);
          }
        }
      }
      if (event) gone = rmt_event<MODE>(s, T, v, t);
    }
    const unsigned long long bg = __ballot(gone);
    if (bg && lane == 0) T.hot[w] = Hw & ~bg;
  }
}

// cur = next; the newly informed with a friend are hot (an empty row: removed at once).
__device__ __forceinline__ void rmt_push_commit(const RmtTrial& T, uint32_t& newly, uint32_t& nhot) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (uint32_t w = wave; w < T.W; w += nwaves) {
    const unsigned long long a = T.next[w], nb = a & ~T.cur[w];
    unsigned long long h = T.hot[w];
    if (nb) {  // wave-uniform; a new bit is a node v < n
      h |= __ballot(((nb >> lane) & 1) && T.deg[(w << 6) + lane] > 0);
      if (lane == 0) {
        T.hot[w] = h;
        T.cur[w] = a;
      }
    }
    if (lane == 0) {
      newly += (uint32_t)__popcll(nb);
      nhot += (uint32_t)__popcll(h);
    }
  }
}

// k_rumor_pull_round: every live node with a friend calls, informed or not,
// hot or removed; a call that reaches a hot u informs an uninformed caller
// (u was served) or was in vain.
template <uint32_t MODE, bool kMasked>
__device__ __forceinline__ void rmt_pull_round(const RmtState& s, const RmtTrial& T, uint32_t t, uint32_t& fired,
                                               uint32_t& sent, uint32_t& msgs) {
  constexpr bool kBlind = (MODE & kRumorBlind) != 0;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (uint32_t w = wave; w < T.W; w += nwaves) {  // wave-uniform
    const uint32_t v = (w << 6) + lane;
    const unsigned long long Iw = T.cur[w];
    const bool informed = (Iw >> lane) & 1;
    uint32_t d = v < s.n ? T.deg[v] : 0u;
    if (kMasked && ((T.fw[w] >> lane) & 1)) d = 0;  // failed: never calls
    bool fresh = false;
    if (d > 0) {
      const u32x4 rr = philox(v, t, 0, T.c3, s.key.k0, s.key.k1);
      const uint32_t j = uniform(rr.x, d);
      ++fired;
      if ((int32_t)uniform(rr.y, 100u) >= s.kd) {  // the call is kept
        ++sent;
        const uint32_t u = T.ids[(size_t)v * s.stride + j] & T.tmask;
        const unsigned long long ubit = 1ull << (u & 63);
        const bool in = u < s.n;
        if (!(kMasked && in && (T.fw[u >> 6] & ubit))) {  // u live: delivered
          ++msgs;
          if (in && (T.hot[u >> 6] & ubit)) {  // u answers with the rumor
            fresh = !informed;
            if (!kBlind) {  // blind: u's event needs no feedback
              unsigned long long* f = (informed ? T.vain : T.served) + (u >> 6);
              if (!(*f & ubit)) atomicOr(f, ubit);  // many callers may share one bit
            }
          }
        }
      }
    }
    const unsigned long long bf = __ballot(fresh);
    if (bf && lane == 0) T.next[w] = Iw | bf;  // the wave's own word: no atomic
  }
}

// k_rumor_pull_commit per word: the round's events, the new hot word, cur = next.
template <uint32_t MODE>
__device__ __forceinline__ void rmt_pull_commit(const RmtState& s, const RmtTrial& T, uint32_t t, uint32_t& newly,
                                                uint32_t& nhot) {
  constexpr bool kBlind = (MODE & kRumorBlind) != 0;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (uint32_t w = wave; w < T.W; w += nwaves) {
    const unsigned long long H = T.hot[w];
    unsigned long long S = 0, V = 0;
    if (!kBlind) {
      S = T.served[w];
      V = T.vain[w];
    }
    const unsigned long long ev = kBlind ? H : (H & V & ~S);  // asked in vain and not served
    bool rm = false;
    if ((ev >> lane) & 1) rm = rmt_event<MODE>(s, T, (w << 6) + lane, t);
    const unsigned long long gone = __ballot(rm);
    const unsigned long long a = T.next[w], b = T.cur[w];
    const unsigned long long h = (H & ~gone) | (a ^ b);  // the newly informed are hot, miss = 0
    if (lane == 0) {
      if (h != H) T.hot[w] = h;
      if (S) T.served[w] = 0;
      if (V) T.vain[w] = 0;
      if (a != b) T.cur[w] = a;
      newly += (uint32_t)__popcll(a ^ b);
      nhot += (uint32_t)__popcll(h);
    }
  }
}

}  // namespace

// Rounds t0 .. t0 + rounds - 1 (rounds <= kMaxWindow) of every trial; row k of
// a trial's tstat block gets round t0 + k's counters (TS_DEAD = kept calls to a
// failed callee, TS_HOT = the hot nodes after the round).
//
// A round is two halves with a barrier after each.  The round half reads cur
// and hot as they were at the start of the round and builds next (and served,
// vain); the commit half turns them into events, the new hot set and
// cur = next, each word by its own wave, and leaves next == cur for the next
// round.  The waves' counter sums go to scratch before the second barrier and
// one lane writes the row after it; scratch is not written again before the
// next round's first barrier.
//
// A push trial with no hot node has empty rounds and its sets stay as they
// are, so its workgroup writes zero rows and loads nothing.  A pull trial is
// never skipped: every live node with a friend still calls and is counted.
template <uint32_t MODE, bool kMasked>
__global__ __launch_bounds__(kRmtMaxBlock) void k_rmt_rounds(const RmtState s, uint32_t t0, uint32_t rounds) {
  constexpr bool kPull = (MODE & kRumorPull) != 0, kFeedback = kPull && !(MODE & kRumorBlind);
  constexpr bool kMiss = !(MODE & kRumorCoin);
  constexpr uint32_t kSets = kFeedback ? 5 : 3;
  extern __shared__ unsigned long long rmt_lds[];
  const uint32_t trial = blockIdx.x;
  uint32_t* __restrict__ rows = s.tstat + (size_t)trial * kMaxWindow * kTStatFields;
  if (!kPull && s.nhot[trial] == 0) {  // block-uniform
    if (threadIdx.x < rounds) {
      uint32_t* row = rows + (size_t)threadIdx.x * kTStatFields;
      row[TS_FIRED] = row[TS_SENT] = row[TS_DEAD] = row[TS_RECV] = row[TS_CRASH] = row[TS_HOT] = 0;
    }
    return;
  }
  const uint32_t W = (s.n + 63) >> 6;
  const uint64_t base = (uint64_t)trial << s.tlog;
  RmtTrial T;
  T.W = W;
  T.cur = rmt_lds;
  T.next = rmt_lds + W;
  T.hot = rmt_lds + 2 * (size_t)W;
  T.served = rmt_lds + 3 * (size_t)W;  // kFeedback only
  T.vain = rmt_lds + 4 * (size_t)W;
  T.scratch = (uint32_t*)(rmt_lds + kSets * (size_t)W);
  T.miss = (uint8_t*)(T.scratch + kRmtCounters * (kRmtMaxBlock / 64));  // kMiss only
  T.deg = s.deg + base;
  T.ids = s.ids + base * s.stride;
  T.fw = kMasked ? s.crash + (base >> 6) : nullptr;
  T.tmask = (uint32_t)((1ull << s.tlog) - 1);
  T.c3 = ctr3(K_RUMOR, s.key.trial + trial);
  unsigned long long* __restrict__ gw = s.recv + (base >> 6);
  unsigned long long* __restrict__ gh = s.hot + (base >> 6);
  unsigned long long* __restrict__ gm = (unsigned long long*)(s.miss + base);  // 64 W bytes = 8 W words
  unsigned long long* lm = (unsigned long long*)T.miss;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;

  for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) {
    const unsigned long long c = gw[w];
    T.cur[w] = c;
    T.next[w] = c;
    T.hot[w] = gh[w];
    if (kFeedback) T.served[w] = T.vain[w] = 0;
  }
  if (kMiss)
    for (uint32_t i = threadIdx.x; i < 8 * W; i += blockDim.x) lm[i] = gm[i];
  __syncthreads();
  uint32_t last_hot = 0;  // thread 0's
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t t = t0 + r;
    uint32_t fired = 0, sent = 0, msgs = 0, newly = 0, nhot = 0;
    if (kPull) rmt_pull_round<MODE, kMasked>(s, T, t, fired, sent, msgs);
    else rmt_push_round<MODE, kMasked>(s, T, t, fired, sent, msgs);
    __syncthreads();
    if (kPull) rmt_pull_commit<MODE>(s, T, t, newly, nhot);
    else rmt_push_commit(T, newly, nhot);
    const uint32_t v5[kRmtCounters] = {fired, sent, msgs, newly, nhot};
#pragma unroll
    for (uint32_t i = 0; i < kRmtCounters; ++i) {
      const uint32_t x = wave_sum(v5[i]);
      if (lane == 0) T.scratch[i * nwaves + wave] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one lane sums the waves' parts and writes the trial's row
      uint32_t tot[kRmtCounters];
      for (uint32_t i = 0; i < kRmtCounters; ++i) {
        tot[i] = 0;
        for (uint32_t k = 0; k < nwaves; ++k) tot[i] += T.scratch[i * nwaves + k];
      }
      uint32_t* row = rows + (size_t)r * kTStatFields;
      row[TS_FIRED] = tot[0];
      row[TS_SENT] = tot[1];
      row[TS_DEAD] = tot[1] - tot[2];
      row[TS_RECV] = tot[3];
      row[TS_CRASH] = 0;
      row[TS_HOT] = last_hot = tot[4];
    }
  }
  for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) {
    gw[w] = T.cur[w];
    gh[w] = T.hot[w];
  }
  if (kMiss)
    for (uint32_t i = threadIdx.x; i < 8 * W; i += blockDim.x) gm[i] = lm[i];
  if (threadIdx.x == 0) s.nhot[trial] = last_hot;
}

// The sender of every trial: `node` in each, or (~0u) the trial's own keyed
// sender (k_ppt_seed's rule).  A thread per trial; trials own disjoint words.
// As k_rumor_seed and k_rumor_pull_seed leave a one-trial context: a failed
// sender starts nothing; a live one is informed, and hot if it has a friend
// (push) or in any case (pull).
__global__ void k_rmt_seed(const RmtState s, uint32_t node, uint32_t* __restrict__ started) {
  const uint32_t trial = blockIdx.x * blockDim.x + threadIdx.x;
  if (trial >= s.trials) return;
  uint32_t v = node;
  if (node == ~0u)
    v = uniform(philox(0, 0, 0, ctr3(K_SENDER, s.key.trial + trial), s.key.k0, s.key.k1).x, s.n);
  const uint64_t g = ((uint64_t)trial << s.tlog) + v;
  const unsigned long long bit = 1ull << (g & 63);
  const bool ok = !s.crash || !(s.crash[g >> 6] & bit);
  bool hot = false;
  if (ok) {
    s.recv[g >> 6] |= bit;
    hot = (s.mode & kRumorPull) || s.deg[g] > 0;
    if (hot) s.hot[g >> 6] |= bit;
  }
  started[trial] = ok ? 1u : 0u;
  s.nhot[trial] = hot ? 1u : 0u;
}

namespace {

template <uint32_t MODE>
const void* rounds_kernel_of(bool masked) {
  return masked ? (const void*)k_rmt_rounds<MODE, true> : (const void*)k_rmt_rounds<MODE, false>;
}

// The instantiation of gs_params.rumor_mode `mode`.
const void* rounds_kernel(uint32_t mode, bool masked) {
  switch (mode & 7u) {
    case 0: return rounds_kernel_of<0>(masked);
    case 1: return rounds_kernel_of<1>(masked);
    case 2: return rounds_kernel_of<2>(masked);
    case 3: return rounds_kernel_of<3>(masked);
    case 4: return rounds_kernel_of<4>(masked);
    case 5: return rounds_kernel_of<5>(masked);
    case 6: return rounds_kernel_of<6>(masked);
    default: return rounds_kernel_of<7>(masked);
  }
}

}  // namespace

// What the device grants one workgroup of this mode's kernel (trial_lds_limit,
// gs_trials_host.cpp).  (The masked instantiation has the same plan: the mask
// is not in LDS.)
hipError_t rmt_lds_limit(int device, uint32_t mode, uint64_t* limit, const char** where) {
  return trial_lds_limit(device, rounds_kernel(mode, false), limit, where);
}

hipError_t rmt_prepare(int device, uint32_t mode, uint32_t lds_bytes) {
  const void* f[] = {rounds_kernel(mode, false), rounds_kernel(mode, true)};
  return trial_raise_lds(device, f, 2, lds_bytes);
}

// s.crash set: the masked instantiation (the same LDS).
hipError_t rmt_rounds(const RmtState& s, uint32_t t0, uint32_t rounds, hipStream_t st) {
  if (rounds == 0) return hipSuccess;
  if (rounds > kMaxWindow || s.block == 0 || s.block > kRmtMaxBlock || s.lds_bytes == 0) return hipErrorInvalidValue;
  RmtState arg = s;
  void* args[] = {&arg, &t0, &rounds};
  return hipLaunchKernel(rounds_kernel(s.mode, s.crash != nullptr), dim3(s.trials), dim3(s.block), args, s.lds_bytes,
                         st);
}

hipError_t rmt_seed(const RmtState& s, uint32_t node, uint32_t* started, hipStream_t st) {
  hipLaunchKernelGGL(k_rmt_seed, dim3((s.trials + 255) / 256), dim3(256), 0, st, s, node, started);
  return hipGetLastError();
}

}  // namespace gs
