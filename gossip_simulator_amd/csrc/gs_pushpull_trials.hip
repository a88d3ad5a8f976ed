// gs_pushpull_trials.hip -- batched Monte Carlo trials of the push-pull model
// ("trial-resident rounds").
//
// One workgroup runs one trial.  The trial's informed set lives in LDS as two
// bitsets (`cur`, the set every call of the round reads, and `next`, the set
// being built), so a launch runs up to kMaxWindow consecutive rounds with no
// global atomic and no launch per round: the words are loaded from the
// context's recv bitset once, the rounds run between workgroup barriers, and
// the words are stored back.  Draws, outcomes and counters are those of
// k_pp_round (gs_pp_round.hip), keyed by the trial's own number: trial i of
// the batch is a one-trial context with params.trial + i and, when the batch
// has failure masks, trial i's mask (the kMasked instantiation below).
//
// Layout (the batched layout of gs_ctx.cpp): global node trial << tlog | v,
// deg and rows at that index, the trial's informed words at word offset
// (trial << tlog) / 64 of recv (tlog >= 14: whole words, disjoint per trial).
// Padding nodes v >= n of a trial's slot never call and are never counted.
// Wave64: a wave takes one 64-node word at a time, a lane per node, so the
// word's informed bits are one wave-uniform LDS read and its pulls one ballot.
#include "gs_internal.h"
#include "gs_ppt_plan.h"

namespace gs {

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;  // lane 0
}

// The waves' sums of the round's four counters into scratch (kPptCounters *
// nwaves u32 of LDS, counter-major); the caller's barrier publishes them.
__device__ __forceinline__ void wave_sums4(uint32_t* scratch, const uint32_t (&v)[kPptCounters]) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
  for (uint32_t i = 0; i < kPptCounters; ++i) {
    const uint32_t s = wave_sum(v[i]);
    if (lane == 0) scratch[i * nwaves + wave] = s;
  }
}

}  // namespace

// Rounds t0 .. t0 + rounds - 1 (rounds <= kMaxWindow) of every trial; row k of
// a trial's tstat block gets round t0 + k's counters (TS_DEAD = kept pushes
// that reached nobody: none without a failure mask).
//
// kMasked (per-trial failure masks, gs_set_failed on a batch): the trial's
// failed set F is a third bitset in LDS (ppt_plan_masked), loaded once per
// launch from the trial's words of s.crash and read-only.  k_pp_round's rules:
// a failed v has degree 0 for the round (not fired, never calls); a kept push
// to a failed u counts as sent and informs nobody (TS_DEAD); a pull needs no
// check, an informed u being live.  The wave's own word of F is one
// wave-uniform LDS read, a push target's failed bit one LDS gather.  The
// unmasked instantiation has none of it.
template <bool kMasked>
__global__ __launch_bounds__(kPptMaxBlock) void k_ppt_rounds(const PptState s, uint32_t t0, uint32_t rounds) {
  extern __shared__ unsigned long long ppt_lds[];
  const uint32_t W = (s.n + 63) >> 6;
  unsigned long long* cur = ppt_lds;
  unsigned long long* next = ppt_lds + W;
  unsigned long long* F = ppt_lds + 2 * (size_t)W;  // kMasked only; written by the load below alone
  uint32_t* scratch = (uint32_t*)(ppt_lds + (kMasked ? 3 : 2) * (size_t)W);
  const uint32_t trial = blockIdx.x;
  const uint64_t base = (uint64_t)trial << s.tlog;
  unsigned long long* __restrict__ gw = s.recv + (base >> 6);
  const uint8_t* __restrict__ deg = s.deg + base;
  const uint32_t* __restrict__ ids = s.ids + base * s.stride;
  const uint32_t tmask = (uint32_t)((1ull << s.tlog) - 1);
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial + trial);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  uint32_t* __restrict__ rows = s.tstat + (size_t)trial * kMaxWindow * kTStatFields;

  for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) cur[w] = gw[w];
  if (kMasked) {
    const unsigned long long* __restrict__ fw = s.crash + (base >> 6);
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) F[w] = fw[w];
  }
  __syncthreads();
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t t = t0 + r;
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) next[w] = cur[w];
    __syncthreads();
    uint32_t fired = 0, sent = 0, msgs = 0;
    for (uint32_t w = wave; w < W; w += nwaves) {  // wave-uniform
      const uint32_t v = (w << 6) + lane;
      const unsigned long long Iw = cur[w];
      uint32_t d = v < s.n ? deg[v] : 0u;
      if (kMasked && ((F[w] >> lane) & 1)) d = 0;  // failed: never calls
      bool pulled = false;
      if (d > 0) {
        const u32x4 x = philox(v, t, 0, c3, s.key.k0, s.key.k1);
        const uint32_t u = ids[(size_t)v * s.stride + uniform(x.x, d)] & tmask;
        const bool kept = (int32_t)uniform(x.y, 100u) >= s.kd;
        const unsigned long long ubit = 1ull << (u & 63);
        ++fired;
        if ((Iw >> lane) & 1) {  // informed: push (unmasked: every u is live)
          if (kept) {
            ++sent;
            if (!kMasked || u >= s.n || !(F[u >> 6] & ubit)) {  // u live: delivered
              ++msgs;
              if (u < s.n) atomicOr(&next[u >> 6], ubit);
            }
          }
        } else if (kept && u < s.n && (cur[u >> 6] & ubit)) {  // pull from an informed u
          ++sent;
          ++msgs;
          pulled = true;
        }
      }
      const unsigned long long bal = __ballot(pulled);
      if (lane == 0 && bal) atomicOr(&next[w], bal);
    }
    __syncthreads();
    uint32_t newly = 0;
    for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) newly += __popcll(next[w] & ~cur[w]);
    const uint32_t v4[kPptCounters] = {fired, sent, msgs, newly};
    uint32_t* row = rows + (size_t)r * kTStatFields;
    wave_sums4(scratch, v4);
    __syncthreads();
    if (threadIdx.x == 0) {  // one lane sums the waves' parts and writes the trial's row
      uint32_t tot[kPptCounters];
      for (uint32_t i = 0; i < kPptCounters; ++i) {
        tot[i] = 0;
        for (uint32_t k = 0; k < nwaves; ++k) tot[i] += scratch[i * nwaves + k];
      }
      row[TS_FIRED] = tot[0];
      row[TS_SENT] = tot[1];
      row[TS_DEAD] = tot[1] - tot[2];
      row[TS_RECV] = tot[3];
      row[TS_CRASH] = 0;
    }
    unsigned long long* tmp = cur;
    cur = next;
    next = tmp;
    __syncthreads();
  }
  for (uint32_t w = threadIdx.x; w < W; w += blockDim.x) gw[w] = cur[w];
}

// The sender of every trial is informed: `node` in each, or (~0u) the trial's
// own keyed sender (simulator.go:240 per trial).  A thread per trial; trials
// own disjoint words.  With a failure mask (s.crash) a trial whose sender is
// failed stays empty, as k_pp_seed leaves a one-trial context; started[trial]
// (when not null) = 1 if the trial's sender was informed.
__global__ void k_ppt_seed(const PptState s, uint32_t node, uint32_t* __restrict__ started) {
  const uint32_t trial = blockIdx.x * blockDim.x + threadIdx.x;
  if (trial >= s.trials) return;
  uint32_t v = node;
  if (node == ~0u)
    v = uniform(philox(0, 0, 0, ctr3(K_SENDER, s.key.trial + trial), s.key.k0, s.key.k1).x, s.n);
  const uint64_t g = ((uint64_t)trial << s.tlog) + v;
  const unsigned long long bit = 1ull << (g & 63);
  const bool ok = !s.crash || !(s.crash[g >> 6] & bit);
  if (ok) s.recv[g >> 6] |= bit;
  if (started) started[trial] = ok ? 1u : 0u;
}

// k_pp_live_edges restricted to one trial's rows and bits: live[trial] = 1 if
// some informed node has an uninformed friend or some uninformed node an
// informed one.  A workgroup per trial; only trials with need[trial] set are
// scanned (those whose last poll informed nobody new).  live is zeroed by the
// host; every writer stores the same 1.  With a failure mask (s.crash) the
// rule is k_pp_live_edges': a failed v makes no call, and an informed v's
// failed friend cannot be informed (an informed friend is always live).
__global__ __launch_bounds__(256) void k_ppt_stalled(const PptState s, const uint8_t* __restrict__ need,
                                                     uint32_t* __restrict__ live) {
  const uint32_t trial = blockIdx.x;
  if (!need[trial]) return;
  const uint64_t base = (uint64_t)trial << s.tlog;
  const unsigned long long* __restrict__ gw = s.recv + (base >> 6);
  const unsigned long long* __restrict__ fw = s.crash ? s.crash + (base >> 6) : nullptr;
  const uint32_t tmask = (uint32_t)((1ull << s.tlog) - 1);
  bool any = false;
  for (uint32_t v = threadIdx.x; v < s.n && !any; v += blockDim.x) {
    if (fw && ((fw[v >> 6] >> (v & 63)) & 1)) continue;
    const bool iv = (gw[v >> 6] >> (v & 63)) & 1;
    const uint32_t d = s.deg[base + v];
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t u = s.ids[(base + v) * s.stride + j] & tmask;
      if (u >= s.n) continue;
      const bool iu = (gw[u >> 6] >> (u & 63)) & 1;
      const bool fu = fw && ((fw[u >> 6] >> (u & 63)) & 1);
      if (iv ? (!iu && !fu) : iu) { any = true; break; }
    }
  }
  if (any) live[trial] = 1u;
}

namespace {

const void* rounds_kernel(bool masked) {
  return masked ? (const void*)k_ppt_rounds<true> : (const void*)k_ppt_rounds<false>;
}

}  // namespace

// What the device grants one workgroup of that instantiation (trial_lds_limit,
// gs_trials_host.cpp; the masked one has its own plan: F is in LDS).
hipError_t ppt_lds_limit(int device, bool masked, uint64_t* limit, const char** where) {
  return trial_lds_limit(device, rounds_kernel(masked), limit, where);
}

// Per instantiation: the unmasked one once per context, at create; the masked
// one when the context gets its mask (raising the limit again is idempotent).
hipError_t ppt_prepare(int device, bool masked, uint32_t lds_bytes) {
  const void* f = rounds_kernel(masked);
  return trial_raise_lds(device, &f, 1, lds_bytes);
}

// s.crash set: the masked instantiation with the masked plan's LDS.
hipError_t ppt_rounds(const PptState& s, uint32_t t0, uint32_t rounds, hipStream_t st) {
  if (rounds == 0) return hipSuccess;
  if (rounds > kMaxWindow) return hipErrorInvalidValue;
  if (s.crash) {
    if (s.lds_masked == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ppt_rounds<true>, dim3(s.trials), dim3(s.block), s.lds_masked, st, s, t0, rounds);
  } else {
    hipLaunchKernelGGL(k_ppt_rounds<false>, dim3(s.trials), dim3(s.block), s.lds_bytes, st, s, t0, rounds);
  }
  return hipGetLastError();
}

hipError_t ppt_seed(const PptState& s, uint32_t node, uint32_t* started, hipStream_t st) {
  hipLaunchKernelGGL(k_ppt_seed, dim3((s.trials + 255) / 256), dim3(256), 0, st, s, node, started);
  return hipGetLastError();
}

hipError_t ppt_stalled(const PptState& s, const uint8_t* need, uint32_t* live, hipStream_t st) {
  hipLaunchKernelGGL(k_ppt_stalled, dim3(s.trials), dim3(256), 0, st, s, need, live);
  return hipGetLastError();
}

}  // namespace gs
