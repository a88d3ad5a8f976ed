// gs_pp_dense.hip -- push-pull gossip rounds (extension, config C5): the
// model, the round's recipe over every mode (pp_round, pp_commit), and the
// top-down dense round's word summaries and commit.
//
// The reference only floods (simulator.go:140-149: every receipt re-broadcasts
// to every friend).  Config C5 asks for push-pull gossip as well; it has no
// reference semantics, so the model is the one oracle/gsoracle.h states (and
// DESIGN.md section 4.5): one tick = one synchronous round; every live node v with a
// non-empty friends list draws r = Philox{v, t, 0, PUSHPULL}, calls
// u = friends[v][U_deg(r.x)], and the call is lost iff U_100(r.y) < kd
// (the -droprate quantisation of simulator.go:172).  With I = informed set at
// the start of the round: v in I pushes to u (u informed iff live); v not in I
// pulls from u in I.  Failed nodes (gs_set_failed) never call or answer.
//
// Layout: one lane per node, one wave per 64-bit word of the bitsets, so a
// wave's pulls land in its own word with one atomicOr of the ballot.  Pushes
// scatter into `next` (atomicOr, only when u is neither informed nor failed);
// `next` starts every round equal to `recv`, and k_pp_commit makes
// recv = next and counts the newly informed.  Per round at N = 1e9: the
// friends table is streamed once (a wave's 64 rows are contiguous), the
// 125-MB recv bitset is gathered once per call (Infinity-Cache resident).
// Word summaries (k_pp_summary, one bit per 64-node word, 2 MB each, L2
// resident) skip that gather where its answer is known: a pull from a word
// with no informed node fails, and a push into a word with no live
// uninformed node changes nothing (without a failed mask).  A second level
// (k_pp_summary2, one bit per 4096-node block, 61 KB at N = 1e9) sits in LDS
// in front of them, so the early and late rounds, where almost every call is
// decided by the summaries, cost the table stream only.
//
// The round kernels of every mode (PPMode, gs_internal.h; k_pp_round too) and
// the tables they need are in the files gs_pp_dev.h lists (k_pp_round: gs_pp_round.hip).
#include "gs_pp_dev.h"

namespace gs {
namespace {

// sumA bit w = recv word w has an informed node; sumB bit w = it has a node
// that is neither informed nor failed (bits past n count as such: the
// summary only ever skips work whose outcome it proves).
__global__ __launch_bounds__(kPPBlock) void k_pp_summary(const DevState s, unsigned long long* __restrict__ sumA,
                                                         unsigned long long* __restrict__ sumB, const PPCtl* ctl) {
  if (ctl && ctl->mode != PP_DENSE) return;
  const uint64_t Wr = (s.W + 63) & ~63ull;  // whole waves stay in the loop together
  for (uint64_t w = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; w < Wr;
       w += (uint64_t)gridDim.x * kPPBlock) {
    unsigned long long r = 0, f = ~0ull;
    if (w < s.W) { r = s.recv[w]; f = s.crash[w]; }
    const unsigned long long a = __ballot(r != 0), b = __ballot(w < s.W && (r | f) != ~0ull);
    if ((threadIdx.x & 63) == 0) { sumA[w >> 6] = a; sumB[w >> 6] = b; }
  }
}

// Second level: bit j of sumA2/sumB2 = summary word j of sumA/sumB is non-zero.
__global__ __launch_bounds__(kPPBlock) void k_pp_summary2(const unsigned long long* __restrict__ sum1, uint64_t S1,
                                                          unsigned long long* __restrict__ sum2, uint64_t S2,
                                                          const PPCtl* ctl) {
  if (ctl && ctl->mode != PP_DENSE) return;
  const uint64_t Sr = (S1 + 63) & ~63ull;
  for (uint64_t j = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; j < Sr; j += (uint64_t)gridDim.x * kPPBlock) {
    const bool in = j < S1;
    const unsigned long long a = __ballot(in && sum1[j] != 0), b = __ballot(in && sum1[S1 + j] != 0);
    if ((threadIdx.x & 63) == 0) { sum2[j >> 6] = a; sum2[S2 + (j >> 6)] = b; }
  }
}

// *out = popcount of words[0, n) (n = 0: *out = 0).
__global__ __launch_bounds__(kPPBlock) void k_pp_count(const unsigned long long* __restrict__ words,
                                                       unsigned long long n, unsigned long long* out) {
  __shared__ uint64_t sh[kPPBlock / 64];
  if (n == 0) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = 0;
    return;
  }
  uint64_t c = 0;
  for (uint64_t w = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; w < n; w += (uint64_t)gridDim.x * kPPBlock)
    c += (uint64_t)__popcll(words[w]);
  const uint64_t ws = wave_sum64(c);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t b = 0;
    for (uint32_t k = 0; k < kPPBlock / 64; ++k) b += sh[k];
    if (b) atomicAdd(out, (unsigned long long)b);
  }
}

// dst[w] |= src[i * words + w] for every slice i < nslices (the bits other
// shards set in this shard's range during a pull-answer round).
__global__ __launch_bounds__(kPPBlock) void k_pp_or_slices(unsigned long long* __restrict__ dst,
                                                           const unsigned long long* __restrict__ src,
                                                           uint32_t nslices, uint64_t words) {
  for (uint64_t w = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; w < words; w += (uint64_t)gridDim.x * kPPBlock) {
    unsigned long long x = dst[w];
    for (uint32_t i = 0; i < nslices; ++i) x |= src[(size_t)i * words + w];
    dst[w] = x;
  }
}

__global__ __launch_bounds__(kPPBlock) void k_pp_commit(const DevState s,
                                                        const unsigned long long* __restrict__ next,
                                                        uint32_t t, PPCtl* ctl) {
  __shared__ uint64_t sh[kPPBlock / 64];
  if (ctl && ctl->mode == PP_EARLY) return;
  uint64_t newly = 0;
  for (uint64_t w = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; w < s.W;
       w += (uint64_t)gridDim.x * kPPBlock) {
    const unsigned long long nx = next[w], old = s.recv[w];
    newly += (uint64_t)__popcll(nx & ~old);
    if (nx != old) s.recv[w] = nx;
  }
  const uint64_t ws = wave_sum64(newly);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t b = 0;
    for (uint32_t k = 0; k < kPPBlock / 64; ++k) b += sh[k];
    if (b) {
      atomicAdd(&s.stats[(size_t)(t % kStatSlots) * kStatFields + ST_RECV], (unsigned long long)b);
      if (ctl) atomicAdd(&ctl->ninf, (unsigned long long)b);
    }
  }
}
}  // namespace

// One round: every mode's kernels are queued, and those whose mode the round
// (k_pp_mode, from PPCtl) is not in return at once.
hipError_t pp_round(const DevState& s, unsigned long long* next, unsigned long long* sum, uint32_t t,
                    bool l2_only_flag, const PPSparse& sp, hipStream_t st) {
  if (!pp_state_ok(s) || !next) return hipErrorInvalidValue;
  pp_launch_early(s, next, sp, t, st);
  unsigned long long* sumA = sum;
  unsigned long long* sumB = sum + pp_summary_words(s.W);
  const uint32_t sblocks = grid_for(s.W, kPPBlock, 4096);
  hipLaunchKernelGGL(k_pp_summary, dim3(sblocks), dim3(kPPBlock), 0, st, s, sumA, sumB, sp.ctl);
  const uint64_t S1 = pp_summary_words(s.W), S2 = pp_summary2_words(s.W);
  unsigned long long* sum2 = sum + 2 * S1;
  const uint32_t s2blocks = grid_for(S1, kPPBlock, 1024);
  hipLaunchKernelGGL(k_pp_summary2, dim3(s2blocks), dim3(kPPBlock), 0, st, sum, S1, sum2, S2, sp.ctl);
  pp_launch_topdown(s, next, sumA, sumB, sum2, S2, t, l2_only_flag, sp, st);
  pp_launch_answer(s, next, sp, t, st);
  return hipGetLastError();
}

hipError_t pp_commit(const DevState& s, const unsigned long long* next, uint32_t t, const PPSparse& sp,
                     hipStream_t st) {
  const uint32_t blocks = grid_for(s.W, kPPBlock, 2048);
  hipLaunchKernelGGL(k_pp_commit, dim3(blocks), dim3(kPPBlock), 0, st, s, next, t, sp.ctl);
  pp_launch_early_commit(s, next, sp, t, st);
  return hipGetLastError();
}

hipError_t pp_count(const unsigned long long* words, uint64_t nwords, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(k_pp_count, dim3(1), dim3(1), 0, st, words, 0ull, out);  // zero the total
  const uint32_t blocks = grid_for(nwords, kPPBlock, 2048);
  hipLaunchKernelGGL(k_pp_count, dim3(blocks ? blocks : 1), dim3(kPPBlock), 0, st, words, nwords, out);
  return hipGetLastError();
}

hipError_t pp_or_slices(unsigned long long* dst, const unsigned long long* src, uint32_t nslices, uint64_t words,
                        hipStream_t st) {
  const uint32_t blocks = grid_for(words, kPPBlock, 2048);
  hipLaunchKernelGGL(k_pp_or_slices, dim3(blocks ? blocks : 1), dim3(kPPBlock), 0, st, dst, src, nslices, words);
  return hipGetLastError();
}

}  // namespace gs
