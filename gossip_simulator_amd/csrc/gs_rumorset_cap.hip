// gs_rumorset_cap.hip -- bounded rumor sets: a payload cap per message and
// rumors that start later than round 0 (gs_rumorset_set_payload,
// gs_rumorset_begin_at).
//
// The calls of a round are section 4.9's: one table read, one Philox draw and
// one mask lookup per caller for all R rumors.  What a connection moves is
// not: with want_u = H[v] & ~H[u] and want_v = H[u] & ~H[v], the caller's
// message carries give = pick(want_u, o_push) and the reply take =
// pick(want_v, o_pull), at most B rumors each (gs_pick.h), the offsets taken
// from the z and w words of the draw the caller has already made.  The cap is
// per message, so next[u] is still an OR over u's callers and nothing depends
// on lane or atomic order.
//
// k_rsc_round has k_rs_round's persistent grid, wave-per-word and
// lane-per-node layout, the one atomicOr only where give != 0 and the plain
// store into own[v]; it reduces six counters (the round's fired, sent and
// messages, and the broadcast's wanted, carried and bound) per wave and per
// block before one atomic each.  k_rs_commit and k_rs_publish (gs_rumorset.hip)
// serve both paths unchanged: a late rumor is injected by k_rsc_inject as a bit
// in next[sender] between round s_j's kernel and its commit, so the commit
// counts it, folds it into have and rebuilds the holds-every-rumor word.
#include "gs_rumorset.h"
#include "gs_pick.h"
#include "gs_wave.h"

namespace gs {
namespace {

constexpr uint32_t kRscBlock = 256;  // (rs_grid's block)

// Per-block sums of six counters, one atomic each where non-zero: the first
// three into acc (the round's, cleared by k_rs_publish), the others into
// traffic (the broadcast's).
__device__ __forceinline__ void block_add6(uint64_t* sh, const uint64_t (&v)[6], RsCtl* c) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint32_t i = 0; i < 6; ++i) {
    const uint64_t s = wave_sum64(v[i]);
    if (lane == 0) sh[i * (kRscBlock / 64) + wv] = s;
  }
  __syncthreads();
  if (tid < 6) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < kRscBlock / 64; ++k) s += sh[tid * (kRscBlock / 64) + k];
    unsigned long long* dst = tid < 3 ? &c->acc[tid] : &c->traffic[tid - 3];
    if (s) atomicAdd(dst, (unsigned long long)s);
  }
}

// One wave, lane j owns rumor j: k_rs_seed with starts.  `now` has bit j where
// rumor j starts at begin (s_j = 0).  Every rumor whose sender is not failed is
// live from here on, injected or not: it counts in the live mask, in pending
// and in the holds-every-rumor test, so nobody holds all of them and the stop
// word stays 0 until the last one is in.
__global__ void k_rsc_seed(const DevState s, const RsState r, const RsSenders snd, unsigned long long now,
                           unsigned long long cover) {
  if (blockIdx.x) return;
  const uint32_t j = threadIdx.x;
  RsCtl* c = r.ctl;
  const uint32_t node = j < r.R ? snd.node[j] : 0u;
  const unsigned long long nbit = 1ull << (node & 63);
  const bool alive = j < r.R && !(s.check_crashed && (s.crash[node >> 6] & nbit));
  const bool in = alive && ((now >> j) & 1);
  const unsigned long long live = __ballot(alive);
  if (in) atomicOr(r.have + node, 1ull << j);
  const uint32_t lead = live ? (uint32_t)__builtin_ctzll(live) : 0u;
  const uint32_t first = __shfl(node, lead, 64);
  const bool one = live && __ballot(in && node == first) == live;
  if (one && j == lead) s.recv[node >> 6] = nbit;
  const unsigned long long cnt = in ? 1ull : 0ull;
  c->cnt[j] = cnt;
  const unsigned long long unc = __ballot(alive && cnt < cover);
  const unsigned long long got = __ballot(in);
  if (j == 0) {
    const unsigned long long pend = (unsigned long long)__popcll(unc);
    c->cover = cover;
    c->live = live;
    c->received = (unsigned long long)__popcll(got);
    c->pending = pend;
    c->stop = live == 0 ? kRumorQuiescent : pend == 0 ? kRumorCovered : 0u;
  }
}

// One wave, lane j owns rumor j: the rumors of `mask` (live, s_j = this round)
// enter at their senders, as bits of next that the round's commit folds in.
__global__ void k_rsc_inject(const RsState r, const RsSenders snd, unsigned long long mask) {
  if (blockIdx.x) return;
  const uint32_t j = threadIdx.x;
  if (j < r.R && ((mask >> j) & 1)) atomicOr(r.next + snd.node[j], 1ull << j);  // (two may enter at one node)
}

template <uint32_t PICK>
__global__ __launch_bounds__(kRscBlock) void k_rsc_round(const DevState s, const RsState r, uint32_t t, uint32_t B) {
  __shared__ uint64_t sh[6 * (kRscBlock / 64)];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial);
  const bool cc = s.check_crashed;
  const uint32_t R = r.R;
  uint64_t fired = 0, sent = 0, msgs = 0, wanted = 0, carried = 0, bound = 0;
  const uint64_t waves = (uint64_t)gridDim.x * (kRscBlock / 64);
  // w is wave-uniform: whole waves stay in the loop together
  for (uint64_t w = ((uint64_t)blockIdx.x * kRscBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const unsigned long long Cw = cc ? s.crash[w] : 0ull;
    const uint64_t v = w * 64 + lane;
    if (v >= s.n || ((Cw >> lane) & 1)) continue;
    const uint32_t d = s.deg[v];
    if (d == 0) continue;  // a live node with a friend calls every round
    const unsigned long long hv = r.have[v];
    const u32x4 rr = philox((uint32_t)v, t, 0, c3, s.key.k0, s.key.k1);
    const uint32_t j = uniform(rr.x, d);
    ++fired;
    if ((int32_t)uniform(rr.y, 100u) < s.kd) continue;  // the call is lost
    ++sent;
    const uint32_t u = s.ids[v * s.stride + j];
    if (cc && ((s.crash[u >> 6] >> (u & 63)) & 1)) continue;  // a failed callee: no connection
    const unsigned long long hu = r.have[u];  // (u == v: a connection that changes nothing)
    msgs += (uint64_t)(hv != 0) + (uint64_t)(hu != 0);
    const unsigned long long want_u = hv & ~hu, want_v = hu & ~hv;
    if ((want_u | want_v) == 0) continue;  // nothing wanted either way: no payload, no counter moves
    const unsigned long long give = rs_pick(want_u, B, PICK, PICK == kPickRotate ? uniform(rr.z, R) : 0u, R);
    const unsigned long long take = rs_pick(want_v, B, PICK, PICK == kPickRotate ? uniform(rr.w, R) : 0u, R);
    const uint32_t pu = pick_popc(want_u), pv = pick_popc(want_v);
    wanted += pu + pv;
    carried += pick_popc(give) + pick_popc(take);
    bound += (uint64_t)(pu > B) + (uint64_t)(pv > B);
    if (give) atomicOr(r.next + u, give);  // the result is not used
    if (take) r.own[v] = take;
  }
  const uint64_t v6[6] = {fired, sent, msgs, wanted, carried, bound};
  block_add6(sh, v6, r.ctl);
}

}  // namespace

hipError_t rsc_seed(const DevState& s, const RsState& r, const RsSenders& snd, unsigned long long now,
                    unsigned long long cover, hipStream_t st) {
  hipLaunchKernelGGL(k_rsc_seed, dim3(1), dim3(64), 0, st, s, r, snd, now, cover);
  return hipGetLastError();
}

hipError_t rsc_inject(const RsState& r, const RsSenders& snd, unsigned long long mask, hipStream_t st) {
  hipLaunchKernelGGL(k_rsc_inject, dim3(1), dim3(64), 0, st, r, snd, mask);
  return hipGetLastError();
}

hipError_t rsc_round(const DevState& s, const RsState& r, uint32_t t, uint32_t payload, uint32_t pick, uint32_t grid,
                     hipStream_t st) {
  if (pick == kPickHigh)
    hipLaunchKernelGGL(k_rsc_round<kPickHigh>, dim3(grid), dim3(kRscBlock), 0, st, s, r, t, payload);
  else if (pick == kPickRotate)
    hipLaunchKernelGGL(k_rsc_round<kPickRotate>, dim3(grid), dim3(kRscBlock), 0, st, s, r, t, payload);
  else
    hipLaunchKernelGGL(k_rsc_round<kPickLow>, dim3(grid), dim3(kRscBlock), 0, st, s, r, t, payload);
  return hipGetLastError();
}

}  // namespace gs
