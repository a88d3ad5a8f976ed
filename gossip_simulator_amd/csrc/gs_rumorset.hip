// gs_rumorset.hip -- up to 64 push-pull broadcasts in one pass
// (gs_create_rumorset).
//
// Who calls whom in a push-pull round, and which calls are lost, does not
// depend on who is informed (section 4.5): every live v with a friend draws
// r = Philox{v, t, 0, PUSHPULL}, calls u = friends[v][U_deg(r.x)], and the call
// is lost iff U_100(r.y) < kd.  So R broadcasts over one table with one seed
// share every table read and every draw: have[v] is a u64 whose bit j says
// that v holds rumor j, and a kept call to a live u moves everything both
// ends know, next[u] |= H[v] and next[v] |= H[u], with H the words at the
// start of the round.
//
// Layout: a dense engine shaped like gs_median.hip.  The round streams the
// table in node order, a wave per 64-node word and a lane per node, and reads
// have only.  u's end is one atomicOr into next[u], issued only when v has
// something u lacks; v's own end is a plain store into own[v], which no other
// lane touches.  k_rs_commit streams have, next and own in node order, merges
// them, counts the new bits per rumor and rebuilds the recv word (the nodes
// that hold every started rumor); k_rs_publish folds the counts and writes the
// stats row and the stop word, so rounds queue without a host sync.  Nothing
// depends on lane or atomic order.
#include "gs_rumorset.h"
#include "gs_wave.h"

namespace gs {
namespace {

constexpr uint32_t kRsBlock = 256;

// Per-block sums of three counters into acc[0..3), one atomic each (gs_median.hip's).
__device__ __forceinline__ void block_add(uint64_t* sh, const uint64_t (&v)[3], unsigned long long* acc) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint32_t i = 0; i < 3; ++i) {
    const uint64_t s = wave_sum64(v[i]);
    if (lane == 0) sh[i * (kRsBlock / 64) + wv] = s;
  }
  __syncthreads();
  if (tid < 3) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < kRsBlock / 64; ++k) s += sh[tid * (kRsBlock / 64) + k];
    if (s) atomicAdd(&acc[tid], (unsigned long long)s);
  }
}

// OR over the wave's 64 lanes: every lane gets the result.
__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v) {
#pragma unroll
  for (uint32_t o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// One wave, lane j owns rumor j.  A live sender gets its bit (two rumors may
// share a sender: atomicOr); a failed one starts nothing and its rumor is dead.
__global__ void k_rs_seed(const DevState s, const RsState r, const RsSenders snd, unsigned long long cover) {
  if (blockIdx.x) return;
  const uint32_t j = threadIdx.x;
  RsCtl* c = r.ctl;
  const uint32_t node = j < r.R ? snd.node[j] : 0u;
  const unsigned long long nbit = 1ull << (node & 63);
  const bool started = j < r.R && !(s.check_crashed && (s.crash[node >> 6] & nbit));
  const unsigned long long live = __ballot(started);
  if (started) atomicOr(r.have + node, 1ull << j);
  // a node holds every started rumor already only if they all start there
  const uint32_t lead = live ? (uint32_t)__builtin_ctzll(live) : 0u;
  const uint32_t first = __shfl(node, lead, 64);
  const bool one = live && __ballot(started && node == first) == live;
  if (one && j == lead) s.recv[node >> 6] = nbit;
  const unsigned long long cnt = started ? 1ull : 0ull;
  c->cnt[j] = cnt;
  const unsigned long long unc = __ballot(started && cnt < cover);
  if (j == 0) {
    const unsigned long long pend = (unsigned long long)__popcll(unc);
    c->cover = cover;
    c->live = live;
    c->received = (unsigned long long)__popcll(live);
    c->pending = pend;
    c->stop = live == 0 ? kRumorQuiescent : pend == 0 ? kRumorCovered : 0u;
  }
}

__global__ __launch_bounds__(kRsBlock) void k_rs_round(const DevState s, const RsState r, uint32_t t) {
  __shared__ uint64_t sh[3 * (kRsBlock / 64)];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial);
  const bool cc = s.check_crashed;
  uint64_t fired = 0, sent = 0, msgs = 0;
  const uint64_t waves = (uint64_t)gridDim.x * (kRsBlock / 64);
  // w is wave-uniform: whole waves stay in the loop together
  for (uint64_t w = ((uint64_t)blockIdx.x * kRsBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
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
    msgs += (uint64_t)(hv != 0) + (uint64_t)(hu != 0);  // the caller pushes, the callee answers
    const unsigned long long give = hv & ~hu, take = hu & ~hv;
    if (give) atomicOr(r.next + u, give);  // thousands of callers may share one word; the result is not used
    if (take) r.own[v] = take;
  }
  const uint64_t v3[3] = {fired, sent, msgs};
  block_add(sh, v3, r.ctl->acc);
}

// have |= next | own per node, a wave per word: have written where it grew,
// next / own cleared where set, the new bits counted per rumor (one ballot per
// rumor that gained a node in this word, into the block's LDS counters) and
// the recv word rebuilt where the word changed.
__global__ __launch_bounds__(kRsBlock) void k_rs_commit(const DevState s, const RsState r) {
  __shared__ uint32_t cnt[kRsMax];  // at most n per rumor even on a grid of one block, and n < 2^31 (check_params)
  const uint32_t lane = threadIdx.x & 63;
  if (threadIdx.x < kRsMax) cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long live = r.ctl->live;
  const uint64_t waves = (uint64_t)gridDim.x * (kRsBlock / 64);
  for (uint64_t w = ((uint64_t)blockIdx.x * kRsBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const uint64_t v = w * 64 + lane;
    const bool in = v < s.n;
    unsigned long long h = 0, nw = 0;
    if (in) {
      h = r.have[v];
      const unsigned long long nx = r.next[v], ow = r.own[v];
      nw = (nx | ow) & ~h;
      if (nw) r.have[v] = h | nw;
      if (nx) r.next[v] = 0;
      if (ow) r.own[v] = 0;
    }
    if (__ballot(nw != 0) == 0) continue;  // wave-uniform: late in a run most words gain nothing
    unsigned long long m = wave_or64(nw);
    while (m) {
      const uint32_t b = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      const uint32_t k = (uint32_t)__popcll(__ballot((nw >> b) & 1));
      if (lane == 0) atomicAdd(&cnt[b], k);
    }
    const unsigned long long full = __ballot(in && (h | nw) == live);  // (live != 0 here: a bit was gained)
    if (lane == 0) s.recv[w] = full;  // the wave's own word: no atomic
  }
  __syncthreads();
  if (threadIdx.x < kRsMax && cnt[threadIdx.x])
    atomicAdd(&r.ctl->newc[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// One wave, lane j owns rumor j: the cumulative counts, their ring slot, the
// round's stats row and the stop word.
__global__ void k_rs_publish(const DevState s, const RsState r, uint32_t t) {
  if (blockIdx.x) return;
  const uint32_t j = threadIdx.x;
  RsCtl* c = r.ctl;
  const unsigned long long nc = c->newc[j], total = c->cnt[j] + nc;
  if (nc) {
    c->cnt[j] = total;
    c->newc[j] = 0;
  }
  r.ring[(size_t)(t % kStatSlots) * kRsMax + j] = total;
  const unsigned long long live = c->live;
  const unsigned long long unc = __ballot(((live >> j) & 1) && total < c->cover);
  const unsigned long long fresh = wave_sum64(nc);
  if (j == 0) {
    unsigned long long* row = s.stats + (size_t)(t % kStatSlots) * kStatFields;
    const unsigned long long pend = (unsigned long long)__popcll(unc);
    row[ST_FIRED] = c->acc[RS_FIRED];
    row[ST_SENT] = c->acc[RS_SENT];
    row[ST_MSGS] = c->acc[RS_MSGS];
    row[ST_RECV] = fresh;
    row[ST_CRASH] = 0;
    row[ST_SCHED] = pend;  // pending: the started rumors still below 99 %
    row[ST_ERR] = row[ST_RSVD] = 0;
    c->received += fresh;
    c->pending = pend;
    c->acc[RS_FIRED] = c->acc[RS_SENT] = c->acc[RS_MSGS] = 0;
    c->stop = live == 0 ? kRumorQuiescent : pend == 0 ? kRumorCovered : 0u;
  }
}

__global__ __launch_bounds__(kRsBlock) void k_rs_column(const DevState s, const RsState r, uint32_t rumor,
                                                        unsigned long long* out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kRsBlock / 64);
  for (uint64_t w = ((uint64_t)blockIdx.x * kRsBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const uint64_t v = w * 64 + lane;
    const unsigned long long col = __ballot(v < s.n && ((r.have[v] >> rumor) & 1));
    if (lane == 0) out[w] = col;
  }
}

}  // namespace

uint32_t rs_grid(uint64_t n, uint32_t want) {
  const uint64_t cap = std::max<uint64_t>(1, (n + kRsBlock - 1) / kRsBlock);
  return (uint32_t)std::min<uint64_t>(cap, want ? want : 2048u);  // 256 CUs x 8 blocks
}

hipError_t rs_seed(const DevState& s, const RsState& r, const RsSenders& snd, unsigned long long cover,
                   hipStream_t st) {
  hipLaunchKernelGGL(k_rs_seed, dim3(1), dim3(64), 0, st, s, r, snd, cover);
  return hipGetLastError();
}

hipError_t rs_round(const DevState& s, const RsState& r, uint32_t t, uint32_t grid, hipStream_t st) {
  hipLaunchKernelGGL(k_rs_round, dim3(grid), dim3(kRsBlock), 0, st, s, r, t);
  return hipGetLastError();
}

hipError_t rs_commit(const DevState& s, const RsState& r, uint32_t t, uint32_t grid, hipStream_t st) {
  hipLaunchKernelGGL(k_rs_commit, dim3(grid), dim3(kRsBlock), 0, st, s, r);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rs_publish, dim3(1), dim3(64), 0, st, s, r, t);
  return hipGetLastError();
}

hipError_t rs_column(const DevState& s, const RsState& r, uint32_t rumor, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(k_rs_column, dim3(rs_grid(s.n, 0)), dim3(kRsBlock), 0, st, s, r, rumor, out);
  return hipGetLastError();
}

}  // namespace gs
