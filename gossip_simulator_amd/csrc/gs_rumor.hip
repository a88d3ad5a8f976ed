// gs_rumor.hip -- rumor mongering with loss of interest (GS_MODEL_RUMOR).
//
// The third classic epidemic protocol (Demers et al., "Epidemic algorithms for
// replicated database maintenance"), with no reference counterpart
// (simulator.go only floods); the model is the one DESIGN.md section 4.7
// states.  One tick = one synchronous round.  An informed live node with a
// non-empty friends list is HOT: each round it draws
// r = Philox{v, t, 0, RUMOR}, calls u = friends[v][U_deg(r.x)], and the call is
// lost iff U_100(r.y) < kd (the -droprate quantisation of simulator.go:172).
// A kept call to a live u either informs u (u not in I, the informed set at
// the start of the round: u is hot from the next round) or, u in I, counts as
// a miss of v; after k misses v is REMOVED and never calls again.  The run
// ends by itself when no node is hot.
//
// Layout: a list engine.  The hot set is a u32 list; a persistent grid walks
// the round's read list a lane per entry and builds the next round's write
// list: every surviving caller re-appends itself, and the lane whose atomicOr
// into `next` set a fresh node's bit appends that node (so a node enters a
// list at most once, whatever the number of pushes that reach it).  Appends
// are reserved once per wave (ballot + mbcnt).  Every decision reads recv, the
// informed set as it was at the start of the round, so the outcome does not
// depend on lane or atomic order; list order is free.  k_rumor_commit then
// makes recv = next and counts the new bits, and k_rumor_publish writes the
// round's stats row, swaps the list lengths and evaluates gs_run's stop rule,
// all on the device: rounds queue without a host sync, and a round on an empty
// list does nothing.
#include "gs_internal.h"

namespace gs {
namespace {

constexpr uint32_t kRmBlock = 256;

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (uint32_t o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Per-block sums of nf <= 3 counters into acc[0..nf), one atomic each.
__device__ __forceinline__ void block_add(uint64_t* sh, const uint64_t (&v)[3], uint32_t nf,
                                          unsigned long long* acc) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < 3 * (kRmBlock / 64)) sh[tid] = 0;
  __syncthreads();
  for (uint32_t i = 0; i < nf; ++i) {
    const uint64_t s = wave_sum64(v[i]);
    if (lane == 0) sh[i * (kRmBlock / 64) + wv] = s;
  }
  __syncthreads();
  if (tid < nf) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < kRmBlock / 64; ++k) s += sh[tid * (kRmBlock / 64) + k];
    if (s) atomicAdd(&acc[tid], (unsigned long long)s);
  }
}

// Lanes below this one whose bit is set in the ballot b.
__device__ __forceinline__ uint32_t lanes_below(unsigned long long b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// The sender is informed unless failed, and hot if it has a friend.
__global__ void k_rumor_seed(const DevState s, const RumorState r, uint32_t* list0, uint32_t node,
                             unsigned long long cover) {
  if (blockIdx.x || threadIdx.x) return;
  RumorCtl* c = r.ctl;
  unsigned long long rec = 0, hot = 0;
  const unsigned long long bit = 1ull << (node & 63);
  if (!(s.check_crashed && (s.crash[node >> 6] & bit))) {  // a failed sender starts nothing
    s.recv[node >> 6] |= bit;
    r.next[node >> 6] |= bit;
    rec = 1;
    if (s.deg[node] > 0) {  // an empty row: removed at once
      list0[0] = node;
      hot = 1;
    }
  }
  c->cover = cover;
  c->received = rec;
  c->rlen = c->peak = hot;
  c->stop = hot ? 0u : (rec >= cover ? kRumorCovered : kRumorQuiescent);
}

__global__ __launch_bounds__(kRmBlock) void k_rumor_round(const DevState s, const RumorState r,
                                                          const uint32_t* __restrict__ rlist,
                                                          uint32_t* __restrict__ wlist, uint32_t t) {
  __shared__ uint64_t sh[3 * (kRmBlock / 64)];
  const uint64_t len = r.ctl->rlen;
  if (len == 0) return;  // quiescent: nothing calls
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_RUMOR, s.key.trial);
  const bool cc = s.check_crashed;
  uint64_t fired = 0, sent = 0, msgs = 0;
  const uint64_t lenr = (len + 63) & ~63ull;  // whole waves stay in the loop together
  for (uint64_t i = (uint64_t)blockIdx.x * kRmBlock + threadIdx.x; i < lenr; i += (uint64_t)gridDim.x * kRmBlock) {
    bool keep = false, fresh = false;
    uint32_t v = 0, u = 0;
    if (i < len) {
      v = rlist[i];
      const uint32_t d = s.deg[v];  // > 0: only nodes with a friend enter a list
      uint32_t m = r.miss[v];
      const u32x4 rr = philox(v, t, 0, c3, s.key.k0, s.key.k1);
      const uint32_t j = uniform(rr.x, d);
      ++fired;
      keep = true;
      if ((int32_t)uniform(rr.y, 100u) >= s.kd) {  // the call is kept
        ++sent;
        u = s.ids[(uint64_t)v * s.stride + j];
        const unsigned long long ubit = 1ull << (u & 63);
        const unsigned long long Iu = s.recv[u >> 6];
        const unsigned long long Cu = cc ? s.crash[u >> 6] : 0ull;
        if (!(Cu & ubit)) {  // u live: delivered, and u answers
          ++msgs;
          if (Iu & ubit) {  // u knew the rumor at the start of the round: a miss
            ++m;
            r.miss[v] = (uint8_t)m;
            keep = m < r.k;
          } else {
            const unsigned long long old = atomicOr(&r.next[u >> 6], ubit);
            // the first push to reach u this round lists it (an empty row: removed at once)
            fresh = !(old & ubit) && s.deg[u] > 0;
          }
        }
      }
    }
    const unsigned long long bk = __ballot(keep), bf = __ballot(fresh);
    const uint32_t nk = (uint32_t)__popcll(bk), nf = (uint32_t)__popcll(bf);
    if (nk + nf) {  // wave-uniform: one reservation per wave
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(&r.ctl->wlen, (unsigned long long)(nk + nf));
      base = __shfl(base, 0, 64);
      const uint64_t pk = base + lanes_below(bk), pf = base + nk + lanes_below(bf);
      if (keep && pk < s.n) wlist[pk] = v;
      if (fresh && pf < s.n) wlist[pf] = u;
    }
  }
  const uint64_t v3[3] = {fired, sent, msgs};
  block_add(sh, v3, 3, r.ctl->acc);
}

// recv = next; acc[RA_NEW] += the bits the round set.
__global__ __launch_bounds__(kRmBlock) void k_rumor_commit(const DevState s, const RumorState r) {
  __shared__ uint64_t sh[3 * (kRmBlock / 64)];
  if (r.ctl->rlen == 0) return;  // no round ran
  uint64_t nb = 0;
  for (uint64_t w = (uint64_t)blockIdx.x * kRmBlock + threadIdx.x; w < s.W; w += (uint64_t)gridDim.x * kRmBlock) {
    const unsigned long long a = r.next[w], b = s.recv[w];
    if (a != b) {
      s.recv[w] = a;
      nb += (uint64_t)__popcll(a ^ b);
    }
  }
  const uint64_t v3[3] = {nb, 0, 0};
  block_add(sh, v3, 1, r.ctl->acc + RA_NEW);
}

// The round's stats row, the next round's list length and the stop rule.
__global__ void k_rumor_publish(const DevState s, const RumorState r, uint32_t t) {
  if (blockIdx.x || threadIdx.x) return;
  RumorCtl* c = r.ctl;
  unsigned long long* row = s.stats + (size_t)(t % kStatSlots) * kStatFields;
  const unsigned long long hot = c->wlen;
  row[ST_FIRED] = c->acc[RA_FIRED];
  row[ST_SENT] = c->acc[RA_SENT];
  row[ST_MSGS] = c->acc[RA_MSGS];
  row[ST_RECV] = c->acc[RA_NEW];
  row[ST_CRASH] = 0;
  row[ST_SCHED] = hot;  // pending: the hot nodes after the round
  row[ST_ERR] = row[ST_RSVD] = 0;
  c->received += c->acc[RA_NEW];
  if (hot > c->peak) c->peak = hot;
  c->rlen = hot;
  c->wlen = 0;
  c->acc[RA_FIRED] = c->acc[RA_SENT] = c->acc[RA_MSGS] = c->acc[RA_NEW] = 0;
  c->stop = hot ? 0u : (c->received >= c->cover ? kRumorCovered : kRumorQuiescent);
}

// out (a copy of recv) loses the bits of the hot nodes: informed and not hot.
__global__ __launch_bounds__(kRmBlock) void k_rumor_removed(const RumorState r, const uint32_t* __restrict__ rlist,
                                                            unsigned long long* out) {
  const uint64_t len = r.ctl->rlen;
  for (uint64_t i = (uint64_t)blockIdx.x * kRmBlock + threadIdx.x; i < len; i += (uint64_t)gridDim.x * kRmBlock) {
    const uint32_t v = rlist[i];
    atomicAnd(&out[v >> 6], ~(1ull << (v & 63)));
  }
}

}  // namespace

uint32_t rumor_grid(uint64_t n, uint32_t want) {
  const uint64_t cap = std::max<uint64_t>(1, (n + kRmBlock - 1) / kRmBlock);
  return (uint32_t)std::min<uint64_t>(cap, want ? want : 2048u);  // 256 CUs x 8 blocks
}

hipError_t rumor_seed(const DevState& s, const RumorState& r, uint32_t* list0, uint32_t node, unsigned long long cover,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_rumor_seed, dim3(1), dim3(64), 0, st, s, r, list0, node, cover);
  return hipGetLastError();
}

hipError_t rumor_round(const DevState& s, const RumorState& r, const uint32_t* rlist, uint32_t* wlist, uint32_t t,
                       uint32_t grid, hipStream_t st) {
  hipLaunchKernelGGL(k_rumor_round, dim3(grid), dim3(kRmBlock), 0, st, s, r, rlist, wlist, t);
  return hipGetLastError();
}

hipError_t rumor_commit(const DevState& s, const RumorState& r, uint32_t t, hipStream_t st) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (s.W + kRmBlock - 1) / kRmBlock), 2048);
  hipLaunchKernelGGL(k_rumor_commit, dim3(grid), dim3(kRmBlock), 0, st, s, r);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rumor_publish, dim3(1), dim3(64), 0, st, s, r, t);
  return hipGetLastError();
}

hipError_t rumor_removed(const RumorState& r, const uint32_t* rlist, unsigned long long* out, uint32_t grid,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_rumor_removed, dim3(grid), dim3(kRmBlock), 0, st, r, rlist, out);
  return hipGetLastError();
}

}  // namespace gs
