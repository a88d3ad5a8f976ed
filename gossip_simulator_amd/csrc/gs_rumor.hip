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
//
// gs_params.rumor_mode (section 4.7.1) selects the variants.  GS_RUMOR_BLIND
// and GS_RUMOR_COIN change what an event is and what it does; in the push
// modes they are a template parameter of k_rumor_round.  GS_RUMOR_PULL has
// every live node call and the hot nodes answer: a dense engine over bitsets
// (hot, served, vain) at the end of this file, with no lists.
#include "gs_internal.h"
#include "gs_wave.h"

namespace gs {
namespace {

constexpr uint32_t kRmBlock = 256;

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

// MODE: the push modes' GS_RUMOR_BLIND | GS_RUMOR_COIN bits.  They change only
// what an event is and what it does to `keep`; 0 is the model as first stated,
// and its instantiation is the body as it was (the `event` path compiles away).
template <uint32_t MODE>
__global__ __launch_bounds__(kRmBlock) void k_rumor_round(const DevState s, const RumorState r,
                                                          const uint32_t* __restrict__ rlist,
                                                          uint32_t* __restrict__ wlist, uint32_t t) {
  constexpr bool kBlind = (MODE & kRumorBlind) != 0, kCoin = (MODE & kRumorCoin) != 0;
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
      uint32_t m = r.miss[v];  // (unused with a coin)
      const u32x4 rr = philox(v, t, 0, c3, s.key.k0, s.key.k1);
      const uint32_t j = uniform(rr.x, d);
      ++fired;
      keep = true;
      bool event = kBlind;  // MODE != 0.  blind: every round v is hot, reply or not
      if ((int32_t)uniform(rr.y, 100u) >= s.kd) {  // the call is kept
        ++sent;
        u = s.ids[(uint64_t)v * s.stride + j];
        const unsigned long long ubit = 1ull << (u & 63);
        const unsigned long long Iu = s.recv[u >> 6];
        const unsigned long long Cu = cc ? s.crash[u >> 6] : 0ull;
        if (!(Cu & ubit)) {  // u live: delivered, and u answers
          ++msgs;
          if (Iu & ubit) {  // u knew the rumor at the start of the round: a miss
            if constexpr (MODE == 0) {
              ++m;
              r.miss[v] = (uint8_t)m;
              keep = m < r.k;
            } else {
              event = true;
            }
          } else {
            const unsigned long long old = atomicOr(&r.next[u >> 6], ubit);
            // the first push to reach u this round lists it (an empty row: removed at once)
            fresh = !(old & ubit) && s.deg[u] > 0;
          }
        }
      }
      if (MODE != 0 && event) {
        if (kCoin) {  // removed with probability 1/k; the miss counts stay 0
          keep = uniform(philox(v, t, 1, c3, s.key.k0, s.key.k1).x, r.k) != 0;
        } else {
          ++m;
          r.miss[v] = (uint8_t)m;
          keep = m < r.k;
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

// ---- the pull modes: a dense engine -----------------------------------------
// Every live node with a friend calls every round, so the round streams the
// table in node order: a wave per 64-node word, a lane per node.  There are no
// lists; the hot set is a bitset, and the feedback of a round is two more
// (served, vain), which k_rumor_pull_commit turns into events and clears.

// A live sender is informed and hot, friend or not (it answers, it need not call).
__global__ void k_rumor_pull_seed(const DevState s, const RumorState r, uint32_t node, unsigned long long cover) {
  if (blockIdx.x || threadIdx.x) return;
  RumorCtl* c = r.ctl;
  unsigned long long rec = 0;
  const unsigned long long bit = 1ull << (node & 63);
  if (!(s.check_crashed && (s.crash[node >> 6] & bit))) {  // a failed sender starts nothing
    s.recv[node >> 6] |= bit;
    r.next[node >> 6] |= bit;
    r.hot[node >> 6] |= bit;
    rec = 1;
  }
  c->cover = cover;
  c->received = rec;
  c->rlen = c->peak = rec;
  c->stop = rec ? 0u : (rec >= cover ? kRumorCovered : kRumorQuiescent);
}

template <bool BLIND>
__global__ __launch_bounds__(kRmBlock) void k_rumor_pull_round(const DevState s, const RumorState r, uint32_t t) {
  __shared__ uint64_t sh[3 * (kRmBlock / 64)];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_RUMOR, s.key.trial);
  const bool cc = s.check_crashed;
  uint64_t fired = 0, sent = 0, msgs = 0;
  const uint64_t waves = (uint64_t)gridDim.x * (kRmBlock / 64);
  // w is wave-uniform: whole waves stay in the loop together
  for (uint64_t w = ((uint64_t)blockIdx.x * kRmBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const unsigned long long Iw = s.recv[w];
    const unsigned long long Cw = cc ? s.crash[w] : 0ull;
    const uint64_t v = w * 64 + lane;
    const bool informed = (Iw >> lane) & 1;
    bool fresh = false;
    if (v < s.n && !((Cw >> lane) & 1)) {
      const uint32_t d = s.deg[v];
      if (d > 0) {  // a live node with a friend calls, informed or not, hot or removed
        const u32x4 rr = philox((uint32_t)v, t, 0, c3, s.key.k0, s.key.k1);
        const uint32_t j = uniform(rr.x, d);
        ++fired;
        if ((int32_t)uniform(rr.y, 100u) >= s.kd) {  // the call is kept
          ++sent;
          const uint32_t u = s.ids[v * s.stride + j];
          const unsigned long long ubit = 1ull << (u & 63);
          const unsigned long long Cu = cc ? s.crash[u >> 6] : 0ull;
          if (!(Cu & ubit)) {  // u live: delivered
            ++msgs;
            if (r.hot[u >> 6] & ubit) {  // u answers with the rumor
              fresh = !informed;
              if (!BLIND) {  // blind: u's event needs no feedback
                unsigned long long* f = (informed ? r.vain : r.served) + (u >> 6);
                if (!(*f & ubit)) atomicOr(f, ubit);  // thousands of callers may share one bit
              }
            }
          }
        }
      }
    }
    const unsigned long long bf = __ballot(fresh);
    if (bf && lane == 0) r.next[w] = Iw | bf;  // the wave's own word: no atomic
  }
  const uint64_t v3[3] = {fired, sent, msgs};
  block_add(sh, v3, 3, r.ctl->acc);
}

// Per word: the round's events, the new hot word, recv = next; acc[RA_NEW] +=
// the new bits and ctl->wlen += the hot bits.  A lane streams one word; the
// words with an event are then taken one at a time by the whole wave, a lane
// per node, for the miss count or the coin.
template <uint32_t MODE>
__global__ __launch_bounds__(kRmBlock) void k_rumor_pull_commit(const DevState s, const RumorState r, uint32_t t) {
  constexpr bool kBlind = (MODE & kRumorBlind) != 0, kCoin = (MODE & kRumorCoin) != 0;
  __shared__ uint64_t sh[3 * (kRmBlock / 64)];
  if (r.ctl->rlen == 0) return;  // nobody hot: nobody was informed and nobody has an event
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_RUMOR, s.key.trial);
  uint64_t nb = 0, nh = 0;
  const uint64_t Wr = (s.W + 63) & ~63ull;  // whole waves stay in the loop together
  for (uint64_t w = (uint64_t)blockIdx.x * kRmBlock + threadIdx.x; w < Wr; w += (uint64_t)gridDim.x * kRmBlock) {
    const bool in = w < s.W;
    const unsigned long long H = in ? r.hot[w] : 0ull;
    unsigned long long S = 0, V = 0;
    if (!kBlind && in) {
      S = r.served[w];
      V = r.vain[w];
    }
    const unsigned long long ev = kBlind ? H : (H & V & ~S);  // asked in vain and not served
    unsigned long long gone = 0;
    unsigned long long todo = __ballot(ev != 0);
    while (todo) {  // wave-uniform
      const uint32_t l = (uint32_t)__builtin_ctzll(todo);
      todo &= todo - 1;
      const unsigned long long E = __shfl(ev, l, 64);
      bool rm = false;
      if ((E >> lane) & 1) {
        const uint64_t v = (w - lane + l) * 64 + lane;
        if (kCoin) {
          rm = uniform(philox((uint32_t)v, t, 1, c3, s.key.k0, s.key.k1).x, r.k) == 0;
        } else {
          const uint32_t m = r.miss[v] + 1u;
          r.miss[v] = (uint8_t)m;
          rm = m >= r.k;
        }
      }
      const unsigned long long rb = __ballot(rm);
      if (lane == l) gone = rb;
    }
    if (in) {
      const unsigned long long a = r.next[w], b = s.recv[w];
      const unsigned long long h = (H & ~gone) | (a ^ b);  // the newly informed are hot, miss = 0
      if (h != H) r.hot[w] = h;
      if (S) r.served[w] = 0;
      if (V) r.vain[w] = 0;
      if (a != b) {
        s.recv[w] = a;
        nb += (uint64_t)__popcll(a ^ b);
      }
      nh += (uint64_t)__popcll(h);
    }
  }
  const uint64_t v3[3] = {nb, 0, 0};
  block_add(sh, v3, 1, r.ctl->acc + RA_NEW);
  __syncthreads();  // sh is reused
  const uint64_t h3[3] = {nh, 0, 0};
  block_add(sh, h3, 1, &r.ctl->wlen);
}

__global__ __launch_bounds__(kRmBlock) void k_rumor_pull_removed(const DevState s, const RumorState r,
                                                                 unsigned long long* out) {
  for (uint64_t w = (uint64_t)blockIdx.x * kRmBlock + threadIdx.x; w < s.W; w += (uint64_t)gridDim.x * kRmBlock)
    out[w] = s.recv[w] & ~r.hot[w];
}

uint32_t words_grid(uint64_t W) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (W + kRmBlock - 1) / kRmBlock), 2048);
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
  switch (r.mode & (kRumorBlind | kRumorCoin)) {
    case 0: hipLaunchKernelGGL(k_rumor_round<0>, dim3(grid), dim3(kRmBlock), 0, st, s, r, rlist, wlist, t); break;
    case 1: hipLaunchKernelGGL(k_rumor_round<1>, dim3(grid), dim3(kRmBlock), 0, st, s, r, rlist, wlist, t); break;
    case 2: hipLaunchKernelGGL(k_rumor_round<2>, dim3(grid), dim3(kRmBlock), 0, st, s, r, rlist, wlist, t); break;
    default: hipLaunchKernelGGL(k_rumor_round<3>, dim3(grid), dim3(kRmBlock), 0, st, s, r, rlist, wlist, t); break;
  }
  return hipGetLastError();
}

hipError_t rumor_pull_seed(const DevState& s, const RumorState& r, uint32_t node, unsigned long long cover,
                           hipStream_t st) {
  hipLaunchKernelGGL(k_rumor_pull_seed, dim3(1), dim3(64), 0, st, s, r, node, cover);
  return hipGetLastError();
}

hipError_t rumor_pull_round(const DevState& s, const RumorState& r, uint32_t t, uint32_t grid, hipStream_t st) {
  if (r.mode & kRumorBlind)
    hipLaunchKernelGGL(k_rumor_pull_round<true>, dim3(grid), dim3(kRmBlock), 0, st, s, r, t);
  else
    hipLaunchKernelGGL(k_rumor_pull_round<false>, dim3(grid), dim3(kRmBlock), 0, st, s, r, t);
  return hipGetLastError();
}

hipError_t rumor_pull_commit(const DevState& s, const RumorState& r, uint32_t t, hipStream_t st) {
  const uint32_t grid = words_grid(s.W);
  switch (r.mode & (kRumorBlind | kRumorCoin)) {
    case 0: hipLaunchKernelGGL(k_rumor_pull_commit<0>, dim3(grid), dim3(kRmBlock), 0, st, s, r, t); break;
    case 1: hipLaunchKernelGGL(k_rumor_pull_commit<1>, dim3(grid), dim3(kRmBlock), 0, st, s, r, t); break;
    case 2: hipLaunchKernelGGL(k_rumor_pull_commit<2>, dim3(grid), dim3(kRmBlock), 0, st, s, r, t); break;
    default: hipLaunchKernelGGL(k_rumor_pull_commit<3>, dim3(grid), dim3(kRmBlock), 0, st, s, r, t); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rumor_publish, dim3(1), dim3(64), 0, st, s, r, t);
  return hipGetLastError();
}

hipError_t rumor_pull_removed(const DevState& s, const RumorState& r, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(k_rumor_pull_removed, dim3(words_grid(s.W)), dim3(kRmBlock), 0, st, s, r, out);
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
