// gs_pp_early.hip -- push-pull: the round's mode, the sparse early rounds
// over the informed list (PP_EARLY, gs_internal.h) and the seed that starts
// the list.  The model is stated in gs_pp_dense.hip.
#include "gs_pp_dev.h"

namespace gs {
namespace {

// ---- sparse early rounds ------------------------------------------------------
// Round mode and the list bookkeeping (one block of kPPSegs threads): the
// previous early round's appends join the list unless a segment overflowed.
__global__ __launch_bounds__(kPPSegs) void k_pp_mode(PPCtl* c) {
  __shared__ unsigned long long sc[kPPSegs];
  const uint32_t tid = threadIdx.x;
  const bool was_early = c->mode == PP_EARLY;
  const bool ok = c->early_ok && !c->ovf;
  unsigned long long len = 0;
  if (tid < c->nseg) {
    len = c->segcnt[tid];
    c->seglen[tid] = len;
  }
  sc[tid] = len;
  __syncthreads();
  if (tid == 0) {
    unsigned long long a = 0;
    for (uint32_t k = 0; k < c->nseg; ++k) {
      c->segpre[k] = a;
      a += sc[k];
    }
    c->segpre[c->nseg] = a;
    const bool early = ok && c->ninf <= c->thr;
    c->mode = early ? PP_EARLY : c->ninf >= c->bthr ? PP_BOTTOM : c->ninf >= c->athr ? PP_ANSWER : PP_DENSE;
    c->nearly += c->mode == PP_EARLY;
    c->nbottom += c->mode == PP_BOTTOM;
    c->nanswer += c->mode == PP_ANSWER;
    if (!early) c->early_ok = 0;  // |I| only grows: the list is never needed again
    (void)was_early;
  }
}

// Appends v to the informed list when this lane's atomicOr on `next` set its
// bit first: one atomic per wave on segment blockIdx % nseg's counter (the
// lanes taking part may be any subset of the wave).
__device__ __forceinline__ void pp_append(PPCtl* c, uint32_t* ilist, uint32_t seg, unsigned long long cap,
                                          bool take, uint32_t v) {
  const unsigned long long bal = __ballot(take);
  if (!bal) return;
  const uint32_t lane = threadIdx.x & 63, lead = (uint32_t)__builtin_ctzll(bal);
  unsigned long long base = 0;
  if (lane == lead) base = atomicAdd(&c->segcnt[seg], (unsigned long long)__popcll(bal));
  base = __shfl(base, lead, 64);
  if (take) {
    const unsigned long long at =
        base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (at < cap) ilist[(size_t)seg * cap + at] = v;
    else c->ovf = 1u;
  }
}

// One early round: lane per informed node u of the
// list.  u's own call is a push (u informed => live); every in-edge (v, j)
// of u whose caller v is live, uninformed, picks slot j and is not lost is a
// successful pull.  Same draws and counters as k_pp_round.
__global__ __launch_bounds__(kPPBlock) void k_ppe_round(const DevState s, unsigned long long* __restrict__ next,
                                                        PPSparse sp, uint32_t t) {
  __shared__ uint64_t sh[3 * (kPPBlock / 64)];
  __shared__ unsigned long long pre[kPPSegs + 1];
  PPCtl* c = sp.ctl;
  if (c->mode != PP_EARLY) return;
  const uint32_t nseg = c->nseg;
  const unsigned long long cap = c->seg_cap;
  for (uint32_t k = threadIdx.x; k <= nseg; k += kPPBlock) pre[k] = c->segpre[k];
  __syncthreads();
  const unsigned long long nl = pre[nseg];
  const uint32_t myseg = blockIdx.x % nseg;
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial);
  const bool cc = s.check_crashed, packed = pp_rslot_packed(s.stride);
  uint64_t sent = 0, msgs = 0;
  const uint64_t G = (uint64_t)gridDim.x * kPPBlock;
  const uint64_t nlr = (nl + 63) & ~63ull;  // whole waves iterate together (pp_append)
  for (uint64_t i = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; i < nlr; i += G) {
    const bool live = i < nl;
    uint32_t u = 0;
    if (live) {  // list index -> (segment, entry)
      uint32_t lo = 0, hi = nseg - 1;
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= i) lo = mid; else hi = mid - 1;
      }
      u = sp.ilist[(size_t)lo * cap + (i - pre[lo])];
    }
    // own call: push
    bool take = false;
    uint32_t w = 0;
    const uint32_t d = live ? s.deg[u] : 0u;
    if (d > 0) {
      const u32x4 r = philox(u, t, 0, c3, s.key.k0, s.key.k1);
      if ((int32_t)uniform(r.y, 100u) >= s.kd) {
        w = s.ids[(uint64_t)u * s.stride + uniform(r.x, d)];
        const unsigned long long wb = 1ull << (w & 63);
        ++sent;
        if (!(cc && (s.crash[w >> 6] & wb))) {  // w live: delivered
          ++msgs;
          if (!(s.recv[w >> 6] & wb)) take = !(atomicOr(&next[w >> 6], wb) & wb);
        }
      }
    }
    pp_append(c, sp.ilist, myseg, cap, take, w);
    // pulls from u: u's in-edges
    unsigned long long q = live ? (u ? sp.rend[u - 1] : 0ull) : 0ull;
    const unsigned long long e = live ? sp.rend[u] : 0ull;
    while (__ballot(q < e)) {
      bool tk = false;
      uint32_t v = 0;
      if (q < e) {
        v = sp.rsrc[q];
        const uint32_t x = sp.rslot[q];
        const uint32_t j = packed ? x & 15u : x;
        ++q;
        const unsigned long long vb = 1ull << (v & 63);
        // v informed: its own list entry pushes; v failed: never calls
        if (!(s.recv[v >> 6] & vb) && !(cc && (s.crash[v >> 6] & vb))) {
          const u32x4 r = philox(v, t, 0, c3, s.key.k0, s.key.k1);
          if (uniform(r.x, packed ? (x >> 4) + 1 : s.deg[v]) == j && (int32_t)uniform(r.y, 100u) >= s.kd) {
            ++sent;
            ++msgs;
            tk = !(atomicOr(&next[v >> 6], vb) & vb);
          }
        }
      }
      pp_append(c, sp.ilist, myseg, cap, tk, v);
    }
  }
  const uint64_t v3[3] = {blockIdx.x == 0 && threadIdx.x == 0 ? c->ncallers : 0ull, sent, msgs};
  const uint32_t f3[3] = {ST_FIRED, ST_SENT, ST_MSGS};
  block_add<kPPBlock>(sh, v3, 3, s.stats + (size_t)(t % kStatSlots) * kStatFields, f3);
}

// The early round's newly informed nodes join recv (next holds them already):
// from the list, or -- if a segment overflowed -- from the bitsets.
__global__ __launch_bounds__(kPPBlock) void k_ppe_commit(const DevState s, const unsigned long long* __restrict__ next,
                                                         PPSparse sp, uint32_t t) {
  __shared__ uint64_t sh[kPPBlock / 64];
  __shared__ unsigned long long s_b[kPPSegs], s_e[kPPSegs];
  PPCtl* c = sp.ctl;
  if (c->mode != PP_EARLY) return;
  const uint64_t G = (uint64_t)gridDim.x * kPPBlock, gid = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x;
  uint64_t newly = 0;
  const bool ovf = c->ovf != 0;
  const uint32_t nseg = c->nseg;
  if (!ovf) {  // the segments' bounds staged once per block (a chain of 2 * nseg loads per thread before)
    for (uint32_t sg = threadIdx.x; sg < nseg; sg += kPPBlock) {
      s_b[sg] = c->seglen[sg];
      s_e[sg] = c->segcnt[sg];
    }
    __syncthreads();
  }
  if (ovf) {
    for (uint64_t w = gid; w < s.W; w += G) {
      const unsigned long long nx = next[w], old = s.recv[w];
      newly += (uint64_t)__popcll(nx & ~old);
      if (nx != old) s.recv[w] = nx;
    }
  } else {
    const unsigned long long cap = c->seg_cap;
    for (uint32_t sg = 0; sg < nseg; ++sg) {
      const unsigned long long b = s_b[sg], e = s_e[sg];
      for (uint64_t k = b + gid; k < e; k += G) {
        const uint32_t v = sp.ilist[(size_t)sg * cap + k];
        atomicOr(&s.recv[v >> 6], 1ull << (v & 63));
        ++newly;
      }
    }
  }
  const uint64_t ws = wave_sum64(newly);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t b = 0;
    for (uint32_t k = 0; k < kPPBlock / 64; ++k) b += sh[k];
    if (b) {
      atomicAdd(&s.stats[(size_t)(t % kStatSlots) * kStatFields + ST_RECV], (unsigned long long)b);
      atomicAdd(&c->ninf, (unsigned long long)b);
    }
  }
}

// The counts of k_pp_callers, from an earlier count of the same table and mask.
__global__ void k_pp_set_callers(PPCtl* c, unsigned long long ncallers, unsigned long long nlive0) {
  c->ncallers = ncallers;
  c->nlive0 = nlive0;
}

// Live nodes with a non-empty row (each calls once per round).
__global__ __launch_bounds__(kPPBlock) void k_pp_callers(const DevState s, PPCtl* c) {
  uint64_t k = 0, z = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < s.n; v += (uint64_t)gridDim.x * kPPBlock) {
    const bool live = !((s.crash[v >> 6] >> (v & 63)) & 1);
    k += live && s.deg[v] > 0;
    z += live && s.deg[v] == 0;
  }
  k = wave_sum64(k);
  z = wave_sum64(z);
  if ((threadIdx.x & 63) == 0 && k) atomicAdd(&c->ncallers, (unsigned long long)k);
  if ((threadIdx.x & 63) == 0 && z) atomicAdd(&c->nlive0, (unsigned long long)z);
}

// Sender (simulator.go:239-241 for the flood model): informed at begin unless
// failed; flag[0] = 1 if it was informed.  ctl (zeroed, ncallers counted):
// the informed list starts as the sender.
__global__ void k_pp_seed(const DevState s, unsigned long long* next, uint32_t node, uint32_t* flag, PPSparse sp,
                          unsigned long long thr, unsigned long long bthr, unsigned long long athr) {
  const unsigned long long bit = 1ull << (node & 63);
  const bool ok = node != ~0u && !(s.crash[node >> 6] & bit);  // ~0u: the sender is another shard's
  if (ok) {
    s.recv[node >> 6] |= bit;
    next[node >> 6] |= bit;
  }
  *flag = ok ? 1u : 0u;
  if (sp.ctl) {  // ctl was zeroed: the list is segment 0 = {sender}
    PPCtl* c = sp.ctl;
    c->ninf = ok ? 1 : 0;
    c->thr = thr;
    c->bthr = bthr;
    c->athr = athr;
    c->nseg = (uint32_t)(s.n >> 12 < kPPSegs ? (s.n >> 12 ? s.n >> 12 : 1) : kPPSegs);
    c->seg_cap = (s.n + c->nseg - 1) / c->nseg;
    c->mode = PP_DENSE;
    c->early_ok = sp.ilist ? 1 : 0;  // shards keep no informed list: never sparse
    c->segcnt[0] = ok ? 1 : 0;
    if (ok && sp.ilist) sp.ilist[0] = node;
  }
}
}  // namespace

void pp_launch_early(const DevState& s, unsigned long long* next, const PPSparse& sp, uint32_t t, hipStream_t st) {
  if (sp.ctl) {
    hipLaunchKernelGGL(k_pp_mode, dim3(1), dim3(kPPSegs), 0, st, sp.ctl);
    // early rounds: the list grows at most ~(1 + in-degree)-fold per round;
    // a fixed grid, idle blocks leave at once
    hipLaunchKernelGGL(k_ppe_round, dim3(2048), dim3(kPPBlock), 0, st, s, next, sp, t);
  }
}

void pp_launch_early_commit(const DevState& s, const unsigned long long* next, const PPSparse& sp, uint32_t t,
                            hipStream_t st) {
  if (sp.ctl) hipLaunchKernelGGL(k_ppe_commit, dim3(1024), dim3(kPPBlock), 0, st, s, next, sp, t);
}

hipError_t pp_seed(const DevState& s, unsigned long long* next, uint32_t node, uint32_t* flag,
                   const PPSparse& sp, unsigned long long thr, unsigned long long bthr, unsigned long long athr,
                   const unsigned long long* callers, hipStream_t st) {
  if (sp.ctl) {
    hipError_t e = hipMemsetAsync(sp.ctl, 0, sizeof(PPCtl), st);
    if (e != hipSuccess) return e;
    if (callers) {
      hipLaunchKernelGGL(k_pp_set_callers, dim3(1), dim3(1), 0, st, sp.ctl, callers[0], callers[1]);
    } else {
      const uint32_t blocks = grid_for(s.n, kPPBlock, 4096);
      hipLaunchKernelGGL(k_pp_callers, dim3(blocks), dim3(kPPBlock), 0, st, s, sp.ctl);
    }
  }
  hipLaunchKernelGGL(k_pp_seed, dim3(1), dim3(1), 0, st, s, next, node, flag, sp, thr, bthr, athr);
  return hipGetLastError();
}

}  // namespace gs
