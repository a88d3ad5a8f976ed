// gs_pp_fmask.hip -- push-pull: what a failure mask (gs_set_failed) is turned
// into before the rounds -- the per-caller failed-slot mask (PPSparse::fmask),
// its has-a-failed-friend bits (fany) and the failed in-edge bits (rfail) --
// and gs_run's exact stop test over the same sets.
#include "gs_pp_dev.h"

namespace gs {
namespace {

// fmask[v] bit j = ids[v][j] is failed: each failed node marks its in-edges.
__global__ __launch_bounds__(kPPBlock) void k_pp_fmask(const DevState s, const unsigned long long* rend,
                                                       const uint32_t* rsrc, const uint8_t* rslot, uint32_t* fm4) {
  for (uint64_t f = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; f < s.n; f += (uint64_t)gridDim.x * kPPBlock) {
    if (!((s.crash[f >> 6] >> (f & 63)) & 1)) continue;
    for (unsigned long long q = f ? rend[f - 1] : 0ull; q < rend[f]; ++q) {
      const uint32_t v = rsrc[q];
      atomicOr(&fm4[v >> 2], (1u << (rslot[q] & 15u)) << (8 * (v & 3)));  // stride <= 8: packed
    }
  }
}

// Exact stop test (gs_run): out += edges (v, friends[v][j]) over which a call
// could still change the informed set -- v live and informed with a live
// uninformed friend (push), or v live and uninformed with an informed friend
// (pull).  Zero means no later round can inform anyone.  Run only when a poll
// window informed nobody new.
__global__ __launch_bounds__(kPPBlock) void k_pp_live_edges(const DevState s, uint32_t* out) {
  uint32_t cnt = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < s.n; v += (uint64_t)gridDim.x * kPPBlock) {
    const unsigned long long bit = 1ull << (v & 63);
    if (s.crash[v >> 6] & bit) continue;
    const bool iv = (s.recv[v >> 6] & bit) != 0;
    const uint32_t d = s.deg[v];
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t u = s.ids[v * s.stride + j];  // global id
      const unsigned long long ub = 1ull << (u & 63);
      const bool iu = (s.grecv[u >> 6] & ub) != 0, fu = (s.gcrash[u >> 6] & ub) != 0;
      if (iv ? (!iu && !fu) : iu) { ++cnt; break; }
    }
  }
  const uint32_t w = wave_sum64(cnt);
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(out, w);
}

// rfail bit q: in-edge q's caller rsrc[q] is failed (the pull-answer rounds'
// answer test; rfail zeroed before).  Built from the failed callers' side: a
// thread per failed-set word, and for each failed caller v and slot j the
// in-edge (v, j) is found in friend w's short in-list (a pass over every
// in-edge with a gather of its caller's failed word took 175 ms at N = 1e9).
// In-lists longer than this are not scanned per failed caller (the scan is
// the friend's whole in-list, so a hub listed by many failed callers would
// cost quadratically): k_pp_rfail_hubs walks them once instead.
constexpr uint32_t kRfailScan = 64;

// *hub = 1 when some failed caller has a friend whose in-list is longer than
// kRfailScan: only then does k_pp_rfail_hubs walk the in-lists (ADVICE r05:
// it read every rend entry, ~8 GB at N = 1e9, whether or not a hub existed).
__global__ __launch_bounds__(kPPBlock) void k_pp_rfail(const DevState s, const unsigned long long* __restrict__ rend,
                                                       const uint32_t* __restrict__ rsrc,
                                                       const uint8_t* __restrict__ rslot, uint32_t* __restrict__ rfail,
                                                       uint32_t* __restrict__ hub) {
  for (uint64_t wd = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; wd < s.W;
       wd += (uint64_t)gridDim.x * blockDim.x) {
    for (unsigned long long m = s.crash[wd]; m; m &= m - 1) {
      const uint64_t v = (wd << 6) + (uint64_t)__builtin_ctzll(m);
      if (v >= s.n) break;
      const uint32_t d = s.deg[v];
      for (uint32_t j = 0; j < d; ++j) {
        const uint32_t w = s.ids[v * s.stride + j];
        const unsigned long long qb = w ? rend[w - 1] : 0ull, qe = rend[w];
        if (qe - qb > kRfailScan) {  // a hub: k_pp_rfail_hubs
          if (!*hub) atomicOr(hub, 1u);
          continue;
        }
        for (unsigned long long q = qb; q < qe; ++q)
          if (rsrc[q] == (uint32_t)v && (rslot[q] & 15u) == j) {
            atomicOr(&rfail[q >> 5], 1u << (q & 31));
            break;
          }
      }
    }
  }
}

// The in-edges of every node with more than kRfailScan of them: one wave per
// such node walks its in-list once and marks the edges whose caller failed
// (linear in the hubs' in-degrees).
__global__ __launch_bounds__(kPPBlock) void k_pp_rfail_hubs(const DevState s, const unsigned long long* __restrict__ rend,
                                                            const uint32_t* __restrict__ rsrc,
                                                            uint32_t* __restrict__ rfail,
                                                            const uint32_t* __restrict__ hub) {
  if (!*hub) return;  // no failed caller lists a hub
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t w0 = wave * 64; w0 < s.n; w0 += nwaves * 64) {
    // the wave's 64 candidate nodes, one per lane; then each hub among them in turn
    const uint64_t w = w0 + lane;
    const unsigned long long qe = w < s.n ? rend[w] : 0ull, qb = w < s.n && w ? rend[w - 1] : 0ull;
    for (unsigned long long hubs = __ballot(w < s.n && qe - qb > kRfailScan); hubs; hubs &= hubs - 1) {
      const uint32_t h = (uint32_t)__builtin_ctzll(hubs);
      const unsigned long long hb = __shfl(qb, h, 64), he = __shfl(qe, h, 64);
      for (unsigned long long q = hb + lane; q < he; q += 64) {
        const uint32_t v = rsrc[q];
        if ((s.crash[v >> 6] >> (v & 63)) & 1ull) atomicOr(&rfail[q >> 5], 1u << (q & 31));
      }
    }
  }
}

// fany bit v: node v has a failed friend (fmask[v] != 0): the lane-per-word
// bottom-up ranges read a node's degree and mask byte only then.  A thread
// per 64-node word.
__global__ __launch_bounds__(kPPBlock) void k_pp_fmask_any(const uint8_t* __restrict__ fmask, uint64_t n,
                                                           unsigned long long* __restrict__ fany) {
  const uint64_t W = (n + 63) >> 6;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < W; w += (uint64_t)gridDim.x * blockDim.x) {
    unsigned long long bits = 0;
    for (uint32_t b = 0; b < 64; ++b) {
      const uint64_t v = (w << 6) + b;
      if (v < n && fmask[v]) bits |= 1ull << b;
    }
    fany[w] = bits;
  }
}

// fmask[v] bit j = friend j of own caller v is failed (replicated failed set).
__global__ __launch_bounds__(kPPBlock) void k_pp_fmask_rows(const DevState s, uint8_t* fmask) {
  for (uint64_t v = (uint64_t)blockIdx.x * kPPBlock + threadIdx.x; v < s.n; v += (uint64_t)gridDim.x * kPPBlock) {
    const uint32_t d = s.deg[v];
    uint32_t m = 0;
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t u = s.ids[v * s.stride + j];
      if ((s.gcrash[u >> 6] >> (u & 63)) & 1) m |= 1u << j;
    }
    fmask[v] = (uint8_t)m;
  }
}
}  // namespace

hipError_t pp_live_edges(const DevState& s, uint32_t* out, hipStream_t st) {
  if (!pp_state_ok(s)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(out, 0, 4, st);
  if (e != hipSuccess) return e;
  const uint32_t blocks = grid_for(s.n, kPPBlock, 8192);
  hipLaunchKernelGGL(k_pp_live_edges, dim3(blocks), dim3(kPPBlock), 0, st, s, out);
  return hipGetLastError();
}

hipError_t pp_fmask_build(const DevState& s, const unsigned long long* rend, const uint32_t* rsrc,
                          const uint8_t* rslot, uint8_t* fmask, hipStream_t st) {
  hipError_t e = hipMemsetAsync(fmask, 0, (s.n + 3) & ~3ull, st);
  if (e != hipSuccess) return e;
  const uint32_t blocks = grid_for(s.n, kPPBlock, 8192);
  hipLaunchKernelGGL(k_pp_fmask, dim3(blocks), dim3(kPPBlock), 0, st, s, rend, rsrc, rslot, (uint32_t*)fmask);
  return hipGetLastError();
}

hipError_t pp_rfail_build(const DevState& s, const unsigned long long* rend, const uint32_t* rsrc,
                          const uint8_t* rslot, uint32_t* rfail, hipStream_t st) {
  const uint64_t NW = (s.n * s.stride + 31) >> 5;  // at most; word NW + 1 is the hub flag
  uint32_t* hub = rfail + NW + 1;
  hipError_t e = hipMemsetAsync(rfail, 0, (NW + 2) * 4, st);
  if (e != hipSuccess) return e;
  const uint32_t blocks = grid_for(s.W, kPPBlock, 8192);
  hipLaunchKernelGGL(k_pp_rfail, dim3(blocks ? blocks : 1), dim3(kPPBlock), 0, st, s, rend, rsrc, rslot, rfail, hub);
  const uint32_t hblocks = grid_for(s.n, 64 * (kPPBlock / 64), 4096);  // a wave per 64 nodes
  hipLaunchKernelGGL(k_pp_rfail_hubs, dim3(hblocks ? hblocks : 1), dim3(kPPBlock), 0, st, s, rend, rsrc, rfail, hub);
  return hipGetLastError();
}

hipError_t pp_fmask_any(const uint8_t* fmask, uint64_t n, unsigned long long* fany, hipStream_t st) {
  const uint64_t W = (n + 63) >> 6;
  const uint32_t blocks = grid_for(W, kPPBlock, 8192);
  hipLaunchKernelGGL(k_pp_fmask_any, dim3(blocks), dim3(kPPBlock), 0, st, fmask, n, fany);
  return hipGetLastError();
}

hipError_t pp_fmask_rows(const DevState& s, uint8_t* fmask, hipStream_t st) {
  if (!pp_state_ok(s) || !fmask) return hipErrorInvalidValue;
  const uint32_t blocks = grid_for(s.n, kPPBlock, 8192);
  hipLaunchKernelGGL(k_pp_fmask_rows, dim3(blocks), dim3(kPPBlock), 0, st, s, fmask);
  return hipGetLastError();
}

}  // namespace gs
