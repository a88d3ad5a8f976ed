// gs_win_units.hip -- the window engine's bookkeeping (gs_win_dev.h has the
// pipeline):
//   units     fires per (fine bucket f, tick k), bucket-major; hipcub scan ->
//             firing index
//   groupmap  first unit of every 64-node group of firing indices
// and, for device-driven windows, the cut, the unit scan on the device and the
// close (per-tick counters, the stop rule).
#include <hipcub/hipcub.hpp>

#include "gs_win_dev.h"

namespace gs {
namespace {

// Units = (fine bucket f, tick k), bucket-major (u = f*Ls + k, Ls = the layout
// stride: L, or lmax for device-driven windows): the L fire lists of one
// bucket are expanded back to back, so friends-row lines that several ticks of
// the window share are fetched once into the XCD's L2.  usize = fires;
// tfires[k] = fires per tick (the window cut).  Also zeroes the window's
// counters (one launch instead of several memsets).
__device__ __forceinline__ void units_body(const WinState& w, uint32_t t0, uint32_t L) {
  __shared__ uint32_t s_t[kMaxWindow];
  uint32_t Ls = L;
  if (w.ctl) {
    L = win_open(w, t0);
    if (!L) return;
    Ls = w.lstride;
  }
  const uint32_t units = Ls * w.nfine;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  // 256-bucket tiles: the L fcount rows are read coalesced (bucket fastest),
  // transposed in LDS and written bucket-major, coalesced.
  __shared__ uint32_t s_tile[256 * (kMaxWindow + 1)];
  uint32_t acc[kMaxWindow];
#pragma unroll
  for (uint32_t k = 0; k < kMaxWindow; ++k) acc[k] = 0;
  if (threadIdx.x < kMaxWindow) s_t[threadIdx.x] = 0;
  if (tid == 0) w.usize[units] = 0;
  __syncthreads();
  __shared__ uint32_t s_ts[kMaxWindow];  // this tile's fires per tick
  uint32_t slot[kMaxWindow];  // ring slot of tick t0 + k (uniform)
#pragma unroll
  for (uint32_t k = 0; k < kMaxWindow; ++k) slot[k] = k < L ? (t0 + k) % w.R : 0u;
  for (uint32_t f0 = blockIdx.x * 256; f0 < w.nfine; f0 += gridDim.x * 256) {
    const uint32_t f = f0 + threadIdx.x;
    if (threadIdx.x < kMaxWindow) s_ts[threadIdx.x] = 0;
    // all L loads in flight before the first use (one latency, not L)
    uint32_t cv[kMaxWindow];
#pragma unroll
    for (uint32_t k = 0; k < kMaxWindow; ++k)
      cv[k] = k < L && k < Ls && f < w.nfine ? w.fcount[(size_t)slot[k] * w.nfine + f] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kMaxWindow; ++k) {
      if (k < Ls) {
        s_tile[threadIdx.x * (kMaxWindow + 1) + k] = cv[k];
        acc[k] += cv[k];
      }
    }
    __syncthreads();
    // per-tile sums for the device-driven unit scan (k_cut, k_unitscan)
#pragma unroll
    for (uint32_t k = 0; k < kMaxWindow; ++k) {
      if (k < Ls) {
        const uint32_t c = wave_sum(s_tile[threadIdx.x * (kMaxWindow + 1) + k]);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_ts[k], c);
      }
    }
    __syncthreads();
    if (threadIdx.x < Ls) w.tsum[(size_t)(f0 >> 8) * kMaxWindow + threadIdx.x] = s_ts[threadIdx.x];
    const uint32_t nb = min(256u, w.nfine - f0), base = f0 * Ls;
    for (uint32_t i = threadIdx.x; i < nb * Ls; i += 256) {
      const uint32_t b = i / Ls, k = i - b * Ls;
      w.usize[base + i] = s_tile[b * (kMaxWindow + 1) + k];
    }
    __syncthreads();
  }
#pragma unroll
  for (uint32_t k = 0; k < kMaxWindow; ++k)
    if (acc[k]) atomicAdd(&s_t[k], acc[k]);
  __syncthreads();
  if (threadIdx.x < L && s_t[threadIdx.x]) atomicAdd(&w.tfires[threadIdx.x], (unsigned long long)s_t[threadIdx.x]);
  for (uint32_t i = tid; i < kRegions; i += nth) { w.chist[i] = 0; w.cfill[i] = 0; }
  for (uint32_t i = tid; i < w.nfine; i += nth) w.ffill[i] = 0;
  if (w.dd && tid == 0) {  // this shard's gathered row: flag word, buffer capacities
    w.cfill[kRegions] = 0;
    w.cfill[kRegions + 1] = w.ctl->fmsg_cap;
    w.cfill[kRegions + 2] = w.ctl->xs_cap;
    w.cfill[kRegions + 3] = w.ctl->xr_cap;
  }
  // host-driven windows clear the overflow flags here; device-driven and shard
  // windows keep them until the host has redone the window
  if (tid == 0 && !w.ctl && !w.abort_on_err) *w.err &= ~(kErrCoarse | kErrFine);
}
__global__ __launch_bounds__(256) void k_units(const WinState w, uint32_t t0, uint32_t L) { units_body(w, t0, L); }

// The device-driven shard windows of an in-process group launch each small
// per-shard kernel once for all M shards: shard blockIdx.y (or blockIdx.x for
// the one-block kernels) reads its window state from a device array.
__global__ __launch_bounds__(256) void k_units_m(const WinState* __restrict__ ws, uint32_t t0, uint32_t L) {
  units_body(ws[blockIdx.y], t0, L);
}

// Device-driven windows: the cut (as the host-driven engine makes it: a
// window holds whole ticks while its friend slots fit `budget`), the coarse
// region plan of the window's T friend slots, and the window's place in ctl.
// One block.
__device__ __forceinline__ void cut_body(const WinState& w, unsigned long long budget) {
  __shared__ unsigned long long s_sz[256];
  __shared__ unsigned long long s_T;
  __shared__ uint32_t s_go, s_L;
  WinCtl* c = w.ctl;
  const uint32_t b = threadIdx.x;  // 256 threads: thread b plans coarse bin b
  __shared__ unsigned long long s_tf[kMaxWindow];
  if (win_abort(w)) return;  // keep ctl: the host redoes the failed window
  uint32_t t = 0;
  const uint32_t Lw = win_open(w, t);
  // every load this kernel needs is issued up front (one latency, not a chain)
  const unsigned long long cap = c->cmsg_cap;
  __shared__ unsigned long long s_own[kMaxWindow];  // device-driven shards: this shard's fires per tick
  if (b < kMaxWindow) {
    if (w.dd) {  // the cut from every shard's gathered counts: the same window on every shard
      unsigned long long g = 0;
      for (uint32_t r = 0; r < w.G; ++r) g += w.gcnt[(size_t)r * kMaxWindow + b];
      s_tf[b] = g;
      s_own[b] = w.tfires[b];
    } else {
      s_tf[b] = w.tfires[b];
    }
  }
  unsigned long long ts[4][kMaxWindow];  // this thread's tiles' fires per tick
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
#pragma unroll
    for (uint32_t k = 0; k < kMaxWindow; ++k)
      ts[j][k] = Lw && b * 4 + j < w.ncoarse ? w.tsum[(size_t)(b * 4 + j) * kMaxWindow + k] : 0ull;
  __syncthreads();
  if (b == 0) {
    s_go = Lw != 0;
    if (!Lw) {  // stopped or past tend: the rest of this window does nothing
      c->L = 0;
      c->Tn = 0;
    } else {
      uint32_t L = 1;
      unsigned long long Tn = s_tf[0];
      while (L < Lw && (Tn + s_tf[L]) * w.stride <= budget) Tn += s_tf[L++];
      if (w.dd) {  // this shard's own fires (its row is zeroed by k_unitscan, after every shard's cut)
        Tn = 0;
        for (uint32_t k = 0; k < L; ++k) Tn += s_own[k];
      } else {
        for (uint32_t k = 0; k < kMaxWindow; ++k) w.tfires[k] = 0;
      }
      c->t = t;
      c->L = L;
      s_L = L;
      c->tnext = t + L;
      c->Tn = Tn;
      // owner expand (shards): the plan of gs_shards.cpp's plan_coarse_owner over
      // the longest row; unsharded: over the stride
      c->T = Tn * (w.owner ? w.slots : w.stride);
      s_T = c->T;
    }
  }
  __syncthreads();
  if (!s_go) return;
  {
    // firing index of each 256-bucket tile's first unit (ticks >= L count as
    // empty): k_unitscan finishes the scan inside the tiles (ncoarse <= 1024)
    const uint32_t L = s_L, nt = w.ncoarse;
    unsigned long long v[4], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      v[j] = 0;
#pragma unroll
      for (uint32_t k = 0; k < kMaxWindow; ++k) v[j] += k < L ? ts[j][k] : 0ull;
      sum += v[j];
    }
    unsigned long long tot;
    unsigned long long pre = block_exscan_u64<4>(sum, &s_sz[0], &tot);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t tile = b * 4 + j;
      if (tile < nt) w.toff[tile] = pre;
      pre += v[j];
    }
    if (b == 0) w.toff[nt] = tot;
    __syncthreads();
  }
  // coarse regions: each sub-region gets 1/8 of its bin's node share of T,
  // plus 512 (plan_coarse on the host)
  unsigned long long sub = 0;
  if (!w.owner) {
    const unsigned long long lo = (unsigned long long)b << kCoarseShift;
    const unsigned long long hi = min((unsigned long long)w.n, lo + (1ull << kCoarseShift));
    const double xr = (double)kXRoundNodes * w.stride;  // one expand round's slots (kXRoundNodes)
    sub = b < w.ncoarse
              ? (unsigned long long)(((double)s_T / kCoarseSub + xr) * (double)(hi - lo) / (double)w.n) + 512
              : 0ull;
  } else {  // bin b = owner d * obins + 2^22-node chunk of d's range (plan_coarse_owner)
    const uint32_t d = b / w.obins, k = b % w.obins;
    unsigned long long cnt = 0;
    if (d < w.G) {
      const unsigned long long dlo = (unsigned long long)d * w.seg_per;
      const unsigned long long dhi = min(dlo + w.seg_per, (unsigned long long)w.nglob);
      const unsigned long long lo = dlo + ((unsigned long long)k << kCoarseShift);
      const unsigned long long hi = min(dhi, lo + (1ull << kCoarseShift));
      cnt = hi > lo ? hi - lo : 0ull;
    }
    const double xr = (double)kXRoundNodes * w.slots;
    sub = cnt ? (unsigned long long)(((double)s_T / kCoarseSub + xr) * (double)cnt / (double)w.nglob) + 512 : 0ull;
  }
  unsigned long long total;
  const unsigned long long base = block_exscan_u64<4>(sub * kCoarseSub, &s_sz[0], &total);
  if (total > cap) {  // the buffer is too small: no region at all, the host grows and redoes
    for (uint32_t x = 0; x < kCoarseSub; ++x) w.ccap[b * kCoarseSub + x] = 0;
    if (b == 0) {
      w.ccap[kRegions] = 0;
      atomicOr(w.err, kErrCoarse);
      if (w.dd) atomicOr(reinterpret_cast<unsigned int*>(&w.cfill[kRegions]), kErrCoarse);  // every shard stops
    }
    return;
  }
  for (uint32_t x = 0; x < kCoarseSub; ++x) w.ccap[b * kCoarseSub + x] = base + x * sub;
  if (b == 255) w.ccap[kRegions] = total;
}
__global__ __launch_bounds__(256) void k_cut(const WinState w, unsigned long long budget) { cut_body(w, budget); }
__global__ __launch_bounds__(256) void k_cut_m(const WinState* __restrict__ ws, unsigned long long budget) {
  cut_body(ws[blockIdx.x], budget);
}

// Device-driven windows: the unit scan inside each 256-bucket tile (thread =
// bucket, its Ls units contiguous; ticks >= L count as empty), offset by the
// tile's start from k_cut, and the group map of those units.  One block per
// tile.  (Host-driven windows: hipcub scan + k_groupmap.)
__device__ __forceinline__ void unitscan_body(const WinState& w) {
  __shared__ unsigned long long s_x[4];
  if (blockIdx.x >= w.ncoarse) return;  // shards of a group: the grid covers the largest
  uint32_t t0;
  const uint32_t L = win_live(w, t0, 0);
  if (!L) return;
  const uint32_t Ls = w.lstride, tile = blockIdx.x, f = tile * 256 + threadIdx.x;
  // device-driven shards: every shard's cut has read this shard's gathered
  // counts; its row restarts at 0 for the next window's k_units
  if (w.dd && tile == 0 && threadIdx.x < kMaxWindow) w.tfires[threadIdx.x] = 0;
  unsigned long long sz[kMaxWindow], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kMaxWindow; ++k)  // all loads in flight, then the sum
    sz[k] = k < L && f < w.nfine ? w.usize[(size_t)f * Ls + k] : 0ull;
#pragma unroll
  for (uint32_t k = 0; k < kMaxWindow; ++k) sum += sz[k];
  unsigned long long tot;
  unsigned long long a = w.toff[tile] + block_exscan_u64<4>(sum, s_x, &tot);
  if (f >= w.nfine) return;
#pragma unroll
  for (uint32_t k = 0; k < kMaxWindow; ++k) {
    if (k >= Ls) break;
    const uint32_t u = f * Ls + k;
    w.unit_off[u] = a;
    const unsigned long long b = a + sz[k];
    for (unsigned long long q = (a + 63) >> 6; (q << 6) < b; ++q) w.gmap[q] = u;
    a = b;
  }
  if (f == w.nfine - 1) w.unit_off[(size_t)w.nfine * Ls] = a;
}
__global__ __launch_bounds__(256) void k_unitscan(const WinState w) { unitscan_body(w); }
__global__ __launch_bounds__(256) void k_unitscan_m(const WinState* __restrict__ ws) { unitscan_body(ws[blockIdx.y]); }

// gmap[q] = unit holding firing index 64*q.
__global__ void k_groupmap(const WinState w, uint32_t L) {
  if (w.ctl) {
    uint32_t t0;
    if (!win_live(w, t0, 0)) return;
    L = w.lstride;
  }
  const uint32_t units = L * w.nfine;
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
    const unsigned long long a = w.unit_off[u], b = w.unit_off[u + 1];
    for (unsigned long long q = (a + 63) >> 6; (q << 6) < b; ++q) w.gmap[q] = u;
  }
}

__global__ void k_stats_reduce(const WinState w, uint32_t t0, uint32_t L) {  // as k_close's block
  if (w.abort_on_err && win_abort(w)) return;  // the redo of the window reduces them
  const uint32_t i = threadIdx.x / kCloseLanes, part = threadIdx.x % kCloseLanes;
  const uint32_t k = i / kStatFields, fld = i % kStatFields;
  if (k >= L) return;
  const unsigned long long sum = stat_shard_sum(w, i, part);
  if (part == 0 && sum) w.stats[(size_t)((t0 + k) % kStatSlots) * kStatFields + fld] += sum;
}

// Device-driven windows: the window's per-tick counters (stats ring, and
// staging slot `slot` for the host with the window's snapshot), the poll
// rule's running state and, at a poll tick, gs_run's stop rule
// (simulator.go:243-248: covered at float32 99 %; the engine also stops when
// nothing is pending or max_ticks has passed).  One block of 128 threads.
__global__ void k_close(const WinState w, uint32_t slot) {  // kMaxWindow * kStatFields * kCloseLanes threads
  __shared__ unsigned long long rows[kMaxWindow][kStatFields];
  WinCtl* c = w.ctl;
  unsigned long long* st = w.stage + (size_t)slot * kStageWords;
  uint32_t t0 = 0;
  const uint32_t L = win_live(w, t0, 0);
  const uint32_t i = threadIdx.x / kCloseLanes, part = threadIdx.x % kCloseLanes, tid = threadIdx.x;
  const uint32_t k = i / kStatFields, fld = i % kStatFields;
  if (k < L) {  // k is uniform over each lane group
    const unsigned long long sum = stat_shard_sum(w, i, part);
    if (part == 0) {
      rows[k][fld] = sum;
      w.stats[(size_t)((t0 + k) % kStatSlots) * kStatFields + fld] = sum;
      st[8 + k * kStatFields + fld] = sum;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  uint32_t stop = c->stop;
  if (L) {
    for (uint32_t j = 0; j < L; ++j) {
      c->recv += rows[j][ST_RECV];
      c->crashed += rows[j][ST_CRASH];
      c->pending += rows[j][ST_SCHED] - rows[j][ST_FIRED];
    }
    const uint32_t tl = t0 + L - 1;  // windows never cross a poll tick
    if (c->poll && (tl - c->pbase) % c->poll == 0 && !stop) {
      if (c->recv >= c->cover) stop = 1 + GS_RUN_COVERED;
      else if (c->pending == 0) stop = 1 + GS_RUN_QUIESCENT;
      else if (tl >= c->max_ticks) stop = 1 + GS_RUN_MAX_TICKS;
      c->stop = stop;
    }
  }
  st[0] = t0;
  st[1] = L;
  st[2] = stop;
  st[3] = *w.err;
  st[4] = L ? c->Tn : 0;
}

// started (batched trials with per-trial failure masks, else null): a failed
// sender never broadcasts, so its trial schedules nothing; started[i] = 1 for
// the trials that did.
__global__ void k_schedule_win(const WinState w, uint32_t node, uint32_t t, uint32_t trials, uint32_t n,
                               uint32_t* __restrict__ started) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= trials) return;
  uint32_t local = node;
  if (trials > 1 || node == ~0u) {
    uint32_t v = node;
    if (node == ~0u) v = uniform(philox(0, 0, 0, ctr3(K_SENDER, w.key.trial + i), w.key.k0, w.key.k1).x, n);
    local = (i << w.tlog) | v;  // batched contexts have base 0
  }
  if (started) {
    const bool dead = (w.crash[local >> 6] >> (local & 63)) & 1;
    started[i] = dead ? 0u : 1u;
    if (dead) return;
  }
  uint32_t kn, c3;
  node_key(w.tlog, w.tmask, w.key, (uint64_t)w.base + local, K_DELAY, kn, c3);
  const uint32_t off = fire_offset(w.delay_low, w.delay_span, philox(kn, t, 0, c3, w.key.k0, w.key.k1).x);
  const uint32_t s = (t + off) % w.R;
  const uint32_t f = local >> kFineLog;
  const uint32_t pos = atomicAdd(&w.fcount[(size_t)s * w.nfine + f], 1u);
  w.flist[((size_t)s * w.nfine + f) * kFineNodes + pos] = (uint16_t)(local & (kFineNodes - 1));
}

}  // namespace

hipError_t win_units_g(const WinGroup& g, uint32_t L, hipStream_t s) {
  const uint32_t blocks = std::max<uint32_t>(std::min<uint32_t>((g.nfine_max + 255) / 256, 4096), 1);
  hipLaunchKernelGGL(k_units_m, dim3(blocks, g.M), dim3(256), 0, s, g.ws, 0u, L);
  return hipGetLastError();
}

hipError_t win_cut_g(const WinGroup& g, unsigned long long budget, hipStream_t s) {
  hipLaunchKernelGGL(k_cut_m, dim3(g.M), dim3(256), 0, s, g.ws, budget);
  return hipGetLastError();
}

hipError_t win_unitscan_g(const WinGroup& g, hipStream_t s) {
  hipLaunchKernelGGL(k_unitscan_m, dim3(std::max<uint32_t>(g.ncoarse_max, 1), g.M), dim3(256), 0, s, g.ws);
  return hipGetLastError();
}

hipError_t win_units(const WinState& w, uint32_t t0, uint32_t L, hipStream_t s) {
  (void)L;
  const uint32_t blocks = std::max<uint32_t>(std::min<uint32_t>((w.nfine + 255) / 256, 4096), 1);
  hipLaunchKernelGGL(k_units, dim3(blocks), dim3(256), 0, s, w, t0, L);
  return hipGetLastError();
}

hipError_t win_cut(const WinState& w, unsigned long long budget, hipStream_t s) {
  hipLaunchKernelGGL(k_cut, dim3(1), dim3(256), 0, s, w, budget);
  return hipGetLastError();
}

hipError_t win_unitscan(const WinState& w, hipStream_t s) {
  hipLaunchKernelGGL(k_unitscan, dim3(w.ncoarse), dim3(256), 0, s, w);
  return hipGetLastError();
}

hipError_t win_close(const WinState& w, uint32_t slot, hipStream_t s) {
  hipLaunchKernelGGL(k_close, dim3(1), dim3(kMaxWindow * kStatFields * kCloseLanes), 0, s, w, slot);
  return hipGetLastError();
}

hipError_t win_scan_units(const WinState& w, uint32_t L, void* tmp, size_t& tmp_bytes, hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, (const unsigned long long*)w.usize,
                                          w.unit_off, (int)(L * w.nfine + 1), s);
}

hipError_t win_groupmap(const WinState& w, uint32_t L, hipStream_t s) {
  const uint32_t units = L * w.nfine;
  const uint32_t blocks = std::min<uint32_t>((units + 255) / 256, 4096);
  hipLaunchKernelGGL(k_groupmap, dim3(blocks ? blocks : 1), dim3(256), 0, s, w, L);
  return hipGetLastError();
}

hipError_t win_stats_reduce(const WinState& w, uint32_t t0, uint32_t L, hipStream_t s) {
  hipLaunchKernelGGL(k_stats_reduce, dim3(1), dim3(kMaxWindow * kStatFields * kCloseLanes), 0, s, w, t0, L);
  return hipGetLastError();
}

hipError_t win_schedule(const WinState& w, uint32_t node, uint32_t tick, uint32_t trials, uint32_t n,
                        hipStream_t s, uint32_t* started) {
  hipLaunchKernelGGL(k_schedule_win, dim3((trials + 255) / 256), dim3(256), 0, s, w, node, tick, trials, n, started);
  return hipGetLastError();
}

}  // namespace gs
