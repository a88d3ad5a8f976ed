// gs_pp_dev.h -- what the push-pull engine's translation units share.
//
// One file per round mode or preparation step:
//   word summaries, commit; pp_round / pp_commit, which
//   queue every mode's kernels for a round           gs_pp_dense.hip
//   sparse early rounds over the informed list, seed gs_pp_early.hip
//   the three table-streaming round kernels (top-down,
//   bottom-up, pull-answer), the sharded round       gs_pp_round.hip
//   the pull-answer rounds' deferred sets            gs_pp_defer.hip
//   reverse table, both builders (hipcub only here)  gs_pp_rev.hip
//   failure masks, the exact stop test               gs_pp_fmask.hip
// (k_pp_round sits with k_ppb_round and k_ppa_round: all three instantiate
// block_add<1024>, and alone in a file the compiler folds that call's
// arguments before inlining and schedules the kernel's tail differently.)
//
// Here: only what more than one of them uses, and the launchers through which
// pp_round and pp_commit reach the kernels of the other files (kernels stay
// in anonymous namespaces).  A constant or helper with one user lives beside
// that user; what the host code calls is declared in gs_internal.h; wave and
// block primitives that other engines use too are in gs_wave.h.
#pragma once
#include "gs_internal.h"
#include "gs_wave.h"

namespace gs {

constexpr uint32_t kPPBlock = 256;

// Every context sets grecv / gcrash (ctx_setup: = recv / crash; push-pull
// shards: the replicated sets); a launch without them would fault.
inline bool pp_state_ok(const DevState& s) { return s.recv && s.crash && s.grecv && s.gcrash; }

// Per-block sums of nf <= 3 counters over a block of B threads (sh: 3 * B / 64
// words of LDS) into row[fld[0..nf)], one atomic each.
namespace {
template <uint32_t B>
__device__ __forceinline__ void block_add(uint64_t* sh, const uint64_t (&v)[3], uint32_t nf,
                                          unsigned long long* row, const uint32_t (&fld)[3]) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < 3 * (B / 64)) sh[tid] = 0;
  __syncthreads();
  for (uint32_t i = 0; i < nf; ++i) {
    const uint64_t s = wave_sum64(v[i]);
    if (lane == 0) sh[i * (B / 64) + wv] = s;
  }
  __syncthreads();
  if (tid < nf) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < B / 64; ++k) s += sh[tid * (B / 64) + k];
    if (s) atomicAdd(&row[fld[tid]], (unsigned long long)s);
  }
}
}  // namespace

// One round's launches outside gs_pp_dense.hip, in the order pp_round and
// pp_commit queue them.  All but the top-down round do nothing without sp.ctl,
// and each kernel returns at once unless ctl->mode is its own; errors:
// hipGetLastError.
// gs_pp_early.hip: the round's mode (k_pp_mode), then the early round.
void pp_launch_early(const DevState& s, unsigned long long* next, const PPSparse& sp, uint32_t t, hipStream_t st);
// gs_pp_round.hip: the top-down round over the summaries pp_round just built.
void pp_launch_topdown(const DevState& s, unsigned long long* next, const unsigned long long* sumA,
                       const unsigned long long* sumB, const unsigned long long* sum2, uint64_t S2, uint32_t t,
                       bool l2_only_flag, const PPSparse& sp, hipStream_t st);
// gs_pp_round.hip: the bottom-up round, the pull-answer round and (through
// pp_launch_deferred) its deferred sets.
void pp_launch_answer(const DevState& s, unsigned long long* next, const PPSparse& sp, uint32_t t, hipStream_t st);
// gs_pp_defer.hip: with deferred sets (sp.dset), the partition of the nlists
// per-workgroup lists k_ppa_round filled and the OR into next.
void pp_launch_deferred(const DevState& s, unsigned long long* next, const PPSparse& sp, uint32_t nlists,
                        hipStream_t st);
// gs_pp_early.hip: the early round's commit.
void pp_launch_early_commit(const DevState& s, const unsigned long long* next, const PPSparse& sp, uint32_t t,
                            hipStream_t st);

}  // namespace gs
