// gs_pp_round.hip -- push-pull: the rounds that stream the table -- top-down
// (PP_DENSE, k_pp_round) and the two that walk the reverse table
// (gs_pp_rev.hip) instead: bottom-up (PP_BOTTOM) and pull-answer (PP_ANSWER,
// gs_internal.h; its deferred sets are applied in gs_pp_defer.hip) -- and the
// sharded round, which runs one of those two.  The model is stated in gs_pp_dense.hip.
#include "gs_pp_dev.h"

namespace gs {
namespace {

// Each wave owns kPPU consecutive bitset words per pass and issues the loads
// of all of them phase by phase (state words + deg, then the friend id, then
// the peer word's summary, then the peer-word gathers), so kPPU independent
// dependency chains are in flight per wave: one word per pass left the launch
// bound by the chain's latency (8.8 ms per round with no gathers at all).
constexpr uint32_t kPPU = 8;

// The second-level summaries (2 x S2 words, 61 KB at N = 1e9) are staged in
// LDS when they fit (S2 > 0): a call whose peer's 4096-node block has no
// informed node (pull) or no live uninformed node (push) then skips the L2
// summary load too.  Persistent 1024-thread blocks, two per CU.
constexpr uint32_t kPPRoundBlock = 1024;
constexpr uint64_t kPPMaxS2 = 4000;  // 2 x 31.25 KB of dynamic LDS (under the 64 KB default)

__global__ __launch_bounds__(kPPRoundBlock) void k_pp_round(const DevState s,
                                                            unsigned long long* __restrict__ next,
                                                            const unsigned long long* __restrict__ sumA,
                                                            const unsigned long long* __restrict__ sumB,
                                                            const unsigned long long* __restrict__ sum2,
                                                            uint32_t S2, uint32_t t, const PPCtl* ctl,
                                                            const uint8_t* __restrict__ fmask) {
  __shared__ uint64_t sh[3 * (kPPRoundBlock / 64)];
  extern __shared__ unsigned long long l2sum[];  // [0,S2) A2, [S2,2*S2) B2
  if (ctl && ctl->mode != PP_DENSE) return;
  for (uint32_t j = threadIdx.x; j < 2 * S2; j += kPPRoundBlock) l2sum[j] = sum2[j];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial);
  const bool cc = s.check_crashed;
  uint64_t fired = 0, sent = 0, msgs = 0;
  const uint64_t W = (s.n + 63) >> 6;
  const uint64_t wid = (uint64_t)blockIdx.x * (kPPRoundBlock / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kPPRoundBlock / 64) * kPPU;
  for (uint64_t w0 = wid * kPPU; w0 < W; w0 += step) {  // wave-uniform
    unsigned long long Iw[kPPU], Fw[kPPU];
    uint32_t d[kPPU], u[kPPU], fm[kPPU];
    bool push[kPPU], kept[kPPU], sbit[kPPU];
#pragma unroll
    for (uint32_t i = 0; i < kPPU; ++i) {
      const uint64_t word = w0 + i, v = (word << 6) + lane;
      const bool inb = word < W;
      Iw[i] = inb ? s.recv[word] : 0ull;
      Fw[i] = inb ? s.crash[word] : ~0ull;
      d[i] = v < s.n ? s.deg[v] : 0u;
      fm[i] = fmask && v < s.n ? fmask[v] : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kPPU; ++i) {
      const uint64_t v = ((w0 + i) << 6) + lane;
      if ((Fw[i] >> lane) & 1) d[i] = 0;  // failed (or past the table): never calls
      push[i] = (Iw[i] >> lane) & 1;
      u[i] = 0;
      kept[i] = false;
      if (d[i] > 0) {
        const u32x4 r = philox((uint32_t)v, t, 0, c3, s.key.k0, s.key.k1);
        const uint32_t j = uniform(r.x, d[i]);
        u[i] = s.ids[v * s.stride + j];
        fm[i] = (fm[i] >> j) & 1;  // the picked friend is failed (fmask)
        kept[i] = (int32_t)uniform(r.y, 100u) >= s.kd;
      }
    }
    // summaries (L2 resident): push -> u's word has a live uninformed node;
    // pull -> u's word has an informed node.  A dropped call needs neither.
#pragma unroll
    for (uint32_t i = 0; i < kPPU; ++i) {
      sbit[i] = false;
      if (kept[i]) {
        const bool top = S2 == 0 || ((l2sum[(push[i] ? S2 : 0u) + (u[i] >> 18)] >> ((u[i] >> 12) & 63)) & 1);
        if (top) sbit[i] = ((push[i] ? sumB : sumA)[u[i] >> 12] >> ((u[i] >> 6) & 63)) & 1;
      }
    }
    unsigned long long Iu[kPPU], Cu[kPPU];
#pragma unroll
    for (uint32_t i = 0; i < kPPU; ++i) {
      // pulls gather the peer's word; a push needs no gather (its atomicOr
      // below is idempotent and returns nothing, so the wave does not wait)
      Iu[i] = (sbit[i] && !push[i]) ? s.recv[u[i] >> 6] : 0ull;
      // the failed-mask gather only when a mask was set (gs_set_failed) and
      // no per-node failed-slot mask replaces it
      Cu[i] = (cc && !fmask && kept[i] && push[i]) ? s.crash[u[i] >> 6]
              : (fm[i] ? (1ull << (u[i] & 63)) : 0ull);
    }
#pragma unroll
    for (uint32_t i = 0; i < kPPU; ++i) {
      const unsigned long long ubit = 1ull << (u[i] & 63);
      bool pulled = false;
      if (d[i] > 0) ++fired;
      if (kept[i]) {
        if (push[i]) {
          ++sent;
          if (!(Cu[i] & ubit)) {  // u live: delivered
            ++msgs;
            // sbit clear: every live node of u's word is informed already
            if (sbit[i]) atomicOr(&next[u[i] >> 6], ubit);
          }
        } else if (Iu[i] & ubit) {  // pull from an informed u (u informed => u live)
          ++sent;
          ++msgs;
          pulled = true;
        }
      }
      const unsigned long long bal = __ballot(pulled);
      if (lane == 0 && bal) atomicOr(&next[w0 + i], bal);
    }
  }
  const uint64_t v3[3] = {fired, sent, msgs};
  const uint32_t f3[3] = {ST_FIRED, ST_SENT, ST_MSGS};
  block_add<kPPRoundBlock>(sh, v3, 3, s.stats + (size_t)(t % kStatSlots) * kStatFields, f3);
}

// Bottom-up dense round (PPMode PP_BOTTOM, gs_internal.h).  Same draws,
// outcomes and counters as k_pp_round.  A wave owns ranges of kPPRange words
// (4096 nodes) and streams them a lane per node: an informed caller counts
// its push (sent; msgs unless fmask marks the picked friend failed) and reads
// nothing else; an uninformed live node joins the wave's LDS queue.  Each 64
// queued nodes are resolved together, a lane each: the pull (friend id + the
// friend's recv word) and the push receipts, found among the node's in-edges
// (v, j) -- v's pick is recomputed from the packed slot byte (no deg gather),
// and only a kept pick of slot j costs a gather of v's recv word.  So the
// dependent-load chain runs for full waves of uninformed nodes however few
// are left, and the range's newly informed gather in LDS and are stored, not
// OR'ed (the wave owns its words).
#ifndef GS_PPB
#define GS_PPB 8
#endif
constexpr uint32_t kPPB = GS_PPB;   // words loaded together while streaming
constexpr uint32_t kPPRange = 64;   // words per wave range (multiple of kPPB)
constexpr uint32_t kPPQ = 128;      // queue entries per wave (<= 63 left + 64 appended)
constexpr uint32_t kPPEdges = 4;    // in-edges loaded per batch
#ifndef GS_PPS_BLOCK
#define GS_PPS_BLOCK 1024
#endif
constexpr uint32_t kPPSBlock = GS_PPS_BLOCK;  // k_ppb_round / k_ppa_round workgroup
constexpr uint32_t kPPWaves = kPPSBlock / 64;
constexpr uint32_t kPPSGrid = 512 * 1024 / kPPSBlock;  // at most 8192 waves per launch

// Position of the k-th set bit of m (k < popc(m)).
__device__ __forceinline__ uint32_t nth_bit(unsigned long long m, uint32_t k) {
  uint32_t pos = 0, x = (uint32_t)m, c = (uint32_t)__popc(x);
  if (k >= c) { k -= c; x = (uint32_t)(m >> 32); pos = 32; }
  c = (uint32_t)__popc(x & 0xFFFFu);
  if (k >= c) { k -= c; x >>= 16; pos += 16; }
  c = (uint32_t)__popc(x & 0xFFu);
  if (k >= c) { k -= c; x >>= 8; pos += 8; }
  c = (uint32_t)__popc(x & 0xFu);
  if (k >= c) { k -= c; x >>= 4; pos += 4; }
  c = (uint32_t)__popc(x & 0x3u);
  if (k >= c) { k -= c; x >>= 2; pos += 2; }
  return pos + (k >= (x & 1u) ? 1u : 0u);
}

// The set bits of a wave's 64 words (lane l holds the mask of word l of the
// range), in node order, 64 at a time: f(cnt, off) runs wave-wide with lane
// j < cnt holding the node offset (word * 64 + bit) of the next bit.  A wave
// scan of the popcounts, then a binary search of the lane's word in LDS (pre:
// 64 u32, msk: 64 u64 of the wave) and the bit's rank inside it: the queue of
// a range is its nodes in order, so a 64-node batch touches few lines of the
// in-edge lists and of the degree bytes.
template <class F>
__device__ __forceinline__ void for_each_bit(unsigned long long m, uint32_t* pre, unsigned long long* msk, F&& f) {
  const uint32_t lane = threadIdx.x & 63, c = (uint32_t)__popcll(m);
  const uint32_t x = (uint32_t)wave_inscan((int)c);
  const uint32_t total = (uint32_t)__shfl((int)x, 63, 64);
  if (!total) return;
  pre[lane] = x - c;
  msk[lane] = m;
  wave_lds_sync();
  for (uint32_t p0 = 0; p0 < total; p0 += 64) {
    const uint32_t p = p0 + lane;
    uint32_t off = 0;
    if (p < total) {
      uint32_t lo = 0, hi = 63;  // the last word whose first bit ranks <= p
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= p) lo = mid; else hi = mid - 1;
      }
      off = (lo << 6) + nth_bit(msk[lo], p - pre[lo]);
    }
    f(min(64u, total - p0), off);
  }
  wave_lds_sync();  // pre / msk are reused by the next range
}

// Node u's in-edges [qb, qe): from the compact view (PPSparse::rend16 /
// rbase: the dense rounds read 2 B per node of it instead of 8 of rend, and
// they read it for most nodes) or from rend.
__device__ __forceinline__ void in_edges(const PPSparse& sp, uint64_t u, unsigned long long& qb,
                                         unsigned long long& qe) {
  if (sp.rend16) {
    const unsigned long long b = sp.rbase[u >> 6];
    qb = b + ((u & 63) ? (unsigned long long)sp.rend16[u - 1] : 0ull);
    qe = b + sp.rend16[u];
  } else {
    qb = u ? sp.rend[u - 1] : 0ull;
    qe = sp.rend[u];
  }
}

// Resolves queue entries [0, cnt) (cnt <= 64), one per lane.  Entry = node
// offset in the range (12 bits) | deg << 16.
__device__ __forceinline__ void ppb_resolve(const DevState& s, const PPSparse& sp, uint32_t t, uint32_t c3,
                                            const uint32_t* q, uint32_t cnt, uint64_t base,
                                            unsigned long long* nb, uint64_t& sent, uint64_t& msgs) {
  const uint32_t lane = threadIdx.x & 63;
  if (lane >= cnt) return;
  const uint32_t e = q[lane], loc = e & 0xFFFu, d = e >> 16;
  const uint64_t v = base + loc;  // local id (global s.gbase + v)
  unsigned long long qb, qe;
  in_edges(sp, v, qb, qe);
  bool pull = false;
  uint32_t u = 0;
  if (d > 0) {
    const u32x4 r = philox((uint32_t)(s.gbase + v), t, 0, c3, s.key.k0, s.key.k1);
    if ((int32_t)uniform(r.y, 100u) >= s.kd) {
      u = s.ids[v * s.stride + uniform(r.x, d)];
      pull = true;
    }
  }
  const unsigned long long Iu = pull ? s.grecv[u >> 6] : 0ull;  // u is a global id
  const bool pulled = pull && ((Iu >> (u & 63)) & 1);  // u informed => u live
  // a node its own pull informs needs no push receipt (sp.pullfirst: the
  // in-edge scan waits for the pull's two dependent loads, and skips)
  bool got = sp.pullfirst && pulled;
  for (unsigned long long q0 = qb; q0 < qe && !got; q0 += kPPEdges) {
    uint32_t src[kPPEdges], x[kPPEdges];
#pragma unroll
    for (uint32_t k = 0; k < kPPEdges; ++k) {
      const bool in = q0 + k < qe;
      src[k] = in ? sp.rsrc[q0 + k] : 0u;
      x[k] = in ? sp.rslot[q0 + k] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPPEdges; ++k) {
      if (q0 + k >= qe) break;
      const u32x4 r = philox(src[k], t, 0, c3, s.key.k0, s.key.k1);
      if (uniform(r.x, (x[k] >> 4) + 1) == (x[k] & 15u) && (int32_t)uniform(r.y, 100u) >= s.kd)
        got |= ((s.grecv[src[k] >> 6] >> (src[k] & 63)) & 1) != 0;
    }
  }
  if (pulled) {
    ++sent;
    ++msgs;
  }
  if (pulled || got) atomicOr(&nb[loc >> 6], 1ull << (loc & 63));
}

__global__ __launch_bounds__(kPPSBlock) void k_ppb_round(const DevState s, unsigned long long* __restrict__ next,
                                                             const PPSparse sp, uint32_t t) {
  __shared__ uint64_t sh[3 * kPPWaves];
  __shared__ uint32_t s_q[kPPWaves][kPPQ];
  __shared__ unsigned long long s_nb[kPPWaves][kPPRange];
  __shared__ uint32_t s_pre[kPPWaves][64];
  __shared__ unsigned long long s_msk[kPPWaves][64];
  if (sp.ctl->mode != PP_BOTTOM) return;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* q = s_q[wv];
  unsigned long long* nb = s_nb[wv];
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial);
  const uint8_t* __restrict__ fmask = sp.fmask;
  uint64_t fired = 0, sent = 0, msgs = 0;
  const uint64_t W = (s.n + 63) >> 6;
  const uint64_t nrange = (W + kPPRange - 1) / kPPRange;
  // every live node calls (no empty rows) and no failed-slot mask: an
  // informed caller's push needs only its loss draw (sent = delivered), so
  // its degree byte is not loaded -- in the late rounds, nearly every node's
  const bool nodeg = sp.ctl->nlive0 == 0 && !fmask && sp.nodeg;
  // GS_PPB_WORDS (A/B): 0 a lane per node throughout, 1 a lane per word, 2 a
  // lane per word where no word holds more than sp.word_maxu live uninformed
  // nodes (default; 64, i.e. always)
  const uint32_t ppb_words = sp.words;
  // lane-per-word ranges: every live node calls, and a failed-slot mask (if
  // any) has its has-a-failed-friend bits
  const bool wordok = sp.ctl->nlive0 == 0 && sp.nodeg && (!fmask || sp.fany);
  for (uint64_t rg = (uint64_t)blockIdx.x * kPPWaves + wv; rg < nrange; rg += (uint64_t)gridDim.x * kPPWaves) {
    const uint64_t w0 = rg * kPPRange, base = w0 << 6;
    nb[lane] = 0;
    uint32_t qn = 0;  // wave-uniform
    bool by_word = false;
    const uint64_t word = w0 + lane;
    unsigned long long mi = 0, mu = 0;
    if (wordok && ppb_words) {
      if (word < W) {
        const uint64_t left = s.n - (word << 6);
        const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1);
        const unsigned long long Iw = s.recv[word], Fw = s.crash[word];
        mi = Iw & ~Fw & valid;
        mu = ~Iw & ~Fw & valid;
      }
      uint32_t mx = (uint32_t)__popcll(mu);  // the most live uninformed nodes of one word
#pragma unroll
      for (uint32_t o = 32; o >= 1; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
      by_word = ppb_words == 1 || mx <= sp.word_maxu;
    }
    if (by_word) {
      // a lane per WORD of the range: an informed caller costs its loss draw
      // and a bit scan, no per-node load, ballot or queue step (the late
      // rounds, where nearly every caller is informed, are VALU-bound); the
      // range's live uninformed nodes are resolved 64 at a time in node order
      // (for_each_bit)
      fired += (uint64_t)(__popcll(mi) + __popcll(mu));  // nodeg: every live node calls
      const uint32_t vb = (uint32_t)(s.gbase + (word << 6));
      unsigned long long mf = fmask && word < W ? sp.fany[word] & mi : 0ull;
      uint32_t pushed = 0, dead = 0;
      while (mi) {
        const uint32_t b = (uint32_t)__builtin_ctzll(mi);
        mi &= mi - 1;
        const u32x4 r = philox(vb + b, t, 0, c3, s.key.k0, s.key.k1);
        pushed += (int32_t)uniform(r.y, 100u) >= s.kd ? 1u : 0u;
      }
      // callers with a failed friend (a push to it is sent, not delivered): a
      // second pass with their draws made again, so the loop above never waits
      // for a degree or mask byte (one of ~17 callers at 1 % failed, but in
      // nearly every step of a 64-lane wave)
      while (mf) {
        const uint32_t b = (uint32_t)__builtin_ctzll(mf);
        mf &= mf - 1;
        const uint64_t v = (word << 6) + b;
        const uint32_t fm = fmask[v], d = s.deg[v];
        const u32x4 r = philox(vb + b, t, 0, c3, s.key.k0, s.key.k1);
        if ((int32_t)uniform(r.y, 100u) >= s.kd) dead += (fm >> uniform(r.x, d)) & 1;
      }
      sent += pushed;
      msgs += pushed - dead;
      for_each_bit(mu, s_pre[wv], s_msk[wv], [&](uint32_t cnt, uint32_t off) {
        q[lane] = lane < cnt ? off | (uint32_t)s.deg[base + off] << 16 : 0u;
        wave_lds_sync();
        ppb_resolve(s, sp, t, c3, q, cnt, base, nb, sent, msgs);
        wave_lds_sync();
      });
    }
    for (uint32_t wi = 0; wi < kPPRange && !by_word; wi += kPPB) {
      unsigned long long Iw[kPPB];
      uint32_t d[kPPB], fm[kPPB];
      bool live[kPPB];
#pragma unroll
      for (uint32_t i = 0; i < kPPB; ++i) {
        const uint64_t word = w0 + wi + i, v = (word << 6) + lane;
        const bool inb = word < W;
        Iw[i] = inb ? s.recv[word] : ~0ull;
        const unsigned long long Fw = inb ? s.crash[word] : ~0ull;
        live[i] = v < s.n && !((Fw >> lane) & 1);
        d[i] = live[i] && !(nodeg && ((Iw[i] >> lane) & 1)) ? s.deg[v] : (live[i] ? 1u : 0u);
        fm[i] = fmask && live[i] ? fmask[v] : 0u;
      }
#pragma unroll
      for (uint32_t i = 0; i < kPPB; ++i) {
        const uint64_t v = ((w0 + wi + i) << 6) + lane;
        const bool inf = (Iw[i] >> lane) & 1;
        if (d[i] > 0) {
          ++fired;
          if (inf) {  // push: the receiver finds it
            const u32x4 r = philox((uint32_t)(s.gbase + v), t, 0, c3, s.key.k0, s.key.k1);
            if ((int32_t)uniform(r.y, 100u) >= s.kd) {
              ++sent;
              if (!((fm[i] >> uniform(r.x, d[i])) & 1)) ++msgs;
            }
          }
        }
        const bool enq = live[i] && !inf;
        const unsigned long long bal = __ballot(enq);
        if (enq) {
          const uint32_t at = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
          q[at] = (uint32_t)(v - base) | d[i] << 16;
        }
        qn += (uint32_t)__popcll(bal);
        if (qn >= 64) {
          wave_lds_sync();
          ppb_resolve(s, sp, t, c3, q, 64, base, nb, sent, msgs);
          const uint32_t rest = qn - 64;
          const uint32_t keep = lane < rest ? q[64 + lane] : 0u;
          wave_lds_sync();
          if (lane < rest) q[lane] = keep;
          qn = rest;
        }
      }
    }
    wave_lds_sync();
    if (qn) ppb_resolve(s, sp, t, c3, q, qn, base, nb, sent, msgs);
    wave_lds_sync();
    const unsigned long long x = nb[lane];
    if (x && word < W) next[word] = s.recv[word] | x;
    wave_lds_sync();  // nb and q are reused by the next range
  }
  const uint64_t v3[3] = {fired, sent, msgs};
  const uint32_t f3[3] = {ST_FIRED, ST_SENT, ST_MSGS};
  block_add<kPPSBlock>(sh, v3, 3, s.stats + (size_t)(t % kStatSlots) * kStatFields, f3);
}

// Pull-answer round (PP_ANSWER): same draws, outcomes and counters as
// k_pp_round.  A wave streams ranges of kPPRange words, a lane per node, and
// queues its INFORMED nodes in LDS; each 64 queued nodes are resolved
// together, a lane each: the node's own call (a push, as top-down: one
// no-return atomicOr into its friend's word unless the friend is failed) and
// the pulls it answers -- its in-edges (v, j) whose caller v picks slot j
// (recomputed from the packed slot byte) and is not lost; only such an
// in-edge costs a gather of v's recv / failed words (v must be live and
// uninformed: its call is a pull from this informed node, counted here).
// Every live caller is counted as fired from ctl->ncallers.
// Node x is informed this round: appended to this workgroup's deferred list
// (the active lanes with `take`, one LDS atomic per wave and call), or, with
// no deferred buffers or a full list, an atomicOr into next.
__device__ __forceinline__ void pp_set(const PPSparse& sp, unsigned long long* __restrict__ next, bool take,
                                       uint32_t x, uint32_t* s_dn) {
  if (!sp.dset) {
    if (take) atomicOr(&next[x >> 6], 1ull << (x & 63));
    return;
  }
  const unsigned long long act = __ballot(1), bal = __ballot(take);
  if (!bal) return;
  const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((long long)act) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(s_dn, (uint32_t)__popcll(bal));
  base = __shfl(base, (int)leader, 64);
  if (take) {
    const uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (pos < sp.dcap) sp.dset[(size_t)blockIdx.x * sp.dcap + pos] = x;
    else atomicOr(&next[x >> 6], 1ull << (x & 63));
  }
}

__device__ __forceinline__ void ppa_resolve(const DevState& s, const PPSparse& sp, uint32_t t, uint32_t c3,
                                            const uint32_t* q, uint32_t cnt, uint64_t base,
                                            unsigned long long* __restrict__ next, uint64_t& sent, uint64_t& msgs,
                                            uint32_t* s_dn) {
  const uint32_t lane = threadIdx.x & 63;
  if (lane >= cnt) return;
  const uint32_t e = q[lane], loc = e & 0xFFFu, d = e >> 16;
  const uint64_t u = base + loc;  // informed (so live)
  const bool cc = s.check_crashed;
  {  // u's own call: a push
    bool take = false;
    uint32_t w = 0;
    if (d > 0) {
      const u32x4 r = philox((uint32_t)(s.gbase + u), t, 0, c3, s.key.k0, s.key.k1);
      if ((int32_t)uniform(r.y, 100u) >= s.kd) {
        const uint32_t j = uniform(r.x, d);
        w = s.ids[u * s.stride + j];
        ++sent;
        const bool dead = sp.fmask ? ((sp.fmask[u] >> j) & 1) != 0
                                   : (cc && ((s.gcrash[w >> 6] >> (w & 63)) & 1));
        if (!dead) {
          ++msgs;
          take = true;
        }
      }
    }
#if defined(GS_PP_NOATOMIC)  // timing probe only: the round's sets are not made
    if (take && w == 0xFFFFFFFFu) next[0] = 1;
#elif defined(GS_PP_CHECKFIRST)  // an informed target's bit is set already (next starts as recv)
    if (take && !((s.grecv[w >> 6] >> (w & 63)) & 1)) atomicOr(&next[w >> 6], 1ull << (w & 63));
#else
    pp_set(sp, next, take, w, s_dn);
#endif
  }
  unsigned long long qb, qe;
  in_edges(sp, u, qb, qe);
  for (unsigned long long q0 = qb; q0 < qe; q0 += kPPEdges) {
    uint32_t src[kPPEdges], x[kPPEdges];
#pragma unroll
    for (uint32_t k = 0; k < kPPEdges; ++k) {
      const bool in = q0 + k < qe;
      src[k] = in ? sp.rsrc[q0 + k] : 0u;
      x[k] = in ? sp.rslot[q0 + k] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPPEdges; ++k) {
      bool take = false;
      if (q0 + k < qe) {
        const u32x4 r = philox(src[k], t, 0, c3, s.key.k0, s.key.k1);
        if (uniform(r.x, (x[k] >> 4) + 1) == (x[k] & 15u) && (int32_t)uniform(r.y, 100u) >= s.kd) {
          const unsigned long long vb = 1ull << (src[k] & 63);
          const bool iv = (s.grecv[src[k] >> 6] & vb) != 0;
          // v failed: its in-edge's bit (sp.rfail: a line the in-edge scan
          // reads anyway) instead of a gather of v's failed word
          const uint64_t q = q0 + k;
          const bool fv = cc && (sp.rfail ? ((sp.rfail[q >> 5] >> (q & 31)) & 1u) != 0
                                          : (s.gcrash[src[k] >> 6] & vb) != 0);
          if (!iv && !fv) {  // v's pull from this informed node succeeds
            ++sent;
            ++msgs;
            take = true;
          }
        }
      }
#if defined(GS_PP_NOATOMIC)
      if (take && src[k] == 0xFFFFFFFFu) next[0] = 1;
#else
      pp_set(sp, next, take, src[k], s_dn);
#endif
    }
  }
}

__global__ __launch_bounds__(kPPSBlock) void k_ppa_round(const DevState s, unsigned long long* __restrict__ next,
                                                             const PPSparse sp, uint32_t t) {
  __shared__ uint64_t sh[3 * kPPWaves];
  __shared__ uint32_t s_q[kPPWaves][kPPQ];
  __shared__ uint32_t s_dn;  // this workgroup's deferred sets
  __shared__ uint32_t s_pre[kPPWaves][64];
  __shared__ unsigned long long s_msk[kPPWaves][64];
  PPCtl* c = sp.ctl;
  if (c->mode != PP_ANSWER) return;
  static_assert(kPPSGrid <= kPPDLists, "one deferred list per workgroup");
  if (threadIdx.x == 0) s_dn = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* q = s_q[wv];
  const uint32_t c3 = ctr3(K_PUSHPULL, s.key.trial);
  uint64_t sent = 0, msgs = 0;
  const uint64_t W = (s.n + 63) >> 6;
  const uint64_t nrange = (W + kPPRange - 1) / kPPRange;
  for (uint64_t rg = (uint64_t)blockIdx.x * kPPWaves + wv; rg < nrange; rg += (uint64_t)gridDim.x * kPPWaves) {
    const uint64_t w0 = rg * kPPRange, base = w0 << 6;
    uint32_t qn = 0;  // wave-uniform
    // a lane per WORD of the range where no word holds more than
    // sp.word_maxi informed nodes: the range's informed nodes are resolved 64
    // at a time in node order (for_each_bit), so a sparse range costs its
    // informed nodes / 64 batches instead of 64 word steps
    bool by_word = false;
    const uint64_t word = w0 + lane;
    unsigned long long mi = 0;
    if (sp.words) {
      mi = word < W ? s.recv[word] : 0ull;  // informed => live and in range
      uint32_t mx = (uint32_t)__popcll(mi);
#pragma unroll
      for (uint32_t o = 32; o >= 1; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
      by_word = sp.words == 1 || mx <= sp.word_maxi;
    }
    if (by_word)
      for_each_bit(mi, s_pre[wv], s_msk[wv], [&](uint32_t cnt, uint32_t off) {
        q[lane] = lane < cnt ? off | (uint32_t)s.deg[base + off] << 16 : 0u;
        wave_lds_sync();
        ppa_resolve(s, sp, t, c3, q, cnt, base, next, sent, msgs, &s_dn);
        wave_lds_sync();
      });
    for (uint32_t wi = 0; wi < kPPRange && !by_word; wi += kPPB) {
      unsigned long long Iw[kPPB];
      uint32_t d[kPPB];
#pragma unroll
      for (uint32_t i = 0; i < kPPB; ++i) {
        const uint64_t word = w0 + wi + i, v = (word << 6) + lane;
        Iw[i] = word < W ? s.recv[word] : 0ull;
        d[i] = ((Iw[i] >> lane) & 1) ? s.deg[v] : 0u;
      }
#pragma unroll
      for (uint32_t i = 0; i < kPPB; ++i) {
        const uint64_t v = ((w0 + wi + i) << 6) + lane;
        const bool enq = (Iw[i] >> lane) & 1;  // informed => live and in range
        const unsigned long long bal = __ballot(enq);
        if (enq) {
          const uint32_t at = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
          q[at] = (uint32_t)(v - base) | d[i] << 16;
        }
        qn += (uint32_t)__popcll(bal);
        if (qn >= 64) {
          wave_lds_sync();
          ppa_resolve(s, sp, t, c3, q, 64, base, next, sent, msgs, &s_dn);
          const uint32_t rest = qn - 64;
          const uint32_t keep = lane < rest ? q[64 + lane] : 0u;
          wave_lds_sync();
          if (lane < rest) q[lane] = keep;
          qn = rest;
        }
      }
    }
    wave_lds_sync();
    if (qn) ppa_resolve(s, sp, t, c3, q, qn, base, next, sent, msgs, &s_dn);
    wave_lds_sync();
  }
  if (sp.dset) {
    __syncthreads();
    if (threadIdx.x == 0) sp.dcnt[blockIdx.x] = s_dn < sp.dcap ? s_dn : sp.dcap;
  }
  const uint64_t v3[3] = {blockIdx.x == 0 && threadIdx.x == 0 ? c->ncallers : 0ull, sent, msgs};
  const uint32_t f3[3] = {ST_FIRED, ST_SENT, ST_MSGS};
  block_add<kPPSBlock>(sh, v3, 3, s.stats + (size_t)(t % kStatSlots) * kStatFields, f3);
}

// Shards: the round's mode, chosen by the host from the global informed count
// (the same on every shard: the replicated set), and the round counters.
__global__ void k_pp_set_mode(PPCtl* c, uint32_t mode) {
  c->mode = mode;
  c->nbottom += mode == PP_BOTTOM;
  c->nanswer += mode == PP_ANSWER;
}
}  // namespace

void pp_launch_topdown(const DevState& s, unsigned long long* next, const unsigned long long* sumA,
                       const unsigned long long* sumB, const unsigned long long* sum2, uint64_t S2, uint32_t t,
                       bool l2_only_flag, const PPSparse& sp, hipStream_t st) {
  // 0: no LDS stage, every call checks L2 (N > ~1.02e9; GS_FLAG_PP_L2_ONLY
  // forces it so the parity tests cover that path at small N)
  const bool l2_only = S2 > kPPMaxS2 || l2_only_flag;
  const uint32_t S2l = l2_only ? 0u : (uint32_t)S2;
  const uint64_t groups = (s.W + kPPU - 1) / kPPU;  // one wave per kPPU words
  const uint32_t blocks = grid_for(groups, kPPRoundBlock / 64, 512);
  hipLaunchKernelGGL(k_pp_round, dim3(blocks), dim3(kPPRoundBlock), (size_t)2 * S2l * 8, st, s, next, sumA,
                     sumB, sum2, S2l, t, (const PPCtl*)sp.ctl, sp.fmask);
}

void pp_launch_answer(const DevState& s, unsigned long long* next, const PPSparse& sp, uint32_t t, hipStream_t st) {
  if (sp.ctl) {  // no-op unless the round is bottom-up
    const uint64_t nrange = (s.W + kPPRange - 1) / kPPRange;
    const uint32_t bblocks = grid_for(nrange, kPPWaves, kPPSGrid);
    hipLaunchKernelGGL(k_ppb_round, dim3(bblocks), dim3(kPPSBlock), 0, st, s, next, sp, t);
    if (sp.dset) {
      const uint32_t nfine = (uint32_t)((s.n + 16383) >> 14);
      (void)hipMemsetAsync(sp.dcnt, 0, ((size_t)kPPDLists + kPPDRegions + nfine) * 8, st);
    }
    hipLaunchKernelGGL(k_ppa_round, dim3(bblocks), dim3(kPPSBlock), 0, st, s, next, sp, t);
    pp_launch_deferred(s, next, sp, bblocks, st);
  }
}

hipError_t pp_round_shard(const DevState& s, unsigned long long* next, unsigned long long* gnext, uint32_t t,
                          const PPSparse& sp, uint32_t mode, hipStream_t st) {
  if (!pp_state_ok(s) || !next || !sp.ctl || !sp.rend || !sp.rsrc || !sp.rslot || (s.check_crashed && !sp.fmask) ||
      (mode == PP_ANSWER && !gnext) || (mode != PP_ANSWER && mode != PP_BOTTOM))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pp_set_mode, dim3(1), dim3(1), 0, st, sp.ctl, mode);
  const uint64_t nrange = (s.W + kPPRange - 1) / kPPRange;
  const uint32_t bblocks = grid_for(nrange, kPPWaves, kPPSGrid);
  if (mode == PP_BOTTOM)
    hipLaunchKernelGGL(k_ppb_round, dim3(bblocks ? bblocks : 1), dim3(kPPSBlock), 0, st, s, next, sp, t);
  else
    hipLaunchKernelGGL(k_ppa_round, dim3(bblocks ? bblocks : 1), dim3(kPPSBlock), 0, st, s, gnext, sp, t);
  return hipGetLastError();
}

}  // namespace gs
