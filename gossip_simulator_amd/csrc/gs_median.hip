// gs_median.hip -- median-counter push-pull (GS_MODEL_MEDIAN).
//
// The median-counter algorithm of Karp, Schindelhauer, Shenker and Voecking
// ("Randomized rumor spreading", FOCS 2000), with no reference counterpart
// (simulator.go only floods); the model is the one DESIGN.md section 4.8
// states.  One tick = one synchronous round.  Every live node with a friend
// that is not done draws r = Philox{v, t, 0, MEDIAN}, calls
// u = friends[v][U_deg(r.x)], and the call is lost iff U_100(r.y) < kd.  A kept
// call to a live u is a connection: the rumor moves both ways on it, and each
// end is a partner of the other.  An informed node carries a counter (B-m); it
// advances when more of its partners are at least as far along as it is than
// behind it, after k steps it enters the final phase (C-1 .. C-k), and then
// it is done (D).  A partner in C pulls an A or B node straight into C-1.
//
// Layout: a dense engine shaped like the pull modes of gs_rumor.hip.  The
// round streams the table in node order, a wave per 64-node word and a lane
// per node, and reads st, the states at the start of the round, only.  A
// connection has two ends.  v's own end goes to own[v], a byte that no other
// lane touches.  u's end commutes: one atomicAdd into tally[u] when u is in B
// (ge and lt in separate words of a u64), or one atomicOr into the gotb / gotc
// bitsets, issued only when a plain read finds the bit clear.  Nothing depends
// on lane or atomic order.  k_median_commit then streams the same arrays in
// node order, applies the transition table, clears the round buffers and
// rebuilds the recv word; k_median_publish writes the stats row and the stop
// word, so rounds queue without a host sync.
#include "gs_median.h"
#include "gs_wave.h"

namespace gs {
namespace {

constexpr uint32_t kMdBlock = 256;

// Per-block sums of nf <= 3 counters into acc[0..nf), one atomic each.
__device__ __forceinline__ void block_add(uint64_t* sh, const uint64_t (&v)[3], uint32_t nf,
                                          unsigned long long* acc) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < 3 * (kMdBlock / 64)) sh[tid] = 0;
  __syncthreads();
  for (uint32_t i = 0; i < nf; ++i) {
    const uint64_t s = wave_sum64(v[i]);
    if (lane == 0) sh[i * (kMdBlock / 64) + wv] = s;
  }
  __syncthreads();
  if (tid < nf) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < kMdBlock / 64; ++k) s += sh[tid * (kMdBlock / 64) + k];
    if (s) atomicAdd(&acc[tid], (unsigned long long)s);
  }
}

__device__ __forceinline__ bool active(uint32_t s) { return s != 0 && s != kMedianDone; }

// A live sender becomes B-1; a failed one starts nothing.
__global__ void k_median_seed(const DevState s, const MedianState m, uint32_t node, unsigned long long cover) {
  if (blockIdx.x || threadIdx.x) return;
  RumorCtl* c = m.ctl;
  unsigned long long rec = 0;
  const unsigned long long bit = 1ull << (node & 63);
  if (!(s.check_crashed && (s.crash[node >> 6] & bit))) {
    s.recv[node >> 6] |= bit;
    m.st[node] = 1;
    rec = 1;
  }
  c->cover = cover;
  c->received = rec;
  c->rlen = c->peak = rec;
  c->stop = rec ? 0u : (rec >= cover ? kRumorCovered : kRumorQuiescent);
}

__global__ __launch_bounds__(kMdBlock) void k_median_round(const DevState s, const MedianState m, uint32_t t) {
  __shared__ uint64_t sh[3 * (kMdBlock / 64)];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c3 = ctr3(K_MEDIAN, s.key.trial);
  const bool cc = s.check_crashed;
  const uint32_t k = m.k;
  uint64_t fired = 0, sent = 0, msgs = 0;
  const uint64_t waves = (uint64_t)gridDim.x * (kMdBlock / 64);
  // w is wave-uniform: whole waves stay in the loop together
  for (uint64_t w = ((uint64_t)blockIdx.x * kMdBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const unsigned long long Cw = cc ? s.crash[w] : 0ull;
    const uint64_t v = w * 64 + lane;
    if (v >= s.n || ((Cw >> lane) & 1)) continue;
    const uint32_t sv = m.st[v];
    const uint32_t d = s.deg[v];
    if (d == 0 || sv == kMedianDone) continue;  // a live node with a friend calls until it is done
    const u32x4 rr = philox((uint32_t)v, t, 0, c3, s.key.k0, s.key.k1);
    const uint32_t j = uniform(rr.x, d);
    ++fired;
    if ((int32_t)uniform(rr.y, 100u) < s.kd) continue;  // the call is lost
    ++sent;
    const uint32_t u = s.ids[v * s.stride + j];
    const unsigned long long ubit = 1ull << (u & 63);
    if (cc && (s.crash[u >> 6] & ubit)) continue;  // a failed callee: no connection
    const uint32_t su = m.st[u];  // (u == v: v is its own partner, once for each end)
    const bool av = active(sv), au = active(su);
    msgs += (uint64_t)av + (uint64_t)au;  // the caller pushes, the callee answers
    // v's end: its partner u
    uint32_t o = kOwnNone;
    if (au) {
      if (su > k) o = kOwnC;
      else if (sv == 0) o = kOwnGe;  // an A caller: a B partner
      else if (sv <= k) o = su >= sv ? kOwnGe : kOwnLt;
    } else if (su == 0 && av && sv <= k) {
      o = kOwnLt;
    }
    if (o) m.own[v] = (uint8_t)o;
    // u's end: its partner v.  Only an A or B callee keeps count.
    if (su > k) continue;
    if (sv > k) {  // a C caller (sv is not D here)
      unsigned long long* f = m.gotc + (u >> 6);
      if (!(*f & ubit)) atomicOr(f, ubit);  // thousands of callers may share one word
    } else if (su == 0) {
      if (sv) {  // a B caller informs an A callee
        unsigned long long* f = m.gotb + (u >> 6);
        if (!(*f & ubit)) atomicOr(f, ubit);
      }
    } else {  // u in B-su, v in A or B-sv
      atomicAdd(m.tally + u, sv >= su ? kTallyGe : kTallyLt);
    }
  }
  const uint64_t v3[3] = {fired, sent, msgs};
  block_add(sh, v3, 3, m.ctl->acc);
}

// The transition table per node, a wave per word: st written where it changed,
// own / tally / gotb / gotc cleared where set, the recv word rebuilt by one
// ballot; acc[RA_NEW] += the new bits and ctl->wlen += the active nodes.
__global__ __launch_bounds__(kMdBlock) void k_median_commit(const DevState s, const MedianState m) {
  __shared__ uint64_t sh[3 * (kMdBlock / 64)];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t k = m.k;
  uint64_t nb = 0, na = 0;
  const uint64_t waves = (uint64_t)gridDim.x * (kMdBlock / 64);
  for (uint64_t w = ((uint64_t)blockIdx.x * kMdBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const uint64_t v = w * 64 + lane;
    const bool in = v < s.n;
    const unsigned long long gb = m.gotb[w], gc = m.gotc[w];
    uint32_t s0 = 0, s1 = 0;
    if (in) {
      s0 = s1 = m.st[v];
      const uint32_t o = m.own[v];
      const bool c = ((gc >> lane) & 1) || o == kOwnC;
      if (s0 == 0) {
        if (c) s1 = k + 1;
        else if (((gb >> lane) & 1) || o == kOwnGe) s1 = 1;
      } else if (s0 <= k) {
        const unsigned long long T = m.tally[v];
        if (T) m.tally[v] = 0;
        const uint32_t ge = (uint32_t)T + (o == kOwnGe), lt = (uint32_t)(T >> 32) + (o == kOwnLt);
        if (c) s1 = k + 1;
        else if (ge > lt) s1 = s0 < k ? s0 + 1 : k + 1;
      } else if (s0 != kMedianDone) {
        s1 = s0 == 2 * k ? kMedianDone : s0 + 1;
      }
      if (s1 != s0) m.st[v] = (uint8_t)s1;
      if (o) m.own[v] = 0;
    }
    const unsigned long long fresh = __ballot(s0 == 0 && s1 != 0), inf = __ballot(s1 != 0);
    const unsigned long long act = __ballot(active(s1));
    if (lane == 0) {  // the wave's own words: no atomic
      if (fresh) s.recv[w] = inf;
      if (gb) m.gotb[w] = 0;
      if (gc) m.gotc[w] = 0;
      nb += (uint64_t)__popcll(fresh);
      na += (uint64_t)__popcll(act);
    }
  }
  const uint64_t v3[3] = {nb, 0, 0};
  block_add(sh, v3, 1, m.ctl->acc + RA_NEW);
  __syncthreads();  // sh is reused
  const uint64_t a3[3] = {na, 0, 0};
  block_add(sh, a3, 1, &m.ctl->wlen);
}

// The round's stats row and the stop rule (k_rumor_publish's, on the same block).
__global__ void k_median_publish(const DevState s, const MedianState m, uint32_t t) {
  if (blockIdx.x || threadIdx.x) return;
  RumorCtl* c = m.ctl;
  unsigned long long* row = s.stats + (size_t)(t % kStatSlots) * kStatFields;
  const unsigned long long act = c->wlen;
  row[ST_FIRED] = c->acc[RA_FIRED];
  row[ST_SENT] = c->acc[RA_SENT];
  row[ST_MSGS] = c->acc[RA_MSGS];
  row[ST_RECV] = c->acc[RA_NEW];
  row[ST_CRASH] = 0;
  row[ST_SCHED] = act;  // pending: the active nodes after the round
  row[ST_ERR] = row[ST_RSVD] = 0;
  c->received += c->acc[RA_NEW];
  if (act > c->peak) c->peak = act;
  c->rlen = act;
  c->wlen = 0;
  c->acc[RA_FIRED] = c->acc[RA_SENT] = c->acc[RA_MSGS] = c->acc[RA_NEW] = 0;
  c->stop = act ? 0u : (c->received >= c->cover ? kRumorCovered : kRumorQuiescent);
}

__global__ __launch_bounds__(kMdBlock) void k_median_done(const DevState s, const MedianState m,
                                                          unsigned long long* out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kMdBlock / 64);
  for (uint64_t w = ((uint64_t)blockIdx.x * kMdBlock + threadIdx.x) >> 6; w < s.W; w += waves) {
    const uint64_t v = w * 64 + lane;
    const unsigned long long done = __ballot(v < s.n && m.st[v] == kMedianDone);
    if (lane == 0) out[w] = done;
  }
}

}  // namespace

uint32_t median_grid(uint64_t n, uint32_t want) {
  const uint64_t cap = std::max<uint64_t>(1, (n + kMdBlock - 1) / kMdBlock);
  return (uint32_t)std::min<uint64_t>(cap, want ? want : 2048u);  // 256 CUs x 8 blocks
}

hipError_t median_seed(const DevState& s, const MedianState& m, uint32_t node, unsigned long long cover,
                       hipStream_t st) {
  hipLaunchKernelGGL(k_median_seed, dim3(1), dim3(64), 0, st, s, m, node, cover);
  return hipGetLastError();
}

hipError_t median_round(const DevState& s, const MedianState& m, uint32_t t, uint32_t grid, hipStream_t st) {
  hipLaunchKernelGGL(k_median_round, dim3(grid), dim3(kMdBlock), 0, st, s, m, t);
  return hipGetLastError();
}

hipError_t median_commit(const DevState& s, const MedianState& m, uint32_t t, hipStream_t st) {
  hipLaunchKernelGGL(k_median_commit, dim3(median_grid(s.n, 0)), dim3(kMdBlock), 0, st, s, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_median_publish, dim3(1), dim3(64), 0, st, s, m, t);
  return hipGetLastError();
}

hipError_t median_done_set(const DevState& s, const MedianState& m, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(k_median_done, dim3(median_grid(s.n, 0)), dim3(kMdBlock), 0, st, s, m, out);
  return hipGetLastError();
}

}  // namespace gs
