// gs_ctx.cpp -- the lifetime of a context: parameter checks, set-up of every
// kind (plain, batched, shard, rank, replica, group) and destroy_one; each
// block of resources is released directly below the function that allocates it.
#include "gs_ctx.h"

namespace gs {

namespace {

uint32_t ring_slots(const gs_params& p) { return p.delay_high > 2 ? (uint32_t)p.delay_high : 2u; }

uint32_t ceil_log2(uint64_t x) {
  uint32_t b = 0;
  while ((1ull << b) < x) ++b;
  return b;
}

int check_params(const gs_params* p, bool rumor_trials, bool median_trials, std::string& why) {
  if (!p) { why = "params is NULL"; return GS_EINVAL; }
  if (p->n == 0) { why = "n must be >= 1 (simulator.go:240 panics on rand.Intn(0))"; return GS_EINVAL; }
  if (p->n > 0x7FFFFFFFull) { why = "n must be < 2^31"; return GS_EINVAL; }
  if (p->delay_high <= p->delay_low) {
    why = "delayhigh must exceed delaylow (simulator.go:167 panics on rand.Intn(<=0))";
    return GS_EINVAL;
  }
  if (p->fanout < 0 || p->fanin < 0 || p->fanout > 255 || p->fanin > 255) {
    why = "fanout/fanin must be in [0, 255]";
    return GS_EINVAL;
  }
  if (ring_slots(*p) > 4096) { why = "delayhigh must be <= 4096"; return GS_EINVAL; }
  if (p->model > GS_MODEL_MEDIAN) {
    why = "model must be GS_MODEL_FLOOD, GS_MODEL_PUSHPULL, GS_MODEL_RUMOR or GS_MODEL_MEDIAN";
    return GS_EINVAL;
  }
  if (p->model == GS_MODEL_MEDIAN && (p->rumor_k < 1 || p->rumor_k > 127)) {
    why = "GS_MODEL_MEDIAN needs 1 <= rumor_k <= 127, not " + std::to_string(p->rumor_k);
    return GS_EINVAL;
  }
  if (p->model == GS_MODEL_MEDIAN && p->trials > 1 && !median_trials) {
    why = "GS_MODEL_MEDIAN with trials > 1: the median-counter model runs one trial per context";
    return GS_EINVAL;
  }
  if (p->model == GS_MODEL_RUMOR && (p->rumor_k < 1 || p->rumor_k > 255)) {
    why = "GS_MODEL_RUMOR needs 1 <= rumor_k <= 255, not " + std::to_string(p->rumor_k);
    return GS_EINVAL;
  }
  if (p->model == GS_MODEL_RUMOR && (p->rumor_mode & ~(GS_RUMOR_BLIND | GS_RUMOR_COIN | GS_RUMOR_PULL))) {
    why = "GS_MODEL_RUMOR: rumor_mode " + std::to_string(p->rumor_mode) +
          " has a bit that is none of GS_RUMOR_BLIND, GS_RUMOR_COIN, GS_RUMOR_PULL";
    return GS_EINVAL;
  }
  if (p->model == GS_MODEL_RUMOR && p->trials > 1 && !rumor_trials) {
    why = "GS_MODEL_RUMOR with trials > 1: the rumor model runs one trial per context (gs_create_trials makes a batch)";
    return GS_EINVAL;
  }
  // batched trials (either model) live at trial << tlog | node in one 31-bit id space
  if (p->trials > 1 && ((uint64_t)p->trials << std::max<uint32_t>(kFineLog, ceil_log2(p->n))) > 0x7FFFFFFFull) {
    why = "trials x 2^ceil(log2 n) must be < 2^31 (batch fewer trials per context)";
    return GS_EINVAL;
  }
  return GS_OK;
}

// Batched trials: the per-trial counter rows (tb bytes, and their pinned
// copy) and, for push-pull trials, the stall check's cb bytes.
bool alloc_trial_rows(gs_ctx* c, size_t tb, size_t cb) {
  return dev_malloc((void**)&c->bt.d_tstat, tb) == hipSuccess &&
         hipHostMalloc((void**)&c->bt.h_tstat, tb) == hipSuccess && grow(c->bt.chk, cb);
}

void release_trials(gs_ctx* c) {
  if (c->bt.d_tstat) (void)dev_free(c->bt.d_tstat);
  if (c->bt.h_tstat) (void)hipHostFree(c->bt.h_tstat);
  release(c->bt.chk);
}

// Window-engine buffers.  Sizes at n = 1e9, R = 20: flist 40 GB (two bytes
// per node per ring slot), fcount 4.9 MB; message buffers grow on demand.
int alloc_window(gs_ctx* c) {
  const DevState& s = c->st;
  WinState& w = c->ws;
  w.n = s.n;
  w.W = s.W;
  w.nfine = (uint32_t)((s.n + kFineNodes - 1) >> kFineLog);
  w.ncoarse = (w.nfine + 255) / 256;
  w.R = s.R;
  w.delay_low = s.delay_low;
  w.delay_span = s.delay_span;
  w.kd = s.kd;
  w.kc = s.kc;
  w.key = s.key;
  w.base = (uint32_t)c->lo;
  w.tlog = c->tlog;
  w.tmask = c->tlog >= 32 ? ~0u : (1u << c->tlog) - 1;
  // a batched context's fine buckets are whole-trial runs of 2^(tlog-14) with
  // the last ones of each trial partly or wholly past its n nodes
  w.tnodes = c->trials > 1 && c->tlog <= kCoarseShift && !c->shard ? (uint32_t)c->p.n : 0u;
  w.G = c->G;
  w.rank = c->rank;
  w.seg_per = (uint32_t)c->seg_per;
  w.csub = kCoarseSub;
  w.noxcd = getenv("GS_PART2_NOXCD") ? 1u : 0u;  // A/B knob: k_part2 tiles in region order
  {
    const char* xp = getenv("GS_XPAIR");  // A/B knob: 0 = k_expand's packed rows fetched per lane
    w.nopair = xp && atoi(xp) == 0 ? 1u : 0u;
  }
  w.ccap_end = nullptr;
  w.csrc = nullptr;
  if (c->shard) {  // owner expand (k_expand's coarse_bin)
    w.owner = 1;
    w.obins = 256 / c->G;
    w.oseg_q = (uint32_t)(c->seg_per >> kFineLog);
    w.oseg_magic = 0xFFFFFFFFu / w.oseg_q;
    if (dev_malloc(&c->wn.d_rtab, kRtabWords * 8) != hipSuccess ||
        hipHostMalloc((void**)&c->wn.h_rtab, kRtabWords * 8) != hipSuccess)
      return fail(c, GS_ENOMEM, "cannot allocate the shard's receive layout");
  }
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t units = (size_t)kMaxWindow * w.nfine + 1;
  const size_t b_fc = al((size_t)w.R * w.nfine * 4), b_units = al(units * 8),
               b_small = al(kRegions * 8) * 2 + al((kRegions + 1) * 8) + al((kRegions + 1) * 4) + al(kMaxWindow * 8),
               b_fhist = al(((size_t)w.ncoarse * 256 + 1) * 8), b_fbase = al(((size_t)w.nfine + 1) * 8),
               b_ffill = al((size_t)w.nfine * 8),
               b_sst = al((size_t)kStatShards * kMaxWindow * kStatFields * 8),
               b_rlcnt = al((size_t)w.nfine * 4) + al(((size_t)w.nfine + 2) * 4),
               b_tsum = al((size_t)w.ncoarse * kMaxWindow * 8) + al(((size_t)w.ncoarse + 1) * 8);
  const size_t total = b_fc + 2 * b_units + b_small + b_fhist + b_fbase + b_ffill + b_sst + b_rlcnt + b_tsum;
  if (dev_malloc(&c->wn.d_win, total) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate window-engine buffers");
  const size_t flist = (size_t)w.R * w.nfine * kFineNodes * 2;
  if (dev_malloc(&c->wn.d_flist, flist) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate " + std::to_string(flist >> 20) + " MiB of fire lists");
  char* q = (char*)c->wn.d_win;
  w.fcount = (uint32_t*)q; q += b_fc;
  w.usize = (unsigned long long*)q; q += b_units;
  w.unit_off = (unsigned long long*)q; q += b_units;
  w.chist = (unsigned long long*)q; q += al(kRegions * 8);
  w.cfill = (unsigned long long*)q; q += al(kRegions * 8);
  w.ccap = (unsigned long long*)q; q += al((kRegions + 1) * 8);
  w.tprefix = (uint32_t*)q; q += al((kRegions + 1) * 4);
  w.tfires = (unsigned long long*)q;
  q = (char*)c->wn.d_win + b_fc + 2 * b_units + b_small;
  w.fhist = (unsigned long long*)q; q += b_fhist;
  w.fstart = (unsigned long long*)q; q += b_fbase;
  w.ffill = (unsigned long long*)q; q += b_ffill;
  w.sstats = (unsigned long long*)q; q += b_sst;
  w.rlcnt = (uint32_t*)q; q += al((size_t)w.nfine * 4);
  w.lgl = (uint32_t*)q; q += al(((size_t)w.nfine + 2) * 4);
  w.tsum = (unsigned long long*)q; q += al((size_t)w.ncoarse * kMaxWindow * 8);
  w.toff = (unsigned long long*)q; q += al(((size_t)w.ncoarse + 1) * 8);
  if (dev_malloc(&c->wn.d_rlmsg, (size_t)w.nfine * kRolledCap * 4) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the rolled-receipt lists");
  w.rlmsg = (uint32_t*)c->wn.d_rlmsg;
  w.dbg = nullptr;
  if (getenv("GS_STAMPS") && dev_malloc(&w.dbg, kDbgWords * 8) == hipSuccess)
    (void)hipMemset(w.dbg, 0, kDbgWords * 8);
  w.flist = (uint16_t*)c->wn.d_flist;
  c->wn.fcount_bytes = (size_t)w.R * w.nfine * 4;
  if (hipMemsetAsync(c->wn.d_win, 0, total, c->stream) != hipSuccess)
    return fail(c, GS_EDEVICE, "memset of window buffers failed");
  c->wn.misc_words = std::max<size_t>(4096, (size_t)c->G * kMaxWindow + 64);
  if (hipHostMalloc((void**)&c->wn.h_cap, (kRegions + 1) * 8) != hipSuccess ||
      hipHostMalloc((void**)&c->wn.h_misc, c->wn.misc_words * 8) != hipSuccess ||
      hipHostMalloc((void**)&c->wn.h_err, 64) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate pinned window buffers");
  if (c->trials > 1) {
    if (!alloc_trial_rows(c, (size_t)c->trials * kMaxWindow * kTStatFields * 4, 0))
      return fail(c, GS_ENOMEM, "cannot allocate per-trial counters");
    w.tstat = c->bt.d_tstat;
  }
  return GS_OK;
}

// (the message buffers gmap / cmsg / fmsg / tmp grow in the window loops)
void release_window(gs_ctx* c) {
  WinEngine& e = c->wn;
  for (void* p : {e.d_win, e.d_flist, e.d_rlmsg, (void*)e.d_rtab, (void*)c->ws.dbg})
    if (p) (void)dev_free(p);
  for (Buf* b : {&e.gmap, &e.cmsg, &e.fmsg, &e.tmp}) release(*b);
  for (void* p : {(void*)e.h_cap, (void*)e.h_misc, (void*)e.h_err, (void*)e.h_rtab})
    if (p) (void)hipHostFree(p);
}

int ctx_setup(gs_ctx* c, const gs_params* params, int device, bool shard, uint32_t G, uint32_t rank,
              std::string& why) {
  c->p = *params;
  c->p.device = device;
  c->dev = device;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    why = "no HIP device visible (libgossip_hip needs an MI355X)";
    return GS_EDEVICE;
  }
  if (c->dev < 0 || c->dev >= ndev) {
    why = "device " + std::to_string(c->dev) + " out of range (" + std::to_string(ndev) + " visible)";
    return GS_EDEVICE;
  }
  hipDeviceProp_t prop;
  if (hipSetDevice(c->dev) != hipSuccess || hipGetDeviceProperties(&prop, c->dev) != hipSuccess ||
      strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    why = "device " + std::to_string(c->dev) + " is not gfx950";
    return GS_EDEVICE;
  }
  if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    why = "cannot create a stream";
    return GS_EDEVICE;
  }
  c->stream = c->own;
  DevState& s = c->st;
  const uint32_t stride0 = (uint32_t)std::max(c->p.fanout, c->p.fanin);
  c->pp = c->p.model == GS_MODEL_PUSHPULL && !c->rset;  // (a rumor set has its own engine and buffers)
  c->rumor = c->p.model == GS_MODEL_RUMOR;
  c->median = c->p.model == GS_MODEL_MEDIAN;
  c->pp_l2_only = (c->p.flags & GS_FLAG_PP_L2_ONLY) != 0;
  c->trials = std::max<uint32_t>(1, c->p.trials);
  c->ntot = c->p.n;
  if (c->trials > 1) {
    c->tlog = std::max<uint32_t>(kFineLog, ceil_log2(c->p.n));
    c->ntot = (uint64_t)c->trials << c->tlog;  // < 2^31 (check_params)
  }
  c->shard = shard;
  c->G = G;
  c->rank = rank;
  if (shard && c->rumor) {
    why = "GS_MODEL_RUMOR runs on one device: no node-range shards";
    return GS_EINVAL;
  }
  if (shard && c->median) {
    why = "GS_MODEL_MEDIAN runs on one device: no node-range shards";
    return GS_EINVAL;
  }
  if (shard) {
    if (c->pp && !pp_rslot_packed(stride0)) {
      why = "push-pull node-range shards need rows of at most 16 slots (bottom-up rounds)";
      return GS_EINVAL;
    }
    c->seg_per = (((c->p.n + G - 1) / G) + kFineNodes - 1) & ~(uint64_t)(kFineNodes - 1);
    if ((uint64_t)(G - 1) * c->seg_per >= c->p.n) {
      why = "n = " + std::to_string(c->p.n) + " is too small for " + std::to_string(G) +
            " shards of whole 16384-node buckets";
      return GS_EINVAL;
    }
    c->pp_shard = c->pp;
    c->rs.segw = c->seg_per / 64;
    c->lo = rank * c->seg_per;
    c->hi = std::min<uint64_t>(c->lo + c->seg_per, c->p.n);
    c->ntot = c->hi - c->lo;
  }
  s.lo = 0;
  s.hi = (uint32_t)c->ntot;
  s.n = c->ntot;
  s.W = (s.n + 63) / 64;
  s.C = (uint32_t)((s.n + (1ull << kChunkNodesLog) - 1) >> kChunkNodesLog);
  s.CS = (s.C + kShards - 1) / kShards;
  s.chunk_lo = 0;
  s.chunk_hi = s.C;
  s.sharded = 0;
  s.R = ring_slots(c->p);
  s.delay_low = c->p.delay_low;
  s.delay_span = (uint32_t)(c->p.delay_high - c->p.delay_low);
  s.kd = gs_threshold(c->p.drop_rate);
  s.kc = gs_threshold(c->p.crash_rate);
  s.key = Key{(uint32_t)c->p.seed, (uint32_t)(c->p.seed >> 32), c->p.trial};
  // Engine: the window engine unless the ring is too long for LDS, rows are
  // wider than 32 or the tick engine is forced; push-pull has its own kernels.
  // (its coarse partition has 256 bins of 2^22 nodes: at most 2^30 nodes per context)
  c->win = !c->pp && !c->rumor && !c->median && !c->rset && s.R <= kWinMaxRing && !(c->p.flags & GS_FLAG_TICK_ENGINE) && stride0 <= kWinMaxStride &&
           s.n <= (1ull << (kCoarseShift + 8));
  if (((c->trials > 1 && !c->ppt && !c->rmt && !c->mdt) || (shard && !c->pp)) && !c->win) {
    why = "batched trials and node-range shards run on the window engine (delayhigh <= 256, "
          "fanout/fanin <= 32, no GS_FLAG_TICK_ENGINE, at most 2^30 nodes per context or shard)";
    return GS_EINVAL;
  }
  // owner expand: every shard's range fits its 256 / G coarse bins of 2^22 nodes
  // and a group's received blocks take source index G of the receive layout's
  // 8-bit source field (kSrcShift): G <= 255
  static_assert(kSrcShift + 8 == 64, "8-bit source index in the receive layout");
  if (shard && !c->pp && (G > 255 || ((c->seg_per + (1ull << kCoarseShift) - 1) >> kCoarseShift) > 256 / G)) {
    why = "flood node-range shards: each of the G <= 255 shards' ranges must fit 256 / G bins of 2^22 nodes "
          "(n up to about 2^30)";
    return GS_EINVAL;
  }
  // One state allocation, 256-B aligned sub-buffers; everything before
  // `stats` is per-broadcast state that gs_reset clears.
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const bool tick = !c->win && !c->pp && !c->rumor && !c->median && !c->rset;
  // (batched push-pull trials build `next` in LDS: no second bitset, no summaries;
  // the rumor model has the second bitset and no summaries, its batched trials neither)
  const size_t b_sum = c->pp && !c->ppt ? al(pp_summary_total_words(s.W) * 8) : 0;
  const size_t b_next = (c->pp && !c->ppt) || (c->rumor && !c->rmt) ? al(s.W * 8) + b_sum : 0;
  const size_t b_bits = al(s.W * 8), b_ring = tick ? al((size_t)s.R * s.W * 8) : 0,
               b_cflag = tick ? al((size_t)s.R * s.C * 4) : 0,
               b_clist = tick ? al((size_t)s.R * kShards * s.CS * 4) : 0,
               b_ccount = tick ? al((size_t)s.R * kShards * kCounterStride * 4) : 0,
               b_stats = al((size_t)kStatSlots * kStatFields * 8);
  const size_t b_roll = c->win ? b_bits : 0;
  const size_t total = 2 * b_bits + b_roll + b_next + b_ring + b_cflag + b_clist + b_ccount + b_stats + 256;
  c->state_bytes = total;
  if (dev_malloc(&c->d_state, total) != hipSuccess) {
    why = "cannot allocate " + std::to_string(total) + " bytes of device state";
    return GS_ENOMEM;
  }
  char* q = (char*)c->d_state;
  s.recv = (unsigned long long*)q; q += b_bits;
  s.crash = (unsigned long long*)q; q += b_bits;
  s.rollw = b_roll ? (uint32_t*)q : nullptr; q += b_roll;
  c->d_next = b_next ? (unsigned long long*)q : nullptr;
  c->d_ppsum = b_sum ? (unsigned long long*)(q + al(s.W * 8)) : nullptr;
  q += b_next;
  s.ring = (unsigned long long*)q; q += b_ring;
  s.cflag = (uint32_t*)q; q += b_cflag;
  s.clist = (uint32_t*)q; q += b_clist;
  s.ccount = (uint32_t*)q; q += b_ccount;
  s.stats = (unsigned long long*)q; q += b_stats;
  c->d_err = (uint32_t*)q;
  c->d_flag = c->d_err + 1;
  s.err = c->d_err;
  s.grecv = s.recv;  // a push-pull shard points these at the replicated sets (attach_pp_sets)
  s.gcrash = s.crash;
  s.gbase = 0;
  if (tick && s.kc > 0 && dev_malloc(&c->d_cnt, s.n * 4) != hipSuccess) {
    why = "cannot allocate arrival counters";
    return GS_ENOMEM;
  }
  s.cnt = c->d_cnt;
  if (c->win) {
    int rc = alloc_window(c);
    if (rc) { why = c->err; return rc; }
  }
  if (c->rumor) {
    int rc = rumor_alloc(c);
    if (rc) { why = c->err; return rc; }
  }
  if (c->median) {
    int rc = median_alloc(c);
    if (rc) { why = c->err; return rc; }
  }
  if (c->rset) {
    int rc = rs_alloc(c);
    if (rc) { why = c->err; return rc; }
  }
  if (c->ppt) {  // per-trial counter rows and the stall check's buffers
    const size_t tb = (size_t)c->trials * kMaxWindow * kTStatFields * 4;
    const size_t cb = (((size_t)c->trials + 3) & ~(size_t)3) + (size_t)c->trials * 4;
    if (!alloc_trial_rows(c, tb, cb)) {
      why = "cannot allocate the per-trial counters";
      return GS_ENOMEM;
    }
    PptState& pt = c->pt;
    pt.recv = s.recv;
    pt.tstat = c->bt.d_tstat;
    pt.n = (uint32_t)c->p.n;
    pt.trials = c->trials;
    pt.tlog = c->tlog;
    pt.kd = s.kd;
    pt.key = s.key;
  }
  if ((c->rmt || c->mdt) && !alloc_trial_rows(c, (size_t)c->trials * kMaxWindow * kTStatFields * 4, 0)) {
    why = "cannot allocate the per-trial counters";
    return GS_ENOMEM;
  }
  c->tacc.assign(c->trials, TrialAcc{});
  c->async_off = getenv("GS_SYNC_WINDOWS") != nullptr;
  c->winlog = getenv("GS_WINLOG") != nullptr;
  if (hipMemsetAsync(c->d_state, 0, total, c->stream) != hipSuccess ||
      (c->d_cnt && hipMemsetAsync(c->d_cnt, 0, s.n * 4, c->stream) != hipSuccess) ||
      hipHostMalloc((void**)&c->h_stats, (size_t)kStatSlots * kStatFields * 8) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    why = "device initialisation failed";
    return GS_EDEVICE;
  }
  return GS_OK;
}

// (d_failed is allocated by the first failure mask, set_failed)
void release_state(gs_ctx* c) {
  for (void* p : {c->d_state, (void*)c->d_cnt, (void*)c->d_failed})
    if (p) (void)dev_free(p);
  if (c->h_stats) (void)hipHostFree(c->h_stats);
}

int check_ppt_n(const gs_params* p, int device, std::string& why, PptPlan* pl) {
  *pl = PptPlan{};
  if (p->trials <= 1 || p->model != GS_MODEL_PUSHPULL) return GS_OK;
  int ndev = 0;
  uint64_t lim = 0;
  const bool asked = hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev &&
                     ppt_lds_limit(device, false, &lim) == hipSuccess;
  if (!asked) {
    (void)hipGetLastError();
    why = "batched push-pull trials need n within the device's LDS per workgroup (gs_pp_trials_max_n), and HIP "
          "device " + std::to_string(device) + " is not visible: n = " + std::to_string(p->n) + " is not accepted";
    return GS_EINVAL;
  }
  const PptPlan plan = ppt_plan(p->n, lim);
  if (!plan.fits) {
    why = "batched push-pull trials keep a trial's informed set in one workgroup's LDS: n must be <= " +
          std::to_string(ppt_max_n(lim)) + " on this device (gs_pp_trials_max_n), not " + std::to_string(p->n);
    return GS_EINVAL;
  }
  if (plan.lds_bytes > 65536 && ppt_prepare(device, false, (uint32_t)plan.lds_bytes) != hipSuccess) {
    why = "cannot raise the trial-resident kernel's dynamic LDS limit";
    return GS_EDEVICE;
  }
  *pl = plan;
  return GS_OK;
}

// Push-pull shard c uses the replicated informed / failed sets ig / fg
// (G * segw words each): its own nodes are words [rank * segw, ...).
void attach_pp_sets(gs_ctx* c, unsigned long long* ig, unsigned long long* fg, unsigned long long* gn) {
  c->rs.d_ig = ig;
  c->rs.d_fg = fg;
  c->rs.d_gn = gn;
  DevState& s = c->st;
  s.grecv = ig;
  s.gcrash = fg;
  s.gbase = c->lo;
  s.recv = ig + (size_t)c->rank * c->rs.segw;
  s.crash = fg + (size_t)c->rank * c->rs.segw;
}

// Allocates and zeroes up to three bitsets of `words` words (null outputs are
// skipped): the replicated informed / failed sets and the pull-answer set.
int alloc_pp_sets(gs_ctx* c, uint64_t words, unsigned long long** ig, unsigned long long** fg,
                  unsigned long long** gn) {
  for (unsigned long long** q : {ig, fg, gn}) {
    if (!q) continue;
    *q = nullptr;
    if (dev_malloc(q, words * 8) != hipSuccess)
      return fail(c, GS_ENOMEM, "cannot allocate the replicated informed / failed sets");
    CK(c, hipMemsetAsync(*q, 0, words * 8, c->stream));
  }
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

// A rank owns its sets (own_ig); a group's members borrow the group's
// (release_group frees those).
void release_sets(gs_ctx* c) {
  if (!c->rs.own_ig) return;
  for (unsigned long long* q : {c->rs.d_ig, c->rs.d_fg, c->rs.d_gn, c->rs.d_gst})
    if (q) (void)dev_free(q);
}

// The replica of push-pull shards on device `dev` (gs_ctx::rep): an unsharded
// push-pull context whose informed / failed sets are the replicated ig / fg.
// It gets the full table at load time (partition_pp).  GS_PP_NO_REPLICA=1:
// none (every round runs sharded bottom-up; A/B and memory-tight runs).
int make_replica(const gs_params* params, int dev, unsigned long long* ig, unsigned long long* fg, gs_ctx** out) {
  *out = nullptr;
  if (getenv("GS_PP_NO_REPLICA")) return GS_OK;
  gs_params rp = *params;
  rp.trials = 1;
  gs_ctx* r = nullptr;
  RC(create_one(&rp, dev, false, 1, 0, &r));
  r->st.recv = r->st.grecv = ig;
  r->st.crash = r->st.gcrash = fg;
  r->st.gbase = 0;
  *out = r;
  return GS_OK;
}

// GS_STAMPS: the phase counters the window kernels left in ws.dbg, on stderr.
void print_stamps(gs_ctx* c) {
  if (!c->ws.dbg) return;
  unsigned long long h[kDbgWords];
  if (hipMemcpy(h, c->ws.dbg, sizeof h, hipMemcpyDeviceToHost) == hipSuccess && h[kXStamp0]) {
    const double r = 1e-3 / h[kXStamp0];  // k_expand phases (GS_XSTAMPS builds)
    fprintf(stderr, "[stamps] k_expand: %llu rounds (wave 0), mean kcycles per round: lookup %.2f rows %.2f "
            "draws %.2f scan+scatter %.2f barrier %.2f writeout %.2f\n", h[kXStamp0], h[kXStamp0 + 1] * r,
            h[kXStamp0 + 2] * r, h[kXStamp0 + 3] * r, h[kXStamp0 + 4] * r, h[kXStamp0 + 5] * r, h[kXStamp0 + 6] * r);
  }
  if (hipMemcpy(h, c->ws.dbg, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
    for (int cls = 0; cls < 2; ++cls) {  // k_resolve phases (GS_STAMPS=1), thread 0 of every workgroup
      const unsigned long long* d = h + cls * kStampPhases;
      if (!d[0]) continue;
      fprintf(stderr, "[stamps] k_resolve %s: %llu buckets, mean kcycles per bucket per phase:",
              cls ? "M>=1024" : "M<1024", d[0]);
      for (uint32_t i = 1; i < kStampPhases; ++i) fprintf(stderr, " %.2f", d[i] * 1e-3 / d[0]);
      fprintf(stderr, "\n");
    }
}

// What the group itself owns, device by device (its members and their own
// resources are destroyed as contexts); leaves the first device current.
void release_group(gs_ctx* g) {
  Group& r = g->gr;
  for (size_t i = 0; i < r.devs.size(); ++i) {
    (void)hipSetDevice(r.devs[i]);
    if (i < r.buf.size()) release(r.buf[i]);
    for (auto* sets : {&r.ig, &r.fg, &r.gn})
      if (i < sets->size() && (*sets)[i]) (void)dev_free((*sets)[i]);
  }
  for (hipEvent_t e : r.ev_c) (void)hipEventDestroy(e);
  for (hipEvent_t e : r.ev_x) (void)hipEventDestroy(e);
  for (gs_ctx* rep : r.reps) destroy_one(rep);
  if (!r.devs.empty()) (void)hipSetDevice(r.devs[0]);
}

// (xsend / xrecv grow in the shard windows, h_xbuf in grow_pinned; the
// communicator is destroyed before any buffer, in destroy_one)
void release_exchange(gs_ctx* c) {
  Exchange& x = c->xc;
  if (x.d_gcounts) (void)dev_free(x.d_gcounts);
  if (x.d_glay) (void)dev_free(x.d_glay);
  if (x.h_glay) (void)hipHostFree(x.h_glay);
  release(x.xsend);
  release(x.xrecv);
  if (x.h_xbuf) (void)hipHostFree(x.h_xbuf);
}

}  // namespace

// The rest of a rank context once its exchange is set: gathered fire counts
// (flood) or its own replicated sets (push-pull).
int finish_rank(gs_ctx* c, gs_ctx** out) {
  (void)hipSetDevice(c->dev);
  if (dev_malloc(&c->xc.d_gcounts, (size_t)c->G * kMaxWindow * 8 + (size_t)kMaxWindow * 8) != hipSuccess ||
      (!c->pp_shard && (dev_malloc(&c->xc.d_glay, (size_t)c->G * (kRegions + 1) * 8) != hipSuccess ||
                        hipHostMalloc((void**)&c->xc.h_glay, (size_t)c->G * (kRegions + 1) * 8) != hipSuccess))) {
    destroy_one(c);
    return GS_ENOMEM;
  }
  if (c->pp_shard) {
    unsigned long long *ig = nullptr, *fg = nullptr, *gn = nullptr, *gst = nullptr;
    if (alloc_pp_sets(c, (uint64_t)c->G * c->rs.segw, &ig, &fg, &gn) ||
        alloc_pp_sets(c, (uint64_t)c->G * c->rs.segw, &gst, nullptr, nullptr)) {
      fprintf(stderr, "gs_create_rank: %s\n", c->err.c_str());
      for (unsigned long long* q : {ig, fg, gn, gst})
        if (q) (void)dev_free(q);
      destroy_one(c);
      return GS_ENOMEM;
    }
    c->rs.own_ig = true;
    c->rs.d_gst = gst;
    attach_pp_sets(c, ig, fg, gn);
    if (make_replica(&c->p, c->dev, ig, fg, &c->rs.rep)) {
      destroy_one(c);
      return GS_ENOMEM;
    }
    c->rs.own_rep = c->rs.rep != nullptr;
  }
  *out = c;
  return GS_OK;
}

// The body of gs_create_multi: shards of one broadcast, or trial batches,
// over `devices`.
int create_multi(const gs_params* params, const int* devices, int ndev, gs_ctx** out) {
  RC(rumor_refuse(params, "gs_create_multi"));
  RC(median_refuse(params, "gs_create_multi"));
  gs_ctx* g = new gs_ctx();
  g->group = true;
  g->p = *params;
  g->dev = devices[0];
  g->trials = std::max<uint32_t>(1, params->trials);
  g->gtrials = g->trials > 1;
  if (g->gtrials && (uint32_t)ndev > g->trials) ndev = (int)g->trials;
  for (int i = 0; i < ndev; ++i) {
    gs_params mp = *params;
    gs_ctx* m = nullptr;
    int rc;
    if (g->gtrials) {  // trials [t0, t1) on member i
      const uint32_t t0 = (uint32_t)((uint64_t)g->trials * i / ndev), t1 = (uint32_t)((uint64_t)g->trials * (i + 1) / ndev);
      mp.trial = params->trial + t0;
      mp.trials = t1 - t0;
      rc = create_one(&mp, devices[i], false, 1, 0, &m);
    } else {
      rc = create_one(&mp, devices[i], true, (uint32_t)ndev, (uint32_t)i, &m);
    }
    if (rc) {
      destroy_one(g);
      return rc;
    }
    g->gr.mem.push_back(m);
    auto it = std::find(g->gr.devs.begin(), g->gr.devs.end(), devices[i]);
    if (it == g->gr.devs.end()) {
      g->gr.devs.push_back(devices[i]);
      g->gr.dev_of.push_back((int)g->gr.devs.size() - 1);
    } else {
      g->gr.dev_of.push_back((int)(it - g->gr.devs.begin()));
    }
  }
  g->gr.buf.resize(g->gr.devs.size());
  g->pp = params->model == GS_MODEL_PUSHPULL;
  if (g->pp && !g->gtrials) {  // push-pull shards: one pair of replicated sets per device
    g->gr.ig.assign(g->gr.devs.size(), nullptr);
    g->gr.fg.assign(g->gr.devs.size(), nullptr);
    g->gr.gn.assign(g->gr.devs.size(), nullptr);
    for (size_t d = 0; d < g->gr.devs.size(); ++d) {
      std::vector<gs_ctx*> ms;
      for (size_t i = 0; i < g->gr.mem.size(); ++i)
        if ((size_t)g->gr.dev_of[i] == d) ms.push_back(g->gr.mem[i]);
      (void)hipSetDevice(g->gr.devs[d]);
      if (alloc_pp_sets(ms[0], (uint64_t)g->gr.mem.size() * ms[0]->rs.segw, &g->gr.ig[d], &g->gr.fg[d], &g->gr.gn[d])) {
        fprintf(stderr, "gs_create_multi: %s\n", ms[0]->err.c_str());
        destroy_one(g);
        return GS_ENOMEM;
      }
      for (gs_ctx* m : ms) attach_pp_sets(m, g->gr.ig[d], g->gr.fg[d], g->gr.gn[d]);
      gs_ctx* r = nullptr;
      if (make_replica(params, g->gr.devs[d], g->gr.ig[d], g->gr.fg[d], &r)) {
        destroy_one(g);
        return GS_ENOMEM;
      }
      g->gr.reps.push_back(r);
      for (gs_ctx* m : ms) m->rs.rep = r;
    }
  }
  for (size_t i = 0; i < g->gr.mem.size(); ++i) {
    hipEvent_t e;
    (void)hipSetDevice(g->gr.mem[i]->dev);
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      destroy_one(g);
      return GS_EDEVICE;
    }
    g->gr.ev_c.push_back(e);
  }
  for (size_t d = 0; d < g->gr.devs.size(); ++d) {
    hipEvent_t e;
    (void)hipSetDevice(g->gr.devs[d]);
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      destroy_one(g);
      return GS_EDEVICE;
    }
    g->gr.ev_x.push_back(e);
  }
  g->tacc.assign(g->gtrials ? 0 : 1, TrialAcc{});
  *out = g;
  return GS_OK;
}

void refresh_state(gs_ctx* c) {
  DevState& s = c->st;
  s.deg = c->d_deg;
  s.ids = c->d_ids;
  if (c->win) refresh_window(c);
  if (c->ppt) {
    c->pt.deg = c->d_deg;
    c->pt.ids = c->d_ids;
    c->pt.stride = s.stride;
  }
}

bool covered(uint64_t recv, uint64_t n) {
  // simulator.go:246-248, in float32
  volatile float a = (float)recv, b = (float)n;
  volatile float pct = a / b;
  return pct >= 0.99f;
}

// Host copies of the broadcast counters a gs_ctx keeps: for a group, the
// group's own fields; members and ranks keep theirs.
void reset_counters(gs_ctx* c) {
  c->t = c->fired = c->sent = c->msgs = c->recv = c->crashed = c->pending = 0;
  for (TrialAcc& a : c->tacc) a = TrialAcc{};
}

// Per-tick host bookkeeping shared by every flood/push-pull context: c's
// cumulative counters and (one trial) its TrialAcc.
void account_tick(gs_ctx* c, uint64_t tick, const unsigned long long* s, gs_tick_stats* o) {
  c->t = tick;
  c->fired += s[ST_FIRED];
  c->sent += s[ST_SENT];
  c->msgs += s[ST_MSGS];
  c->recv += s[ST_RECV];
  c->crashed += s[ST_CRASH];
  // push-pull: every informed node keeps calling
  c->pending = c->pp ? c->recv : c->pending + s[ST_SCHED] - s[ST_FIRED];
  if (c->tacc.size() == 1 && c->trials == 1) {
    TrialAcc& a = c->tacc[0];
    a.fired = c->fired; a.sent = c->sent; a.msgs = c->msgs; a.recv = c->recv; a.crash = c->crashed;
    if (!a.tick99 && covered(a.recv, c->p.n)) a.tick99 = tick;
  }
  if (o) *o = gs_tick_stats{c->t, s[ST_FIRED], s[ST_SENT], s[ST_MSGS], c->recv, c->crashed, c->pending};
}

// Ticks [t0, t0 + batch) of the shards ms: their h_stats rows summed and
// accounted on acc; tick t0 + i goes to out[i].
void account_members(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint64_t t0, uint32_t batch, gs_tick_stats* out) {
  for (uint32_t i = 0; i < batch; ++i) {
    const size_t row = (size_t)((t0 + i) % kStatSlots) * kStatFields;
    unsigned long long sum[kStatFields] = {0};
    for (uint32_t f = 0; f < kStatFields; ++f)
      for (gs_ctx* m : ms) sum[f] += m->h_stats[row + f];
    account_tick(acc, t0 + i, sum, out ? &out[i] : nullptr);
  }
}

// Batched push-pull trials: n is a parameter bounded by what `device` grants
// one workgroup (gs_ppt_plan.h), so it is validated with the other
// parameters, before any device state is set up; *pl gets the plan (block 0:
// not such a context).  Before this combination existed gs_create refused it
// with GS_EINVAL without looking at the device, and C clients probe that
// (tests/c/abi_test.c, run where no GPU is visible).  Where the device cannot
// be asked for its limit the combination still cannot be accepted, and that
// answer is kept: GS_EINVAL, with a message that says no device was visible.
// Every other create without a device fails with GS_EDEVICE in ctx_setup.
// ppt_lds_limit with its failure in words ("" on success): the HIP call that
// failed and the runtime's error string.
std::string ppt_limit_error(int device, bool masked, uint64_t* lim) {
  const char* where = "";
  const hipError_t e = ppt_lds_limit(device, masked, lim, &where);
  return trial_limit_error(where, device, e);
}

// A batched push-pull context about to take failure masks: the masked LDS
// plan of its n on its device.  GS_EINVAL with the limit in `why` where n is
// past it; nothing of the context is changed.
int ppt_masked_plan(const gs_ctx* c, PptPlan* plan, std::string& why) {
  uint64_t lim = 0;
  why = ppt_limit_error(c->dev, true, &lim);
  if (!why.empty()) return GS_EDEVICE;
  *plan = ppt_plan_masked(c->p.n, lim);
  if (plan->fits) return GS_OK;
  why = "batched push-pull trials with failure masks keep a third bitset in one workgroup's LDS: n must be <= " +
        std::to_string(ppt_max_n_masked(lim)) + " on device " + std::to_string(c->dev) +
        " (gs_pp_trials_max_n_masked), not " + std::to_string(c->p.n);
  return GS_EINVAL;
}

// Why this thread's last failed create failed: there is no context to carry
// it, so gs_last_error(NULL) returns it.
thread_local std::string g_create_err;

int create_one(const gs_params* params, int device, bool shard, uint32_t G, uint32_t rank, gs_ctx** out,
               bool rumor_trials, bool median_trials, uint32_t rumorset) {
  std::string why;
  PptPlan pl;
  RmtPlan rpl;
  MdtPlan mpl;
  int rc = check_params(params, rumor_trials, median_trials, why);
  if (!rc) rc = check_ppt_n(params, device, why, &pl);
  if (!rc) rc = check_rmt_n(params, device, why, &rpl);
  bool packed = false;
  if (!rc) rc = check_mdt_n(params, median_trials, device, why, &mpl, &packed);
  if (!rc) {
    gs_ctx* c = new gs_ctx();
    c->rset = rumorset != 0;  // a rumor set (gs_create_rumorset checked the rest)
    c->rumors = rumorset;
    if (mpl.block) {  // batched median trials: the plan check_mdt_n made for this device
      c->mdt = true;
      c->mdt16 = packed;
      c->mplan = mpl;
    }
    if (rpl.block) {  // batched rumor trials: the plan check_rmt_n made for this device
      c->rmt = true;
      c->rplan = rpl;
    }
    if (pl.block) {  // batched push-pull trials: the plan check_ppt_n made for this device
      c->ppt = true;
      c->pt.block = pl.block;
      c->pt.lds_bytes = (uint32_t)pl.lds_bytes;
    }
    rc = ctx_setup(c, params, device, shard, G, rank, why);
    if (!rc) {
      *out = c;
      return GS_OK;
    }
    destroy_one(c);
  }
  fprintf(stderr, "gs_create: %s\n", why.c_str());
  g_create_err = why;
  return rc;
}

// Every kind of context: what a kind does not own is null or empty here, and
// its release does nothing.
void destroy_one(gs_ctx* c) {
  if (!c) return;
  for (gs_ctx* m : c->gr.mem) destroy_one(m);
  if (c->rs.own_rep) destroy_one(c->rs.rep);
  (void)hipSetDevice(c->dev);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->xc.comm && rccl().ok) (void)rccl().comm_destroy(c->xc.comm);
  print_stamps(c);
  release_group(c);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  overlay_free(&c->ovw, c->stream);
  release_sets(c);
  release_exchange(c);
  release_table(c);
  release_state(c);
  release_window(c);
  release_trials(c);
  release_sparse(c);
  release_rumor(c);
  release_median(c);
  release_rumorset(c);
  release_async(c);
  release_dd(c);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
}

}  // namespace gs
