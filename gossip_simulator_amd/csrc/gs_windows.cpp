// gs_windows.cpp -- the unsharded flood engines: host-driven windows
// (run_windows), device-driven windows (run_async) and the tick engine.
#include "gs_ctx.h"

namespace gs {

namespace {

// Coarse region plan: each of bin b's 8 sub-regions gets 1/8 of the bin's
// node share of the window's T message bound plus 512, or exactly
// `exact[region]` (region = bin * 8 + sub).
void plan_coarse(gs_ctx* c, uint64_t T, const unsigned long long* exact) {
  const WinState& w = c->ws;
  unsigned long long a = 0;
  for (uint32_t b = 0; b < 256; ++b) {
    const uint64_t lo = (uint64_t)b << kCoarseShift;
    const uint64_t hi = std::min<uint64_t>(w.n, lo + (1ull << kCoarseShift));
    const double xr = (double)kXRoundNodes * w.stride;  // one expand round's slots (gs_internal.h)
    const unsigned long long sub =
        b < w.ncoarse ? (unsigned long long)(((double)T / kCoarseSub + xr) * (double)(hi - lo) / (double)w.n) + 512
                      : 0ull;
    for (uint32_t x = 0; x < kCoarseSub; ++x) {
      const uint32_t r = b * kCoarseSub + x;
      c->wn.h_cap[r] = a;
      if (b >= w.ncoarse) continue;
      a += exact ? exact[r] : sub;
    }
  }
  c->wn.h_cap[kRegions] = a;
}

// Batched trials (trials > 1, tlog <= kCoarseShift): a message never leaves
// its sender's trial, so it lands in the sender's coarse bin, and the
// sub-region it goes to is the XCD whose rounds expanded the sender
// (xcd_rounds in gs_win_expand.hip).  fb[b] = the first firing index of bin b
// (bins are contiguous in the bucket-major unit order), fb[ncoarse] = Tn.
// Region (b, x) gets an exact upper bound -- the window's firing nodes of bin
// b in XCD x's rounds, times the row length -- so it never overflows: the
// node-share estimate of plan_coarse assumed targets spread over every bin
// and overflowed almost every window of a C3 batch (each then expanded three
// times: estimate, count, redo).
void plan_coarse_trials(gs_ctx* c, const unsigned long long* fb, unsigned long long Tn) {
  const WinState& w = c->ws;
  uint32_t per_round = 0;
  const uint32_t blocks = win_expand_geometry(w, Tn, &per_round, nullptr, nullptr);
  const unsigned long long rounds = (Tn + per_round - 1) / per_round;
  const bool by_xcd = blocks && (blocks & 7) == 0;
  const unsigned long long per = (rounds + 7) >> 3;
  std::vector<unsigned long long> cap(kRegions, 0);
  for (uint32_t b = 0; b < w.ncoarse; ++b) {
    const unsigned long long lo = fb[b], hi = fb[b + 1];
    for (unsigned long long r = lo / per_round; lo < hi && r * per_round < hi; ++r) {
      const unsigned long long a = std::max(lo, r * per_round), e = std::min(hi, (r + 1) * per_round);
      const uint32_t x = by_xcd ? (uint32_t)std::min<unsigned long long>(r / per, 7) : (uint32_t)((r % blocks) & 7);
      cap[b * kCoarseSub + x] += (e - a) * w.slots;
    }
  }
  unsigned long long a = 0;
  for (uint32_t r = 0; r < kRegions; ++r) {
    c->wn.h_cap[r] = a;
    a += cap[r] ? cap[r] + 16 : 0;
  }
  c->wn.h_cap[kRegions] = a;
}

// Window engine: ticks [t0, t0 + n) as windows of <= min(max(delaylow,1),10)
// ticks (gs_win_*.hip).  One host sync per window reads its task count.
int run_windows(gs_ctx* c, uint64_t t0, uint32_t n, bool timing, uint64_t tchunk) {
  RC(expand_view(c));
  WinState& w = c->ws;
  const uint32_t Lmax = std::min<uint32_t>(std::max<int32_t>(c->p.delay_low, 1), kBitTicks);
  uint32_t done = 0, widx = 0;
  std::vector<std::pair<uint32_t, uint32_t>> evs;
  // Receipts per fine bucket are ~density * 16384 whatever N is; a window whose
  // slots would overflow k_resolve's LDS message buffer on average is cut short.
  const uint64_t slot_budget = (uint64_t)w.nfine * kWinSlotsPerBucket;
  // batched trials: each coarse bin's first firing index comes back with the
  // window's fire counts (plan_coarse_trials)
  const bool trial_plan = c->trials > 1 && c->tlog <= kCoarseShift && !c->shard;
  while (done < n) {
    const uint32_t Lw = std::min(Lmax, n - done);
    const uint32_t t = (uint32_t)(t0 + done);
    w.tofs = (uint32_t)(t - tchunk);
    auto units = [&](uint32_t Lu) -> int {
      CK(c, hipMemsetAsync(w.tfires, 0, kMaxWindow * 8, c->stream));
      CK(c, win_units(w, t, Lu, c->stream));
      size_t need = 0;
      CK(c, win_scan_units(w, Lu, nullptr, need, c->stream));
      if (!grow(c->wn.tmp, need)) return fail(c, GS_ENOMEM, "cannot allocate scan scratch");
      need = c->wn.tmp.bytes;
      CK(c, win_scan_units(w, Lu, c->wn.tmp.p, need, c->stream));
      CK(c, hipMemcpyAsync(c->wn.h_misc, w.tfires, kMaxWindow * 8, hipMemcpyDeviceToHost, c->stream));
      if (trial_plan)
        CK(c, hipMemcpy2DAsync(c->wn.h_misc + kMaxWindow, 8, w.unit_off, (size_t)256 * Lu * 8, 8, w.ncoarse,
                               hipMemcpyDeviceToHost, c->stream));
      CK(c, hipStreamSynchronize(c->stream));
      return GS_OK;
    };
    RC(units(Lw));
    // fires per tick -> the window's length under the slot budget
    uint32_t L = 1;
    unsigned long long Tn = c->wn.h_misc[0];  // broadcasts firing in the window
    while (L < Lw && (Tn + c->wn.h_misc[L]) * w.stride <= slot_budget) Tn += c->wn.h_misc[L++];
    // units are bucket-major: a cut window is laid out again for its L ticks
    if (L < Lw) RC(units(L));
    const unsigned long long T = Tn * w.stride;  // friend slots of the firing nodes
    if (trial_plan && Tn) {
      // batched trials: exact per-(bin, XCD) bounds from the bins' first firing
      // indices (unit_off at every 256 * L-th unit, copied by units())
      std::vector<unsigned long long> fb(c->wn.h_misc + kMaxWindow, c->wn.h_misc + kMaxWindow + w.ncoarse);
      fb.push_back(Tn);
      plan_coarse_trials(c, fb.data(), Tn);
    } else {
      plan_coarse(c, T, nullptr);
    }
    const uint64_t fcap = T + T / 8 + (uint64_t)w.ncoarse * 256 * 513 + 16;
    if (!grow(c->wn.gmap, ((Tn + 63) / 64 + 1) * 4) || !grow(c->wn.cmsg, (c->wn.h_cap[kRegions] + 16) * 4) ||
        !grow(c->wn.fmsg, (fcap + 16) * 4))  // buf_cap(fmsg) >= fcap (the device-driven windows' bound)
      return fail(c, GS_ENOMEM, "cannot allocate " + std::to_string(T) + " window messages");
    w.gmap = (uint32_t*)c->wn.gmap.p;
    w.cmsg = (uint32_t*)c->wn.cmsg.p;
    w.fmsg = (uint32_t*)c->wn.fmsg.p;
    if (timing)
      while (c->ev.size() < (size_t)(widx + 1) * 5) {
        hipEvent_t ev;
        CK(c, hipEventCreate(&ev));
        c->ev.push_back(ev);
      }
    hipEvent_t* e = timing ? &c->ev[(size_t)widx * 5] : nullptr;
    if (T) {
      CK(c, hipMemcpyAsync(w.ccap, c->wn.h_cap, (kRegions + 1) * 8, hipMemcpyHostToDevice, c->stream));
      CK(c, win_groupmap(w, L, c->stream));
      if (e) CK(c, hipEventRecord(e[0], c->stream));
      CK(c, win_expand(w, t, L, Tn, 1, c->stream));
      if (e) CK(c, hipEventRecord(e[1], c->stream));
      CK(c, win_plan(w, false, c->stream));
      CK(c, win_part2(w, T, true, c->stream));
      if (e) CK(c, hipEventRecord(e[2], c->stream));
      // regions sized from estimates: check, and redo exactly on overflow
      CK(c, hipMemcpyAsync(c->wn.h_misc, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
      CK(c, hipStreamSynchronize(c->stream));
      uint32_t err = (uint32_t)c->wn.h_misc[0];
      if (err & kErrCoarse) {
        ++c->timing.coarse_redos;
        CK(c, hipMemsetAsync(w.chist, 0, kRegions * 8, c->stream));
        CK(c, win_expand(w, t, L, Tn, 0, c->stream));
        CK(c, hipMemcpyAsync(c->wn.h_misc, w.chist, kRegions * 8, hipMemcpyDeviceToHost, c->stream));
        CK(c, hipStreamSynchronize(c->stream));
        plan_coarse(c, T, c->wn.h_misc);
        CK(c, hipMemcpyAsync(w.ccap, c->wn.h_cap, (kRegions + 1) * 8, hipMemcpyHostToDevice, c->stream));
        CK(c, hipMemsetAsync(w.cfill, 0, kRegions * 8, c->stream));
        CK(c, win_expand(w, t, L, Tn, 2, c->stream));
        CK(c, win_plan(w, false, c->stream));
        err = kErrFine;  // the fine regions must be redone as well
      }
      if (err & kErrFine) {
        CK(c, hipMemsetAsync(w.fhist, 0, ((size_t)w.ncoarse * 256 + 1) * 8, c->stream));
        CK(c, win_plan(w, true, c->stream));
        CK(c, win_part2(w, T, false, c->stream));
        size_t need2 = 0;
        CK(c, win_scan_fine(w, nullptr, need2, c->stream));
        if (!grow(c->wn.tmp, need2)) return fail(c, GS_ENOMEM, "cannot allocate scan scratch");
        need2 = c->wn.tmp.bytes;
        CK(c, win_scan_fine(w, c->wn.tmp.p, need2, c->stream));
        CK(c, hipMemsetAsync(w.ffill, 0, (size_t)w.nfine * 8, c->stream));
        CK(c, win_part2(w, T, true, c->stream));
        ++c->timing.exact_redos;
      }
    } else if (e) {
      CK(c, hipEventRecord(e[0], c->stream));
      CK(c, hipEventRecord(e[1], c->stream));
      CK(c, hipEventRecord(e[2], c->stream));
    }
    // the window's fire lists are consumed: later ticks t + R may reuse the slots
    const uint32_t s0 = t % w.R;
    const uint32_t first = std::min(L, w.R - s0);
    CK(c, hipMemsetAsync(w.fcount + (size_t)s0 * w.nfine, 0, (size_t)first * w.nfine * 4, c->stream));
    if (first < L) CK(c, hipMemsetAsync(w.fcount, 0, (size_t)(L - first) * w.nfine * 4, c->stream));
    if (e) CK(c, hipEventRecord(e[3], c->stream));
    if (T) CK(c, win_resolve(w, t, L, c->stream));
    if (T) CK(c, win_stats_reduce(w, t, L, c->stream));
    if (e) {
      CK(c, hipEventRecord(e[4], c->stream));
      evs.emplace_back(widx * 5, T ? 1u : 0u);
    }
    ++widx;
    done += L;
  }
  if (timing) {
    CK(c, hipStreamSynchronize(c->stream));
    for (auto& pr : evs) {
      hipEvent_t* e = &c->ev[pr.first];
      float ms = 0;
      CK(c, hipEventElapsedTime(&ms, e[0], e[1]));
      c->timing.expand_ms += ms;
      c->timing.deliver_ms += ms;
      CK(c, hipEventElapsedTime(&ms, e[1], e[2]));
      c->timing.part_ms += ms;
      c->timing.deliver_ms += ms;
      CK(c, hipEventElapsedTime(&ms, e[3], e[4]));
      c->timing.resolve_ms += ms;
      c->timing.deliver_launches += pr.second;
      c->timing.resolve_launches += pr.second;
      c->timing.windows += 1;
    }
  }
  uint32_t err = 0;
  CK(c, hipMemcpyAsync(&err, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  if (err & 4) return fail(c, GS_EOVERFLOW, "too many arrivals at one node in one tick");
  return GS_OK;
}

int async_setup(gs_ctx* c) {
  if (!c->aw.d_ctl) CK(c, dev_malloc(&c->aw.d_ctl, sizeof(WinCtl)));
  RC(alloc_stage(c));
  // the message buffers keep the size the windows so far needed: a window
  // that needs more is flagged and redone host-driven, which grows them
  if (!grow(c->wn.gmap, ((c->ntot + 1 + 63) / 64 + 1) * 4) || !grow(c->wn.cmsg, 64) || !grow(c->wn.fmsg, 64))
    return fail(c, GS_ENOMEM, "cannot allocate the window message buffers");
  return GS_OK;
}

}  // namespace

// The staging slots of the device-driven windows (run_async, dd_run): k_close
// writes each window's results straight into pinned host memory (no copy
// launch per window); d_stage is its device address.
int alloc_stage(gs_ctx* c) {
  if (c->aw.h_stage) return GS_OK;
  CK(c, hipHostMalloc((void**)&c->aw.h_stage, (size_t)kSlots * kStageWords * 8,
                      hipHostMallocMapped | hipHostMallocPortable));
  CK(c, hipHostGetDevicePointer((void**)&c->aw.d_stage, c->aw.h_stage, 0));
  for (uint32_t i = 0; i < kSlots; ++i) {
    hipEvent_t e;
    CK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->aw.wev.push_back(e);
  }
  return GS_OK;
}

void release_async(gs_ctx* c) {
  if (c->aw.d_ctl) (void)dev_free(c->aw.d_ctl);
  if (c->aw.h_stage) (void)hipHostFree(c->aw.h_stage);  // (d_stage maps it)
  for (hipEvent_t e : c->aw.wev) (void)hipEventDestroy(e);
}

void refresh_window(gs_ctx* c) {
  WinState& w = c->ws;
  w.deg = c->st.deg;
  w.ids = c->st.ids;
  w.recv = c->st.recv;
  w.crash = c->st.crash;
  w.rollw = c->st.rollw;
  w.stats = c->st.stats;
  w.err = c->d_err;
  w.stride = c->st.stride;
  w.slots = c->row_slots && c->row_slots < c->st.stride ? c->row_slots : c->st.stride;
  w.stride_magic = c->st.stride_magic;
  w.abort_on_err = c->shard ? 1u : 0u;
}

// ---- device-driven windows ----------------------------------------------------
// The unsharded one-trial window engine runs gs_step / gs_run without a host
// round trip per window: k_cut makes the window cut and coarse plan on the
// device, k_close applies gs_run's poll rule there, every kernel reads the
// window from ctl, and the host enqueues window i before it reads window
// i-1's results (staging slot + event), so the GPU never waits on it.  A
// partition overflow (skewed targets, or a message buffer too small) makes
// every later kernel a no-op; the host then finishes with run_windows, which
// redoes that window exactly and grows the buffers.
bool async_ok(const gs_ctx* c) {
  return c->win && !c->pp && !c->shard && !c->group && c->trials == 1 && !c->async_off &&
         !(c->p.flags & GS_FLAG_TIMING);
}

uint64_t cover_threshold(uint64_t n) {  // smallest r with covered(r, n)
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (covered(mid, n)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Ticks c->t+1 .. tend-1, or (poll > 0) until gs_run's rule stops the run at a
// poll.  on_tick(tick, row) sees every tick's counters in order.  *stop gets
// 1 + GS_RUN_* if a poll stopped the run; *fallback = true if a window
// overflowed (the caller continues host-driven from c->t).
int run_async(gs_ctx* c, uint64_t tend, uint32_t poll, uint64_t max_ticks, const OnTick& on_tick, uint32_t* stop,
              bool* fallback) {
  *stop = 0;
  *fallback = false;
  RC(async_setup(c));
  RC(expand_view(c));
  WinState w = c->ws;
  w.ctl = c->aw.d_ctl;
  w.stage = c->aw.d_stage;
  w.lstride = std::min<uint32_t>(std::max<int32_t>(c->p.delay_low, 1), kBitTicks);
  w.gmap = (uint32_t*)c->wn.gmap.p;
  w.cmsg = (uint32_t*)c->wn.cmsg.p;
  w.fmsg = (uint32_t*)c->wn.fmsg.p;
  WinCtl h{};
  h.tnext = (uint32_t)(c->t + 1);
  h.tend = (uint32_t)std::min<uint64_t>(tend, 0xFFFFFFFFull);
  h.poll = poll;
  h.pbase = (uint32_t)c->t;
  h.lmax = w.lstride;
  h.recv = c->recv;
  h.crashed = c->crashed;
  h.pending = c->pending;
  h.cover = cover_threshold(c->p.n);
  h.max_ticks = max_ticks;
  h.cmsg_cap = c->wn.cmsg.bytes / 4 > 16 ? c->wn.cmsg.bytes / 4 - 16 : 0;
  h.fmsg_cap = c->wn.fmsg.bytes / 4 > 16 ? c->wn.fmsg.bytes / 4 - 16 : 0;
  CK(c, hipMemcpyAsync(c->aw.d_ctl, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
  CK(c, hipMemsetAsync(w.tfires, 0, kMaxWindow * 8, c->stream));
  const uint64_t budget = (uint64_t)w.nfine * kWinSlotsPerBucket;
  // launch sizes: grid-stride kernels, sized for the dense windows
  const uint64_t Tn_bound = std::min<uint64_t>(c->ntot + 1, 4096ull * 1024),
                 T_bound = std::min<uint64_t>((c->ntot + 1) * w.stride, 2048ull * 16384);
  auto enqueue = [&](uint32_t slot) -> int {
    // units (+ tile sums) -> cut (+ tile offsets) -> unit scan and group map
    // inside the tiles; the rolled replay consumes the window's fire lists
    CK(c, win_units(w, 0, w.lstride, c->stream));
    CK(c, win_cut(w, budget, c->stream));
    CK(c, win_unitscan(w, c->stream));
    CK(c, win_expand(w, 0, w.lstride, Tn_bound, 1, c->stream));
    CK(c, win_plan(w, false, c->stream));
    CK(c, win_part2(w, T_bound, true, c->stream));
    CK(c, win_resolve(w, 0, w.lstride, c->stream));
    CK(c, win_close(w, slot, c->stream));
    CK(c, hipEventRecord(c->aw.wev[slot], c->stream));
    return GS_OK;
  };
  // window i-1's results: 0 = go on, 1 = finished (the enqueued window i is a no-op)
  auto absorb = [&](uint32_t slot, int* what) -> int {
    CK(c, hipEventSynchronize(c->aw.wev[slot]));
    const unsigned long long* st = c->aw.h_stage + (size_t)slot * kStageWords;
    const uint32_t t0 = (uint32_t)st[0], L = (uint32_t)st[1];
    *what = 0;
    if (st[3] & (kErrCoarse | kErrFine)) {  // overflow: later windows did nothing
      *fallback = true;
      *what = 1;
      return GS_OK;
    }
    if (c->winlog) fprintf(stderr, "[win] t0=%u L=%u Tn=%llu stop=%llu\n", t0, L, st[4], st[2]);
    for (uint32_t k = 0; k < L; ++k) on_tick((uint64_t)t0 + k, st + 8 + (size_t)k * kStatFields);
    if (st[2]) *stop = (uint32_t)st[2];
    if (st[2] || L == 0 || (uint64_t)t0 + L >= tend) *what = 1;
    return GS_OK;
  };
  RC(enqueue(0));
  for (uint32_t i = 1;; ++i) {
    RC(enqueue(i % kSlots));
    int what = 0;
    RC(absorb((i - 1) % kSlots, &what));
    if (what) break;
  }
  CK(c, hipStreamSynchronize(c->stream));
  if (*fallback) {  // undo what the failed window left: its partial counters and flags
    uint32_t e = 0;
    CK(c, hipMemcpy(&e, c->d_err, 4, hipMemcpyDeviceToHost));
    e &= ~(kErrCoarse | kErrFine);
    CK(c, hipMemcpy(c->d_err, &e, 4, hipMemcpyHostToDevice));
    CK(c, hipMemsetAsync(c->ws.sstats, 0, (size_t)kStatShards * kMaxWindow * kStatFields * 8, c->stream));
    CK(c, hipMemsetAsync(c->ws.tfires, 0, kMaxWindow * 8, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  }
  uint32_t err = 0;
  CK(c, hipMemcpy(&err, c->d_err, 4, hipMemcpyDeviceToHost));
  if (err & kErrArrivals) return fail(c, GS_EOVERFLOW, "too many arrivals at one node in one tick");
  return GS_OK;
}

// on_tick of a step's device-driven windows: tick *k of the step is accounted
// on acc and goes to out[*k].
OnTick step_sink(gs_ctx* acc, gs_tick_stats* out, uint32_t* k) {
  return [=](uint64_t tick, const unsigned long long* row) {
    account_tick(acc, tick, row, out ? &out[*k] : nullptr);
    ++*k;
  };
}

// gs_step of a plain or batched context on the window, tick or push-pull
// engine (unsharded).
int plain_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out) {
  CK(c, hipSetDevice(c->dev));
  if (async_ok(c) && ticks > 0) {  // device-driven windows
    uint32_t stop = 0, k = 0;
    bool fallback = false;
    RC(run_async(c, c->t + ticks + 1, 0, ~0ull, step_sink(c, out, &k), &stop, &fallback));
    if (!fallback) return GS_OK;
    ticks -= k;  // a window overflowed: the rest host-driven (it redoes that window exactly)
    if (out) out += k;
  }
  const bool timing = (c->p.flags & GS_FLAG_TIMING) != 0;
  const bool flood = c->st.kc == 0;
  const bool batched = c->trials > 1;
  uint32_t done = 0;
  while (done < ticks) {
    // batched trials: chunks of <= kMaxWindow ticks (the per-trial counter rows)
    const uint32_t batch = std::min<uint32_t>(ticks - done, batched ? kMaxWindow : kStatSlots);
    const uint64_t t0 = c->t + 1;
    // zero this batch's stats entries (ring-indexed)
    const StatSpans sp = stat_spans(t0, batch);
    for (int j = 0; j < sp.n; ++j) CK(c, hipMemsetAsync(c->st.stats + sp.off[j], 0, sp.words[j] * 8, c->stream));
    if (batched)
      CK(c, hipMemsetAsync(c->bt.d_tstat, 0, (size_t)c->trials * kMaxWindow * kTStatFields * 4, c->stream));
    const uint32_t nev = timing && !c->win ? batch * (flood || c->pp ? 2 : 4) : 0;
    while (c->ev.size() < nev) {
      hipEvent_t e;
      CK(c, hipEventCreate(&e));
      c->ev.push_back(e);
    }
    if (c->win) RC(run_windows(c, t0, batch, timing, t0));
    for (uint32_t i = 0; i < batch && c->pp; ++i) {  // push-pull rounds
      const uint32_t tt = (uint32_t)(t0 + i);
      hipEvent_t* e = timing ? &c->ev[(size_t)i * 2] : nullptr;
      if (e) CK(c, hipEventRecord(e[0], c->stream));
      CK(c, pp_round(c->st, c->d_next, c->d_ppsum, tt, c->pp_l2_only, c->sp, c->stream));
      CK(c, pp_commit(c->st, c->d_next, tt, c->sp, c->stream));
      if (e) CK(c, hipEventRecord(e[1], c->stream));
    }
    for (uint32_t i = 0; i < batch && !c->win && !c->pp; ++i) {
      const uint32_t tt = (uint32_t)(t0 + i);
      hipEvent_t* e = timing ? &c->ev[(size_t)i * (flood ? 2 : 4)] : nullptr;
      if (e) CK(c, hipEventRecord(e[0], c->stream));
      CK(c, launch_tick(c->st, tt, flood ? MODE_FLOOD : MODE_COUNT, c->stream));
      if (e) CK(c, hipEventRecord(e[1], c->stream));
      if (!flood) {
        if (e) CK(c, hipEventRecord(e[2], c->stream));
        CK(c, launch_tick(c->st, tt, MODE_RESOLVE, c->stream));
        if (e) CK(c, hipEventRecord(e[3], c->stream));
      }
      CK(c, launch_slot_reset(c->st, tt % c->st.R, c->stream));
    }
    for (int j = 0; j < sp.n; ++j)
      CK(c, hipMemcpyAsync(c->h_stats + sp.off[j], c->st.stats + sp.off[j], sp.words[j] * 8, hipMemcpyDeviceToHost,
                           c->stream));
    if (batched)
      CK(c, hipMemcpyAsync(c->bt.h_tstat, c->bt.d_tstat, (size_t)c->trials * kMaxWindow * kTStatFields * 4,
                           hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    if (!c->win && !c->pp && !flood) {  // the tick engine's 16-bit receipt counts (MODE_COUNT)
      uint32_t err = 0;
      CK(c, hipMemcpy(&err, c->d_err, 4, hipMemcpyDeviceToHost));
      if (err & kErrArrivals) return fail(c, GS_EOVERFLOW, "too many arrivals at one node in one tick");
    }
    if (timing && !c->win) {
      for (uint32_t i = 0; i < batch; ++i) {
        hipEvent_t* e = &c->ev[(size_t)i * (flood || c->pp ? 2 : 4)];
        float ms = 0;
        CK(c, hipEventElapsedTime(&ms, e[0], e[1]));
        c->timing.deliver_ms += ms;
        c->timing.deliver_launches++;
        if (!flood && !c->pp) {
          CK(c, hipEventElapsedTime(&ms, e[2], e[3]));
          c->timing.resolve_ms += ms;
          c->timing.resolve_launches++;
        }
      }
    }
    for (uint32_t i = 0; i < batch; ++i) {
      const unsigned long long* s = c->h_stats + (size_t)((t0 + i) % kStatSlots) * kStatFields;
      account_tick(c, t0 + i, s, out ? &out[done + i] : nullptr);
    }
    if (batched) account_trials(c, t0, batch);
    done += batch;
  }
  return GS_OK;
}

}  // namespace gs
