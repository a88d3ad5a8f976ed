// gs_median_host.cpp -- the host side of median-counter push-pull
// (GS_MODEL_MEDIAN): its buffers, the round loop and
// gs_run's stop rule.  One trial on one device (the kernels are in
// gs_median.hip).
#include "gs_ctx.h"

namespace gs {

namespace {

MedianState median_state(const gs_ctx* c) {
  return MedianState{(RumorCtl*)c->md.ctlb.p, (uint8_t*)c->md.st.p, (uint8_t*)c->md.own.p,
                     (unsigned long long*)c->md.tally.p, (unsigned long long*)c->md.gotb.p,
                     (unsigned long long*)c->md.gotc.p, c->p.rumor_k};
}

// The round's counters on the host (rumor_account's rule): tick_99 is taken at
// polls only.
void median_account(gs_ctx* c, uint64_t tick, const unsigned long long* s, bool poll, gs_tick_stats* o) {
  c->t = tick;
  c->fired += s[ST_FIRED];
  c->sent += s[ST_SENT];
  c->msgs += s[ST_MSGS];
  c->recv += s[ST_RECV];
  c->pending = s[ST_SCHED];  // the active nodes after the round
  TrialAcc& a = c->tacc[0];
  a.fired = c->fired; a.sent = c->sent; a.msgs = c->msgs; a.recv = c->recv;
  if (poll && !a.tick99 && covered(a.recv, c->p.n)) a.tick99 = tick;
  if (o) *o = gs_tick_stats{c->t, s[ST_FIRED], s[ST_SENT], s[ST_MSGS], c->recv, 0, c->pending};
}

}  // namespace

// The combinations the model does not run: every create but gs_create.
int median_refuse(const gs_params* params, const char* what) {
  if (!params || params->model != GS_MODEL_MEDIAN) return GS_OK;
  g_create_err = std::string(what) + " with GS_MODEL_MEDIAN: the median-counter model runs one trial on one device "
                 "(gs_create)";
  fprintf(stderr, "%s: %s\n", what, g_create_err.c_str());
  return GS_EINVAL;
}

// Nothing of the flood's window buffers, push-pull's reverse table or the
// rumor model's lists: the state bytes, the own-contribution bytes, the tally
// and two bitsets.  At n = 1e9: 1 + 1 + 8 GB and 2 x 125 MB, from the block
// cache like every buffer of 64 MiB or more.
int median_alloc(gs_ctx* c) {
  const uint64_t n = c->st.n;
  MedianBufs& b = c->md;
  if (!grow(b.st, n) || !grow(b.own, n) || !grow(b.tally, n * 8) || !grow(b.gotb, c->st.W * 8) ||
      !grow(b.gotc, c->st.W * 8) || !grow(b.ctlb, sizeof(RumorCtl)) ||
      hipHostMalloc((void**)&b.h_ctl, sizeof(RumorCtl)) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the median-counter model's state");
  return GS_OK;
}

// (done grows at the first gs_read_removed)
void release_median(gs_ctx* c) {
  MedianBufs& b = c->md;
  for (Buf* q : {&b.st, &b.own, &b.tally, &b.gotb, &b.gotc, &b.ctlb, &b.done}) release(*q);
  if (b.h_ctl) (void)hipHostFree(b.h_ctl);
}

// A live sender becomes B-1 (received = 1, as in push-pull); a failed one
// starts nothing and the first poll is quiescent.
int median_begin(gs_ctx* c, uint64_t sender) {
  CK(c, hipSetDevice(c->dev));
  // GS_MEDIAN_GRID: the round kernel's blocks (read per broadcast, so tests can
  // make a short table take several passes of the grid)
  const char* e = getenv("GS_MEDIAN_GRID");
  MedianBufs& b = c->md;
  b.grid = median_grid(c->st.n, e ? (uint32_t)std::min(std::max(atoi(e), 1), 4096) : 0u);
  CK(c, hipMemsetAsync(b.ctlb.p, 0, sizeof(RumorCtl), c->stream));
  CK(c, hipMemsetAsync(b.st.p, 0, c->st.n, c->stream));
  CK(c, hipMemsetAsync(b.own.p, 0, c->st.n, c->stream));
  CK(c, hipMemsetAsync(b.tally.p, 0, c->st.n * 8, c->stream));
  for (Buf* q : {&b.gotb, &b.gotc}) CK(c, hipMemsetAsync(q->p, 0, c->st.W * 8, c->stream));
  CK(c, median_seed(c->st, median_state(c), (uint32_t)sender, cover_threshold(c->p.n), c->stream));
  CK(c, hipMemcpyAsync(b.h_ctl, b.ctlb.p, sizeof(RumorCtl), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  c->recv = c->tacc[0].recv = b.h_ctl->received;
  c->pending = b.h_ctl->rlen;
  c->begun = true;
  return GS_OK;
}

// `ticks` rounds, enqueued without a host sync between them; the stats rows
// and the control block come back once per call (per kStatSlots rounds).
// every_tick_polls: each tick is a poll (gs_step returns every tick's row);
// else only the call's last tick is (gs_run).
int median_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls) {
  CK(c, hipSetDevice(c->dev));
  const bool timing = (c->p.flags & GS_FLAG_TIMING) != 0;
  const MedianState ms = median_state(c);
  MedianBufs& b = c->md;
  uint32_t done = 0;
  while (done < ticks) {
    const uint32_t batch = std::min<uint32_t>(ticks - done, timing ? 256u : kStatSlots);
    const uint64_t t0 = c->t + 1;
    const StatSpans sp = stat_spans(t0, batch);
    while (timing && c->ev.size() < (size_t)batch * 3) {
      hipEvent_t ev;
      CK(c, hipEventCreate(&ev));
      c->ev.push_back(ev);
    }
    for (uint32_t i = 0; i < batch; ++i) {
      const uint32_t tt = (uint32_t)(t0 + i);
      hipEvent_t* ev = timing ? &c->ev[(size_t)i * 3] : nullptr;
      if (ev) CK(c, hipEventRecord(ev[0], c->stream));
      CK(c, median_round(c->st, ms, tt, b.grid, c->stream));
      if (ev) CK(c, hipEventRecord(ev[1], c->stream));
      CK(c, median_commit(c->st, ms, tt, c->stream));
      if (ev) CK(c, hipEventRecord(ev[2], c->stream));
    }
    for (int j = 0; j < sp.n; ++j)
      CK(c, hipMemcpyAsync(c->h_stats + sp.off[j], c->st.stats + sp.off[j], sp.words[j] * 8, hipMemcpyDeviceToHost,
                           c->stream));
    CK(c, hipMemcpyAsync(b.h_ctl, b.ctlb.p, sizeof(RumorCtl), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < batch && timing; ++i) {
      float ms_ = 0;
      CK(c, hipEventElapsedTime(&ms_, c->ev[(size_t)i * 3], c->ev[(size_t)i * 3 + 1]));
      c->timing.deliver_ms += ms_;  // the round kernel
      c->timing.deliver_launches++;
      CK(c, hipEventElapsedTime(&ms_, c->ev[(size_t)i * 3 + 1], c->ev[(size_t)i * 3 + 2]));
      c->timing.resolve_ms += ms_;  // commit + publish
      c->timing.resolve_launches++;
    }
    for (uint32_t i = 0; i < batch; ++i) {
      const unsigned long long* s = c->h_stats + (size_t)((t0 + i) % kStatSlots) * kStatFields;
      const bool poll = every_tick_polls || done + i + 1 == ticks;
      median_account(c, t0 + i, s, poll, out ? &out[done + i] : nullptr);
    }
    if (b.h_ctl->received != c->recv || b.h_ctl->rlen != c->pending)
      return fail(c, GS_EDEVICE, "the median control block and the stats rows disagree");
    done += batch;
  }
  return GS_OK;
}

// The run goes to its own end: it stops at the first poll with no active node
// (the device's stop word: covered or quiescent by the float32 rule at that
// poll), or at max_ticks.  Reaching 99 % does not stop it.
int median_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
               int32_t* status) {
  if (!c->begun) return fail(c, GS_EINVAL, "gs_broadcast_begin first");
  size_t k = 0;
  int32_t st = GS_RUN_MAX_TICKS;
  uint64_t f0 = c->fired, s0 = c->sent, m0 = c->msgs;
  for (;;) {
    RC(median_step(c, poll, nullptr, false));
    if (out && k < cap)
      out[k] = gs_tick_stats{c->t, c->fired - f0, c->sent - s0, c->msgs - m0, c->recv, 0, c->pending};
    ++k;
    f0 = c->fired; s0 = c->sent; m0 = c->msgs;
    if (c->md.h_ctl->stop) { st = (int32_t)c->md.h_ctl->stop - 1; break; }
    if (c->t >= max_ticks) break;
  }
  snap_trial(c, 0, st);
  if (nout) *nout = k;
  if (status) *status = st;
  return GS_OK;
}

// removed = the D set, built from the state bytes.
int median_read_removed(gs_ctx* c, uint64_t* words, size_t nwords) {
  if (!words || nwords < c->st.W) return fail(c, GS_EINVAL, "need ceil(n/64) words");
  CK(c, hipSetDevice(c->dev));
  if (!grow(c->md.done, c->st.W * 8)) return fail(c, GS_ENOMEM, "cannot allocate the done set");
  unsigned long long* d = (unsigned long long*)c->md.done.p;
  if (c->begun) CK(c, median_done_set(c->st, median_state(c), d, c->stream));
  else CK(c, hipMemsetAsync(d, 0, c->st.W * 8, c->stream));  // (st is the last run's: nothing is informed)
  CK(c, hipMemcpyAsync(words, d, c->st.W * 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

int median_read_state(gs_ctx* c, uint8_t* st, size_t n) {
  if (!c->median) return fail(c, GS_EINVAL, "gs_read_median_state needs a GS_MODEL_MEDIAN context");
  if (!st || n < c->p.n) return fail(c, GS_EINVAL, "need n bytes");
  CK(c, hipSetDevice(c->dev));
  if (!c->begun) {  // (st is the last run's: every node is uninformed)
    memset(st, 0, c->p.n);
    return GS_OK;
  }
  CK(c, hipMemcpyAsync(st, c->md.st.p, c->p.n, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

}  // namespace gs
