// gs_rumor_host.cpp -- the host side of rumor mongering (GS_MODEL_RUMOR,
// DESIGN.md section 4.7): its buffers and what it gives the shared round loop
// (gs_round_host.cpp: the step loop and gs_run's stop rule).
// One trial on one device (the kernels are in gs_rumor.hip), or a batch of
// trials, a workgroup each (gs_create_trials; gs_rumor_trials.hip).
#include "gs_ctx.h"

namespace gs {

namespace {

static_assert(kRumorBlind == GS_RUMOR_BLIND && kRumorCoin == GS_RUMOR_COIN && kRumorPull == GS_RUMOR_PULL,
              "the kernels' mode bits are gossip.h's");

RumorState rumor_state(const gs_ctx* c) {
  return RumorState{(RumorCtl*)c->rm.ctlb.p, c->d_next, (uint8_t*)c->rm.miss.p, c->p.rumor_k, c->p.rumor_mode,
                    (unsigned long long*)c->rm.hot.p, (unsigned long long*)c->rm.served.p,
                    (unsigned long long*)c->rm.vain.p};
}

bool pull(const gs_ctx* c) { return (c->p.rumor_mode & GS_RUMOR_PULL) != 0; }

// What the shared round loop (gs_round_host.cpp) runs for this context: the
// dense round of the pull modes, or the list round, which swaps the two lists
// after its commit.
RoundEngine rumor_engine(gs_ctx* c) {
  const RumorState rs = rumor_state(c);
  const bool dense = pull(c);
  RumorCtl* h = c->rm.h_ctl;
  RoundEngine e{};
  e.name = "rumor";
  e.round = [c, rs, dense](uint32_t tt) -> int {
    if (dense)
      CK(c, rumor_pull_round(c->st, rs, tt, c->rm.grid, c->stream));
    else
      CK(c, rumor_round(c->st, rs, (const uint32_t*)c->rm.list[c->rm.cur].p, (uint32_t*)c->rm.list[c->rm.cur ^ 1].p,
                        tt, c->rm.grid, c->stream));
    return GS_OK;
  };
  e.commit = [c, rs, dense](uint32_t tt) -> int {
    CK(c, dense ? rumor_pull_commit(c->st, rs, tt, c->stream) : rumor_commit(c->st, rs, tt, c->stream));
    c->rm.cur ^= 1;
    return GS_OK;
  };
  e.ctl = RoundCtl{c->rm.ctlb.p, h, sizeof(RumorCtl), &h->received, &h->rlen, &h->stop};
  return e;
}

// ---- batched trials --------------------------------

RmtState rmt_state(const gs_ctx* c) {
  RmtState r{};
  r.deg = c->st.deg;
  r.ids = c->st.ids;
  r.recv = c->st.recv;
  r.hot = (unsigned long long*)c->rm.hot.p;
  r.miss = (uint8_t*)c->rm.miss.p;
  r.crash = c->failed ? c->st.crash : nullptr;
  r.tstat = c->bt.d_tstat;
  r.nhot = (uint32_t*)c->rm.tri.p;
  r.n = (uint32_t)c->p.n;
  r.trials = c->trials;
  r.tlog = c->tlog;
  r.stride = c->st.stride;
  r.block = c->rplan.block;
  r.lds_bytes = (uint32_t)c->rplan.lds_bytes;
  r.k = c->p.rumor_k;
  r.mode = c->p.rumor_mode;
  r.kd = c->st.kd;
  r.key = c->st.key;
  return r;
}

// Every trial's sender (k_rmt_seed): the trials that started are informed, and
// the hot counts come back with them.
int rmt_begin(gs_ctx* c, uint64_t sender) {
  CK(c, hipSetDevice(c->dev));
  const uint32_t T = c->trials;
  const RmtState rs = rmt_state(c);
  uint32_t* started = rs.nhot + T;
  CK(c, hipMemsetAsync(c->rm.hot.p, 0, c->st.W * 8, c->stream));
  CK(c, hipMemsetAsync(c->rm.miss.p, 0, c->st.n, c->stream));
  CK(c, rmt_seed(rs, (uint32_t)sender, started, c->stream));
  CK(c, hipMemcpyAsync(c->bt.h_tstat, rs.nhot, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  c->recv = c->pending = 0;
  for (uint32_t tr = 0; tr < T; ++tr) {
    c->bt.live[tr] = c->bt.h_tstat[tr];
    c->tacc[tr].start = c->tacc[tr].recv = c->bt.h_tstat[T + tr];
    c->recv += c->tacc[tr].recv;
    c->pending += c->bt.live[tr];
  }
  c->begun = true;
  return GS_OK;
}

// The batch's rounds on the shared loops (gs_trials_host.cpp): the launcher,
// and a row's messages = the kept calls less those to a failed callee.
TrialLaunch rmt_launch(gs_ctx* c) {
  return [c, rs = rmt_state(c)](uint64_t t0, uint32_t batch) -> int {
    CK(c, rmt_rounds(rs, (uint32_t)t0, batch, c->stream));
    return GS_OK;
  };
}
uint64_t rmt_row_msgs(const uint32_t* r) { return (uint64_t)r[TS_SENT] - r[TS_DEAD]; }

// removed = recv & ~hot in every mode of the batch; trials x ceil(n/64) words, trial-major.
int rmt_read_removed(gs_ctx* c, uint64_t* words, size_t nwords) {
  const uint64_t Wn = (c->p.n + 63) / 64;
  if (!words || nwords < Wn * c->trials) return fail(c, GS_EINVAL, "need ceil(n/64) words per trial");
  CK(c, hipSetDevice(c->dev));
  if (!grow(c->rm.removed, c->st.W * 8)) return fail(c, GS_ENOMEM, "cannot allocate the removed set");
  unsigned long long* d = (unsigned long long*)c->rm.removed.p;
  RumorState r{};
  r.hot = (unsigned long long*)c->rm.hot.p;
  if (c->begun) CK(c, rumor_pull_removed(c->st, r, d, c->stream));
  else CK(c, hipMemsetAsync(d, 0, c->st.W * 8, c->stream));  // (hot is the last run's: nothing is informed)
  return trial_read_words(c, words, d);
}

}  // namespace

// rmt_lds_limit with its failure in words ("" on success).
std::string rmt_limit_error(int device, uint32_t mode, uint64_t* lim) {
  const char* where = "";
  const hipError_t e = rmt_lds_limit(device, mode, lim, &where);
  return trial_limit_error(where, device, e);
}

// Batched rumor trials (gs_create_trials): n is bounded by what `device`
// grants one workgroup (gs_rmt_plan.h), so it is validated with the other
// parameters, after check_params and before any device state is set up; *pl
// gets the plan (block 0: not such a context).  With no device to ask the
// parameters were valid as far as they can be checked: GS_EDEVICE.
int check_rmt_n(const gs_params* p, int device, std::string& why, RmtPlan* pl) {
  *pl = RmtPlan{};
  if (p->trials <= 1 || p->model != GS_MODEL_RUMOR) return GS_OK;
  RC(trial_device_check(device, why));
  uint64_t lim = 0;
  why = rmt_limit_error(device, p->rumor_mode, &lim);
  if (!why.empty()) {
    (void)hipGetLastError();
    return GS_EDEVICE;
  }
  const RmtPlan plan = rmt_plan(p->n, p->rumor_mode, lim);
  if (!plan.fits) {
    why = "batched rumor trials keep a trial's sets and miss counts in one workgroup's LDS: with rumor_mode " +
          std::to_string(p->rumor_mode) + " n must be <= " + std::to_string(rmt_max_n(p->rumor_mode, lim)) +
          " on this device (gs_rumor_trials_max_n), not " + std::to_string(p->n);
    return GS_EINVAL;
  }
  if (plan.lds_bytes > 65536 && rmt_prepare(device, p->rumor_mode, (uint32_t)plan.lds_bytes) != hipSuccess) {
    (void)hipGetLastError();
    why = "cannot raise the trial-resident rumor kernel's dynamic LDS limit";
    return GS_EDEVICE;
  }
  *pl = plan;
  return GS_OK;
}

// The combinations the model does not run: the creates with more than one
// device or process (trials do not communicate: a caller puts one
// gs_create_trials context per device, with an offset params.trial).
int rumor_refuse(const gs_params* params, const char* what) {
  if (!params || params->model != GS_MODEL_RUMOR) return GS_OK;
  g_create_err = std::string(what) + " with GS_MODEL_RUMOR: the rumor model runs on one device (gs_create, or "
                 "gs_create_trials for a batch of trials)";
  fprintf(stderr, "%s: %s\n", what, g_create_err.c_str());
  return GS_EINVAL;
}

// Nothing of the flood's window buffers or push-pull's reverse table: two
// lists, the miss bytes and the control block.  At n = 1e9: 4 + 4 + 1 GB,
// from the block cache like every buffer of 64 MiB or more.  The pull modes
// have three bitsets (3 x 125 MB) in place of the lists.
// A batched context takes none of the lists: hot and miss over the padded id
// space, and two words per trial.
int rumor_alloc(gs_ctx* c) {
  const uint64_t n = c->st.n;
  if (c->rmt) {
    if (!grow(c->rm.hot, c->st.W * 8) || !grow(c->rm.miss, n) || !grow(c->rm.tri, (size_t)c->trials * 8))
      return fail(c, GS_ENOMEM, "cannot allocate the batched rumor trials' hot sets and miss counts");
    c->bt.live.assign(c->trials, 0);
    return GS_OK;
  }
  const bool sets = pull(c);
  if (sets ? !grow(c->rm.hot, c->st.W * 8) || !grow(c->rm.served, c->st.W * 8) || !grow(c->rm.vain, c->st.W * 8)
           : !grow(c->rm.list[0], n * 4) || !grow(c->rm.list[1], n * 4))
    return fail(c, GS_ENOMEM, sets ? "cannot allocate the rumor model's hot sets"
                                   : "cannot allocate the rumor model's hot lists");
  if (!grow(c->rm.miss, n) || !grow(c->rm.ctlb, sizeof(RumorCtl)) ||
      hipHostMalloc((void**)&c->rm.h_ctl, sizeof(RumorCtl)) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the rumor model's miss counts");
  return GS_OK;
}

// (removed grows at the first gs_read_removed)
void release_rumor(gs_ctx* c) {
  RumorBufs& b = c->rm;
  for (Buf* q : {&b.list[0], &b.list[1], &b.hot, &b.served, &b.vain, &b.miss, &b.ctlb, &b.removed, &b.tri}) release(*q);
  if (b.h_ctl) (void)hipHostFree(b.h_ctl);
}

// The sender is informed unless failed (received = 1, as in push-pull) and
// hot if it has a friend to call.
int rumor_begin(gs_ctx* c, uint64_t sender) {
  if (c->rmt) return rmt_begin(c, sender);
  CK(c, hipSetDevice(c->dev));
  // GS_RUMOR_GRID: the round kernel's blocks (read per broadcast, so tests can
  // make a short list take several passes of the grid)
  c->rm.grid = rumor_grid(c->st.n, env_grid("GS_RUMOR_GRID"));
  c->rm.cur = 0;
  CK(c, hipMemsetAsync(c->rm.ctlb.p, 0, sizeof(RumorCtl), c->stream));
  CK(c, hipMemsetAsync(c->rm.miss.p, 0, c->st.n, c->stream));
  if (pull(c)) {  // a live sender is hot even with an empty row
    for (Buf* q : {&c->rm.hot, &c->rm.served, &c->rm.vain}) CK(c, hipMemsetAsync(q->p, 0, c->st.W * 8, c->stream));
    CK(c, rumor_pull_seed(c->st, rumor_state(c), (uint32_t)sender, cover_threshold(c->p.n), c->stream));
  } else {
    CK(c, rumor_seed(c->st, rumor_state(c), (uint32_t*)c->rm.list[0].p, (uint32_t)sender, cover_threshold(c->p.n),
                     c->stream));
  }
  CK(c, hipMemcpyAsync(c->rm.h_ctl, c->rm.ctlb.p, sizeof(RumorCtl), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  c->recv = c->tacc[0].recv = c->rm.h_ctl->received;
  c->pending = c->rm.h_ctl->rlen;
  c->begun = true;
  return GS_OK;
}

// The rounds and the run on the shared loop (gs_round_host.cpp; a batch's on
// gs_trials_host.cpp's).  The run stops at the first poll with no hot node
// (covered or quiescent by the float32 rule at that poll), or at max_ticks.
// Reaching 99 % does not stop it.
int rumor_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls) {
  if (c->rmt) return trial_step(c, ticks, out, every_tick_polls, rmt_launch(c), rmt_row_msgs);
  return round_step(c, ticks, out, every_tick_polls, rumor_engine(c));
}

int rumor_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
              int32_t* status) {
  if (!c->begun) return fail(c, GS_EINVAL, "gs_broadcast_begin first");
  if (c->rmt) return trial_run(c, poll, max_ticks, out, cap, nout, status, rmt_launch(c), rmt_row_msgs);
  return round_run(c, poll, max_ticks, out, cap, nout, status, rumor_engine(c));
}

// removed = informed and not hot: a copy of recv less the current list's nodes
// (the pull modes: recv & ~hot).
int rumor_read_removed(gs_ctx* c, uint64_t* words, size_t nwords) {
  if (!c->rumor) return fail(c, GS_EINVAL, "gs_read_removed needs a GS_MODEL_RUMOR context");
  if (c->rmt) return rmt_read_removed(c, words, nwords);
  if (!words || nwords < c->st.W) return fail(c, GS_EINVAL, "need ceil(n/64) words");
  CK(c, hipSetDevice(c->dev));
  if (!grow(c->rm.removed, c->st.W * 8)) return fail(c, GS_ENOMEM, "cannot allocate the removed set");
  unsigned long long* d = (unsigned long long*)c->rm.removed.p;
  if (pull(c)) {  // every word written by the kernel (before a broadcast recv is empty)
    CK(c, rumor_pull_removed(c->st, rumor_state(c), d, c->stream));
  } else {
    CK(c, hipMemcpyAsync(d, c->st.recv, c->st.W * 8, hipMemcpyDeviceToDevice, c->stream));
    if (c->begun)  // (before a broadcast recv is empty and the list is the last run's)
      CK(c, rumor_removed(rumor_state(c), (const uint32_t*)c->rm.list[c->rm.cur].p, d, c->rm.grid, c->stream));
  }
  return read_words(c, words, d);
}

}  // namespace gs
