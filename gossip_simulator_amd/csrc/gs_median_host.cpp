// gs_median_host.cpp -- the host side of median-counter push-pull
// (GS_MODEL_MEDIAN): its buffers and what it gives the
// shared round loop (gs_round_host.cpp: the step loop and gs_run's stop rule).
// One trial on one device (the kernels are in gs_median.hip), or a batch of
// trials, a workgroup each (gs_create_batch; gs_median_trials.hip).
#include "gs_ctx.h"

namespace gs {

namespace {

MedianState median_state(const gs_ctx* c) {
  return MedianState{(RumorCtl*)c->md.ctlb.p, (uint8_t*)c->md.st.p, (uint8_t*)c->md.own.p,
                     (unsigned long long*)c->md.tally.p, (unsigned long long*)c->md.gotb.p,
                     (unsigned long long*)c->md.gotc.p, c->p.rumor_k};
}

// What the shared round loop (gs_round_host.cpp) runs for this context; rlen
// holds the active nodes after the round.
RoundEngine median_engine(gs_ctx* c) {
  const MedianState ms = median_state(c);
  RumorCtl* h = c->md.h_ctl;
  RoundEngine e{};
  e.name = "median";
  e.round = [c, ms](uint32_t tt) -> int {
    CK(c, median_round(c->st, ms, tt, c->md.grid, c->stream));
    return GS_OK;
  };
  e.commit = [c, ms](uint32_t tt) -> int {
    CK(c, median_commit(c->st, ms, tt, c->stream));
    return GS_OK;
  };
  e.ctl = RoundCtl{c->md.ctlb.p, h, sizeof(RumorCtl), &h->received, &h->rlen, &h->stop};
  return e;
}

// ---- batched trials --------------------------------

MdtState mdt_state(const gs_ctx* c) {
  MdtState m{};
  m.deg = c->st.deg;
  m.ids = c->st.ids;
  m.recv = c->st.recv;
  m.st = (uint8_t*)c->md.st.p;
  m.crash = c->failed ? c->st.crash : nullptr;
  m.tstat = c->bt.d_tstat;
  m.n = (uint32_t)c->p.n;
  m.trials = c->trials;
  m.tlog = c->tlog;
  m.stride = c->st.stride;
  m.block = c->mplan.block;
  m.lds_bytes = (uint32_t)c->mplan.lds_bytes;
  m.k = c->p.rumor_k;
  m.kd = c->st.kd;
  m.key = c->st.key;
  return m;
}

// The packed tallies' in-degree guard, once per
// table: with n <= kMdt16MaxNamed the callers of a round are too few to
// overflow a field whatever the table; past that, no node may be named by more
// than kMdt16MaxNamed used slots of its trial's table (slots, not rows: a
// conservative count).  Counted on the device a chunk of trials at a time, a
// u32 per padded node, in scratch that is released before the answer.
int mdt_check_named(gs_ctx* c, const MdtState& ms) {
  if (c->p.n <= kMdt16MaxNamed) return GS_OK;
  const uint64_t per = 1ull << c->tlog;
  const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c->trials, (64ull << 20) / (per * 4)));
  uint32_t* cnt = nullptr;
  if (dev_malloc((void**)&cnt, (size_t)chunk * per * 4 + 8) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the in-degree count of a packed median batch");
  unsigned long long* d_worst = (unsigned long long*)(cnt + (size_t)chunk * per);
  unsigned long long worst = ~0ull;
  uint32_t count = 0, t_lo = 0;
  hipError_t e = hipSuccess;
  for (; t_lo < c->trials && e == hipSuccess && worst == ~0ull; t_lo += chunk) {
    const uint32_t t_hi = std::min<uint32_t>(c->trials, t_lo + chunk);
    e = hipMemsetAsync(cnt, 0, (size_t)(t_hi - t_lo) * per * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_worst, 0xFF, 8, c->stream);
    if (e == hipSuccess) e = mdt_count_named(ms, t_lo, t_hi, kMdt16MaxNamed, cnt, d_worst, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&worst, d_worst, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && worst != ~0ull) {
      e = hipMemcpy(&count, cnt + worst, 4, hipMemcpyDeviceToHost);
      worst += (uint64_t)t_lo * per;
    }
  }
  (void)dev_free(cnt);
  CK(c, e);
  if (worst == ~0ull) return GS_OK;
  return fail(c, GS_EINVAL,
              "GS_FLAG_MEDIAN_PACKED keeps 16-bit tallies: trial " + std::to_string(c->p.trial + (worst >> c->tlog)) +
                  " (index " + std::to_string(worst >> c->tlog) + "): node " + std::to_string(worst & (per - 1)) +
                  " is named by " + std::to_string(count) + " used slots of its table, more than the " +
                  std::to_string(kMdt16MaxNamed) + " a packed batch takes; load another table, or run the batch " +
                  "without the flag (n <= gs_median_trials_max_n)");
}

// Every trial's sender (k_mdt_seed): the trials that started have one informed,
// active node.  The started flags use the first words of the counter rows,
// free between broadcasts.
int mdt_begin(gs_ctx* c, uint64_t sender) {
  CK(c, hipSetDevice(c->dev));
  const uint32_t T = c->trials;
  const MdtState ms = mdt_state(c);
  if (c->mdt16 && !c->named_ok) {
    RC(mdt_check_named(c, ms));
    c->named_ok = true;
  }
  CK(c, hipMemsetAsync(c->md.st.p, 0, c->st.n, c->stream));
  CK(c, mdt_seed(ms, (uint32_t)sender, c->bt.d_tstat, c->stream));
  CK(c, hipMemcpyAsync(c->bt.h_tstat, c->bt.d_tstat, (size_t)T * 4, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  c->recv = c->pending = 0;
  for (uint32_t tr = 0; tr < T; ++tr) {
    c->bt.live[tr] = c->bt.h_tstat[tr];
    c->tacc[tr].start = c->tacc[tr].recv = c->bt.h_tstat[tr];
    c->recv += c->tacc[tr].recv;
    c->pending += c->bt.live[tr];
  }
  c->begun = true;
  return GS_OK;
}

// The batch's rounds on the shared loops (gs_trials_host.cpp): the launcher,
// and a row's messages = the active ends of the round's connections.
TrialLaunch mdt_launch(gs_ctx* c) {
  return [c, ms = mdt_state(c)](uint64_t t0, uint32_t batch) -> int {
    CK(c, mdt_rounds(ms, c->mdt16, (uint32_t)t0, batch, c->stream));
    return GS_OK;
  };
}
uint64_t mdt_row_msgs(const uint32_t* r) { return r[TS_MSGS]; }

// The D set of every trial, built from the state bytes over the padded id
// space (padding bytes are 0); trials x ceil(n/64) words, trial-major.
int mdt_read_removed(gs_ctx* c, uint64_t* words, size_t nwords) {
  const uint64_t Wn = (c->p.n + 63) / 64;
  if (!words || nwords < Wn * c->trials) return fail(c, GS_EINVAL, "need ceil(n/64) words per trial");
  CK(c, hipSetDevice(c->dev));
  if (!grow(c->md.done, c->st.W * 8)) return fail(c, GS_ENOMEM, "cannot allocate the done set");
  unsigned long long* d = (unsigned long long*)c->md.done.p;
  MedianState m{};
  m.st = (uint8_t*)c->md.st.p;
  if (c->begun) CK(c, median_done_set(c->st, m, d, c->stream));
  else CK(c, hipMemsetAsync(d, 0, c->st.W * 8, c->stream));  // (st is the last run's: nothing is informed)
  return trial_read_words(c, words, d);
}

// trials * n bytes, trial-major, without the padding of the internal layout.
int mdt_read_state(gs_ctx* c, uint8_t* st, size_t n) {
  const size_t need = (size_t)c->trials * c->p.n;
  if (!st || n < need) return fail(c, GS_EINVAL, "need trials * n bytes (trial-major)");
  CK(c, hipSetDevice(c->dev));
  if (!c->begun) {  // (st is the last run's: every node is uninformed)
    memset(st, 0, need);
    return GS_OK;
  }
  CK(c, hipMemcpy2DAsync(st, c->p.n, c->md.st.p, (size_t)1 << c->tlog, c->p.n, c->trials, hipMemcpyDeviceToHost,
                         c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

}  // namespace

// mdt_lds_limit with its failure in words ("" on success).
std::string mdt_limit_error(int device, bool packed, uint64_t* lim) {
  const char* where = "";
  const hipError_t e = mdt_lds_limit(device, packed, lim, &where);
  return trial_limit_error(where, device, e);
}

// Batched median trials (gs_create_batch): n is bounded by what `device`
// grants one workgroup (gs_mdt_plan.h), so it is validated with the other
// parameters, after check_params and before any device state is set up; *pl
// gets the plan (block 0: not such a context).  With no device to ask the
// parameters were valid as far as they can be checked: GS_EDEVICE.
// GS_FLAG_MEDIAN_PACKED is read here and nowhere else: gs_create_batch
// (median_trials) makes the batch on the packed plan (*packed); every other
// create and model never looks at the bit.
int check_mdt_n(const gs_params* p, bool median_trials, int device, std::string& why, MdtPlan* pl, bool* packed) {
  *pl = MdtPlan{};
  *packed = false;
  if (p->trials <= 1 || p->model != GS_MODEL_MEDIAN) return GS_OK;
  const bool p16 = median_trials && (p->flags & GS_FLAG_MEDIAN_PACKED) != 0;
  RC(trial_device_check(device, why));
  uint64_t lim = 0;
  why = mdt_limit_error(device, p16, &lim);
  if (!why.empty()) {
    (void)hipGetLastError();
    return GS_EDEVICE;
  }
  const MdtPlan plan = p16 ? mdt16_plan(p->n, lim) : mdt_plan(p->n, lim);
  if (!plan.fits && p16) {
    why = "a packed median batch (GS_FLAG_MEDIAN_PACKED) keeps a trial's state bytes, 16-bit tallies and flag sets "
          "in one workgroup's LDS: n must be <= " + std::to_string(mdt16_max_n(lim)) +
          " on this device (gs_median_trials_max_n_packed), not " + std::to_string(p->n) +
          "; a one-trial context (gs_create) has no such limit";
    return GS_EINVAL;
  }
  if (!plan.fits) {
    why = "batched median trials keep a trial's state bytes, tallies and flag sets in one workgroup's LDS: n must "
          "be <= " + std::to_string(mdt_max_n(lim)) + " on this device (gs_median_trials_max_n), not " +
          std::to_string(p->n) + "; a one-trial context (gs_create) has no such limit";
    return GS_EINVAL;
  }
  if (plan.lds_bytes > 65536 && mdt_prepare(device, p16, (uint32_t)plan.lds_bytes) != hipSuccess) {
    (void)hipGetLastError();
    why = "cannot raise the trial-resident median kernel's dynamic LDS limit";
    return GS_EDEVICE;
  }
  *pl = plan;
  *packed = p16;
  return GS_OK;
}

// gs_load_peers_device on a batch: the trials' tables back to back in device
// memory, spread into the padded id space and validated on the device.
int mdt_load_device(gs_ctx* c, const void* d_deg, const void* d_ids, uint32_t stride) {
  CK(c, hipSetDevice(c->dev));
  c->row_slots = 0;
  RC(alloc_table(c, stride));
  CK(c, hipMemsetAsync(c->d_deg, 0, c->ntot, c->stream));
  CK(c, hipMemsetAsync(c->d_ids, 0, c->ntot * stride * 4ull, c->stream));
  CK(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
  CK(c, mdt_spread_table((const uint8_t*)d_deg, (const uint32_t*)d_ids, (uint32_t)c->p.n, c->trials, c->tlog, stride,
                         c->d_deg, c->d_ids, c->d_err, c->stream));
  uint32_t e = 0;
  CK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  CK(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
  if (e & 1) return fail(c, GS_EINVAL, "a friends-list length exceeds the row stride");
  if (e & 2) return fail(c, GS_EINVAL, "a friend id is >= n");
  return seal_rows(c, c->d_deg, c->d_ids, c->ntot);
}

// The combinations the model does not run: every create but gs_create and
// gs_create_batch.
int median_refuse(const gs_params* params, const char* what) {
  if (!params || params->model != GS_MODEL_MEDIAN) return GS_OK;
  g_create_err = std::string(what) + " with GS_MODEL_MEDIAN: the median-counter model runs one trial on one device "
                 "(gs_create), or a batch of trials through gs_create_batch";
  fprintf(stderr, "%s: %s\n", what, g_create_err.c_str());
  return GS_EINVAL;
}

// Nothing of the flood's window buffers, push-pull's reverse table or the
// rumor model's lists: the state bytes, the own-contribution bytes, the tally
// and two bitsets.  At n = 1e9: 1 + 1 + 8 GB and 2 x 125 MB, from the block
// cache like every buffer of 64 MiB or more.  A batched context keeps the
// rest in LDS: the state bytes over the padded id space only.
int median_alloc(gs_ctx* c) {
  const uint64_t n = c->st.n;
  MedianBufs& b = c->md;
  if (c->mdt) {
    if (!grow(b.st, n)) return fail(c, GS_ENOMEM, "cannot allocate the batched median trials' state bytes");
    c->bt.live.assign(c->trials, 0);
    return GS_OK;
  }
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
  if (c->mdt) return mdt_begin(c, sender);
  CK(c, hipSetDevice(c->dev));
  // GS_MEDIAN_GRID: the round kernel's blocks (read per broadcast, so tests can
  // make a short table take several passes of the grid)
  MedianBufs& b = c->md;
  b.grid = median_grid(c->st.n, env_grid("GS_MEDIAN_GRID"));
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

// The rounds and the run on the shared loop (gs_round_host.cpp; a batch's on
// gs_trials_host.cpp's).  The run stops at the first poll with no active node
// (covered or quiescent by the float32 rule at that poll), or at max_ticks.
// Reaching 99 % does not stop it.
int median_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls) {
  if (c->mdt) return trial_step(c, ticks, out, every_tick_polls, mdt_launch(c), mdt_row_msgs);
  return round_step(c, ticks, out, every_tick_polls, median_engine(c));
}

int median_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
               int32_t* status) {
  if (!c->begun) return fail(c, GS_EINVAL, "gs_broadcast_begin first");
  if (c->mdt) return trial_run(c, poll, max_ticks, out, cap, nout, status, mdt_launch(c), mdt_row_msgs);
  return round_run(c, poll, max_ticks, out, cap, nout, status, median_engine(c));
}

// removed = the D set, built from the state bytes.
int median_read_removed(gs_ctx* c, uint64_t* words, size_t nwords) {
  if (c->mdt) return mdt_read_removed(c, words, nwords);
  if (!words || nwords < c->st.W) return fail(c, GS_EINVAL, "need ceil(n/64) words");
  CK(c, hipSetDevice(c->dev));
  if (!grow(c->md.done, c->st.W * 8)) return fail(c, GS_ENOMEM, "cannot allocate the done set");
  unsigned long long* d = (unsigned long long*)c->md.done.p;
  if (c->begun) CK(c, median_done_set(c->st, median_state(c), d, c->stream));
  else CK(c, hipMemsetAsync(d, 0, c->st.W * 8, c->stream));  // (st is the last run's: nothing is informed)
  return read_words(c, words, d);
}

int median_read_state(gs_ctx* c, uint8_t* st, size_t n) {
  if (!c->median) return fail(c, GS_EINVAL, "gs_read_median_state needs a GS_MODEL_MEDIAN context");
  if (c->mdt) return mdt_read_state(c, st, n);
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
