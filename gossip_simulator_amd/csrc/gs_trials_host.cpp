// gs_trials_host.cpp -- the host scaffold of the trial-resident engines
// (batched push-pull, rumor and median trials): what a
// device grants their rounds kernels, and the step and run loops over the
// per-trial counter rows.  An engine supplies its launcher and how a row
// yields its messages (gs_rumor_host.cpp, gs_median_host.cpp).  The one-trial
// rumor, median and rumor-set engines have their loop in gs_round_host.cpp.
#include "gs_ctx.h"

namespace gs {

hipError_t trial_lds_limit(int device, const void* kernel, uint64_t* limit, const char** where) {
  int dev0 = 0, v = 0;
  const char* dummy;
  if (!where) where = &dummy;
  *where = "hipGetDevice";
  hipError_t e = hipGetDevice(&dev0);
  if (e != hipSuccess) return e;
  *where = "hipSetDevice";
  if ((e = hipSetDevice(device)) != hipSuccess) return e;
  *where = "hipDeviceGetAttribute(MaxSharedMemoryPerBlock)";
  e = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
  if (e == hipSuccess) {
    uint64_t lim = v > 0 ? (uint64_t)v : 0;
    if (lim > 65536) {
      int nb = 0;
      (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lim);
      const hipError_t oe =
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, (int)kTrialMaxBlock, (size_t)lim);
      if (oe != hipSuccess || nb < 1) {
        (void)hipGetLastError();
        lim = 65536;
      }
    }
    *limit = lim;
  }
  (void)hipSetDevice(dev0);
  return e;
}

hipError_t trial_raise_lds(int device, const void* const* kernels, uint32_t count, uint32_t bytes) {
  int dev0 = 0;
  hipError_t e = hipGetDevice(&dev0);
  if (e != hipSuccess) return e;
  if ((e = hipSetDevice(device)) != hipSuccess) return e;
  for (uint32_t i = 0; i < count; ++i) {
    e = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) break;
  }
  (void)hipSetDevice(dev0);
  return e;
}

// A *_lds_limit's failure in words ("" on success): the HIP call that failed
// and the runtime's error string.
std::string trial_limit_error(const char* where, int device, hipError_t e) {
  if (e == hipSuccess) return std::string();
  return std::string(where) + " on device " + std::to_string(device) + ": " + hipGetErrorString(e) + " (hipError_t " +
         std::to_string((int)e) + ")";
}

// Is there a device to ask, and is `device` one of them?  With none the
// parameters were valid as far as they can be checked: GS_EDEVICE.
int trial_device_check(int device, std::string& why) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    why = "no HIP device visible (libgossip_hip needs an MI355X)";
    return GS_EDEVICE;
  }
  if (device < 0 || device >= ndev) {
    why = "device " + std::to_string(device) + " out of range (" + std::to_string(ndev) + " visible)";
    return GS_EDEVICE;
  }
  return GS_OK;
}

// `ticks` rounds of every trial, at most kMaxWindow per launch (launch(t0,
// batch): the engine's rounds kernel on c->stream); out[k] = the sum of the
// trials' rows, pending = their live nodes (TS_HOT, kept per trial in
// c->bt.live).  tick_99 is taken at polls only: every tick, or only the
// call's last.
int trial_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls,
               const TrialLaunch& launch, uint64_t (*row_msgs)(const uint32_t* r)) {
  CK(c, hipSetDevice(c->dev));
  const bool timing = (c->p.flags & GS_FLAG_TIMING) != 0;
  const size_t tb = (size_t)c->trials * kMaxWindow * kTStatFields * 4;
  while (timing && c->ev.size() < 2) {
    hipEvent_t ev;
    CK(c, hipEventCreate(&ev));
    c->ev.push_back(ev);
  }
  uint32_t done = 0;
  while (done < ticks) {
    const uint32_t batch = std::min<uint32_t>(ticks - done, kMaxWindow);
    const uint64_t t0 = c->t + 1;
    if (timing) CK(c, hipEventRecord(c->ev[0], c->stream));
    RC(launch(t0, batch));
    if (timing) CK(c, hipEventRecord(c->ev[1], c->stream));
    CK(c, hipMemcpyAsync(c->bt.h_tstat, c->bt.d_tstat, tb, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    if (timing) {
      float ms = 0;
      CK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
      c->timing.deliver_ms += ms;  // the rounds kernel: `batch` rounds of every trial
      c->timing.deliver_launches++;
    }
    for (uint32_t k = 0; k < batch; ++k) {
      const bool poll = every_tick_polls || done + k + 1 == ticks;
      unsigned long long fired = 0, sent = 0, msgs = 0, live = 0;
      for (uint32_t tr = 0; tr < c->trials; ++tr) {
        const uint32_t* r = c->bt.h_tstat + ((size_t)tr * kMaxWindow + k) * kTStatFields;
        const uint64_t m = row_msgs(r);
        TrialAcc& a = c->tacc[tr];
        a.fired += r[TS_FIRED];
        a.sent += r[TS_SENT];
        a.msgs += m;
        a.recv += r[TS_RECV];
        if (poll && !a.tick99 && covered(a.recv, c->p.n)) a.tick99 = t0 + k;
        c->bt.live[tr] = r[TS_HOT];
        fired += r[TS_FIRED];
        sent += r[TS_SENT];
        msgs += m;
        c->recv += r[TS_RECV];
        live += r[TS_HOT];
      }
      c->t = t0 + k;
      c->fired += fired;
      c->sent += sent;
      c->msgs += msgs;
      c->pending = live;
      if (out) out[done + k] = gs_tick_stats{c->t, fired, sent, msgs, c->recv, 0, c->pending};
    }
    done += batch;
  }
  return GS_OK;
}

// gs_run's rule per trial: a trial stops at the first poll at which it has no
// live node (covered or quiescent by the float32 rule at that poll), else at
// max_ticks; the run ends when all have stopped.
int trial_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
              int32_t* status, const TrialLaunch& launch, uint64_t (*row_msgs)(const uint32_t* r)) {
  size_t k = 0;
  int32_t st = GS_RUN_MAX_TICKS;
  uint64_t f0 = c->fired, s0 = c->sent, m0 = c->msgs;
  for (;;) {
    RC(trial_step(c, poll, nullptr, false, launch, row_msgs));
    if (out && k < cap)
      out[k] = gs_tick_stats{c->t, c->fired - f0, c->sent - s0, c->msgs - m0, c->recv, 0, c->pending};
    ++k;
    f0 = c->fired; s0 = c->sent; m0 = c->msgs;
    uint32_t running = 0;
    for (uint32_t tr = 0; tr < c->trials; ++tr) {
      TrialAcc& a = c->tacc[tr];
      if (a.status != GS_RUN_RUNNING) continue;
      if (c->bt.live[tr] == 0) snap_trial(c, tr, covered(a.recv, c->p.n) ? GS_RUN_COVERED : GS_RUN_QUIESCENT);
      else if (c->t >= max_ticks) snap_trial(c, tr, GS_RUN_MAX_TICKS);
      else ++running;
    }
    if (trials_stopped(c, running, &st)) break;
  }
  if (nout) *nout = k;
  if (status) *status = st;
  return GS_OK;
}

// A bitset d over the padded id space, read back as trials x ceil(n/64) words, trial-major.
int trial_read_words(gs_ctx* c, uint64_t* words, const unsigned long long* d) {
  const uint64_t Wn = (c->p.n + 63) / 64;
  CK(c, hipMemcpy2DAsync(words, Wn * 8, d, ((size_t)1 << c->tlog) / 8, Wn * 8, c->trials, hipMemcpyDeviceToHost,
                         c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

}  // namespace gs
