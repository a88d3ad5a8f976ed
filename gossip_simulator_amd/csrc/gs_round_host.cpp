// gs_round_host.cpp -- the host scaffold of the one-trial engines that end by
// themselves (rumor mongering, median-counter push-pull, the rumor set;
// DESIGN.md section 4.11): the step loop over rounds of two launches, its
// read-back and accounting, and gs_run's loop on the device's stop word.  An
// engine supplies a RoundEngine: its two launchers, its control block and, the
// rumor set only, a second ring and a row hook (gs_rumor_host.cpp,
// gs_median_host.cpp, gs_rumorset_host.cpp).
#include "gs_ctx.h"

namespace gs {

uint32_t env_grid(const char* name) {
  const char* e = getenv(name);
  return e ? (uint32_t)std::min(std::max(atoi(e), 1), 4096) : 0u;
}

int read_words(gs_ctx* c, uint64_t* words, const unsigned long long* d) {
  CK(c, hipMemcpyAsync(words, d, c->st.W * 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

namespace {

// The round's counters on the host: c's cumulative figures and its one
// TrialAcc.  tick_99 is taken at polls only: `poll` says this tick is one.
// An engine with a row hook takes its own tick_99 there.
void round_account(gs_ctx* c, const RoundEngine& e, uint64_t tick, bool poll, gs_tick_stats* o) {
  const size_t slot = (size_t)(tick % kStatSlots);
  const unsigned long long* s = c->h_stats + slot * kStatFields;
  c->t = tick;
  c->fired += s[ST_FIRED];
  c->sent += s[ST_SENT];
  c->msgs += s[ST_MSGS];
  c->recv += s[ST_RECV];
  c->pending = s[ST_SCHED];  // the hot (active) nodes, or the uncovered rumors, after the round
  TrialAcc& a = c->tacc[0];
  a.fired = c->fired; a.sent = c->sent; a.msgs = c->msgs; a.recv = c->recv;
  if (e.row) e.row(tick, e.ring.words ? e.ring.h + slot * e.ring.words : nullptr, poll);
  else if (poll && !a.tick99 && covered(a.recv, c->p.n)) a.tick99 = tick;
  if (o) *o = gs_tick_stats{c->t, s[ST_FIRED], s[ST_SENT], s[ST_MSGS], c->recv, 0, c->pending};
}

}  // namespace

// `ticks` rounds, enqueued without a host sync between them; the stats rows,
// the second ring's slots and the control block come back once per call (per
// kStatSlots rounds; per 256 with GS_FLAG_TIMING, three events a round).
// every_tick_polls: each tick is a poll (gs_step returns every tick's row);
// else only the call's last tick is (gs_run).
int round_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls, const RoundEngine& e) {
  CK(c, hipSetDevice(c->dev));
  const bool timing = (c->p.flags & GS_FLAG_TIMING) != 0;
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
      RC(e.round(tt));
      if (ev) CK(c, hipEventRecord(ev[1], c->stream));
      RC(e.commit(tt));
      if (ev) CK(c, hipEventRecord(ev[2], c->stream));
    }
    for (int j = 0; j < sp.n; ++j) {
      CK(c, hipMemcpyAsync(c->h_stats + sp.off[j], c->st.stats + sp.off[j], sp.words[j] * 8, hipMemcpyDeviceToHost,
                           c->stream));
      if (!e.ring.words) continue;  // a ring slot is ring.words words where a stats row is kStatFields
      const size_t off = sp.off[j] / kStatFields * e.ring.words, words = sp.words[j] / kStatFields * e.ring.words;
      CK(c, hipMemcpyAsync(e.ring.h + off, e.ring.d + off, words * 8, hipMemcpyDeviceToHost, c->stream));
    }
    CK(c, hipMemcpyAsync(e.ctl.h, e.ctl.d, e.ctl.bytes, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < batch && timing; ++i) {
      float ms = 0;
      CK(c, hipEventElapsedTime(&ms, c->ev[(size_t)i * 3], c->ev[(size_t)i * 3 + 1]));
      c->timing.deliver_ms += ms;  // the round kernel
      c->timing.deliver_launches++;
      CK(c, hipEventElapsedTime(&ms, c->ev[(size_t)i * 3 + 1], c->ev[(size_t)i * 3 + 2]));
      c->timing.resolve_ms += ms;  // commit + publish
      c->timing.resolve_launches++;
    }
    for (uint32_t i = 0; i < batch; ++i) {
      const bool poll = every_tick_polls || done + i + 1 == ticks;
      round_account(c, e, t0 + i, poll, out ? &out[done + i] : nullptr);
    }
    if (*e.ctl.received != c->recv || *e.ctl.pending != c->pending)
      return fail(c, GS_EDEVICE, std::string("the ") + e.name + " control block and the stats rows disagree");
    done += batch;
  }
  return GS_OK;
}

// The run goes to the engine's own end: it stops at the first poll at which
// the device's stop word is set (kRumorCovered / kRumorQuiescent: the run
// status plus one), or at max_ticks.
int round_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
              int32_t* status, const RoundEngine& e) {
  size_t k = 0;
  int32_t st = GS_RUN_MAX_TICKS;
  uint64_t f0 = c->fired, s0 = c->sent, m0 = c->msgs;
  for (;;) {
    RC(round_step(c, poll, nullptr, false, e));
    if (out && k < cap)
      out[k] = gs_tick_stats{c->t, c->fired - f0, c->sent - s0, c->msgs - m0, c->recv, 0, c->pending};
    ++k;
    f0 = c->fired; s0 = c->sent; m0 = c->msgs;
    if (*e.ctl.stop) { st = (int32_t)*e.ctl.stop - 1; break; }
    if (c->t >= max_ticks) break;
  }
  snap_trial(c, 0, st);
  if (nout) *nout = k;
  if (status) *status = st;
  return GS_OK;
}

}  // namespace gs
