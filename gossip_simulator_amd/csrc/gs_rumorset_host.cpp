// gs_rumorset_host.cpp -- the host side of concurrent push-pull rumors
// (gs_create_rumorset): the create's refusals, the
// buffers, what it gives the shared round loop (gs_round_host.cpp: the step
// loop and gs_run's stop rule) and the per-rumor results.  One device; the
// kernels are in gs_rumorset.hip and gs_rumorset_cap.hip.
#include "gs_ctx.h"

namespace gs {

namespace {

RsState rs_state(const gs_ctx* c) {
  return RsState{(RsCtl*)c->rsb.ctlb.p, (unsigned long long*)c->rsb.have.p, (unsigned long long*)c->rsb.next.p,
                 (unsigned long long*)c->rsb.own.p, (unsigned long long*)c->rsb.ring.p, c->rumors};
}

// What the shared round loop (gs_round_host.cpp) runs for this context.  A
// capped set's round kernel is gs_rumorset_cap.hip's; the commit half first
// injects the live rumors that enter after this round's commit (the host
// knows the starts).  The count ring comes back beside the stats rows, and a
// row's hook takes its counts: rumor j's tick_99 and the set's (the first poll
// with no started rumor uncovered) are taken at polls only.
RoundEngine rs_engine(gs_ctx* c) {
  const RsState rs = rs_state(c);
  RsBufs& b = c->rsb;
  RoundEngine e{};
  e.name = "rumor set's";
  e.round = [c, rs, &b](uint32_t tt) -> int {
    if (b.payload) CK(c, rsc_round(c->st, rs, tt, b.payload, b.pick, b.grid, c->stream));
    else CK(c, rs_round(c->st, rs, tt, b.grid, c->stream));
    return GS_OK;
  };
  e.commit = [c, rs, &b](uint32_t tt) -> int {
    if (tt <= b.last_start) {
      unsigned long long in = 0;
      for (uint32_t j = 0; j < c->rumors; ++j)
        if (b.start[j] == tt) in |= 1ull << j;
      if (in & b.live) CK(c, rsc_inject(rs, b.snd, in & b.live, c->stream));
    }
    CK(c, rs_commit(c->st, rs, tt, b.grid, c->stream));
    return GS_OK;
  };
  e.ctl = RoundCtl{b.ctlb.p, b.h_ctl, sizeof(RsCtl), &b.h_ctl->received, &b.h_ctl->pending, &b.h_ctl->stop};
  e.ring = RoundRing{rs.ring, b.h_ring, kRsMax};
  e.row = [c, &b](uint64_t tick, const unsigned long long* counts, bool poll) {
    for (uint32_t j = 0; j < c->rumors; ++j) {
      b.count[j] = counts[j];
      if (poll && ((b.live >> j) & 1) && !b.tick99[j] && covered(b.count[j], c->p.n)) b.tick99[j] = tick;
    }
    TrialAcc& a = c->tacc[0];
    if (poll && !a.tick99 && b.live && c->pending == 0) a.tick99 = tick;
  };
  return e;
}

}  // namespace

// What gs_create_rumorset refuses, before any device call.
int rs_check_create(const gs_params* params, uint32_t rumors) {
  std::string why;
  if (!params) why = "params is NULL";
  else if (params->model != GS_MODEL_PUSHPULL)
    why = "gs_create_rumorset: model must be GS_MODEL_PUSHPULL, not " + std::to_string(params->model) +
          " (a rumor set is push-pull's: the calls do not depend on who is informed)";
  else if (rumors < 1 || rumors > GS_RUMORSET_MAX)
    why = "gs_create_rumorset: rumors must be in 1..64 (a bit per rumor in a uint64 per node), not " +
          std::to_string(rumors);
  else if (params->trials > 1)
    why = "gs_create_rumorset: trials must be 0 or 1, not " + std::to_string(params->trials) +
          " (the rumors of a set share one trial's table and draws)";
  else if (params->flags & ~GS_FLAG_TIMING)
    why = "gs_create_rumorset: flags " + std::to_string(params->flags) +
          " has a bit besides GS_FLAG_TIMING (a rumor set has one round kind and no tick engine)";
  if (why.empty()) return GS_OK;
  fprintf(stderr, "%s\n", why.c_str());
  g_create_err = why;
  return GS_EINVAL;
}

// Nothing of push-pull's reverse table, summaries or lists: three words per
// node (24 GB at n = 1e9, from the block cache like every buffer of 64 MiB or
// more), the count ring and the control block.
int rs_alloc(gs_ctx* c) {
  const uint64_t n = c->st.n;
  RsBufs& b = c->rsb;
  const size_t ring = (size_t)kStatSlots * kRsMax * 8;
  if (!grow(b.have, n * 8) || !grow(b.next, n * 8) || !grow(b.own, n * 8) || !grow(b.ring, ring) ||
      !grow(b.ctlb, sizeof(RsCtl)) || hipHostMalloc((void**)&b.h_ctl, sizeof(RsCtl)) != hipSuccess ||
      hipHostMalloc((void**)&b.h_ring, ring) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the rumor set's state");
  return GS_OK;
}

// (col grows at the first gs_read_rumor_column)
void release_rumorset(gs_ctx* c) {
  RsBufs& b = c->rsb;
  for (Buf* q : {&b.have, &b.next, &b.own, &b.ring, &b.ctlb, &b.col}) release(*q);
  if (b.h_ctl) (void)hipHostFree(b.h_ctl);
  if (b.h_ring) (void)hipHostFree(b.h_ring);
}

// senders[j] < 0: rumor j's keyed sender.  A failed sender starts nothing; if
// none starts the first poll is quiescent.  starts (section 4.9.1): rumor j
// enters after round starts[j]'s commit; NULL, or every entry 0, is the begin
// of section 4.9 with its own seed kernel.
int rs_begin(gs_ctx* c, const int64_t* senders, const int64_t* starts) {
  CK(c, hipSetDevice(c->dev));
  // GS_RUMORSET_GRID: the blocks of the round and the commit (read per
  // broadcast, so tests can make a short table take several passes of the grid)
  RsBufs& b = c->rsb;
  b.grid = rs_grid(c->st.n, env_grid("GS_RUMORSET_GRID"));
  b.snd = RsSenders{};
  b.last_start = 0;
  unsigned long long now = 0;
  for (uint32_t j = 0; j < c->rumors; ++j) {
    b.snd.node[j] = senders[j] >= 0 ? (uint32_t)senders[j]
                                    : uniform(draw0(c->st.key, K_SENDER, j, 0, 0), (uint32_t)c->p.n);
    b.sender[j] = b.snd.node[j];
    b.tick99[j] = 0;
    b.start[j] = starts ? (uint32_t)starts[j] : 0u;
    b.last_start = std::max(b.last_start, b.start[j]);
    if (b.start[j] == 0) now |= 1ull << j;
  }
  CK(c, hipMemsetAsync(b.ctlb.p, 0, sizeof(RsCtl), c->stream));
  for (Buf* q : {&b.have, &b.next, &b.own}) CK(c, hipMemsetAsync(q->p, 0, c->st.n * 8, c->stream));
  CK(c, hipMemsetAsync(c->st.recv, 0, c->st.W * 8, c->stream));
  if (b.last_start == 0) CK(c, rs_seed(c->st, rs_state(c), b.snd, cover_threshold(c->p.n), c->stream));
  else CK(c, rsc_seed(c->st, rs_state(c), b.snd, now, cover_threshold(c->p.n), c->stream));
  CK(c, hipMemcpyAsync(b.h_ctl, b.ctlb.p, sizeof(RsCtl), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  b.live = b.h_ctl->live;
  for (uint32_t j = 0; j < kRsMax; ++j) b.count[j] = b.h_ctl->cnt[j];
  c->recv = c->tacc[0].recv = b.h_ctl->received;
  c->pending = b.h_ctl->pending;
  c->begun = true;
  return GS_OK;
}

// The cap of the next broadcasts: refused while one is under way, so that a
// broadcast's traffic counters belong to one cap; gs_reset and gs_set_trial keep it.
int rs_set_payload(gs_ctx* c, uint32_t payload, uint32_t pick) {
  if (!c->rset) return fail(c, GS_EINVAL, "gs_rumorset_set_payload needs a gs_create_rumorset context");
  if (payload > GS_RUMORSET_MAX)
    return fail(c, GS_EINVAL, "payload must be 0 (no cap) or 1..64 rumors per message, not " + std::to_string(payload));
  if (pick > GS_PICK_ROTATE)
    return fail(c, GS_EINVAL, "pick must be GS_PICK_LOW, GS_PICK_HIGH or GS_PICK_ROTATE, not " + std::to_string(pick));
  if (c->begun) return fail(c, GS_EINVAL, "gs_reset before gs_rumorset_set_payload (a broadcast is under way)");
  c->rsb.payload = payload;
  c->rsb.pick = pick;
  return GS_OK;
}

// The counters are k_rsc_round's: an uncapped set (payload 0) runs k_rs_round,
// which counts none of them, so it answers GS_EINVAL (payload 64 counts and
// moves what no cap moves).  As of the last round a gs_step or gs_run read back.
int rs_traffic(gs_ctx* c, gs_rumorset_traffic* out) {
  if (!c->rset) return fail(c, GS_EINVAL, "gs_rumorset_traffic_get needs a gs_create_rumorset context");
  if (!out) return fail(c, GS_EINVAL, "out is NULL");
  const RsBufs& b = c->rsb;
  if (b.payload == 0)
    return fail(c, GS_EINVAL, "gs_rumorset_traffic_get: an uncapped set does not count its traffic "
                              "(gs_rumorset_set_payload(ctx, 64, pick) moves the same and counts)");
  *out = gs_rumorset_traffic{};
  if (c->begun) {
    out->wanted = b.h_ctl->traffic[RS_WANTED];
    out->carried = b.h_ctl->traffic[RS_CARRIED];
    out->bound = b.h_ctl->traffic[RS_BOUND];
  }
  return GS_OK;
}

// The rounds and the run on the shared loop (gs_round_host.cpp): three
// launches a round, one more in a round after which a late rumor enters.  The
// run stops at the first poll with no started rumor below 99 % (the device's
// stop word: covered, or quiescent if no rumor started), or at max_ticks.
// There is no test for "nothing can change": a masked run that cannot reach
// 99 % ends at max_ticks.
int rs_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls) {
  return round_step(c, ticks, out, every_tick_polls, rs_engine(c));
}

int rs_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
           int32_t* status) {
  if (!c->begun) return fail(c, GS_EINVAL, "gs_broadcast_begin or gs_rumorset_begin first");
  return round_run(c, poll, max_ticks, out, cap, nout, status, rs_engine(c));
}

int rs_results(gs_ctx* c, gs_rumor_stats* out, size_t cap, size_t* nout) {
  if (!c->rset) return fail(c, GS_EINVAL, "gs_rumorset_results needs a gs_create_rumorset context");
  const RsBufs& b = c->rsb;
  for (uint32_t j = 0; j < c->rumors && out && j < cap; ++j) {
    const bool on = c->begun && ((b.live >> j) & 1);
    out[j] = gs_rumor_stats{c->begun ? b.sender[j] : -1, on ? b.count[j] : 0, on ? b.tick99[j] : 0, on ? 1 : 0, 0};
  }
  if (nout) *nout = c->rumors;
  return GS_OK;
}

int rs_read_words(gs_ctx* c, uint64_t* have, size_t n) {
  if (!c->rset) return fail(c, GS_EINVAL, "gs_read_rumorset needs a gs_create_rumorset context");
  if (!have || n < c->p.n) return fail(c, GS_EINVAL, "need n words");
  CK(c, hipSetDevice(c->dev));
  if (!c->begun) {  // (have is the last run's: nobody holds a rumor)
    memset(have, 0, c->p.n * 8);
    return GS_OK;
  }
  CK(c, hipMemcpyAsync(have, c->rsb.have.p, c->p.n * 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

int rs_read_column(gs_ctx* c, uint32_t rumor, uint64_t* words, size_t nwords) {
  if (!c->rset) return fail(c, GS_EINVAL, "gs_read_rumor_column needs a gs_create_rumorset context");
  if (rumor >= c->rumors) return fail(c, GS_EINVAL, "rumor must be below the set's " + std::to_string(c->rumors));
  if (!words || nwords < c->st.W) return fail(c, GS_EINVAL, "need ceil(n/64) words");
  CK(c, hipSetDevice(c->dev));
  if (!grow(c->rsb.col, c->st.W * 8)) return fail(c, GS_ENOMEM, "cannot allocate the column bitset");
  unsigned long long* d = (unsigned long long*)c->rsb.col.p;
  if (c->begun) CK(c, rs_column(c->st, rs_state(c), rumor, d, c->stream));
  else CK(c, hipMemsetAsync(d, 0, c->st.W * 8, c->stream));
  return read_words(c, words, d);
}

}  // namespace gs
