// gs_api.cpp -- the C ABI of libgossip_hip.so (include/gossip.h).
//
// Replaces the reference's main() body (simulator.go:207-253): allocation
// (:208-212), overlay (:214-235), broadcast and polling (:237-253).  Four
// kinds of context sit behind the same calls:
//   plain    one device, one stream, one trial (window / tick / push-pull engine)
//   batched  one device, `trials` independent trials laid out at trial << tlog
//            and run at once (config C3): the flood model by the window engine,
//            push-pull by the trial-resident kernel (a workgroup per trial), the
//            rumor model by its own (gs_create_trials only), the median model by
//            its own (gs_create_batch only)
//   shard    one node range [lo, hi) of one broadcast (config C4): a member of a
//            group, or one rank of a multi-process run (RCCL inside)
//   group    gs_create_multi: shards or trial batches over several devices
// A rumor set (gs_create_rumorset) is a plain context with an engine of its own
// (gs_rumorset_host.cpp): up to 64 push-pull broadcasts in one pass.
#include "gs_ctx.h"

using namespace gs;

namespace {

// gs_timing's device-memory fields: the library's process-wide figures
void fill_devmem(gs_timing* out) {
  DevMemStats d;
  gs_devmem_stats(&d);
  out->alloc_ms = d.alloc_ms;
  out->largest_alloc_ms = d.largest_alloc_ms;
  out->free_ms = d.free_ms;
  out->alloc_calls = d.hip_allocs;
  out->alloc_cache_hits = d.cache_hits;
  out->cached_bytes = d.cached_bytes;
}

// Is local node `u` of c crashed (a pre-failed mask)?
int is_failed(gs_ctx* c, uint64_t u, bool* out) {
  *out = false;
  if (!c->failed) return GS_OK;
  unsigned long long w = 0;
  CK(c, hipMemcpyAsync(&w, c->st.crash + u / 64, 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *out = (w >> (u & 63)) & 1;
  return GS_OK;
}

uint64_t keyed_sender(const gs_ctx* c) {
  return uniform(draw0(c->st.key, K_SENDER, 0, 0, 0), (uint32_t)c->p.n);  // simulator.go:240
}

// Batched trials after their senders were seeded or scheduled: waits for the
// stream and sets every trial's TrialAcc::start and *count = the trials that
// started.  `started` is the flag per trial the kernel wrote (the first words
// of d_tstat, free between broadcasts), or null without failure masks: all did.
int read_started(gs_ctx* c, const uint32_t* started, uint32_t* count) {
  if (started) CK(c, hipMemcpyAsync(c->bt.h_tstat, started, (size_t)c->trials * 4, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *count = 0;
  for (uint32_t t = 0; t < c->trials; ++t) {
    c->tacc[t].start = started ? c->bt.h_tstat[t] : 1;
    *count += (uint32_t)c->tacc[t].start;
  }
  return GS_OK;
}

// Schedules the global sender s if c owns it (and it is live); *sched = 1 if so.
int begin_one(gs_ctx* c, uint64_t s, uint32_t* sched) {
  *sched = 0;
  CK(c, hipSetDevice(c->dev));
  if (c->trials > 1) {  // every trial's sender (:240 per trial when s == ~0)
    // per-trial failure masks: a trial whose sender is failed schedules nothing
    uint32_t* started = c->failed ? c->bt.d_tstat : nullptr;
    CK(c, win_schedule(c->ws, (uint32_t)s, 0, c->trials, (uint32_t)c->p.n, c->stream, started));
    RC(read_started(c, started, sched));
    return GS_OK;
  }
  if (s < c->lo || s >= (c->shard ? c->hi : c->p.n)) return GS_OK;  // another shard's node
  const uint64_t u = s - c->lo;
  bool dead = false;
  RC(is_failed(c, u, &dead));
  if (dead) return GS_OK;  // a failed sender never broadcasts
  if (c->win) CK(c, win_schedule(c->ws, (uint32_t)u, 0, 1, (uint32_t)c->p.n, c->stream));
  else CK(c, launch_schedule_one(c->st, (uint32_t)u, 0, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *sched = 1;
  return GS_OK;
}

// Bitset `which` (0 = received, 1 = crashed) of context c into words: a
// shard's own words at their global positions, batched trials trial-major.
int read_bits(gs_ctx* c, int which, uint64_t* words, size_t nwords) {
  const uint64_t Wn = (c->p.n + 63) / 64;
  if (c->group && c->gtrials) {  // every member's trials, back to back: the caller's buffer holds them all
    if (nwords < Wn * c->trials) return fail(c, GS_EINVAL, "need ceil(n/64) words per trial");
    uint64_t off = 0;
    for (gs_ctx* m : c->gr.mem) {
      if (read_bits(m, which, words + off * Wn, nwords - off * Wn)) return fail(c, GS_EINVAL, m->err);
      off += m->trials;
    }
    return GS_OK;
  }
  if (c->group) {
    std::fill(words, words + Wn, 0ull);
    std::vector<uint64_t> tmp(Wn);
    for (gs_ctx* m : c->gr.mem) {
      if (read_bits(m, which, tmp.data(), Wn)) return fail(c, GS_EINVAL, m->err);
      for (uint64_t i = 0; i < Wn; ++i) words[i] |= tmp[i];
    }
    return GS_OK;
  }
  if (nwords < Wn * c->trials) return fail(c, GS_EINVAL, "need ceil(n/64) words per trial");
  CK(c, hipSetDevice(c->dev));
  const unsigned long long* src = which ? c->st.crash : c->st.recv;
  if (c->trials > 1) {
    CK(c, hipMemcpy2DAsync(words, Wn * 8, src, ((size_t)1 << c->tlog) / 8, Wn * 8, c->trials,
                           hipMemcpyDeviceToHost, c->stream));
  } else if (c->shard) {
    std::fill(words, words + Wn, 0ull);
    CK(c, hipMemcpyAsync(words + c->lo / 64, src, c->st.W * 8, hipMemcpyDeviceToHost, c->stream));
  } else {
    CK(c, hipMemcpyAsync(words, src, c->st.W * 8, hipMemcpyDeviceToHost, c->stream));
  }
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_version(void) { return GS_ABI_VERSION; }

const char* gs_strerror(int code) {
  switch (code) {
    case GS_OK: return "ok";
    case GS_EINVAL: return "invalid argument";
    case GS_ELIVELOCK: return "overlay livelock";
    case GS_EREJECT: return "replacement rejection exhausted";
    case GS_ENOMEM: return "out of memory";
    case GS_EDEVICE: return "HIP device error";
    case GS_EOVERFLOW: return "counter overflow";
    default: return "unknown error";
  }
}

const char* gs_last_error(const gs_ctx* c) {
  if (c) return c->err.c_str();
  return g_create_err.empty() ? "NULL context" : g_create_err.c_str();
}

// The limit queries have no context either: a HIP failure is reported like a
// failed create's reason, through gs_last_error(NULL) and on stderr, with the
// call that failed and the runtime's error.
// `refuse` (not empty): an argument the query rejects before it looks at the
// device.  limit(&lim): the engine's *_limit_error; max_n(lim): its plan's.
static int trials_max_n(const char* name, int device, uint64_t* n_max, const std::string& refuse,
                        const std::function<std::string(uint64_t*)>& limit,
                        const std::function<uint64_t(uint64_t)>& max_n) {
  g_create_err.clear();
  if (!n_max) return GS_EINVAL;
  *n_max = 0;
  int ndev = 0;
  int rc = GS_EDEVICE;
  std::string why;
  const hipError_t ce = hipGetDeviceCount(&ndev);
  if (!refuse.empty()) {
    why = refuse;
    rc = GS_EINVAL;
  } else if (ce != hipSuccess) {
    why = std::string("hipGetDeviceCount: ") + hipGetErrorString(ce);
  } else if (device < 0 || device >= ndev) {
    why = "device " + std::to_string(device) + " of " + std::to_string(ndev) + " visible";
  } else {
    uint64_t lim = 0;
    why = limit(&lim);
    if (why.empty()) {
      *n_max = max_n(lim);
      return GS_OK;
    }
  }
  (void)hipGetLastError();
  fprintf(stderr, "%s: %s\n", name, why.c_str());
  g_create_err = why;
  return rc;
}

int gs_pp_trials_max_n(int device, uint64_t* n_max) {
  return trials_max_n("gs_pp_trials_max_n", device, n_max, "",
                      [&](uint64_t* lim) { return ppt_limit_error(device, false, lim); }, ppt_max_n);
}

int gs_pp_trials_max_n_masked(int device, uint64_t* n_max) {
  return trials_max_n("gs_pp_trials_max_n_masked", device, n_max, "",
                      [&](uint64_t* lim) { return ppt_limit_error(device, true, lim); }, ppt_max_n_masked);
}

int gs_median_trials_max_n(int device, uint64_t* n_max) {
  return trials_max_n("gs_median_trials_max_n", device, n_max, "",
                      [&](uint64_t* lim) { return mdt_limit_error(device, false, lim); }, mdt_max_n);
}

int gs_median_trials_max_n_packed(int device, uint64_t* n_max) {
  return trials_max_n("gs_median_trials_max_n_packed", device, n_max, "",
                      [&](uint64_t* lim) { return mdt_limit_error(device, true, lim); }, mdt16_max_n);
}

int gs_rumor_trials_max_n(int device, uint32_t rumor_mode, uint64_t* n_max) {
  std::string refuse;
  if (rumor_mode & ~(GS_RUMOR_BLIND | GS_RUMOR_COIN | GS_RUMOR_PULL))
    refuse = "rumor_mode " + std::to_string(rumor_mode) + " has a bit that is none of GS_RUMOR_BLIND, GS_RUMOR_COIN, "
             "GS_RUMOR_PULL";
  return trials_max_n("gs_rumor_trials_max_n", device, n_max, refuse,
                      [&](uint64_t* lim) { return rmt_limit_error(device, rumor_mode, lim); },
                      [&](uint64_t lim) { return rmt_max_n(rumor_mode, lim); });
}

int gs_create(const gs_params* params, gs_ctx** out) {
  g_create_err.clear();
  if (!out) return GS_EINVAL;
  *out = nullptr;
  return create_one(params, params ? params->device : 0, false, 1, 0, out);
}

// gs_create with the rumor / trials refusal lifted: every other check of the
// parameters still runs before any device call.
int gs_create_trials(const gs_params* params, gs_ctx** out) {
  g_create_err.clear();
  if (!out) return GS_EINVAL;
  *out = nullptr;
  RC(median_refuse(params, "gs_create_trials"));
  return create_one(params, params ? params->device : 0, false, 1, 0, out, true);
}

// gs_create_trials with the median / trials refusal lifted too: every other
// check of the parameters still runs before any device call.
int gs_create_batch(const gs_params* params, gs_ctx** out) {
  g_create_err.clear();
  if (!out) return GS_EINVAL;
  *out = nullptr;
  return create_one(params, params ? params->device : 0, false, 1, 0, out, true, true);
}

// The only way in to a rumor set: the other creates keep every answer they give.
int gs_create_rumorset(const gs_params* params, uint32_t rumors, gs_ctx** out) {
  g_create_err.clear();
  if (!out) return GS_EINVAL;
  *out = nullptr;
  RC(rs_check_create(params, rumors));
  return create_one(params, params->device, false, 1, 0, out, false, false, rumors);
}

int gs_rumorset_begin(gs_ctx* c, const int64_t* senders, size_t count) {
  if (!c) return GS_EINVAL;
  if (!c->rset) return fail(c, GS_EINVAL, "gs_rumorset_begin needs a gs_create_rumorset context");
  if (!c->peers) return fail(c, GS_EINVAL, "load peers or build the overlay first");
  if (c->begun) return fail(c, GS_EINVAL, "broadcast already begun");
  if (!senders || count != c->rumors)
    return fail(c, GS_EINVAL, "the set has " + std::to_string(c->rumors) + " rumors: count must equal it");
  for (size_t j = 0; j < count; ++j)
    if (senders[j] >= 0 && (uint64_t)senders[j] >= c->p.n)
      return fail(c, GS_EINVAL, "sender " + std::to_string(j) + " out of range");
  reset_counters(c);
  return rs_begin(c, senders);
}

int gs_rumorset_begin_at(gs_ctx* c, const int64_t* senders, const int64_t* starts, size_t count) {
  if (!c) return GS_EINVAL;
  if (!c->rset) return fail(c, GS_EINVAL, "gs_rumorset_begin_at needs a gs_create_rumorset context");
  if (!c->peers) return fail(c, GS_EINVAL, "load peers or build the overlay first");
  if (c->begun) return fail(c, GS_EINVAL, "broadcast already begun");
  if (!senders || count != c->rumors)
    return fail(c, GS_EINVAL, "the set has " + std::to_string(c->rumors) + " rumors: count must equal it");
  for (size_t j = 0; j < count; ++j) {
    if (senders[j] >= 0 && (uint64_t)senders[j] >= c->p.n)
      return fail(c, GS_EINVAL, "sender " + std::to_string(j) + " out of range");
    if (starts && (starts[j] < 0 || starts[j] > 0x7FFFFFFFll))
      return fail(c, GS_EINVAL, "start " + std::to_string(j) + " must be a round in 0..2^31-1");
  }
  reset_counters(c);
  return rs_begin(c, senders, starts);
}

int gs_rumorset_set_payload(gs_ctx* c, uint32_t payload, uint32_t pick) {
  if (!c) return GS_EINVAL;
  return rs_set_payload(c, payload, pick);
}

int gs_rumorset_traffic_get(gs_ctx* c, gs_rumorset_traffic* out) {
  if (!c) return GS_EINVAL;
  return rs_traffic(c, out);
}

int gs_rumorset_results(gs_ctx* c, gs_rumor_stats* out, size_t cap, size_t* nout) {
  if (!c) return GS_EINVAL;
  return rs_results(c, out, cap, nout);
}

int gs_read_rumorset(gs_ctx* c, uint64_t* have, size_t n) {
  if (!c) return GS_EINVAL;
  return rs_read_words(c, have, n);
}

int gs_read_rumor_column(gs_ctx* c, uint32_t rumor, uint64_t* words, size_t nwords) {
  if (!c) return GS_EINVAL;
  return rs_read_column(c, rumor, words, nwords);
}

int gs_create_multi(const gs_params* params, const int* devices, int ndev, gs_ctx** out) {
  g_create_err.clear();
  if (!out || !params || !devices || ndev < 1) return GS_EINVAL;
  *out = nullptr;
  return create_multi(params, devices, ndev, out);
}

int gs_comm_unique_id(uint8_t id[GS_COMM_ID_BYTES]) {
  if (!id) return GS_EINVAL;
  const Rccl& r = rccl();
  if (!r.ok) {
    fprintf(stderr, "gs_comm_unique_id: %s\n", r.why.c_str());
    return GS_EDEVICE;
  }
  ncclUniqueId u;
  if (r.get_unique_id(&u) != ncclSuccess) return GS_EDEVICE;
  static_assert(sizeof(ncclUniqueId) == GS_COMM_ID_BYTES, "RCCL unique id size");
  memcpy(id, &u, GS_COMM_ID_BYTES);
  return GS_OK;
}

int gs_create_rank(const gs_params* params, int device, int nranks, int rank, const uint8_t* id, gs_ctx** out) {
  g_create_err.clear();
  if (!out || !params || nranks < 1 || rank < 0 || rank >= nranks) return GS_EINVAL;
  *out = nullptr;
  RC(rumor_refuse(params, "gs_create_rank"));
  RC(median_refuse(params, "gs_create_rank"));
  const uint32_t T = std::max<uint32_t>(1, params->trials);
  if (T > 1) {  // this rank's share of the trials, no communication
    gs_params mp = *params;
    const uint32_t t0 = (uint32_t)((uint64_t)T * rank / nranks), t1 = (uint32_t)((uint64_t)T * (rank + 1) / nranks);
    if (t1 == t0) {
      fprintf(stderr, "gs_create_rank: %u trials leave rank %d none\n", T, rank);
      return GS_EINVAL;
    }
    mp.trial = params->trial + t0;
    mp.trials = t1 - t0;
    return create_one(&mp, device, false, 1, 0, out);
  }
  if (!id) return GS_EINVAL;
  const Rccl& r = rccl();
  if (!r.ok) {
    fprintf(stderr, "gs_create_rank: %s\n", r.why.c_str());
    return GS_EDEVICE;
  }
  gs_ctx* c = nullptr;
  int rc = create_one(params, device, true, (uint32_t)nranks, (uint32_t)rank, &c);
  if (rc) return rc;
  ncclUniqueId u;
  memcpy(&u, id, GS_COMM_ID_BYTES);
  (void)hipSetDevice(device);
  ncclResult_t nr = r.comm_init_rank(&c->xc.comm, nranks, u, rank);
  if (nr != ncclSuccess) {
    fprintf(stderr, "gs_create_rank: ncclCommInitRank: %s\n", rccl_error((int)nr).c_str());
    c->xc.comm = nullptr;
    destroy_one(c);
    return GS_EDEVICE;
  }
  return finish_rank(c, out);
}

int gs_create_rank_exchange(const gs_params* params, int device, int nranks, int rank, const gs_exchange* ex,
                            gs_ctx** out) {
  g_create_err.clear();
  if (!out || !params || !ex || !ex->all_gather || !ex->all_reduce_sum_u64 || nranks < 1 || rank < 0 ||
      rank >= nranks)
    return GS_EINVAL;
  RC(rumor_refuse(params, "gs_create_rank_exchange"));
  RC(median_refuse(params, "gs_create_rank_exchange"));
  if (params->model == GS_MODEL_FLOOD && std::max<uint32_t>(1, params->trials) == 1 && !ex->all_to_allv) {
    fprintf(stderr, "gs_create_rank_exchange: flood shards need the all_to_allv callback\n");
    return GS_EINVAL;
  }
  *out = nullptr;
  if (std::max<uint32_t>(1, params->trials) > 1) return gs_create_rank(params, device, nranks, rank, nullptr, out);
  gs_ctx* c = nullptr;
  int rc = create_one(params, device, true, (uint32_t)nranks, (uint32_t)rank, &c);
  if (rc) return rc;
  c->xc.hx = *ex;
  c->xc.has_hx = true;
  return finish_rank(c, out);
}

int gs_shard_info(const gs_ctx* c, uint32_t index, uint32_t* nshards, uint64_t* lo, uint64_t* hi) {
  if (!c) return GS_EINVAL;
  const bool sg = c->group && !c->gtrials;
  const uint32_t ns = sg ? (uint32_t)c->gr.mem.size() : c->shard ? c->G : 1u;
  if (nshards) *nshards = ns;
  if (index >= ns) return GS_EINVAL;
  const gs_ctx* s = sg ? c->gr.mem[0] : c;
  uint64_t a = 0, b = c->p.n;
  if (s->shard) {
    a = std::min<uint64_t>(index * s->seg_per, c->p.n);
    b = std::min<uint64_t>(a + s->seg_per, c->p.n);
  }
  if (lo) *lo = a;
  if (hi) *hi = b;
  return GS_OK;
}

void gs_destroy(gs_ctx* c) { destroy_one(c); }

// A load or an overlay build writes over the table it replaces before it
// knows whether the new one is good (the copy comes before validate_table, a
// shard group's leader has dropped its partition by then, and an overlay that
// ends in GS_ELIVELOCK has written half its rows): from its first touch to its
// success the context, every group member and a push-pull shard's replica have
// no table, and gs_broadcast_begin / gs_read_peers refuse.
static void drop_table(gs_ctx* c) {
  c->peers = false;
  c->named_ok = false;  // (a packed median batch: the next table is counted at its first begin)
  if (c->rs.rep) c->rs.rep->peers = false;
  for (gs_ctx* r : c->gr.reps)
    if (r) r->peers = false;
  for (gs_ctx* m : c->gr.mem) drop_table(m);
}

int gs_load_peers(gs_ctx* c, const uint8_t* deg, const uint32_t* ids, uint32_t stride) {
  if (!c || !deg || !ids || stride == 0 || stride > 255) return fail(c, GS_EINVAL, "bad peer table");
  if (c->begun) return fail(c, GS_EINVAL, "peers must be loaded before gs_broadcast_begin");
  drop_table(c);
  if (c->group && c->gtrials) {
    uint64_t off = 0;
    for (gs_ctx* m : c->gr.mem) {
      RC(gs_load_peers(m, deg + off * c->p.n, ids + off * c->p.n * stride, stride) ? fail(c, GS_EINVAL, m->err) : 0);
      off += m->trials;
    }
    c->peers = true;
    return GS_OK;
  }
  if (c->group) {
    for (size_t d = 0; d < c->gr.devs.size(); ++d) {
      std::vector<gs_ctx*> ms = on_device(c, d);
      int rc = upload_table(ms[0], deg, ids, stride);
      if (!rc) rc = seal_rows(ms[0], ms[0]->d_deg, ms[0]->d_ids, c->p.n);
      if (!rc) rc = partition_from(ms[0], ms);
      if (rc) return fail(c, rc, ms[0]->err);
    }
    c->peers = true;
    return GS_OK;
  }
  RC(upload_table(c, deg, ids, stride));
  RC(seal_rows(c, c->d_deg, c->d_ids, table_n(c)));
  if (c->shard) RC(partition_from(c, {c}));
  c->peers = true;
  return GS_OK;
}

int gs_load_peers_device(gs_ctx* c, const void* d_deg, const void* d_ids, uint32_t stride) {
  if (!c || !d_deg || !d_ids || stride < 2 || stride > 255)
    return fail(c, GS_EINVAL, "bad device peer table (stride must be in [2,255])");
  if (c->begun) return fail(c, GS_EINVAL, "peers must be loaded before gs_broadcast_begin");
  if (c->mdt) {  // a median batch: tables back to back, as gs_load_peers takes them
    drop_table(c);
    RC(mdt_load_device(c, d_deg, d_ids, stride));
    c->peers = true;
    return GS_OK;
  }
  if (c->group || c->trials > 1)
    return fail(c, GS_EINVAL, "device tables load into one-device, one-trial contexts");
  drop_table(c);
  CK(c, hipSetDevice(c->dev));
  c->row_slots = 0;
  RC(alloc_table(c, stride));
  const uint64_t n = table_n(c);
  CK(c, hipMemcpyAsync(c->d_deg, d_deg, n, hipMemcpyDeviceToDevice, c->stream));
  CK(c, hipMemcpyAsync(c->d_ids, d_ids, n * stride * 4ull, hipMemcpyDeviceToDevice, c->stream));
  RC(validate_table(c, c->d_deg, c->d_ids, n, c->p.n));
  RC(seal_rows(c, c->d_deg, c->d_ids, n));
  if (c->shard) RC(partition_from(c, {c}));
  c->peers = true;
  return GS_OK;
}

int gs_read_peers(gs_ctx* c, uint8_t* deg, uint32_t* ids, uint32_t* stride_out) {
  if (!c || !c->peers) return fail(c, GS_EINVAL, "no peer table");
  if (c->group && c->gtrials) {
    uint32_t s = 0;
    uint64_t off = 0;
    for (gs_ctx* m : c->gr.mem) {
      if (gs_read_peers(m, deg ? deg + off * c->p.n : nullptr, nullptr, &s)) return fail(c, GS_EINVAL, m->err);
      if (ids && gs_read_peers(m, nullptr, ids + off * c->p.n * s, &s)) return fail(c, GS_EINVAL, m->err);
      off += m->trials;
    }
    if (stride_out) *stride_out = s;
    return GS_OK;
  }
  if (c->group || c->shard)
    return fail(c, GS_EINVAL, "a sharded context keeps only its partition of the table");
  const uint32_t S = c->st.stride, So = c->row_slots && c->row_slots < S ? c->row_slots : S;
  if (stride_out) *stride_out = So;
  CK(c, hipSetDevice(c->dev));
  if (c->trials > 1) {  // padded id space -> trial tables back to back, local ids
    const uint64_t np = c->p.n, per = 1ull << c->tlog;
    std::vector<uint8_t> hd(c->ntot);
    std::vector<uint32_t> hi;
    CK(c, hipMemcpyAsync(hd.data(), c->d_deg, c->ntot, hipMemcpyDeviceToHost, c->stream));
    if (ids) {
      hi.resize(c->ntot * S);
      CK(c, hipMemcpyAsync(hi.data(), c->d_ids, c->ntot * S * 4ull, hipMemcpyDeviceToHost, c->stream));
    }
    CK(c, hipStreamSynchronize(c->stream));
    for (uint32_t t = 0; t < c->trials; ++t)
      for (uint64_t v = 0; v < np; ++v) {
        const uint64_t src = t * per + v, dst = t * np + v;
        if (deg) deg[dst] = hd[src];
        if (ids)
          for (uint32_t j = 0; j < So; ++j) {
            const uint32_t x = hi[src * S + j];
            ids[dst * So + j] = x == kEmptyMsg ? x : (x & ((uint32_t)per - 1));
          }
      }
    return GS_OK;
  }
  if (deg) CK(c, hipMemcpyAsync(deg, c->d_deg, c->p.n, hipMemcpyDeviceToHost, c->stream));
  if (ids && So == S) CK(c, hipMemcpyAsync(ids, c->d_ids, c->p.n * S * 4ull, hipMemcpyDeviceToHost, c->stream));
  if (ids && So != S)  // padded rows: the first So slots of each
    CK(c, hipMemcpy2DAsync(ids, So * 4ull, c->d_ids, S * 4ull, So * 4ull, c->p.n, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

int gs_build_overlay(gs_ctx* c, uint64_t max_ticks, gs_window* win, size_t cap, size_t* nwin,
                     uint64_t* final_tick) {
  if (!c) return GS_EINVAL;
  if (c->begun) return fail(c, GS_EINVAL, "overlay must be built before gs_broadcast_begin");
  drop_table(c);
  if (c->group && c->gtrials) {
    std::vector<uint64_t> ft(c->gr.mem.size(), 0);
    std::vector<size_t> nw(c->gr.mem.size(), 0);
    RC(par_members(c, [&](gs_ctx* m, size_t i) {
      return gs_build_overlay(m, max_ticks, i == 0 ? win : nullptr, i == 0 ? cap : 0, &nw[i], &ft[i]);
    }));
    if (nwin) *nwin = nw[0];
    if (final_tick) *final_tick = *std::max_element(ft.begin(), ft.end());
    c->timing.overlay_ms = c->gr.mem[0]->timing.overlay_ms;
    c->peers = true;
    return GS_OK;
  }
  if (c->group) {
    for (size_t d = 0; d < c->gr.devs.size(); ++d) {
      std::vector<gs_ctx*> ms = on_device(c, d);
      int rc = overlay_into(ms[0], max_ticks, d == 0 ? win : nullptr, d == 0 ? cap : 0,
                            d == 0 ? nwin : nullptr, d == 0 ? final_tick : nullptr);
      if (!rc) rc = partition_from(ms[0], ms);
      if (rc) return fail(c, rc, ms[0]->err);
    }
    c->timing.overlay_ms = c->gr.mem[0]->timing.overlay_ms;
    c->peers = true;
    return GS_OK;
  }
  RC(overlay_into(c, max_ticks, win, cap, nwin, final_tick));
  if (c->shard) RC(partition_from(c, {c}));
  c->peers = true;
  return GS_OK;
}

int gs_set_failed(gs_ctx* c, const uint64_t* words, size_t nwords) { return set_failed(c, words, nwords); }

// ---------------------------------------------------------------------------
// Broadcast
// ---------------------------------------------------------------------------

int gs_broadcast_begin(gs_ctx* c, int64_t sender) {
  if (!c) return GS_EINVAL;
  if (c->aborted) return fail(c, GS_EDEVICE, "this rank's exchange failed earlier; the run is over");
  if (!c->peers) return fail(c, GS_EINVAL, "load peers or build the overlay first");
  if (c->begun) return fail(c, GS_EINVAL, "broadcast already begun");
  if (sender >= 0 && (uint64_t)sender >= c->p.n) return fail(c, GS_EINVAL, "sender out of range");
  reset_counters(c);
  if (c->rset) {  // every sender keyed, or rumor j at (sender + j) mod n
    int64_t snd[kRsMax];
    for (uint32_t j = 0; j < c->rumors; ++j) snd[j] = sender < 0 ? -1 : (int64_t)(((uint64_t)sender + j) % c->p.n);
    return rs_begin(c, snd);
  }
  if (c->group && c->gtrials) {
    for (gs_ctx* m : c->gr.mem) {
      if (gs_broadcast_begin(m, sender)) return fail(c, GS_EINVAL, m->err);
      c->recv += m->recv;  // push-pull: every trial's live sender is informed at begin
      c->pending += m->pending;  // the trials that began (all, unless a mask fails a sender)
    }
    c->begun = true;
    return GS_OK;
  }
  const bool batched = c->trials > 1;
  const uint64_t s = sender >= 0 ? (uint64_t)sender : batched ? ~0ull : keyed_sender(c->group ? c->gr.mem[0] : c);
  if (c->ppt) {  // batched push-pull: each trial's sender is informed (unless its mask fails it)
    CK(c, hipSetDevice(c->dev));
    uint32_t* started = c->failed ? c->bt.d_tstat : nullptr;
    uint32_t k = 0;
    CK(c, ppt_seed(c->pt, (uint32_t)s, started, c->stream));
    RC(read_started(c, started, &k));
    for (TrialAcc& a : c->tacc) a.recv = a.start;
    c->recv = c->pending = k;
    c->begun = true;
    return GS_OK;
  }
  if (c->rumor) return rumor_begin(c, s);
  if (c->median) return median_begin(c, s);
  if (c->pp && (c->group || c->pp_shard)) return pp_shard_begin(c, s);
  if (c->pp) {  // push-pull: the sender is informed (unless failed)
    CK(c, hipSetDevice(c->dev));
    RC(pp_prepare(c));
    const uint64_t n = c->st.n;
    const unsigned long long thr = (c->p.flags & GS_FLAG_PP_EARLY) ? n : (n >> pp_shift());
    RC(pp_seed_ctx(c, c->d_next, (uint32_t)s, thr, pp_bottom_thr(c), pp_answer_thr(c)));
    uint32_t ok = 0;
    CK(c, hipMemcpyAsync(&ok, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->recv = c->pending = ok;
    c->begun = true;
    return GS_OK;
  }
  unsigned long long scheduled = 0;
  if (c->group) {
    for (gs_ctx* m : c->gr.mem) {
      reset_counters(m);
      uint32_t k = 0;
      if (int rc = begin_one(m, s, &k)) return fail(c, rc, m->err);
      scheduled += k;
      m->begun = true;
    }
  } else {
    uint32_t k = 0;
    RC(begin_one(c, s, &k));
    scheduled = k;
    if (is_rank(c)) RC(rank_sum(c, &scheduled));  // every rank learns whether the owner scheduled the sender
  }
  c->pending = scheduled;
  for (TrialAcc& a : c->tacc) a.sched = 0;
  c->begun = true;
  return GS_OK;
}

int gs_set_stream(gs_ctx* c, void* hip_stream) {
  if (!c) return GS_EINVAL;
  if (c->group || is_rank(c)) return fail(c, GS_EINVAL, "multi-device contexts keep their own streams");
  CK(c, hipSetDevice(c->dev));
  CK(c, hipStreamSynchronize(c->stream));
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own;
  return GS_OK;
}

int gs_memory_stats(gs_timing* out) {
  if (!out) return GS_EINVAL;
  *out = gs_timing{};
  fill_devmem(out);
  return GS_OK;
}

int gs_trim(int device, size_t* released) {
  const size_t b = gs_devmem_trim(device);
  if (released) *released = b;
  return GS_OK;
}

int gs_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out) {
  if (!c) return GS_EINVAL;
  if (c->aborted) return fail(c, GS_EDEVICE, "this rank's exchange failed earlier; the run is over");
  if (!c->begun) return fail(c, GS_EINVAL, "gs_broadcast_begin first");
  if (c->group && c->gtrials) {
    std::vector<std::vector<gs_tick_stats>> rows(c->gr.mem.size(), std::vector<gs_tick_stats>(ticks));
    RC(par_members(c, [&](gs_ctx* m, size_t i) {
      return gs_step(m, ticks, rows[i].data());
    }));
    std::vector<unsigned long long> s(kStatFields);
    for (uint32_t k = 0; k < ticks; ++k) {
      std::fill(s.begin(), s.end(), 0ull);
      uint64_t pend = 0;
      for (auto& r : rows) {
        s[ST_FIRED] += r[k].fired;
        s[ST_SENT] += r[k].sent;
        s[ST_MSGS] += r[k].messages;
        pend += r[k].pending;
      }
      uint64_t recv = 0, cr = 0;
      for (auto& r : rows) { recv += r[k].received; cr += r[k].crashed; }
      c->t = rows[0][k].tick;
      c->fired += s[ST_FIRED]; c->sent += s[ST_SENT]; c->msgs += s[ST_MSGS];
      c->recv = recv; c->crashed = cr; c->pending = pend;
      if (out) out[k] = gs_tick_stats{c->t, s[ST_FIRED], s[ST_SENT], s[ST_MSGS], recv, cr, pend};
    }
    return GS_OK;
  }
  if (c->rumor) return rumor_step(c, ticks, out, true);
  if (c->median) return median_step(c, ticks, out, true);
  if (c->rset) return rs_step(c, ticks, out, true);
  if (c->pp && (c->group || c->pp_shard)) return pp_shard_step(c, ticks, out);
  if (c->group) return shard_step(c, c->gr.mem, ticks, out);
  if (c->shard) return abort_rank(c, shard_step(c, {c}, ticks, out));
  if (c->ppt) return ppt_step(c, ticks, out);
  return plain_step(c, ticks, out);
}

int gs_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap,
           size_t* nout, int32_t* status) {
  if (!c || poll == 0) return fail(c, GS_EINVAL, "poll must be >= 1");
  if (!c->peers) return fail(c, GS_EINVAL, "load peers or build the overlay first");
  if (c->group && c->gtrials) {  // every batch runs its own trials to their stops
    std::vector<int32_t> sts(c->gr.mem.size(), 0);
    RC(par_members(c, [&](gs_ctx* m, size_t i) {
      return gs_run(m, poll, max_ticks, nullptr, 0, nullptr, &sts[i]);
    }));
    gs_tick_stats tot{};
    uint64_t recv = 0, cr = 0, t = 0, pend = 0;
    c->fired = c->sent = c->msgs = 0;
    for (gs_ctx* m : c->gr.mem) {
      c->fired += m->fired; c->sent += m->sent; c->msgs += m->msgs;
      recv += m->recv; cr += m->crashed; pend += m->pending; t = std::max(t, m->t);
    }
    c->t = t; c->recv = recv; c->crashed = cr; c->pending = pend;
    tot = gs_tick_stats{t, c->fired, c->sent, c->msgs, recv, cr, pend};
    if (out && cap) out[0] = tot;
    if (nout) *nout = 1;
    if (status) *status = *std::max_element(sts.begin(), sts.end());
    return GS_OK;
  }
  if (c->rumor) return rumor_run(c, poll, max_ticks, out, cap, nout, status);
  if (c->median) return median_run(c, poll, max_ticks, out, cap, nout, status);
  if (c->rset) return rs_run(c, poll, max_ticks, out, cap, nout, status);
  size_t k = 0;
  int32_t st = GS_RUN_MAX_TICKS;
  const bool trials = c->trials > 1 && !c->group;
  const bool flood = !c->pp;
  const uint64_t pbase = c->t;
  uint64_t f0 = c->fired, s0 = c->sent, m0 = c->msgs;
  // device-driven windows: the poll rule runs on the device (k_close_dd for
  // shards, k_close otherwise); the run goes on host-driven after an overflow
  std::function<int(const OnTick&, uint32_t*, bool*)> dd;
  std::vector<gs_ctx*> ms;
  if (!c->pp && !c->gtrials && (c->group || c->shard) && dd_ok(c, shards_of(c))) {
    if (c->aborted) return fail(c, GS_EDEVICE, "this rank's exchange failed earlier; the run is over");
    if (!c->begun) return fail(c, GS_EINVAL, "gs_broadcast_begin first");
    ms = shards_of(c);
    for (gs_ctx* m : ms) {
      CK(m, hipSetDevice(m->dev));
      RC(expand_view(m));
    }
    dd = [&](const OnTick& on_tick, uint32_t* stop, bool* fallback) {
      const int rc = dd_run(c, ms, ~0ull, poll, max_ticks, on_tick, stop, fallback);
      return c->group ? rc : abort_rank(c, rc);
    };
  } else if (async_ok(c)) {
    dd = [&](const OnTick& on_tick, uint32_t* stop, bool* fallback) {
      return run_async(c, ~0ull, poll, max_ticks, on_tick, stop, fallback);
    };
  }
  if (dd) {
    uint32_t stop = 0;
    bool fallback = false;
    RC(dd(
        [&](uint64_t tick, const unsigned long long* row) {
          account_tick(c, tick, row, nullptr);
          if ((tick - pbase) % poll) return;
          if (out && k < cap)
            out[k] = gs_tick_stats{c->t, c->fired - f0, c->sent - s0, c->msgs - m0, c->recv, c->crashed, c->pending};
          ++k;
          f0 = c->fired; s0 = c->sent; m0 = c->msgs;
        },
        &stop, &fallback));
    if (!fallback) {
      st = stop ? (int32_t)stop - 1 : GS_RUN_MAX_TICKS;
      if (c->tacc.size() == 1) snap_trial(c, 0, st);
      if (nout) *nout = k;
      if (status) *status = st;
      return GS_OK;
    }
  }
  std::vector<uint64_t> tr0;  // batched push-pull: every trial's informed count before the poll
  for (;;) {
    const uint64_t r0 = c->recv;
    if (trials && c->ppt) {
      tr0.resize(c->trials);
      for (uint32_t tr = 0; tr < c->trials; ++tr) tr0[tr] = c->tacc[tr].recv;
    }
    // one poll (the first may finish a poll the device-driven windows began)
    RC(gs_step(c, (uint32_t)(poll - (c->t - pbase) % poll), nullptr));
    if (out && k < cap)
      out[k] = gs_tick_stats{c->t, c->fired - f0, c->sent - s0, c->msgs - m0, c->recv, c->crashed, c->pending};
    ++k;
    f0 = c->fired; s0 = c->sent; m0 = c->msgs;
    if (trials && c->ppt) {  // each trial stops at its own poll, by the one-trial push-pull rule
      uint32_t running = 0;
      RC(ppt_poll_stops(c, tr0, max_ticks, &running));
      if (trials_stopped(c, running, &st)) break;
      continue;
    }
    if (trials) {  // each trial stops at its own poll (simulator.go:243-251 per process)
      uint32_t running = 0;
      for (uint32_t tr = 0; tr < c->trials; ++tr) {
        TrialAcc& a = c->tacc[tr];
        if (a.status != GS_RUN_RUNNING) continue;
        const uint64_t pend = a.start + a.sched - a.fired;
        if (covered(a.recv, c->p.n)) snap_trial(c, tr, GS_RUN_COVERED);
        else if (pend == 0) snap_trial(c, tr, GS_RUN_QUIESCENT);
        else if (c->t >= max_ticks) snap_trial(c, tr, GS_RUN_MAX_TICKS);
        else ++running;
      }
      if (trials_stopped(c, running, &st)) break;
      continue;
    }
    if (covered(c->recv, c->p.n)) { st = GS_RUN_COVERED; break; }
    if (flood && c->pending == 0) { st = GS_RUN_QUIESCENT; break; }
    if (!flood && c->recv == r0) {  // push-pull: a window that informed nobody new
      bool stalled = false;
      RC(pp_stalled(c, &stalled));
      if (stalled) { st = GS_RUN_QUIESCENT; break; }
    }
    if (c->t >= max_ticks) { st = GS_RUN_MAX_TICKS; break; }
  }
  if (!trials && c->tacc.size() == 1) snap_trial(c, 0, st);
  if (nout) *nout = k;
  if (status) *status = st;
  return GS_OK;
}

int gs_trial_results(gs_ctx* c, gs_trial_stats* out, size_t cap, size_t* nout) {
  if (!c) return GS_EINVAL;
  size_t k = 0;
  auto one = [&](const gs_ctx* x) {
    for (size_t i = 0; i < x->tacc.size(); ++i, ++k) {
      if (!out || k >= cap) continue;
      const TrialAcc& a = x->tacc[i];
      if (a.status != GS_RUN_RUNNING) {
        out[k] = a.snap;
      } else {
        out[k] = gs_trial_stats{(uint64_t)x->p.trial + i, a.tick99, x->t, a.fired, a.sent, a.msgs, a.recv,
                                a.crash, GS_RUN_RUNNING, 0};
      }
    }
  };
  if (c->group && c->gtrials) for (gs_ctx* m : c->gr.mem) one(m);
  else one(c);
  if (nout) *nout = k;
  return GS_OK;
}

int gs_totals(gs_ctx* c, gs_tick_stats* out) {
  if (!c || !out) return GS_EINVAL;
  *out = gs_tick_stats{c->t, c->fired, c->sent, c->msgs, c->recv, c->crashed, c->pending};
  return GS_OK;
}

int gs_read_received(gs_ctx* c, uint64_t* words, size_t nwords) {
  if (!c || !words || nwords < (c->p.n + 63) / 64) return fail(c, GS_EINVAL, "need ceil(n/64) words");
  return read_bits(c, 0, words, nwords);
}

int gs_read_crashed(gs_ctx* c, uint64_t* words, size_t nwords) {
  if (!c || !words || nwords < (c->p.n + 63) / 64) return fail(c, GS_EINVAL, "need ceil(n/64) words");
  return read_bits(c, 1, words, nwords);
}

int gs_read_removed(gs_ctx* c, uint64_t* words, size_t nwords) {
  if (!c) return GS_EINVAL;
  if (c->rset) return fail(c, GS_EINVAL, "gs_read_removed: a rumor set removes nobody (every node calls every round)");
  if (c->median) return median_read_removed(c, words, nwords);
  return rumor_read_removed(c, words, nwords);
}

int gs_read_median_state(gs_ctx* c, uint8_t* st, size_t n) {
  if (!c) return GS_EINVAL;
  if (c->rset)
    return fail(c, GS_EINVAL, "gs_read_median_state needs a GS_MODEL_MEDIAN context (a rumor set: gs_read_rumorset)");
  return median_read_state(c, st, n);
}

int gs_timing_get(gs_ctx* c, gs_timing* out) {
  if (!c || !out) return GS_EINVAL;
  *out = c->group ? c->gr.mem[0]->timing : c->timing;  // a group: its first member's kernels
  if (c->group) out->overlay_ms = c->timing.overlay_ms;
  out->pp_early_rounds = out->pp_bottom_rounds = out->pp_answer_rounds = 0;
  gs_ctx* pc = c->group ? c->gr.mem[0] : c;  // a group: its first shard's rounds (all shards run the same modes)
  if (c->pp && pc->sp.ctl && c->begun) {
    CK(pc, hipSetDevice(pc->dev));
    PPCtl h;
    CK(pc, hipMemcpyAsync(&h, pc->sp.ctl, offsetof(PPCtl, segcnt), hipMemcpyDeviceToHost, pc->stream));
    CK(pc, hipStreamSynchronize(pc->stream));
    out->pp_early_rounds = h.nearly;
    out->pp_bottom_rounds = h.nbottom;
    out->pp_answer_rounds = h.nanswer;
  }
  if (c->pp && c->begun) out->pp_early_rounds += c->rs.rep_rounds;  // shards: the replicas' sparse rounds
  fill_devmem(out);
  return GS_OK;
}

int gs_shard_timing(gs_ctx* c, uint32_t index, gs_timing* out) {
  if (!c || !out) return GS_EINVAL;
  if (!c->group) return index == 0 ? gs_timing_get(c, out) : fail(c, GS_EINVAL, "no such shard");
  if (index >= c->gr.mem.size()) return fail(c, GS_EINVAL, "no such shard");
  *out = c->gr.mem[index]->timing;
  fill_devmem(out);
  return GS_OK;
}

int gs_set_trial(gs_ctx* c, uint32_t trial) {
  if (!c) return GS_EINVAL;
  if (c->begun) return fail(c, GS_EINVAL, "gs_reset before gs_set_trial");
  if (c->group) {
    uint32_t t = trial;
    for (gs_ctx* m : c->gr.mem) {
      RC(gs_set_trial(m, c->gtrials ? t : trial) ? fail(c, GS_EINVAL, m->err) : 0);
      t += m->trials;
    }
    // push-pull shards: the replicas run the sparse early rounds under the same key
    for (gs_ctx* r : c->gr.reps)
      if (r) r->p.trial = r->st.key.trial = trial;
    c->p.trial = trial;
    c->peers = false;
    return GS_OK;
  }
  if (c->rs.rep && c->rs.own_rep) c->rs.rep->p.trial = c->rs.rep->st.key.trial = trial;  // (a rank's own replica)
  c->p.trial = trial;
  c->st.key.trial = trial;
  c->ws.key.trial = trial;
  c->pt.key.trial = trial;
  c->peers = false;  // the overlay of the new trials is still to be built (or loaded)
  reset_counters(c);
  return GS_OK;
}

int gs_set_flags(gs_ctx* c, uint32_t flags) {
  if (!c) return GS_EINVAL;
  c->p.flags = flags;
  for (gs_ctx* m : c->gr.mem) m->p.flags = flags;
  return GS_OK;
}

int gs_reset(gs_ctx* c) {
  if (!c) return GS_EINVAL;
  for (gs_ctx* m : c->gr.mem) RC(gs_reset(m) ? fail(c, GS_EDEVICE, m->err) : 0);
  if (!c->group) {
    CK(c, hipSetDevice(c->dev));
    // everything in the state block except the stats ring, then the error
    // word (a broadcast that overflowed -- kErrArrivals, or a partition flag
    // -- leaves the context usable; table validation reports at load time)
    CK(c, hipMemsetAsync(c->d_state, 0, (char*)c->st.stats - (char*)c->d_state, c->stream));
    if (c->d_err) CK(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
    if (c->d_cnt) CK(c, hipMemsetAsync(c->d_cnt, 0, c->st.n * 4, c->stream));
    if (c->win) CK(c, hipMemsetAsync(c->ws.fcount, 0, c->wn.fcount_bytes, c->stream));
    if (c->failed && !c->pp_shard)
      CK(c, hipMemcpyAsync(c->st.crash, c->d_failed, c->st.W * 8, hipMemcpyDeviceToDevice, c->stream));
    if (c->pp_shard)  // this shard's slice of the replicated informed set
      CK(c, hipMemsetAsync(c->st.recv, 0, c->st.W * 8, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  }
  reset_counters(c);
  c->begun = false;
  return GS_OK;
}

void gs_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const u32x4 r = philox(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

}  // extern "C"
