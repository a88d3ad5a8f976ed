// gs_pushpull_host.cpp -- the host side of push-pull: sparse-round buffers,
// node-range shards and their exchanges, batched trials and their accounting.
#include "gs_ctx.h"

namespace gs {

namespace {

size_t fmask_bytes(uint64_t n) { return ((n + 7) & ~7ull) + ((n + 63) >> 6) * 8; }
unsigned long long* fmask_any(gs_ctx* c) {
  return (unsigned long long*)((char*)c->sr.fmask.p + ((c->st.n + 7) & ~7ull));
}

// ---- push-pull node-range shards (SURVEY.md 8(e)2 for config C5) -------------
// Every shard owns nodes [lo, hi): their rows (calls) and their in-edges
// (pushes they receive), and a replicated copy of the informed set by global
// id.  A round is bottom-up on the own nodes against the replicated set
// (k_ppb_round: same draws and counters as the unsharded rounds, so the union
// equals the unsharded run bit for bit); then the shards exchange their own
// informed words: events only between members that share a device's arrays,
// peer copies between devices, an all-gather between ranks.
int pp_exchange(gs_ctx* acc, const std::vector<gs_ctx*>& ms) {
  if (!acc->group) return x_all_gather(acc, acc->rs.d_ig, acc->rs.segw * 8);
  const bool multi = acc->gr.devs.size() > 1;
  for (size_t i = 0; i < ms.size(); ++i) {
    CK(ms[i], hipSetDevice(ms[i]->dev));
    CK(ms[i], hipEventRecord(acc->gr.ev_c[i], ms[i]->stream));
  }
  if (multi) {
    for (size_t d = 0; d < acc->gr.devs.size(); ++d) {
      gs_ctx* L = nullptr;
      for (size_t i = 0; i < ms.size() && !L; ++i)
        if ((size_t)acc->gr.dev_of[i] == d) L = ms[i];
      CK(L, hipSetDevice(L->dev));
      for (size_t j = 0; j < ms.size(); ++j) {
        const size_t dj = (size_t)acc->gr.dev_of[j];
        if (dj == d) continue;
        CK(L, hipStreamWaitEvent(L->stream, acc->gr.ev_c[j], 0));
        const size_t off = (size_t)ms[j]->rank * ms[j]->rs.segw;
        CK(L, hipMemcpyPeerAsync(acc->gr.ig[d] + off, L->dev, acc->gr.ig[dj] + off, ms[j]->dev, ms[j]->rs.segw * 8,
                                 L->stream));
      }
      CK(L, hipEventRecord(acc->gr.ev_x[d], L->stream));
    }
  }
  for (size_t i = 0; i < ms.size(); ++i) {
    gs_ctx* m = ms[i];
    CK(m, hipSetDevice(m->dev));
    for (size_t j = 0; j < ms.size(); ++j)
      if (j != i && acc->gr.dev_of[j] == acc->gr.dev_of[i]) CK(m, hipStreamWaitEvent(m->stream, acc->gr.ev_c[j], 0));
    if (multi) CK(m, hipStreamWaitEvent(m->stream, acc->gr.ev_x[acc->gr.dev_of[i]], 0));
  }
  return GS_OK;
}

// The replicas of a push-pull shard group (one per device) or rank (one).
std::vector<gs_ctx*> replicas_of(gs_ctx* c) {
  std::vector<gs_ctx*> v;
  if (c->group) {
    for (gs_ctx* r : c->gr.reps)
      if (r) v.push_back(r);
  } else if (c->rs.rep) {
    v.push_back(c->rs.rep);
  }
  return v;
}

// Members sharing a device share its informed set: no member may commit its
// round's new bits into it while another member's round still reads it.
int pp_barrier(gs_ctx* acc, const std::vector<gs_ctx*>& ms) {
  if (!acc->group) return GS_OK;
  for (size_t i = 0; i < ms.size(); ++i) {
    CK(ms[i], hipSetDevice(ms[i]->dev));
    CK(ms[i], hipEventRecord(acc->gr.ev_c[i], ms[i]->stream));
  }
  for (size_t i = 0; i < ms.size(); ++i) {
    CK(ms[i], hipSetDevice(ms[i]->dev));
    for (size_t j = 0; j < ms.size(); ++j)
      if (j != i && acc->gr.dev_of[j] == acc->gr.dev_of[i])
        CK(ms[i], hipStreamWaitEvent(ms[i]->stream, acc->gr.ev_c[j], 0));
  }
  return GS_OK;
}

// The unsharded engine's bottom-up threshold (pp_bottom_thr) for n nodes.
unsigned long long pp_bottom_thr_n(const gs_ctx* c, uint64_t n) {
  if (c->p.flags & GS_FLAG_PP_BOTTOM) return 0;
  const char* e = getenv("GS_PP_BOTTOM256");
  const unsigned long long k = (unsigned long long)std::min(std::max(e ? atoi(e) : 96, 0), 256);
  return k == 256 ? ~0ull : (unsigned long long)(((unsigned __int128)n * k) >> 8);
}

// A rank's pull-answer round set bits in other ranks' ranges of its d_gn:
// slice p goes to rank p (all-to-all), and the slices this rank receives are
// ORed into its own slice before the commit.
int pp_answer_exchange(gs_ctx* c) {
  const uint32_t G = c->G, me = c->rank;
  const uint64_t sw = c->rs.segw;
  unsigned long long* own = c->rs.d_gn + (size_t)me * sw;
  if (c->xc.comm) {
    const Rccl& r = rccl();
    NCK(c, r.group_start());
    for (uint32_t p = 0; p < G; ++p) {
      if (p == me) continue;
      NCK(c, r.send(c->rs.d_gn + (size_t)p * sw, sw, ncclUint64, (int)p, c->xc.comm, c->stream));
      NCK(c, r.recv(c->rs.d_gst + (size_t)p * sw, sw, ncclUint64, (int)p, c->xc.comm, c->stream));
    }
    NCK(c, r.group_end());
  } else {
    if (!grow_pinned(c, (size_t)2 * G * sw * 8)) return fail(c, GS_ENOMEM, "cannot allocate exchange staging");
    char* hs = c->xc.h_xbuf;
    char* hr = c->xc.h_xbuf + (size_t)G * sw * 8;
    std::vector<size_t> sb(G, sw * 8), rb(G, sw * 8);
    sb[me] = rb[me] = 0;
    // send blocks back to back in rank order without this rank's own slice
    size_t at = 0;
    for (uint32_t p = 0; p < G; ++p)
      if (p != me) {
        CK(c, hipMemcpyAsync(hs + at, c->rs.d_gn + (size_t)p * sw, sw * 8, hipMemcpyDeviceToHost, c->stream));
        at += sw * 8;
      }
    CK(c, hipStreamSynchronize(c->stream));
    if (c->xc.hx.all_to_allv(c->xc.hx.user, hs, sb.data(), hr, rb.data()))
      return fail(c, GS_EDEVICE, "the exchange's all_to_allv callback failed");
    at = 0;
    for (uint32_t p = 0; p < G; ++p)
      if (p != me) {
        CK(c, hipMemcpyAsync(c->rs.d_gst + (size_t)p * sw, hr + at, sw * 8, hipMemcpyHostToDevice, c->stream));
        at += sw * 8;
      }
  }
  CK(c, pp_or_slices(own, c->rs.d_gst, G, sw, c->stream));  // the own slot of d_gst stays zero
  return GS_OK;
}

}  // namespace

// Push-pull sparse-round buffers: the reverse table
// once per peer table, the failed-slot mask once per (table, failure mask),
// the informed list and round control.  GS_FLAG_PP_DENSE, or buffers that do
// not fit, leave the dense rounds only (same results).
// The failed-slot mask buffer: fmask bytes [n] (8-aligned), then the fany
// bitset [ceil(n / 64)] (pp_fmask_any).

// pp_seed on context c's state and stream: the live callers are counted
// once per (table, failure mask) version and reused after (a pass over the
// 1e9 degree bytes was 0.76 ms of every push-pull broadcast_begin).  Leaves
// the stream synchronized.
int pp_seed_ctx(gs_ctx* c, unsigned long long* next, uint32_t node, unsigned long long thr, unsigned long long bthr,
                unsigned long long athr) {
  const bool known = c->sp.ctl && c->sr.cl_tver == c->table_ver && c->sr.cl_fver == c->fail_ver;
  CK(c, pp_seed(c->st, next, node, c->d_flag, c->sp, thr, bthr, athr, known ? c->sr.cl_counts : nullptr, c->stream));
  if (c->sp.ctl && !known) {
    CK(c, hipMemcpyAsync(&c->sr.cl_counts[0], &c->sp.ctl->ncallers, 8, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipMemcpyAsync(&c->sr.cl_counts[1], &c->sp.ctl->nlive0, 8, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->sr.cl_tver = c->table_ver;
    c->sr.cl_fver = c->fail_ver;
  }
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

int pp_prepare(gs_ctx* c) {
  c->sp = PPSparse{};
  static const bool load_deg = [] { const char* e = getenv("GS_PP_NODEG"); return e && atoi(e) == 0; }();  // A/B
  c->sp.nodeg = load_deg ? 0u : 1u;
  // k_ppb_round's ranges: 2 = a lane per word where few nodes are uninformed
  // (default), 1 = always, 0 = never (GS_PPB_WORDS, A/B)
  static const uint32_t words = [] { const char* e = getenv("GS_PPB_WORDS"); return e ? (uint32_t)std::min(std::max(atoi(e), 0), 2) : 2u; }();
  c->sp.words = words;
  static const uint32_t maxu = [] { const char* e = getenv("GS_PPB_WORD_MAXU"); return e ? (uint32_t)std::max(atoi(e), 0) : 64u; }();
  c->sp.word_maxu = maxu;
  static const uint32_t maxi = [] { const char* e = getenv("GS_PPA_WORD_MAXI"); return e ? (uint32_t)std::max(atoi(e), 0) : 64u; }();
  c->sp.word_maxi = maxi;
  static const uint32_t pullfirst = [] { const char* e = getenv("GS_PPB_PULLFIRST"); return e && !atoi(e) ? 0u : 1u; }();
  c->sp.pullfirst = pullfirst;
  if (c->pp_shard) {  // bottom-up rounds only: the partition built the reverse table
    c->sp.ctl = (PPCtl*)c->sr.ctlb.p;
    c->sp.rend = (const unsigned long long*)c->sr.rend.p;
    c->sp.rsrc = (const uint32_t*)c->sr.rsrc.p;
    c->sp.rslot = (const uint8_t*)c->sr.rslot.p;
    if (c->failed) {
      if (c->sr.fm_tver != c->table_ver || c->sr.fm_fver != c->fail_ver) {
        if (!grow(c->sr.fmask, fmask_bytes(c->st.n))) return fail(c, GS_ENOMEM, "cannot allocate the failed-slot mask");
        CK(c, pp_fmask_rows(c->st, (uint8_t*)c->sr.fmask.p, c->stream));
        CK(c, pp_fmask_any((const uint8_t*)c->sr.fmask.p, c->st.n, fmask_any(c), c->stream));
        c->sr.fm_tver = c->table_ver;
        c->sr.fm_fver = c->fail_ver;
      }
      c->sp.fmask = (const uint8_t*)c->sr.fmask.p;
      c->sp.fany = fmask_any(c);
    }
    return GS_OK;
  }
  if (c->p.flags & GS_FLAG_PP_DENSE) return GS_OK;
  const DevState& s = c->st;
  const uint64_t n = s.n, E = n * s.stride;
  const auto t0 = std::chrono::steady_clock::now();
  bool built = false;
  if (c->sr.rev_ver != c->table_ver) {
    const size_t scan = pp_rev_scan_bytes(n);
    if (!grow(c->sr.rend, (n + 1) * 8) || !grow(c->sr.rsrc, E * 4) || !grow(c->sr.rslot, E) ||
        !grow(c->sr.scan, scan + 256) || !grow(c->sr.ilist, (n + kPPSegs) * 4) || !grow(c->sr.ctlb, sizeof(PPCtl))) {
      (void)hipGetLastError();
      return GS_OK;  // dense rounds only
    }
    // by partitioning (GS_PP_REV_ATOMIC=1: the atomic count + fill, A/B);
    // the atomic build also takes what the partition cannot (memory, skew)
    // (both switches read per call, so tests can force either path)
    const bool rev_atomic = getenv("GS_PP_REV_ATOMIC") != nullptr;
    bool part = false;
    uint32_t passes = 0;
    if (!rev_atomic) {
      part = pp_rev_build_part(s, (unsigned long long*)c->sr.rend.p, (uint32_t*)c->sr.rsrc.p,
                               (uint8_t*)c->sr.rslot.p, c->stream, &passes) == hipSuccess;
      if (!part) (void)hipGetLastError();
    }
    if (!part)
      CK(c, pp_rev_build(s, (unsigned long long*)c->sr.rend.p, (uint32_t*)c->sr.rsrc.p, (uint8_t*)c->sr.rslot.p,
                         c->sr.scan.p, c->sr.scan.bytes, c->stream));
    c->timing.pp_rev_part = part ? passes : 0;
    c->sr.rev_ver = c->table_ver;
    c->sr.fm_tver = ~0ull;
    built = true;
    // the dense rounds' compact view of rend (2.1 B per node instead of 8)
    c->sr.rend16_ok = false;
    const size_t r16 = (n * 2 + 255) / 256 * 256, rb = ((n >> 6) + 1) * 8;
    if (grow(c->sr.rend16, r16 + rb + 8)) {
      char* base = (char*)c->sr.rend16.p;
      uint32_t* ovf = (uint32_t*)(base + r16 + rb);
      uint32_t h_ovf = 1;
      CK(c, hipMemsetAsync(ovf, 0, 4, c->stream));
      CK(c, pp_rev_compact((const unsigned long long*)c->sr.rend.p, n, (uint16_t*)base,
                           (unsigned long long*)(base + r16), ovf, c->stream));
      CK(c, hipMemcpyAsync(&h_ovf, ovf, 4, hipMemcpyDeviceToHost, c->stream));
      CK(c, hipStreamSynchronize(c->stream));
      c->sr.rend16_ok = h_ovf == 0;
    } else {
      (void)hipGetLastError();  // rend only
    }
  }
  c->sp.ctl = (PPCtl*)c->sr.ctlb.p;
  c->sp.ilist = (uint32_t*)c->sr.ilist.p;
  c->sp.rend = (const unsigned long long*)c->sr.rend.p;
  c->sp.rsrc = (const uint32_t*)c->sr.rsrc.p;
  c->sp.rslot = (const uint8_t*)c->sr.rslot.p;
  // (GS_PP_REND16=0: the dense rounds read rend, A/B; read per call)
  if (c->sr.rend16_ok && !(getenv("GS_PP_REND16") && atoi(getenv("GS_PP_REND16")) == 0)) {
    const size_t r16 = (n * 2 + 255) / 256 * 256;
    c->sp.rend16 = (const uint16_t*)c->sr.rend16.p;
    c->sp.rbase = (const unsigned long long*)((const char*)c->sr.rend16.p + r16);
  }
  // the pull-answer rounds' deferred sets (n <= 2^30; GS_PP_NODEFER=1: atomics, A/B):
  // lists, coarse and fine regions for 0.6 n sets each (more fall back to atomicOr)
  if (!getenv("GS_PP_NODEFER") && n <= (1ull << 30) && pp_rslot_packed(s.stride)) {
    const uint64_t nfine = (n + 16383) >> 14, want = n * 3 / 5;
    const uint64_t dcap = std::max<uint64_t>(4096, (want + kPPDLists - 1) / kPPDLists);
    const uint64_t ccap = std::max<uint64_t>(4096, (want + kPPDRegions - 1) / kPPDRegions), fcap = 16384;
    const size_t elems = (size_t)kPPDLists * dcap + (size_t)kPPDRegions * ccap + (size_t)nfine * fcap;
    if (grow(c->sr.dset, elems * 4) && grow(c->sr.dcnt, ((size_t)kPPDLists + kPPDRegions + nfine) * 8)) {
      c->sp.dset = (uint32_t*)c->sr.dset.p;
      c->sp.dcnt = (unsigned long long*)c->sr.dcnt.p;
      c->sp.dcap = dcap;
      c->sp.ccap = ccap;
      c->sp.fcap = fcap;
    } else {
      (void)hipGetLastError();  // atomics
    }
  }
  if (c->failed && s.stride <= 8) {  // the dense rounds read fmask instead of gathering failed words
    if (c->sr.fm_tver != c->table_ver || c->sr.fm_fver != c->fail_ver) {
      if (!grow(c->sr.fmask, fmask_bytes(n))) {
        (void)hipGetLastError();
        return GS_OK;
      }
      CK(c, pp_fmask_build(s, c->sp.rend, c->sp.rsrc, c->sp.rslot, (uint8_t*)c->sr.fmask.p, c->stream));
      CK(c, pp_fmask_any((const uint8_t*)c->sr.fmask.p, n, fmask_any(c), c->stream));
      // (optional: without it the answer test gathers the caller's failed word)
      if (grow(c->sr.rfail, ((n * s.stride + 31) >> 5) * 4 + 8))  // + the hub flag word
        CK(c, pp_rfail_build(s, c->sp.rend, c->sp.rsrc, c->sp.rslot, (uint32_t*)c->sr.rfail.p, c->stream));
      else
        (void)hipGetLastError();
      c->sr.fm_tver = c->table_ver;
      c->sr.fm_fver = c->fail_ver;
      built = true;
    }
    c->sp.fmask = (const uint8_t*)c->sr.fmask.p;
    c->sp.fany = fmask_any(c);
    c->sp.rfail = c->sr.rfail.p && !getenv("GS_PP_NORFAIL") ? (const uint32_t*)c->sr.rfail.p : nullptr;
  }
  if (built) {
    CK(c, hipStreamSynchronize(c->stream));
    c->timing.prep_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return GS_OK;
}

// (a shard's rend / scan / ctlb / rsrc / rslot are grown by partition_pp)
void release_sparse(gs_ctx* c) {
  PpSparseBufs& b = c->sr;
  for (Buf* q : {&b.rend, &b.rsrc, &b.rslot, &b.ilist, &b.fmask, &b.scan, &b.ctlb, &b.dset, &b.dcnt, &b.rfail, &b.rend16})
    release(*q);
}

// Early rounds while |I| <= n >> shift (GS_PP_SHIFT, default 8, for tuning).
uint32_t pp_shift() {
  const char* e = getenv("GS_PP_SHIFT");
  const int v = e ? atoi(e) : 8;
  return (uint32_t)std::min(std::max(v, 0), 63);
}

// Dense rounds run bottom-up once |I| >= n * GS_PP_BOTTOM256 / 256 (default
// 96), when the reverse table has packed slots and the failed mask (if any)
// has fmask.
unsigned long long pp_bottom_thr(const gs_ctx* c) {
  const bool can = c->sp.ctl && pp_rslot_packed(c->st.stride) && (!c->failed || c->sp.fmask);
  if (!can || (c->p.flags & GS_FLAG_PP_TOPDOWN)) return ~0ull;
  if (c->p.flags & GS_FLAG_PP_BOTTOM) return 0;
  const char* e = getenv("GS_PP_BOTTOM256");
  const unsigned long long k = (unsigned long long)std::min(std::max(e ? atoi(e) : 96, 0), 256);
  return k == 256 ? ~0ull : (unsigned long long)(((unsigned __int128)c->st.n * k) >> 8);
}

// simulator.go:239-241 for the push-pull extension: the owner informs the
// sender (unless failed), every shard resets its round control; the replicas
// (if any) start the broadcast's sparse early rounds.
int pp_shard_begin(gs_ctx* acc, uint64_t sender) {
  std::vector<gs_ctx*> ms = shards_of(acc);
  unsigned long long informed = 0;
  acc->rs.rep_live = false;
  acc->rs.rep_rounds = 0;
  std::vector<gs_ctx*> reps = replicas_of(acc);
  bool sparse = !reps.empty();
  for (gs_ctx* r : reps) {
    CK(r, hipSetDevice(r->dev));
    if (int rc = pp_prepare(r)) return fail(acc, rc, r->err);
    if (!r->sp.ctl || !r->sp.ilist) sparse = false;  // no sparse-round buffers: the shards run every round
  }
  if (sparse)
    for (gs_ctx* r : reps) {
      CK(r, hipSetDevice(r->dev));
      CK(r, hipMemsetAsync(r->d_next, 0, r->st.W * 8, r->stream));
      RC(pp_seed_ctx(r, r->d_next, (uint32_t)sender, r->st.n >> pp_shift(), ~0ull, ~0ull));
    }
  acc->rs.rep_live = sparse;
  acc->rs.pp_gn_ok = false;
  // pull-answer sharded rounds: between ranks (their bits in other ranks' ranges
  // move by an all-to-all) or among the shards of one device (one shared set);
  // shards over several devices of one group run bottom-up only
  const bool onedev = !acc->group || acc->gr.devs.size() == 1;
  bool answer = onedev && !getenv("GS_PP_SHARD_BOTTOM") && (!acc->xc.has_hx || acc->xc.hx.all_to_allv);
  // (pp_prepare builds a masked shard's fmask: the answer test reads it after every shard prepared --
  // read before, the first broadcast after gs_set_failed found none and ran bottom-up only)
  for (gs_ctx* m : ms) {
    CK(m, hipSetDevice(m->dev));
    if (int rc = pp_prepare(m)) return fail(acc, rc, m->err);
  }
  for (gs_ctx* m : ms) answer = answer && m->rs.d_gn && (!m->failed || m->sp.fmask);
  acc->rs.pp_answer = answer;
  for (gs_ctx* m : ms) {
    CK(m, hipSetDevice(m->dev));
    const uint32_t node = sender >= m->lo && sender < m->hi ? (uint32_t)(sender - m->lo) : ~0u;
    RC(pp_seed_ctx(m, m->d_next, node, 0ull, 0ull, ~0ull));
    uint32_t ok = 0;
    CK(m, hipMemcpyAsync(&ok, m->d_flag, 4, hipMemcpyDeviceToHost, m->stream));
    CK(m, hipStreamSynchronize(m->stream));
    informed += ok;
    reset_counters(m);
    m->begun = true;
  }
  if (!acc->group) RC(rank_sum(acc, &informed));  // every rank learns whether the owner informed the sender
  if (int rc = pp_exchange(acc, ms)) return abort_rank(acc, rc);
  acc->recv = acc->pending = informed;
  acc->begun = true;
  return GS_OK;
}

int pp_shard_step(gs_ctx* acc, uint32_t ticks, gs_tick_stats* out) {
  std::vector<gs_ctx*> ms = shards_of(acc);
  std::vector<gs_ctx*> reps = replicas_of(acc);
  uint32_t done = 0;
  while (done < ticks) {
    const uint32_t batch = std::min<uint32_t>(ticks - done, kStatSlots);
    const uint64_t t0 = acc->t + 1;
    const StatSpans sp = stat_spans(t0, batch);
    for (gs_ctx* m : ms) {
      CK(m, hipSetDevice(m->dev));
      for (int j = 0; j < sp.n; ++j) CK(m, hipMemsetAsync(m->st.stats + sp.off[j], 0, sp.words[j] * 8, m->stream));
    }
    for (gs_ctx* r : reps) {
      CK(r, hipSetDevice(r->dev));
      for (int j = 0; j < sp.n; ++j) CK(r, hipMemsetAsync(r->st.stats + sp.off[j], 0, sp.words[j] * 8, r->stream));
    }
    for (uint32_t i = 0; i < batch; ++i) {
      const uint32_t tt = (uint32_t)(t0 + i);
      if (acc->rs.rep_live) {
        // is this round a sparse early round on the replicas (k_pp_mode's test)?
        gs_ctx* r0 = reps[0];
        PPCtl h;
        CK(r0, hipSetDevice(r0->dev));
        CK(r0, hipMemcpyAsync(&h, r0->sp.ctl, offsetof(PPCtl, segcnt), hipMemcpyDeviceToHost, r0->stream));
        CK(r0, hipStreamSynchronize(r0->stream));
        if (h.early_ok && !h.ovf && h.ninf <= h.thr) {
          // every replica runs the same round: the replicated sets stay equal with no exchange
          for (gs_ctx* r : reps) {
            CK(r, hipSetDevice(r->dev));
            CK(r, pp_round(r->st, r->d_next, r->d_ppsum, tt, r->pp_l2_only, r->sp, r->stream));
            CK(r, pp_commit(r->st, r->d_next, tt, r->sp, r->stream));
          }
          for (gs_ctx* r : reps) {
            CK(r, hipSetDevice(r->dev));
            CK(r, hipStreamSynchronize(r->stream));
          }
          // the round's counters, once: the group's first member / rank 0
          if (acc->group || acc->rank == 0) {
            const size_t row = (size_t)(tt % kStatSlots) * kStatFields;
            CK(ms[0], hipSetDevice(ms[0]->dev));
            CK(ms[0], hipMemcpyAsync(ms[0]->st.stats + row, r0->st.stats + row, kStatFields * 8,
                                     hipMemcpyDeviceToDevice, ms[0]->stream));
          }
          ++acc->rs.rep_rounds;
          continue;
        }
        acc->rs.rep_live = false;  // the shards take over
      }
      if (!acc->rs.pp_gn_ok) {  // the round's set starts as the replicated set (per device / rank)
        std::vector<int> done(acc->group ? acc->gr.devs.size() : 1, 0);
        for (size_t i = 0; i < ms.size(); ++i) {
          gs_ctx* m = ms[i];
          const int d = acc->group ? acc->gr.dev_of[i] : 0;
          if (done[d]) continue;
          done[d] = 1;
          CK(m, hipSetDevice(m->dev));
          CK(m, hipMemcpyAsync(m->rs.d_gn, m->rs.d_ig, (size_t)m->G * m->rs.segw * 8, hipMemcpyDeviceToDevice, m->stream));
        }
        RC(pp_barrier(acc, ms));
        acc->rs.pp_gn_ok = true;
      }
      uint32_t mode = PP_BOTTOM;
      if (acc->rs.pp_answer) {  // pull-answer until |I| >= the unsharded engine's bottom-up threshold
        gs_ctx* m0 = ms[0];  // every shard's copy of the replicated set is the same
        unsigned long long* cnt = (unsigned long long*)(m0->d_err + 4);
        unsigned long long ninf = 0;
        CK(m0, hipSetDevice(m0->dev));
        CK(m0, pp_count(m0->rs.d_ig, (uint64_t)m0->G * m0->rs.segw, cnt, m0->stream));
        CK(m0, hipMemcpyAsync(&ninf, cnt, 8, hipMemcpyDeviceToHost, m0->stream));
        CK(m0, hipStreamSynchronize(m0->stream));
        if (ninf >= pp_bottom_thr_n(acc, acc->p.n)) acc->rs.pp_answer = false;
        else mode = PP_ANSWER;
      }
      for (gs_ctx* m : ms) {
        CK(m, hipSetDevice(m->dev));
        CK(m, pp_round_shard(m->st, m->rs.d_gn + (size_t)m->rank * m->rs.segw, m->rs.d_gn, tt, m->sp, mode, m->stream));
      }
      RC(pp_barrier(acc, ms));
      if (mode == PP_ANSWER && !acc->group)  // the bits this rank set in other ranks' ranges go to their owners
        if (int rc = pp_answer_exchange(acc)) return abort_rank(acc, rc);
      for (gs_ctx* m : ms) {
        CK(m, hipSetDevice(m->dev));
        CK(m, pp_commit(m->st, m->rs.d_gn + (size_t)m->rank * m->rs.segw, tt, m->sp, m->stream));
      }
      if (int rc = pp_exchange(acc, ms)) return abort_rank(acc, rc);
    }
    for (gs_ctx* m : ms) {
      CK(m, hipSetDevice(m->dev));
      for (int j = 0; j < sp.n && is_rank(m); ++j)  // the global per-round counters on every rank
        if (int rc = x_all_reduce(m, m->st.stats + sp.off[j], sp.words[j])) return abort_rank(m, rc);
      for (int j = 0; j < sp.n; ++j)
        CK(m, hipMemcpyAsync(m->h_stats + sp.off[j], m->st.stats + sp.off[j], sp.words[j] * 8, hipMemcpyDeviceToHost,
                             m->stream));
    }
    for (gs_ctx* m : ms) {
      CK(m, hipSetDevice(m->dev));
      CK(m, hipStreamSynchronize(m->stream));
    }
    account_members(acc, ms, t0, batch, out ? out + done : nullptr);
    done += batch;
  }
  return GS_OK;
}

// Dense rounds below the bottom-up threshold run pull-answer (informed nodes
// answer the pulls among their in-edges) once |I| >= n * GS_PP_ANSWER256 / 256
// (default 0: every such round; 256 = never, the top-down rounds), when the
// reverse table has packed slots and the failed mask (if any) has fmask.
unsigned long long pp_answer_thr(const gs_ctx* c) {
  const bool can = c->sp.ctl && pp_rslot_packed(c->st.stride) && (!c->failed || c->sp.fmask);
  if (!can || (c->p.flags & GS_FLAG_PP_TOPDOWN)) return ~0ull;
  if (c->p.flags & GS_FLAG_PP_ANSWER) return 0;
  const char* e = getenv("GS_PP_ANSWER256");
  const unsigned long long k = (unsigned long long)std::min(std::max(e ? atoi(e) : 0, 0), 256);
  return k == 256 ? ~0ull : (unsigned long long)(((unsigned __int128)c->st.n * k) >> 8);
}

// Batched trials: fold one chunk's per-trial counters (h_tstat, `nt` ticks
// from tick t0) into the trials' running totals; sums (if given, zeroed
// [nt][kStatFields]) gets each tick's stat row summed over the trials.
void account_trials(gs_ctx* c, uint64_t t0, uint32_t nt, unsigned long long* sums) {
  for (uint32_t tr = 0; tr < c->trials; ++tr) {
    TrialAcc& a = c->tacc[tr];
    for (uint32_t k = 0; k < nt; ++k) {
      const uint32_t* r = c->bt.h_tstat + ((size_t)tr * kMaxWindow + k) * kTStatFields;
      const uint64_t msgs = (uint64_t)r[TS_SENT] - r[TS_DEAD];
      a.fired += r[TS_FIRED];
      a.sent += r[TS_SENT];
      a.msgs += msgs;
      a.recv += r[TS_RECV];
      a.sched += r[TS_RECV];  // every infection schedules one Broadcast
      a.crash += r[TS_CRASH];
      if (!a.tick99 && covered(a.recv, c->p.n)) a.tick99 = t0 + k;
      if (!sums) continue;
      unsigned long long* s = sums + (size_t)k * kStatFields;
      s[ST_FIRED] += r[TS_FIRED];
      s[ST_SENT] += r[TS_SENT];
      s[ST_MSGS] += msgs;
      s[ST_RECV] += r[TS_RECV];
    }
  }
}

// Batched push-pull trials: `ticks` rounds of every trial, at most kMaxWindow
// per launch (the per-trial counter rows); out[k] = the sum of the trials' rows.
int ppt_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out) {
  CK(c, hipSetDevice(c->dev));
  const size_t tb = (size_t)c->trials * kMaxWindow * kTStatFields * 4;
  uint32_t done = 0;
  while (done < ticks) {
    const uint32_t batch = std::min<uint32_t>(ticks - done, kMaxWindow);
    const uint64_t t0 = c->t + 1;
    CK(c, ppt_rounds(c->pt, (uint32_t)t0, batch, c->stream));
    CK(c, hipMemcpyAsync(c->bt.h_tstat, c->bt.d_tstat, tb, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    unsigned long long s[kMaxWindow * kStatFields] = {0};
    account_trials(c, t0, batch, s);
    for (uint32_t k = 0; k < batch; ++k) account_tick(c, t0 + k, s + (size_t)k * kStatFields, out ? &out[done + k] : nullptr);
    done += batch;
  }
  return GS_OK;
}

void snap_trial(gs_ctx* c, uint32_t tr, int32_t status) {
  TrialAcc& a = c->tacc[tr];
  a.status = status;
  a.snap = gs_trial_stats{(uint64_t)c->p.trial + tr, a.tick99, c->t, a.fired, a.sent, a.msgs, a.recv,
                          a.crash, status, 0};
}

// Every trial of a batched context has stopped (`running` of them go on):
// the run's status is the latest stop among them.
bool trials_stopped(const gs_ctx* c, uint32_t running, int32_t* st) {
  if (running) return false;
  *st = GS_RUN_COVERED;
  for (const TrialAcc& a : c->tacc) *st = std::max(*st, a.status);
  return true;
}

// Push-pull's exact stop: can any call still change the informed set?
// Shards: their own callers' edges against the replicated sets, summed.
int pp_stalled(gs_ctx* c, bool* stalled) {
  *stalled = true;
  if (c->st.kd >= 100) return GS_OK;  // every call is lost (simulator.go:172 quantisation)
  unsigned long long live = 0;
  for (gs_ctx* m : shards_of(c)) {
    CK(m, hipSetDevice(m->dev));
    CK(m, pp_live_edges(m->st, m->d_err + 2, m->stream));
    uint32_t h = 0;
    CK(m, hipMemcpyAsync(&h, m->d_err + 2, 4, hipMemcpyDeviceToHost, m->stream));
    CK(m, hipStreamSynchronize(m->stream));
    live += h;
  }
  if (c->pp_shard && !c->group) RC(rank_sum(c, &live));  // a rank: the sum over the ranks
  *stalled = live == 0;
  return GS_OK;
}

// Batched push-pull trials after a poll: snaps every running trial that
// stops here -- covered; or the poll informed nobody new in it (r0: the
// trials' informed counts before the poll) and no call can change its
// informed set any more (pp_stalled's rule on the trial's own rows and bits,
// checked on the device for those trials only); or max_ticks -- and counts
// the rest.
int ppt_poll_stops(gs_ctx* c, const std::vector<uint64_t>& r0, uint64_t max_ticks, uint32_t* running) {
  const uint32_t T = c->trials;
  std::vector<uint8_t> need(T, 0);
  uint32_t nneed = 0;
  for (uint32_t tr = 0; tr < T; ++tr) {
    TrialAcc& a = c->tacc[tr];
    if (a.status != GS_RUN_RUNNING) continue;
    if (covered(a.recv, c->p.n)) snap_trial(c, tr, GS_RUN_COVERED);
    else if (a.recv == r0[tr]) { need[tr] = 1; ++nneed; }
  }
  std::vector<uint32_t> live(T, 0);
  if (nneed && c->st.kd < 100) {  // (kd >= 100: every call is lost, nothing is live)
    uint8_t* d_need = (uint8_t*)c->bt.chk.p;
    uint32_t* d_live = (uint32_t*)(d_need + (((size_t)T + 3) & ~(size_t)3));
    CK(c, hipSetDevice(c->dev));
    CK(c, hipMemcpyAsync(d_need, need.data(), T, hipMemcpyHostToDevice, c->stream));
    CK(c, hipMemsetAsync(d_live, 0, (size_t)T * 4, c->stream));
    CK(c, ppt_stalled(c->pt, d_need, d_live, c->stream));
    CK(c, hipMemcpyAsync(live.data(), d_live, (size_t)T * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  }
  *running = 0;
  for (uint32_t tr = 0; tr < T; ++tr) {
    if (c->tacc[tr].status != GS_RUN_RUNNING) continue;
    if (need[tr] && !live[tr]) snap_trial(c, tr, GS_RUN_QUIESCENT);
    else if (c->t >= max_ticks) snap_trial(c, tr, GS_RUN_MAX_TICKS);
    else ++*running;
  }
  return GS_OK;
}

}  // namespace gs
