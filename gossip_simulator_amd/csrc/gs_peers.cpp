// gs_peers.cpp -- peer tables and the overlay: loading, validating, sealing
// and partitioning a table, building the overlay into it, failure masks.
#include "gs_ctx.h"

namespace {

__global__ void k_validate_peers(const uint8_t* deg, const uint32_t* ids, uint64_t n, uint64_t bound,
                                 uint32_t stride, uint32_t* err) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n;
       v += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = deg[v];
    if (d > stride) { atomicOr(err, 1u); continue; }
    for (uint32_t j = 0; j < d; ++j)
      if (ids[v * stride + j] >= bound) atomicOr(err, 2u);
  }
}

}  // namespace

namespace gs {

namespace {

int set_stride(gs_ctx* c, uint32_t stride) {
  if (stride < 2 || stride > 255) return fail(c, GS_EINVAL, "row stride must be in [2, 255]");
  if (c->win && stride > kWinMaxStride)
    return fail(c, GS_EINVAL, "rows longer than 32 need GS_FLAG_TICK_ENGINE (or fanin > 32 at create)");
  c->st.stride = stride;
  c->st.stride_magic = (uint32_t)((1ull << 32) / stride + 1);
  if (c->win) refresh_window(c);
  return GS_OK;
}

// Shard c keeps the sealed rows of its own nodes [lo, hi) (copied from the
// full table `deg` / `ids` of stride S on c's device): owner expand reads
// only the rows of its own firing nodes.
int own_rows(gs_ctx* c, const uint8_t* deg, const uint32_t* ids, uint32_t S, uint32_t row_slots, hipStream_t st) {
  const uint64_t n = c->ntot;
  if (c->d_deg) (void)dev_free(c->d_deg);
  if (c->d_ids) (void)dev_free(c->d_ids);
  c->d_deg = nullptr;
  c->d_ids = nullptr;
  c->tab_stride = 0;  // not the full-table shape: the next load reallocates
  if (dev_malloc(&c->d_deg, n) != hipSuccess || dev_malloc(&c->d_ids, n * S * 4ull) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the shard's rows");
  RC(set_stride(c, S));
  c->row_slots = row_slots;
  refresh_state(c);
  CK(c, hipMemcpyAsync(c->d_deg, deg + c->lo, n, hipMemcpyDeviceToDevice, st));
  CK(c, hipMemcpyAsync(c->d_ids, ids + c->lo * S, n * S * 4ull, hipMemcpyDeviceToDevice, st));
  CK(c, hipStreamSynchronize(st));
  ++c->table_ver;
  return GS_OK;
}

// Push-pull shards: each member keeps the rows of its own nodes (its callers)
// and the reverse table of its own nodes (in-edges from every caller), built
// from the leader's full table, which is then dropped.
int partition_pp(gs_ctx* leader, const std::vector<gs_ctx*>& ms) {
  uint8_t* fdeg = leader->d_deg;
  uint32_t* fids = leader->d_ids;
  const uint32_t S = leader->st.stride, slots = leader->row_slots;
  const uint64_t N = leader->p.n;
  leader->d_deg = nullptr;
  leader->d_ids = nullptr;
  leader->tab_stride = 0;
  int rc = GS_OK;
  for (gs_ctx* m : ms) {
    const uint64_t n = m->ntot;
    if (m->d_deg) (void)dev_free(m->d_deg);
    if (m->d_ids) (void)dev_free(m->d_ids);
    m->d_deg = nullptr;
    m->d_ids = nullptr;
    if (dev_malloc(&m->d_deg, n) != hipSuccess || dev_malloc(&m->d_ids, n * S * 4ull) != hipSuccess) {
      rc = fail(m, GS_ENOMEM, "cannot allocate the shard's rows");
      break;
    }
    m->tab_stride = 0;  // not the full-table shape: the next load reallocates
    if ((rc = set_stride(m, S))) break;
    refresh_state(m);
    if (hipMemcpyAsync(m->d_deg, fdeg + m->lo, n, hipMemcpyDeviceToDevice, leader->stream) != hipSuccess ||
        hipMemcpyAsync(m->d_ids, fids + m->lo * S, n * S * 4ull, hipMemcpyDeviceToDevice, leader->stream) !=
            hipSuccess) {
      rc = fail(m, GS_EDEVICE, "copying the shard's rows failed");
      break;
    }
    // reverse table of [lo, hi): count + scan, then size the edge arrays
    const size_t scan = pp_rev_range_scan_bytes(n);
    if (!grow(m->sr.rend, (n + 1) * 8) || !grow(m->sr.scan, scan + 256) || !grow(m->sr.ctlb, sizeof(PPCtl))) {
      rc = fail(m, GS_ENOMEM, "cannot allocate the shard's reverse table");
      break;
    }
    unsigned long long* rend = (unsigned long long*)m->sr.rend.p;
    if (pp_rev_count_range(fdeg, fids, N, S, m->lo, m->hi, rend, m->sr.scan.p, m->sr.scan.bytes, leader->stream) !=
        hipSuccess) {
      rc = fail(m, GS_EDEVICE, "counting the shard's in-edges failed");
      break;
    }
    unsigned long long E = 0;
    if (hipMemcpyAsync(&E, rend + n, 8, hipMemcpyDeviceToHost, leader->stream) != hipSuccess ||
        hipStreamSynchronize(leader->stream) != hipSuccess) {
      rc = fail(m, GS_EDEVICE, "reading the shard's in-edge count failed");
      break;
    }
    if (!grow(m->sr.rsrc, std::max<uint64_t>(E, 1) * 4) || !grow(m->sr.rslot, std::max<uint64_t>(E, 1))) {
      rc = fail(m, GS_ENOMEM, "cannot allocate the shard's in-edges");
      break;
    }
    if (pp_rev_fill_range(fdeg, fids, N, S, m->lo, m->hi, rend, (uint32_t*)m->sr.rsrc.p, (uint8_t*)m->sr.rslot.p,
                          leader->stream) != hipSuccess ||
        hipStreamSynchronize(leader->stream) != hipSuccess) {
      rc = fail(m, GS_EDEVICE, "filling the shard's in-edges failed");
      break;
    }
    ++m->table_ver;
    m->sr.rev_ver = m->table_ver;
    m->sr.fm_tver = ~0ull;
    m->peers = true;
  }
  gs_ctx* r = ms[0]->rs.rep;
  if (r && rc == GS_OK) {  // the full table stays on the device as the replica's
    if (r->d_deg) (void)dev_free(r->d_deg);
    if (r->d_ids) (void)dev_free(r->d_ids);
    r->d_deg = fdeg;
    r->d_ids = fids;
    r->tab_stride = S;
    r->row_slots = slots;
    if ((rc = set_stride(r, S))) return fail(leader, rc, r->err);
    refresh_state(r);
    ++r->table_ver;
    r->peers = true;
    return GS_OK;
  }
  (void)dev_free(fdeg);
  (void)dev_free(fids);
  return rc;
}

struct WinSink {
  gs_window* win;
  size_t cap, n;
  static void push(void* self, uint64_t tick, uint64_t mk, uint64_t bk) {
    WinSink* w = (WinSink*)self;
    if (w->win && w->n < w->cap) w->win[w->n] = gs_window{tick, mk, bk};
    ++w->n;
  }
};

}  // namespace

// Nodes of the table this context loads: a shard loads the whole (replicated)
// table and keeps its partition.
uint64_t table_n(const gs_ctx* c) { return c->shard ? c->p.n : c->ntot; }

int alloc_table(gs_ctx* c, uint32_t stride) {
  const uint64_t n = table_n(c);
  if (!(c->d_deg && c->d_ids && c->tab_stride == stride)) {  // same shape: reuse (batch after batch)
    if (c->d_deg) (void)dev_free(c->d_deg);
    if (c->d_ids) (void)dev_free(c->d_ids);
    c->d_deg = nullptr;
    c->d_ids = nullptr;
    c->tab_stride = 0;
    if (dev_malloc(&c->d_deg, n) != hipSuccess || dev_malloc(&c->d_ids, n * stride * 4ull) != hipSuccess)
      return fail(c, GS_ENOMEM, "cannot allocate the peer table on the device");
    c->tab_stride = stride;
  }
  RC(set_stride(c, stride));
  refresh_state(c);
  return GS_OK;
}

// (with the packed view expand_view builds beside the table)
void release_table(gs_ctx* c) {
  for (void* p : {(void*)c->d_deg, (void*)c->d_ids, (void*)c->d_pk})
    if (p) (void)dev_free(p);
}

int validate_table(gs_ctx* c, const uint8_t* deg, const uint32_t* ids, uint64_t n, uint64_t bound) {
  CK(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
  const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_validate_peers, dim3((uint32_t)blocks), dim3(256), 0, c->stream, deg, ids, n, bound,
                     c->st.stride, c->d_err);
  CK(c, hipGetLastError());
  uint32_t e = 0;
  CK(c, hipMemcpyAsync(&e, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  if (e & 1) return fail(c, GS_EINVAL, "a friends-list length exceeds the row stride");
  if (e & 2) return fail(c, GS_EINVAL, "a friend id is >= n");
  return GS_OK;
}

// The window engine reads friend rows without the length byte: slots past a
// node's list are set to kEmptyMsg on the device copy.
int seal_rows(gs_ctx* c, const uint8_t* deg, uint32_t* ids, uint64_t n) {
  ++c->table_ver;  // every table change ends here
  if (!c->win) return GS_OK;
  CK(c, win_seal_rows(deg, ids, n, c->st.stride, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

// k_expand's packed view of the sealed rows (stride 8, rows <= 6 slots: C5's
// fanin 6): five 24-B rows per 128-B line instead of four 32-B ones, built
// once per table version (k_pack_rows, outside any timed step), about 0.8 of
// the table's bytes beside it.  Other shapes -- and GS_NO_PACK=1, an A/B
// knob -- read the table itself.  Called before every window run.
int expand_view(gs_ctx* c) {
  static const bool off = getenv("GS_NO_PACK") != nullptr;
  if (!c->win || c->pp || off || c->st.stride != 8 || c->ws.slots > 6 || !c->d_ids) {
    c->ws.pk = nullptr;
    return GS_OK;
  }
  if (c->pk_ver != c->table_ver || !c->d_pk) {
    const uint64_t rows = c->ntot, bytes = (rows + 4) / 5 * 128;
    if (c->pk_bytes < bytes) {
      if (c->d_pk) (void)dev_free(c->d_pk);
      c->d_pk = nullptr;
      c->pk_bytes = 0;
      if (dev_malloc(&c->d_pk, bytes) != hipSuccess) {  // no room: expand reads the table itself
        (void)hipGetLastError();
        c->d_pk = nullptr;
        c->ws.pk = nullptr;
        return GS_OK;
      }
      c->pk_bytes = bytes;
    }
    CK(c, win_pack_rows(c->d_ids, rows, c->d_pk, c->stream));
    c->pk_ver = c->table_ver;
  }
  c->ws.pk = c->d_pk;
  return GS_OK;
}

// Uploads a host table into `c`'s table buffers (c = a plain/batched context,
// or the device leader of shards) and validates it.
int upload_table(gs_ctx* c, const uint8_t* deg, const uint32_t* ids, uint32_t stride) {
  CK(c, hipSetDevice(c->dev));
  const uint32_t S = stride < 2 ? 2 : stride;
  c->row_slots = 0;  // injected rows are used as given
  RC(alloc_table(c, S));
  const uint64_t n = table_n(c);
  if (c->trials > 1) {  // trial tables back to back -> the padded id space
    const uint64_t np = c->p.n, per = 1ull << c->tlog;
    std::vector<uint8_t> hd(n, 0);
    std::vector<uint32_t> hi(n * S, 0);
    for (uint32_t t = 0; t < c->trials; ++t)
      for (uint64_t v = 0; v < np; ++v) {
        const uint64_t src = t * np + v, dst = t * per + v;
        const uint32_t d = deg[src];
        if (d > stride) return fail(c, GS_EINVAL, "a friends-list length exceeds the row stride");
        hd[dst] = (uint8_t)d;
        for (uint32_t j = 0; j < d; ++j) {
          const uint32_t x = ids[src * stride + j];
          if (x >= np) return fail(c, GS_EINVAL, "a friend id is >= n");
          hi[dst * S + j] = (uint32_t)(t * per) | x;
        }
      }
    CK(c, hipMemcpyAsync(c->d_deg, hd.data(), n, hipMemcpyHostToDevice, c->stream));
    CK(c, hipMemcpyAsync(c->d_ids, hi.data(), n * S * 4, hipMemcpyHostToDevice, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    return GS_OK;
  }
  CK(c, hipMemcpyAsync(c->d_deg, deg, n, hipMemcpyHostToDevice, c->stream));
  if (S == stride) {
    CK(c, hipMemcpyAsync(c->d_ids, ids, n * S * 4, hipMemcpyHostToDevice, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  } else {
    std::vector<uint32_t> tmp(n * S, 0);
    for (uint64_t v = 0; v < n; ++v) tmp[v * S] = ids[v];
    CK(c, hipMemcpyAsync(c->d_ids, tmp.data(), n * S * 4, hipMemcpyHostToDevice, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  }
  return validate_table(c, c->d_deg, c->d_ids, n, c->p.n);
}

// Shards: partition every member on the leader's device from the leader's
// sealed table, then drop the replicated table.
int partition_from(gs_ctx* leader, const std::vector<gs_ctx*>& ms) {
  if (leader->pp_shard) return partition_pp(leader, ms);
  uint8_t* fdeg = leader->d_deg;
  uint32_t* fids = leader->d_ids;
  const uint32_t S = leader->st.stride, slots = leader->row_slots;
  leader->d_deg = nullptr;  // own_rows must not free the full table it copies from
  leader->d_ids = nullptr;
  int rc = GS_OK;
  for (gs_ctx* m : ms) {
    if ((rc = own_rows(m, fdeg, fids, S, slots, leader->stream))) break;
    m->peers = true;
  }
  (void)dev_free(fdeg);
  (void)dev_free(fids);
  return rc;
}

// Members sharing device d (group) or just c.
std::vector<gs_ctx*> on_device(gs_ctx* g, size_t d) {
  std::vector<gs_ctx*> v;
  for (size_t i = 0; i < g->gr.mem.size(); ++i)
    if ((size_t)g->gr.dev_of[i] == d) v.push_back(g->gr.mem[i]);
  return v;
}

// The overlay of c's table_n(c) nodes (all trials of a batched context) into
// c's table buffers.
int overlay_into(gs_ctx* c, uint64_t max_ticks, gs_window* win, size_t cap, size_t* nwin, uint64_t* final_tick) {
  CK(c, hipSetDevice(c->dev));
  const uint32_t fo = (uint32_t)c->p.fanout, fi = (uint32_t)c->p.fanin;
  uint32_t stride = fo > fi ? fo : fi;
  if (stride < 2) stride = 2;
  // Window engine: rows of 5..7 slots are padded to 8 (32 B, 16-B aligned):
  // a row never straddles two 128-B lines and k_expand gathers it with one
  // uint4 + one uint2 load instead of three uint2 loads (C5: 67.3 -> 66.3 ms
  // per broadcast).  gs_read_peers returns the unpadded rows.
  // Rows of 9..31 slots (C4: fanin 19) are padded to a multiple of 4: 16-B
  // aligned rows gathered with uint4 loads.
  c->row_slots = 0;
  if (c->win && stride > 4 && stride < 8) {
    c->row_slots = stride;
    stride = 8;
  } else if (c->win && stride > 8 && (stride & 3)) {
    c->row_slots = stride;
    stride = (stride + 3) & ~3u;
  }
  RC(alloc_table(c, stride));
  const uint64_t n = table_n(c);
  CK(c, hipMemsetAsync(c->d_ids, 0, n * stride * 4ull, c->stream));
  CK(c, hipMemsetAsync(c->d_deg, 0, n, c->stream));
  WinSink ws{win, cap, 0};
  OverlayResult res;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = overlay_build(c->p.n, c->trials, c->tlog, c->p.fanout, c->p.fanin, c->p.delay_low,
                               c->p.delay_high, c->st.key, c->d_deg, c->d_ids, stride, max_ticks, c->stream,
                               OverlayWindowSink{&WinSink::push, &ws}, &res, &c->ovw);
  c->timing.overlay_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->timing.ov_part_ticks = c->ovw.part_ticks;
  c->timing.ov_sort_ticks = c->ovw.sort_ticks;
  c->timing.ov_part_fallbacks = c->ovw.part_fallbacks;
  if (nwin) *nwin = ws.n;
  if (final_tick) *final_tick = res.final_tick;
  // batched contexts rebuild per batch (gs_set_trial): keep the workspace
  if (c->trials <= 1) overlay_free(&c->ovw, c->stream);
  if (rc) return fail(c, rc, res.msg);
  return seal_rows(c, c->d_deg, c->d_ids, n);
}

// The body of gs_set_failed: a group hands every member its part.
int set_failed(gs_ctx* c, const uint64_t* words, size_t nwords) {
  if (!c || !words || nwords < (c->p.n + 63) / 64) return fail(c, GS_EINVAL, "mask needs ceil(n/64) words");
  if (c->begun) return fail(c, GS_EINVAL, "failure mask must be set before gs_broadcast_begin");
  const uint64_t Wn = (c->p.n + 63) / 64;
  if (c->trials > 1 && nwords < Wn * c->trials)
    return fail(c, GS_EINVAL, "batched trials: the mask needs ceil(n/64) words per trial, trial-major");
  if (c->group && c->gtrials) {  // every member its own trials' masks
    // devices may grant different LDS: every member's limit is checked before
    // any member takes a mask, so a refusal leaves the whole context unmasked
    for (gs_ctx* m : c->gr.mem) {
      PptPlan plan;
      std::string why;
      if (m->ppt)
        if (int rc = ppt_masked_plan(m, &plan, why)) return fail(c, rc, why);
    }
    uint64_t off = 0;
    for (gs_ctx* m : c->gr.mem) {
      if (int rc = set_failed(m, words + off * Wn, (size_t)m->trials * Wn)) return fail(c, rc, m->err);
      off += m->trials;
    }
    c->failed = true;
    return GS_OK;
  }
  if (c->trials > 1) {  // trial i's words to its slot of the padded id space (tlog >= 14: whole words)
    CK(c, hipSetDevice(c->dev));
    uint32_t lds_masked = 0;
    if (c->ppt) {  // the masked kernel keeps a third bitset in LDS
      PptPlan plan;
      std::string why;
      if (int rc = ppt_masked_plan(c, &plan, why)) return fail(c, rc, why);
      if (plan.lds_bytes > 65536) CK(c, ppt_prepare(c->dev, true, (uint32_t)plan.lds_bytes));
      lds_masked = (uint32_t)plan.lds_bytes;
    }
    const uint64_t W = c->st.W;
    std::vector<uint64_t> w(words, words + Wn * c->trials);
    if (c->p.n & 63)
      for (uint32_t t = 0; t < c->trials; ++t) w[(t + 1) * Wn - 1] &= (1ull << (c->p.n & 63)) - 1;
    if (!c->d_failed && dev_malloc(&c->d_failed, W * 8) != hipSuccess)
      return fail(c, GS_ENOMEM, "cannot allocate the failure mask");
    CK(c, hipMemsetAsync(c->d_failed, 0, W * 8, c->stream));
    CK(c, hipMemcpy2DAsync(c->d_failed, ((size_t)1 << c->tlog) / 8, w.data(), Wn * 8, Wn * 8, c->trials,
                           hipMemcpyHostToDevice, c->stream));
    CK(c, hipMemcpyAsync(c->st.crash, c->d_failed, W * 8, hipMemcpyDeviceToDevice, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->failed = true;
    c->st.check_crashed = 1;
    ++c->fail_ver;
    if (c->ppt) {
      c->pt.crash = c->st.crash;
      c->pt.lds_masked = lds_masked;
    }
    return GS_OK;
  }
  if (c->group) {
    for (gs_ctx* m : c->gr.mem)
      if (set_failed(m, words, nwords)) return fail(c, GS_EINVAL, m->err);
    c->failed = true;
    return GS_OK;
  }
  CK(c, hipSetDevice(c->dev));
  if (c->pp_shard) {  // the replicated failed set: every word (k_ppb_round reads the callers' friends)
    if (c->st.stride > 8) return fail(c, GS_EINVAL, "push-pull shards take a failure mask with rows <= 8 slots");
    const uint64_t Wg = (c->p.n + 63) / 64;
    std::vector<uint64_t> w(words, words + Wg);
    if (c->p.n & 63) w[Wg - 1] &= (1ull << (c->p.n & 63)) - 1;
    CK(c, hipMemcpyAsync(c->rs.d_fg, w.data(), Wg * 8, hipMemcpyHostToDevice, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    c->failed = true;
    c->st.check_crashed = 1;
    ++c->fail_ver;
    if (c->rs.rep) {  // the replica reads the same replicated failed set
      c->rs.rep->failed = true;
      c->rs.rep->st.check_crashed = 1;
      ++c->rs.rep->fail_ver;
    }
    return GS_OK;
  }
  const uint64_t W = c->st.W, w0 = c->lo / 64;  // this context's words (a shard's own range)
  std::vector<uint64_t> w(words + w0, words + w0 + W);
  if (c->ntot & 63) w[W - 1] &= (1ull << (c->ntot & 63)) - 1;
  if (!c->d_failed && dev_malloc(&c->d_failed, W * 8) != hipSuccess)
    return fail(c, GS_ENOMEM, "cannot allocate the failure mask");
  CK(c, hipMemcpyAsync(c->d_failed, w.data(), W * 8, hipMemcpyHostToDevice, c->stream));
  CK(c, hipMemcpyAsync(c->st.crash, c->d_failed, W * 8, hipMemcpyDeviceToDevice, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  c->failed = true;
  c->st.check_crashed = 1;
  ++c->fail_ver;
  return GS_OK;
}

}  // namespace gs
