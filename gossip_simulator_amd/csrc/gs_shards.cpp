// gs_shards.cpp -- flood node-range shards: the RCCL and host-callback
// exchanges, the five-step shard window, its device-driven twin (dd_run).
#include "gs_ctx.h"

namespace gs {

namespace {

// ---- node-range shards ------------------------------------------------------
// One window for shards `ms` (all shards of a group, or this rank's one shard
// with an exchange), SURVEY.md section 8(e)2 -- owner expand:
//   1. each shard counts its fires per tick; the counts are gathered, so every
//      shard cuts the same window (host sync 1);
//   2. each shard expands its OWN firing nodes (its own friend rows), binning
//      every kept message by the shard that owns its target;
//   3. the region fills and error words are gathered (host sync 2); a shard
//      whose size estimate overflowed redoes its expand with exact counts;
//   4. each shard packs the filled prefixes of its regions into one block per
//      destination, and the blocks move to their owners (device copies, RCCL
//      grouped send/recv, or the caller's all_to_allv);
//   5. each shard partitions and resolves the messages it received.
// Per shard, the expand reads 1/G of the window's rows and the resolve owns
// 1/G of the buckets, so the work per shard shrinks with G.
int sync_all(const std::vector<gs_ctx*>& ms) {
  for (gs_ctx* m : ms) {
    CK(m, hipSetDevice(m->dev));
    CK(m, hipStreamSynchronize(m->stream));
  }
  return GS_OK;
}

// A shard that cannot allocate a window buffer marks its error word
// (kErrNoMem) and keeps taking part in the window's collectives; every rank
// sees the mark at the next gather (counts, layouts, or the end-of-step
// check) and returns GS_ENOMEM there, so no rank waits on a peer that left.
int mark_nomem(gs_ctx* m, const std::string& what) {
  uint32_t e = 0;
  CK(m, hipMemcpyAsync(&e, m->d_err, 4, hipMemcpyDeviceToHost, m->stream));
  CK(m, hipStreamSynchronize(m->stream));
  e |= kErrNoMem;
  CK(m, hipMemcpyAsync(m->d_err, &e, 4, hipMemcpyHostToDevice, m->stream));
  CK(m, hipStreamSynchronize(m->stream));
  m->err = what;
  return GS_OK;
}

// Fire counts of the window's units and their scan; with gather, tfires
// (fires per tick, plus this shard's partition-overflow flag in slot 15) is
// gathered: every rank's into d_gcounts, or the member's into its h_misc.
constexpr uint32_t kFlagSlot = kMaxWindow - 1;
static_assert(kFlagSlot >= kBitTicks, "the flag slot is past the window's ticks");

int shard_units(gs_ctx* m, uint32_t t, uint32_t Lu, bool gather) {
  WinState& w = m->ws;
  CK(m, hipSetDevice(m->dev));
  CK(m, hipMemsetAsync(w.tfires, 0, kMaxWindow * 8, m->stream));
  CK(m, hipMemcpyAsync(w.tfires + kFlagSlot, m->d_err, 4, hipMemcpyDeviceToDevice, m->stream));
  CK(m, win_units(w, t, Lu, m->stream));
  size_t need = 0;
  CK(m, win_scan_units(w, Lu, nullptr, need, m->stream));
  if (!grow(m->wn.tmp, need)) {
    RC(mark_nomem(m, "cannot allocate scan scratch"));
    CK(m, hipMemcpyAsync(w.tfires + kFlagSlot, m->d_err, 4, hipMemcpyDeviceToDevice, m->stream));
  } else {
    need = m->wn.tmp.bytes;
    CK(m, win_scan_units(w, Lu, m->wn.tmp.p, need, m->stream));
  }
  if (!gather) return GS_OK;
  if (is_rank(m)) {
    CK(m, hipMemcpyAsync(m->xc.d_gcounts + (size_t)m->rank * kMaxWindow, w.tfires, kMaxWindow * 8,
                         hipMemcpyDeviceToDevice, m->stream));
    RC(x_all_gather(m, m->xc.d_gcounts, kMaxWindow * 8));
    CK(m, hipMemcpyAsync(m->wn.h_misc, m->xc.d_gcounts, (size_t)m->G * kMaxWindow * 8, hipMemcpyDeviceToHost,
                         m->stream));
  } else {
    CK(m, hipMemcpyAsync(m->wn.h_misc, w.tfires, kMaxWindow * 8, hipMemcpyDeviceToHost, m->stream));
  }
  return GS_OK;
}

// Serial shard pipelines (GS_SHARD_SERIAL=1, in-process shards): each shard's
// phases run alone on the device, so GS_FLAG_TIMING measures one shard's
// device time per window (bench.py's in-process scaling proxy).
bool shard_serial() { return getenv("GS_SHARD_SERIAL") != nullptr; }

// A shard window the host keeps until the next window's count sync has shown
// that no shard's receive-side partition overflowed.
struct ShardWin {
  uint32_t t = 0, L = 0;
  bool live = false;
};

// Coarse plan of shard c's outgoing messages (owner expand): bin b = d *
// obins + k holds the targets in chunk k (2^22 nodes) of shard d's range;
// each of its 8 sub-regions gets 1/8 of the chunk's node share of T plus 512,
// or exactly `exact[region]`.  Bins past G * obins and empty chunks get none.
void plan_coarse_owner(gs_ctx* c, uint64_t T, const unsigned long long* exact) {
  const WinState& w = c->ws;
  const uint64_t N = c->p.n;
  unsigned long long a = 0;
  for (uint32_t b = 0; b < 256; ++b) {
    const uint32_t d = b / w.obins, k = b % w.obins;
    uint64_t cnt = 0;
    if (d < w.G) {
      const uint64_t dlo = (uint64_t)d * c->seg_per, dhi = std::min<uint64_t>(dlo + c->seg_per, N);
      const uint64_t lo = dlo + ((uint64_t)k << kCoarseShift);
      const uint64_t hi = std::min<uint64_t>(dhi, lo + (1ull << kCoarseShift));
      cnt = hi > lo ? hi - lo : 0;
    }
    const double xr = (double)kXRoundNodes * w.slots;  // one expand round's slots (gs_internal.h)
    const unsigned long long sub =
        cnt ? (unsigned long long)(((double)T / kCoarseSub + xr) * (double)cnt / (double)N) + 512 : 0;
    for (uint32_t x = 0; x < kCoarseSub; ++x) {
      const uint32_t r = b * kCoarseSub + x;
      c->wn.h_cap[r] = a;
      if (cnt) a += exact ? exact[r] : sub;
    }
  }
  c->wn.h_cap[kRegions] = a;
}

int shard_events(gs_ctx* m, size_t k) {
  while (m->ev.size() < k) {
    hipEvent_t ev;
    CK(m, hipEventCreate(&ev));
    m->ev.push_back(ev);
  }
  return GS_OK;
}

// Step 2 on shard m: expand its Tn own fires of window [t, t + L).
int shard_expand(gs_ctx* m, uint32_t t, uint32_t L, uint64_t Tn, bool timing) {
  WinState& w = m->ws;
  CK(m, hipSetDevice(m->dev));
  plan_coarse_owner(m, Tn * w.slots, nullptr);
  if (!grow(m->wn.cmsg, (m->wn.h_cap[kRegions] + 16) * 4) || !grow(m->wn.gmap, ((Tn + 63) / 64 + 1) * 4))
    return mark_nomem(m, "cannot allocate " + std::to_string(m->wn.h_cap[kRegions]) + " window messages");
  w.cmsg = (uint32_t*)m->wn.cmsg.p;
  w.gmap = (uint32_t*)m->wn.gmap.p;
  w.tofs = 0;
  CK(m, hipMemcpyAsync(w.ccap, m->wn.h_cap, (kRegions + 1) * 8, hipMemcpyHostToDevice, m->stream));
  CK(m, win_groupmap(w, L, m->stream));
  if (timing) {
    RC(shard_events(m, 7));
    CK(m, hipEventRecord(m->ev[0], m->stream));
  }
  CK(m, win_expand(w, t, L, Tn, 1, m->stream));
  if (timing) CK(m, hipEventRecord(m->ev[1], m->stream));
  return GS_OK;
}

// Step 3: lay[s * (kRegions + 1) + r] = shard s's fill of region r, and
// lay[s * (kRegions + 1) + kRegions] = its error word.
int gather_layouts(const std::vector<gs_ctx*>& ms, std::vector<unsigned long long>& lay) {
  gs_ctx* m0 = ms[0];
  const size_t K1 = kRegions + 1;
  lay.assign((size_t)m0->G * K1, 0);
  if (is_rank(m0)) {
    gs_ctx* m = m0;
    unsigned long long* mine = m->xc.d_glay + (size_t)m->rank * K1;
    CK(m, hipMemcpyAsync(mine, m->ws.cfill, kRegions * 8, hipMemcpyDeviceToDevice, m->stream));
    CK(m, hipMemsetAsync(mine + kRegions, 0, 8, m->stream));
    CK(m, hipMemcpyAsync(mine + kRegions, m->d_err, 4, hipMemcpyDeviceToDevice, m->stream));
    RC(x_all_gather(m, m->xc.d_glay, K1 * 8));
    CK(m, hipMemcpyAsync(m->xc.h_glay, m->xc.d_glay, (size_t)m->G * K1 * 8, hipMemcpyDeviceToHost, m->stream));
    CK(m, hipStreamSynchronize(m->stream));
    std::copy(m->xc.h_glay, m->xc.h_glay + (size_t)m->G * K1, lay.begin());
    return GS_OK;
  }
  for (gs_ctx* m : ms) {
    CK(m, hipSetDevice(m->dev));
    CK(m, hipMemcpyAsync(m->wn.h_misc, m->ws.cfill, kRegions * 8, hipMemcpyDeviceToHost, m->stream));
    CK(m, hipMemcpyAsync(m->wn.h_err, m->d_err, 4, hipMemcpyDeviceToHost, m->stream));
  }
  RC(sync_all(ms));
  for (gs_ctx* m : ms) {
    std::copy(m->wn.h_misc, m->wn.h_misc + kRegions, lay.begin() + (size_t)m->rank * K1);
    lay[(size_t)m->rank * K1 + kRegions] = *m->wn.h_err;
  }
  return GS_OK;
}

// Clears the partition-overflow flags of m's error word (host round trip).
int clear_part_flags(gs_ctx* m) {
  uint32_t e = 0;
  CK(m, hipMemcpyAsync(&e, m->d_err, 4, hipMemcpyDeviceToHost, m->stream));
  CK(m, hipStreamSynchronize(m->stream));
  e &= ~(kErrCoarse | kErrFine);
  CK(m, hipMemcpyAsync(m->d_err, &e, 4, hipMemcpyHostToDevice, m->stream));
  return GS_OK;
}

// Shard m's expand overflowed a region estimate: count its messages per
// region, plan exactly and write them again (the stats were added by the
// first pass).  Rank-local.
int sender_redo(gs_ctx* m, uint32_t t, uint32_t L, uint64_t Tn) {
  WinState& w = m->ws;
  CK(m, hipSetDevice(m->dev));
  RC(clear_part_flags(m));
  CK(m, hipMemsetAsync(w.chist, 0, kRegions * 8, m->stream));
  CK(m, hipMemsetAsync(w.cfill, 0, kRegions * 8, m->stream));
  CK(m, win_expand(w, t, L, Tn, 0, m->stream));
  CK(m, hipMemcpyAsync(m->wn.h_misc, w.chist, kRegions * 8, hipMemcpyDeviceToHost, m->stream));
  CK(m, hipStreamSynchronize(m->stream));
  plan_coarse_owner(m, Tn * w.slots, m->wn.h_misc);
  if (!grow(m->wn.cmsg, (m->wn.h_cap[kRegions] + 16) * 4)) return mark_nomem(m, "cannot allocate the window messages");
  w.cmsg = (uint32_t*)m->wn.cmsg.p;
  CK(m, hipMemcpyAsync(w.ccap, m->wn.h_cap, (kRegions + 1) * 8, hipMemcpyHostToDevice, m->stream));
  CK(m, win_expand(w, t, L, Tn, 2, m->stream));
  ++m->timing.exact_redos;
  return GS_OK;
}

// A rank's local allocation result made collective: every rank returns
// GS_ENOMEM if any rank could not allocate (one u64 all-reduce).
int agree_ok(gs_ctx* m, bool ok, const char* what) {
  unsigned long long* d = m->xc.d_gcounts + (size_t)m->G * kMaxWindow;  // scratch
  m->wn.h_misc[8] = ok ? 0ull : 1ull;
  CK(m, hipMemcpyAsync(d, &m->wn.h_misc[8], 8, hipMemcpyHostToDevice, m->stream));
  RC(x_all_reduce(m, d, 1));
  CK(m, hipMemcpyAsync(&m->wn.h_misc[9], d, 8, hipMemcpyDeviceToHost, m->stream));
  CK(m, hipStreamSynchronize(m->stream));
  if (m->wn.h_misc[9]) return fail(m, GS_ENOMEM, ok ? std::string("another rank: ") + what : std::string(what));
  return GS_OK;
}

// Step 4: moves every block to its owner and sets each shard's receive
// layout (m->wr, m->xc.rtotal).  A block that stays on its device (in-process
// shards of one device; a rank's block to itself) is read in place from its
// sender's message buffer; the others are packed (filled prefixes back to
// back) and sent: peer copies between devices, RCCL grouped send / receive
// or the caller's all_to_allv between ranks.  Destination d's block of a
// sender is its regions [d * obins * 8, (d + 1) * obins * 8).
int shard_exchange(gs_ctx* acc, const std::vector<gs_ctx*>& ms, const std::vector<unsigned long long>& lay,
                   bool timing) {
  gs_ctx* m0 = ms[0];
  const uint32_t G = m0->G, B8 = m0->ws.obins * kCoarseSub, nreg = G * B8;
  const size_t K1 = kRegions + 1;
  const bool rank = is_rank(m0);
  // a group's members are its shards in rank order
  auto travels = [&](uint32_t s, uint32_t d) { return rank ? s != d : acc->gr.dev_of[s] != acc->gr.dev_of[d]; };
  // poff[s][r]: offset of region r in sender s's packed output (~0: stays in place);
  // blk[s][d]: messages of sender s for destination d
  std::vector<unsigned long long> poff((size_t)G * K1, ~0ull), blk((size_t)G * G, 0), ptot(G, 0);
  for (uint32_t s = 0; s < G; ++s) {
    unsigned long long a = 0;
    for (uint32_t r = 0; r < nreg; ++r) {
      const uint32_t d = r / B8;
      const unsigned long long f = lay[(size_t)s * K1 + r];
      blk[(size_t)s * G + d] += f;
      if (!travels(s, d)) continue;
      poff[(size_t)s * K1 + r] = a;
      a += f;
    }
    ptot[s] = a;
  }
  auto bstart = [&](uint32_t s, uint32_t d) { return poff[(size_t)s * K1 + (size_t)d * B8]; };
  auto bsize = [&](uint32_t s, uint32_t d) { return blk[(size_t)s * G + d]; };
  // where each receiver finds the blocks that travel to it: in[i][s]; pack destinations pout[i]
  std::vector<std::vector<unsigned long long>> in(ms.size(), std::vector<unsigned long long>(G, 0));
  std::vector<uint32_t*> inbuf(ms.size(), nullptr), pout(ms.size(), nullptr);
  if (rank) {
    gs_ctx* m = m0;
    const uint32_t me = m->rank;
    unsigned long long rsum = 0;
    for (uint32_t s = 0; s < G; ++s)
      if (s != me) { in[0][s] = rsum; rsum += bsize(s, me); }
    // every rank learns whether every rank has its buffers before any sends
    const bool ok = grow(m->xc.xsend, (ptot[me] + 16) * 4) && grow(m->xc.xrecv, (rsum + 16) * 4);
    RC(agree_ok(m, ok, "cannot allocate the exchange buffers"));
    inbuf[0] = (uint32_t*)m->xc.xrecv.p;
    pout[0] = (uint32_t*)m->xc.xsend.p;
  } else {
    // device D's buffer: its members' packed outputs, then the blocks its
    // members receive from members on other devices
    std::vector<unsigned long long> dtot(acc->gr.devs.size(), 0), O(ms.size(), 0);
    for (size_t i = 0; i < ms.size(); ++i) {
      const int D = acc->gr.dev_of[i];
      O[i] = dtot[D];
      dtot[D] += ptot[i];
    }
    for (size_t i = 0; i < ms.size(); ++i)
      for (uint32_t s = 0; s < G; ++s)
        if (travels(s, (uint32_t)i)) {
          const int D = acc->gr.dev_of[i];
          in[i][s] = dtot[D];
          dtot[D] += bsize(s, (uint32_t)i);
        }
    for (size_t D = 0; D < acc->gr.devs.size(); ++D) {
      if (!dtot[D]) continue;
      CK(acc, hipSetDevice(acc->gr.devs[D]));
      if (!grow(acc->gr.buf[D], (dtot[D] + 16) * 4)) return fail(acc, GS_ENOMEM, "cannot allocate the exchange buffers");
    }
    for (size_t i = 0; i < ms.size(); ++i) {
      inbuf[i] = (uint32_t*)acc->gr.buf[acc->gr.dev_of[i]].p;
      pout[i] = inbuf[i] ? inbuf[i] + O[i] : nullptr;
    }
  }
  // receive layouts (region = bin * (G * 8) + sender * 8 + sub), pack offsets, sources
  for (size_t i = 0; i < ms.size(); ++i) {
    gs_ctx* m = ms[i];
    const uint32_t d = m->rank;
    unsigned long long* rcap = m->wn.h_rtab;
    unsigned long long* rend = rcap + K1;
    unsigned long long* rfill = rend + K1;
    unsigned long long* mypoff = rfill + K1;
    const uint32_t** src = (const uint32_t**)(mypoff + K1);
    std::fill(m->wn.h_rtab, m->wn.h_rtab + kRtabWords, 0ull);
    // sources: rank: 0 = received blocks, 1 = own buffer; group: s = member s's buffer, G = received blocks
    const uint32_t in_src = rank ? 0u : G;
    if (rank) {
      src[0] = inbuf[i];
      src[1] = m->ws.cmsg;
    } else {
      for (uint32_t s = 0; s < G; ++s) src[s] = travels(s, d) ? nullptr : ms[s]->ws.cmsg;
      src[G] = inbuf[i];
    }
    unsigned long long tot = 0;
    for (uint32_t c = 0; c < m->ws.obins; ++c)
      for (uint32_t s = 0; s < G; ++s)
        for (uint32_t x = 0; x < kCoarseSub; ++x) {
          const size_t rr = ((size_t)c * G + s) * kCoarseSub + x, sr = (size_t)d * B8 + c * kCoarseSub + x;
          const unsigned long long f = lay[(size_t)s * K1 + sr];
          unsigned long long at;
          if (!travels(s, d))  // in place: the sender's own region start
            at = ((unsigned long long)(rank ? 1u : s) << kSrcShift) | (rank ? m : ms[s])->wn.h_cap[sr];
          else
            at = ((unsigned long long)in_src << kSrcShift) | (in[i][s] + poff[(size_t)s * K1 + sr] - bstart(s, d));
          rcap[rr] = at;
          rend[rr] = at + f;
          rfill[rr] = f;
          tot += f;
        }
    std::copy(poff.begin() + (size_t)d * K1, poff.begin() + (size_t)(d + 1) * K1, mypoff);
    m->xc.rtotal = tot;
    WinState& wr = m->wr;
    wr = m->ws;
    wr.cmsg = nullptr;
    wr.csrc = (const uint32_t* const*)(m->wn.d_rtab + 4 * K1);
    wr.ccap = m->wn.d_rtab;
    wr.ccap_end = m->wn.d_rtab + K1;
    wr.cfill = m->wn.d_rtab + 2 * K1;
    wr.csub = G * kCoarseSub;
    CK(m, hipSetDevice(m->dev));
    CK(m, hipMemcpyAsync(m->wn.d_rtab, m->wn.h_rtab, kRtabWords * 8, hipMemcpyHostToDevice, m->stream));
    if (timing) CK(m, hipEventRecord(m->ev[2], m->stream));
    if (ptot[d]) CK(m, win_pack(m->ws, m->wn.d_rtab + 3 * K1, nreg, pout[i], m->stream));
    if (timing) CK(m, hipEventRecord(m->ev[3], m->stream));
    if (!rank) CK(m, hipEventRecord(acc->gr.ev_c[i], m->stream));
    if (shard_serial() && !rank) CK(m, hipStreamSynchronize(m->stream));
  }
  if (rank) {
    gs_ctx* m = m0;
    const uint32_t me = m->rank;
    if (m->xc.comm) {
      const Rccl& r = rccl();
      NCK(m, r.group_start());
      for (uint32_t p = 0; p < G; ++p) {
        if (p == me) continue;
        if (bsize(me, p))
          NCK(m, r.send(pout[0] + bstart(me, p), bsize(me, p), ncclUint32, (int)p, m->xc.comm, m->stream));
        if (bsize(p, me))
          NCK(m, r.recv(inbuf[0] + in[0][p], bsize(p, me), ncclUint32, (int)p, m->xc.comm, m->stream));
      }
      NCK(m, r.group_end());
    } else {
      unsigned long long rsum = 0;
      std::vector<size_t> sb(G, 0), rb(G, 0);
      for (uint32_t p = 0; p < G; ++p)
        if (p != me) {
          sb[p] = bsize(me, p) * 4;
          rb[p] = bsize(p, me) * 4;
          rsum += bsize(p, me);
        }
      RC(agree_ok(m, grow_pinned(m, (ptot[me] + rsum) * 4 + 16), "cannot allocate exchange staging"));
      char* hs = m->xc.h_xbuf;
      char* hr = m->xc.h_xbuf + ptot[me] * 4;
      CK(m, hipMemcpyAsync(hs, pout[0], ptot[me] * 4, hipMemcpyDeviceToHost, m->stream));
      CK(m, hipStreamSynchronize(m->stream));
      if (m->xc.hx.all_to_allv(m->xc.hx.user, hs, sb.data(), hr, rb.data()))
        return fail(m, GS_EDEVICE, "the exchange's all_to_allv callback failed");
      CK(m, hipMemcpyAsync(inbuf[0], hr, rsum * 4, hipMemcpyHostToDevice, m->stream));
      CK(m, hipStreamSynchronize(m->stream));
    }
    return GS_OK;
  }
  // group: blocks from other devices are copied in once their senders packed
  // them (blocks on the same device were complete at the layout sync)
  for (size_t i = 0; i < ms.size(); ++i) {
    gs_ctx* m = ms[i];
    CK(m, hipSetDevice(m->dev));
    for (uint32_t s = 0; s < G; ++s) {
      if (!travels(s, (uint32_t)i) || !bsize(s, (uint32_t)i)) continue;
      CK(m, hipStreamWaitEvent(m->stream, acc->gr.ev_c[s], 0));
      CK(m, hipMemcpyPeerAsync(inbuf[i] + in[i][s], m->dev, pout[s] + bstart(s, (uint32_t)i), ms[s]->dev,
                               bsize(s, (uint32_t)i) * 4, m->stream));
    }
  }
  return GS_OK;
}

// Step 5 on shard m: partition and resolve the received messages.
int shard_receive(gs_ctx* m, const ShardWin& sw, bool timing) {
  WinState& wr = m->wr;
  CK(m, hipSetDevice(m->dev));
  const uint64_t R = m->xc.rtotal;
  const uint64_t fcap = R + R / 8 + (uint64_t)wr.ncoarse * 256 * 513 + 16;
  // (+16: buf_cap's slack -- k_rtab checks the next device-driven window's
  // bound against buf_cap, so a buffer grown to exactly fcap aborted it)
  if (!grow(m->wn.fmsg, (fcap + 16) * 4))  // nothing resolved: every rank stops at the next gather
    return mark_nomem(m, "cannot allocate " + std::to_string(R) + " received messages");
  wr.fmsg = m->ws.fmsg = (uint32_t*)m->wn.fmsg.p;
  if (timing) CK(m, hipEventRecord(m->ev[4], m->stream));
  CK(m, win_plan(wr, false, m->stream));
  CK(m, win_part2(wr, R, true, m->stream));
  if (timing) CK(m, hipEventRecord(m->ev[5], m->stream));
  CK(m, win_resolve(wr, sw.t, sw.L, m->stream));
  CK(m, win_stats_reduce(wr, sw.t, sw.L, m->stream));
  if (timing) {
    CK(m, hipEventRecord(m->ev[6], m->stream));
    CK(m, hipStreamSynchronize(m->stream));
    float ex = 0, pk = 0, p2 = 0, rs = 0;
    CK(m, hipEventElapsedTime(&ex, m->ev[0], m->ev[1]));
    CK(m, hipEventElapsedTime(&pk, m->ev[2], m->ev[3]));
    CK(m, hipEventElapsedTime(&p2, m->ev[4], m->ev[5]));
    CK(m, hipEventElapsedTime(&rs, m->ev[5], m->ev[6]));
    m->timing.expand_ms += ex;
    m->timing.part_ms += pk + p2;
    m->timing.deliver_ms += ex + pk + p2;
    m->timing.resolve_ms += rs;
    m->timing.deliver_launches += 1;
    m->timing.resolve_launches += 1;
    m->timing.windows += 1;
  }
  return GS_OK;
}

// Shard m's receive-side partition of window sw overflowed: partition the
// received messages (still in place) again with exact counts and resolve.
int receiver_redo(gs_ctx* m, const ShardWin& sw) {
  WinState& wr = m->wr;
  CK(m, hipSetDevice(m->dev));
  RC(clear_part_flags(m));
  const uint64_t R = m->xc.rtotal;
  CK(m, hipMemsetAsync(wr.ffill, 0, (size_t)wr.nfine * 8, m->stream));
  CK(m, hipMemsetAsync(wr.fhist, 0, ((size_t)wr.ncoarse * 256 + 1) * 8, m->stream));
  CK(m, win_plan(wr, true, m->stream));
  CK(m, win_part2(wr, R, false, m->stream));
  size_t need = 0;
  CK(m, win_scan_fine(wr, nullptr, need, m->stream));
  if (!grow(m->wn.tmp, need)) return mark_nomem(m, "cannot allocate scan scratch");
  need = m->wn.tmp.bytes;
  CK(m, win_scan_fine(wr, m->wn.tmp.p, need, m->stream));
  CK(m, hipMemsetAsync(wr.ffill, 0, (size_t)wr.nfine * 8, m->stream));
  CK(m, win_part2(wr, R, true, m->stream));
  CK(m, win_resolve(wr, sw.t, sw.L, m->stream));
  CK(m, win_stats_reduce(wr, sw.t, sw.L, m->stream));
  ++m->timing.exact_redos;
  return GS_OK;
}

int shard_windows(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint64_t t0, uint32_t n, bool timing) {
  gs_ctx* m0 = ms[0];
  const uint32_t G = m0->G;
  const uint64_t N = m0->p.n;
  const uint32_t stride = m0->ws.stride;
  const uint32_t Lmax = std::min<uint32_t>(std::max<int32_t>(m0->p.delay_low, 1), kBitTicks);
  const uint64_t slot_budget = ((N + kFineNodes - 1) >> kFineLog) * (uint64_t)kWinSlotsPerBucket;
  const size_t K1 = kRegions + 1;
  std::vector<unsigned long long> cnt((size_t)G * kMaxWindow), lay;
  ShardWin prev;
  uint32_t done = 0;
  // 1. fire counts per tick (every shard's, gathered) and every shard's
  //    overflow flag of the previous window
  auto counts = [&](uint32_t t, uint32_t Lw) -> int {
    for (gs_ctx* m : ms) RC(shard_units(m, t, Lw, true));
    RC(sync_all(ms));
    for (uint32_t r = 0; r < G; ++r)
      for (uint32_t k = 0; k < kMaxWindow; ++k)
        cnt[(size_t)r * kMaxWindow + k] = is_rank(m0) ? m0->wn.h_misc[(size_t)r * kMaxWindow + k] : ms[r]->wn.h_misc[k];
    return GS_OK;
  };
  auto flagged = [&]() {
    for (uint32_t r = 0; r < G; ++r)
      if (cnt[(size_t)r * kMaxWindow + kFlagSlot] & (kErrCoarse | kErrFine)) return true;
    return false;
  };
  while (done < n) {
    const uint32_t Lw = std::min(Lmax, n - done);
    const uint32_t t = (uint32_t)(t0 + done);
    RC(counts(t, Lw));
    for (uint32_t r = 0; r < G; ++r)  // a shard could not allocate: every shard stops here
      if (cnt[(size_t)r * kMaxWindow + kFlagSlot] & kErrNoMem)
        return fail(acc, GS_ENOMEM, "shard " + std::to_string(r) + " could not allocate a window buffer");
    if (flagged()) {  // a shard's previous window overflowed its receive partition: it redoes it, then all count again
      for (uint32_t r = 0; r < G; ++r) {
        if (!(cnt[(size_t)r * kMaxWindow + kFlagSlot] & (kErrCoarse | kErrFine))) continue;
        for (gs_ctx* m : ms)
          if (m->rank == r) RC(receiver_redo(m, prev));
      }
      RC(counts(t, Lw));
    }
    auto F = [&](uint32_t k) {
      unsigned long long s = 0;
      for (uint32_t r = 0; r < G; ++r) s += cnt[(size_t)r * kMaxWindow + k];
      return s;
    };
    // the same cut on every shard (global counts), as the unsharded engine would
    uint32_t L = 1;
    unsigned long long Tn = F(0);
    while (L < Lw && (Tn + F(L)) * stride <= slot_budget) Tn += F(L++);
    if (L < Lw)
      for (gs_ctx* m : ms) RC(shard_units(m, t, L, false));
    std::vector<unsigned long long> own(G, 0);
    unsigned long long Ftot = 0;
    for (uint32_t r = 0; r < G; ++r) {
      for (uint32_t k = 0; k < L; ++k) own[r] += cnt[(size_t)r * kMaxWindow + k];
      Ftot += own[r];
    }
    ShardWin sw;
    sw.t = t;
    sw.L = L;
    sw.live = Ftot > 0;
    if (Ftot) {
      // 2. expand own fires
      for (gs_ctx* m : ms) {
        RC(shard_expand(m, t, L, own[m->rank], timing));
        if (shard_serial() && !is_rank(m)) CK(m, hipStreamSynchronize(m->stream));
      }
      // 3. fills and overflow flags; exact redo of an overflowed expand
      RC(gather_layouts(ms, lay));
      auto nomem = [&]() {
        for (uint32_t r = 0; r < G; ++r)
          if (lay[(size_t)r * K1 + kRegions] & kErrNoMem) return true;
        return false;
      };
      if (nomem()) return fail(acc, GS_ENOMEM, "a shard could not allocate its window messages");
      bool redo = false;
      for (uint32_t r = 0; r < G; ++r)
        if (lay[(size_t)r * K1 + kRegions] & kErrCoarse) {
          redo = true;
          for (gs_ctx* m : ms)
            if (m->rank == r) RC(sender_redo(m, t, L, own[r]));
        }
      if (redo) {
        RC(gather_layouts(ms, lay));
        if (nomem()) return fail(acc, GS_ENOMEM, "a shard could not allocate its window messages");
      }
      for (gs_ctx* m : ms) {
        CK(m, hipSetDevice(m->dev));
        CK(m, win_consume_sh(m->ws, t, L, m->stream));
      }
      // 4. pack and move the blocks; 5. partition and resolve what arrived
      RC(shard_exchange(acc, ms, lay, timing));
      for (gs_ctx* m : ms) {
        RC(shard_receive(m, sw, timing));
        if (shard_serial() && !is_rank(m)) CK(m, hipStreamSynchronize(m->stream));
      }
    } else {
      for (gs_ctx* m : ms) {
        CK(m, hipSetDevice(m->dev));
        CK(m, win_consume_sh(m->ws, t, L, m->stream));
      }
    }
    prev = sw;
    done += L;
  }
  // the last window's overflow check (rank-local: the redo needs no exchange)
  for (gs_ctx* m : ms) {
    CK(m, hipSetDevice(m->dev));
    CK(m, hipMemcpyAsync(m->wn.h_err, m->d_err, 4, hipMemcpyDeviceToHost, m->stream));
  }
  RC(sync_all(ms));
  for (gs_ctx* m : ms)
    if (*m->wn.h_err & (kErrCoarse | kErrFine)) {
      RC(receiver_redo(m, prev));
      CK(m, hipMemcpyAsync(m->wn.h_err, m->d_err, 4, hipMemcpyDeviceToHost, m->stream));
      CK(m, hipStreamSynchronize(m->stream));
    }
  // the errors no gather has carried yet (a receipt count overflow, a shard
  // that could not allocate its received messages): every rank returns the
  // same code at the same point (one u64 all-reduce per rank)
  unsigned long long bad = 0;
  for (gs_ctx* m : ms) bad |= *m->wn.h_err & (kErrArrivals | kErrNoMem);
  if (is_rank(m0)) {
    unsigned long long* d = m0->xc.d_gcounts + (size_t)G * kMaxWindow;  // scratch: [arrivals, nomem]
    m0->wn.h_misc[8] = (bad & kErrArrivals) ? 1 : 0;
    m0->wn.h_misc[9] = (bad & kErrNoMem) ? 1 : 0;
    CK(m0, hipMemcpyAsync(d, &m0->wn.h_misc[8], 16, hipMemcpyHostToDevice, m0->stream));
    RC(x_all_reduce(m0, d, 2));
    CK(m0, hipMemcpyAsync(&m0->wn.h_misc[10], d, 16, hipMemcpyDeviceToHost, m0->stream));
    CK(m0, hipStreamSynchronize(m0->stream));
    bad = (m0->wn.h_misc[10] ? kErrArrivals : 0u) | (m0->wn.h_misc[11] ? kErrNoMem : 0u);
  }
  if (bad & kErrNoMem) return fail(acc, GS_ENOMEM, "a shard could not allocate its received messages");
  if (bad & kErrArrivals) return fail(acc, GS_EOVERFLOW, "too many arrivals at one node in one tick");
  return GS_OK;
}

// GS_WINLOG=1: one stderr line per device-driven shard window (and its aborts)
bool dd_log() {
  static const bool on = getenv("GS_WINLOG") != nullptr;
  return on;
}

// Elements a buffer holds for the window kernels (16 of slack, as run_async).
unsigned long long buf_cap(const Buf& b) { return b.bytes / 4 > 16 ? b.bytes / 4 - 16 : 0; }

int dd_setup(gs_ctx* acc, const std::vector<gs_ctx*>& ms) {
  gs_ctx* m0 = ms[0];
  const uint32_t G = m0->G, M = (uint32_t)ms.size();
  CK(acc, hipSetDevice(m0->dev));
  if (!acc->dd.mem) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b1 = al((size_t)G * kMaxWindow * 8), b2 = al((size_t)G * kDDRow * 8),
                 b3 = al((size_t)M * kDDWStat * 8), b4 = al((size_t)M * sizeof(WinCtl)),
                 b5 = al((size_t)(4 * M + 2) * sizeof(void*)), b6 = al((size_t)3 * M * sizeof(WinState));
    CK(acc, dev_malloc(&acc->dd.mem, b1 + b2 + b3 + b4 + b5 + b6));
    char* q = (char*)acc->dd.mem;
    acc->dd.gcnt = (unsigned long long*)q; q += b1;
    acc->dd.glay = (unsigned long long*)q; q += b2;
    acc->dd.wstat = (unsigned long long*)q; q += b3;
    acc->dd.ctl = (WinCtl*)q; q += b4;
    acc->dd.ptrs = (void**)q; q += b5;
    acc->dd.wsm = (WinState*)q;
    CK(acc, hipHostMalloc((void**)&acc->dd.h_ptrs, (size_t)(4 * M + 2) * sizeof(void*)));
    if (is_rank(acc) && G > 1) CK(acc, hipHostMalloc((void**)&acc->dd.h_lay, (size_t)G * kDDRow * 8));
  }
  return alloc_stage(acc);  // (released with the device-driven windows' own: release_async)
}

}  // namespace

void release_dd(gs_ctx* c) {
  if (c->dd.mem) (void)dev_free(c->dd.mem);
  if (c->dd.h_ptrs) (void)hipHostFree(c->dd.h_ptrs);
  if (c->dd.h_lay) (void)hipHostFree(c->dd.h_lay);
}

// ---- multi-process exchange ----------------------------------
// A rank context exchanges through RCCL (gs_create_rank) or the caller's host
// callbacks (gs_create_rank_exchange); both are stream-ordered on c->stream.

bool grow_pinned(gs_ctx* c, size_t bytes) {
  if (c->xc.h_xbytes >= bytes) return true;
  const size_t nb = std::max(bytes, c->xc.h_xbytes + c->xc.h_xbytes / 4);
  if (c->xc.h_xbuf) (void)hipHostFree(c->xc.h_xbuf);
  c->xc.h_xbuf = nullptr;
  c->xc.h_xbytes = 0;
  if (hipHostMalloc((void**)&c->xc.h_xbuf, nb) != hipSuccess) return false;
  c->xc.h_xbytes = nb;
  return true;
}

// In place: rank r's `bytes` at dbuf + r * bytes go to every rank.
int x_all_gather(gs_ctx* c, void* dbuf, size_t bytes) {
  if (c->xc.comm) {
    NCK(c, rccl().all_gather((char*)dbuf + (size_t)c->rank * bytes, dbuf, bytes, ncclUint8, c->xc.comm, c->stream));
    return GS_OK;
  }
  if (!grow_pinned(c, ((size_t)c->G + 1) * bytes)) return fail(c, GS_ENOMEM, "cannot allocate exchange staging");
  char* send = c->xc.h_xbuf + (size_t)c->G * bytes;
  CK(c, hipMemcpyAsync(send, (char*)dbuf + (size_t)c->rank * bytes, bytes, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  if (c->xc.hx.all_gather(c->xc.hx.user, send, c->xc.h_xbuf, bytes))
    return fail(c, GS_EDEVICE, "the exchange's all_gather callback failed");
  CK(c, hipMemcpyAsync(dbuf, c->xc.h_xbuf, (size_t)c->G * bytes, hipMemcpyHostToDevice, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

// In place: element-wise sum of `count` u64 over the ranks.
int x_all_reduce(gs_ctx* c, unsigned long long* dbuf, size_t count) {
  if (c->xc.comm) {
    NCK(c, rccl().all_reduce(dbuf, dbuf, count, ncclUint64, ncclSum, c->xc.comm, c->stream));
    return GS_OK;
  }
  if (!grow_pinned(c, count * 8)) return fail(c, GS_ENOMEM, "cannot allocate exchange staging");
  CK(c, hipMemcpyAsync(c->xc.h_xbuf, dbuf, count * 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  if (c->xc.hx.all_reduce_sum_u64(c->xc.hx.user, (uint64_t*)c->xc.h_xbuf, count))
    return fail(c, GS_EDEVICE, "the exchange's all_reduce_sum_u64 callback failed");
  CK(c, hipMemcpyAsync(dbuf, c->xc.h_xbuf, count * 8, hipMemcpyHostToDevice, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

// Sum of *v over the ranks (through d_gcounts[0], scratch between windows).
int rank_sum(gs_ctx* c, unsigned long long* v) {
  unsigned long long* d = c->xc.d_gcounts;
  CK(c, hipMemcpyAsync(d, v, 8, hipMemcpyHostToDevice, c->stream));
  if (int rc = x_all_reduce(c, d, 1)) return abort_rank(c, rc);
  CK(c, hipMemcpyAsync(v, d, 8, hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return GS_OK;
}

// A rank whose collective failed is torn down so that the other ranks' RCCL
// calls fail instead of waiting for it (and torchrun-style launchers end the
// job when this process exits with the error).
int abort_rank(gs_ctx* c, int rc) {
  if (rc && is_rank(c)) c->aborted = true;
  if (rc && c->xc.comm && rccl().ok && rccl().comm_abort) {
    (void)rccl().comm_abort(c->xc.comm);
    c->xc.comm = nullptr;
  }
  return rc;
}

// ---- device-driven shard windows -------------------
// The shards of one device (a group on one GPU, one stream) or one rank run
// their windows without a host round trip: every shard's fire counts and
// region fills are gathered into device buffers (the shards of a device share
// them; ranks all-gather them with RCCL), k_cut makes the same window cut on
// every shard, k_rtab lays out each shard's receive side, a fine-region
// overflow is re-partitioned exactly inside the window, and k_close_dd applies
// gs_run's poll rule to the global counters.  The host enqueues window i
// before it reads window i-1's staged counters.  A rank whose blocks travel
// to other ranks (G > 1) waits once per window: the grouped send / receive
// needs the block sizes on the host.  A window in which any shard overflowed
// a region estimate or its buffers is stopped on every shard before anything
// is consumed or resolved (kErrAbort), and the host redoes it host-driven.
bool dd_ok(const gs_ctx* acc, const std::vector<gs_ctx*>& ms) {
  if ((acc->p.flags & GS_FLAG_TIMING) || getenv("GS_SYNC_WINDOWS") || shard_serial()) return false;
  const gs_ctx* m0 = ms[0];
  if (m0->pp || !m0->win || !m0->shard) return false;
  if (acc->group) return !acc->gtrials && acc->gr.devs.size() == 1;  // one device: one stream, blocks read in place
  return is_rank(acc);
}

// Windows from acc->t + 1 until tend (exclusive), or (poll > 0) until the poll
// rule stops the run; on_tick(tick, row) sees every tick's global counters in
// order; *stop = 1 + GS_RUN_* if the poll rule stopped the run; *fallback =
// true if a window was stopped by an overflow (nothing of it consumed or
// resolved: the caller redoes it and goes on host-driven from acc->t).
int dd_run(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint64_t tend, uint32_t poll, uint64_t max_ticks,
           const OnTick& on_tick, uint32_t* stop, bool* fallback) {
  *stop = 0;
  *fallback = false;
  RC(dd_setup(acc, ms));
  gs_ctx* m0 = ms[0];
  const uint32_t G = m0->G, M = (uint32_t)ms.size();
  const bool rank = is_rank(m0), travel = rank && G > 1;
  // one in-process shard: its send layout is its receive layout, so the
  // window runs as the unsharded engine's does (no k_rtab, overflows stop the
  // window) -- the G = 1 case of bench.py's sharded flood
  const bool solo = !rank && G == 1 && M == 1;
  const size_t K1 = kRegions + 1;
  hipStream_t st = m0->stream;
  CK(acc, hipSetDevice(m0->dev));
  // the members' own streams (begin, reset, the packed row view) are done
  // before their windows run on m0's stream
  for (gs_ctx* m : ms)
    if (m != m0) CK(acc, hipStreamSynchronize(m->stream));
  const uint32_t Lmax = std::min<uint32_t>(std::max<int32_t>(m0->p.delay_low, 1), kBitTicks);
  const uint64_t N = m0->p.n;
  const unsigned long long budget = ((N + kFineNodes - 1) >> kFineLog) * (unsigned long long)kWinSlotsPerBucket;
  const uint32_t B8 = m0->ws.obins * kCoarseSub, nreg = G * B8;
  // the message buffers keep the size the windows so far needed (an overflow
  // is redone host-driven, which grows them); the group map holds every fire
  bool ok = true;
  for (gs_ctx* m : ms)
    ok = ok && grow(m->wn.gmap, ((m->ntot + 1 + 63) / 64 + 1) * 4) && grow(m->wn.cmsg, 64) && grow(m->wn.fmsg, 64);
  if (rank) RC(agree_ok(m0, ok, "cannot allocate the window message buffers"));
  else if (!ok) return fail(acc, GS_ENOMEM, "cannot allocate the window message buffers");
  // pointer tables: region starts (k_rtab's in-place regions), the receive
  // layout's sources, the members' counters and control blocks
  void** hp = acc->dd.h_ptrs;
  const uint32_t nsrc = rank ? 2u : M + 1;
  void** d_ccaps = acc->dd.ptrs;
  void** d_src = acc->dd.ptrs + M;
  void** d_wst = acc->dd.ptrs + 2 * M + 1;
  void** d_ctls = acc->dd.ptrs + 3 * M + 1;
  for (uint32_t i = 0; i < M; ++i) {
    hp[i] = ms[i]->ws.ccap;
    hp[2 * M + 1 + i] = acc->dd.wstat + (size_t)i * kDDWStat;
    hp[3 * M + 1 + i] = acc->dd.ctl + i;
  }
  if (rank) {
    hp[M] = m0->xc.xrecv.p;
    hp[M + 1] = m0->wn.cmsg.p;
  } else {
    for (uint32_t i = 0; i < M; ++i) hp[M + i] = ms[i]->wn.cmsg.p;
    hp[2 * M] = nullptr;
  }
  CK(acc, hipMemcpyAsync(acc->dd.ptrs, hp, (size_t)(4 * M + 2) * sizeof(void*), hipMemcpyHostToDevice, st));
  // control blocks: the same window state on every member
  std::vector<WinCtl> hc(M);
  for (uint32_t i = 0; i < M; ++i) {
    WinCtl& h = hc[i];
    h = WinCtl{};
    h.tnext = (uint32_t)(acc->t + 1);
    h.tend = (uint32_t)std::min<uint64_t>(tend, 0xFFFFFFFFull);
    h.poll = poll;
    h.pbase = (uint32_t)acc->t;
    h.lmax = Lmax;
    h.recv = acc->recv;
    h.crashed = acc->crashed;
    h.pending = acc->pending;
    h.cover = cover_threshold(N);
    h.max_ticks = max_ticks;
    h.cmsg_cap = buf_cap(ms[i]->wn.cmsg);
    h.fmsg_cap = buf_cap(ms[i]->wn.fmsg);
    h.xs_cap = buf_cap(ms[i]->xc.xsend);
    h.xr_cap = buf_cap(ms[i]->xc.xrecv);
  }
  CK(acc, hipMemcpyAsync(acc->dd.ctl, hc.data(), (size_t)M * sizeof(WinCtl), hipMemcpyHostToDevice, st));
  CK(acc, hipMemsetAsync(acc->dd.gcnt, 0, (size_t)G * kMaxWindow * 8, st));
  // the members' window states (send side, and the receive side as
  // shard_exchange lays it out)
  std::vector<WinState> ws(M), wr(M);
  std::vector<uint64_t> tn_bound(M);
  for (uint32_t i = 0; i < M; ++i) {
    gs_ctx* m = ms[i];
    WinState w = m->ws;
    w.ctl = acc->dd.ctl + i;
    w.stage = acc->aw.d_stage;
    w.lstride = Lmax;
    w.dd = 1;
    w.guard = 0;
    w.abort_on_err = 0;
    w.gcnt = acc->dd.gcnt;
    w.glay = acc->dd.glay;
    w.tfires = acc->dd.gcnt + (size_t)m->rank * kMaxWindow;
    w.cfill = acc->dd.glay + (size_t)m->rank * kDDRow;
    w.wstat = acc->dd.wstat + (size_t)i * kDDWStat;
    w.nglob = N;
    w.solo = solo ? 1u : 0u;
    w.gmap = (uint32_t*)m->wn.gmap.p;
    w.cmsg = (uint32_t*)m->wn.cmsg.p;
    w.fmsg = (uint32_t*)m->wn.fmsg.p;
    ws[i] = w;
    if (solo) {
      wr[i] = w;
      tn_bound[i] = std::min<uint64_t>(m->ntot + 1, 4096ull * 1024);
      continue;
    }
    WinState r = w;
    r.cmsg = nullptr;
    r.csrc = (const uint32_t* const*)(m->wn.d_rtab + 4 * K1);
    r.ccap = m->wn.d_rtab;
    r.ccap_end = m->wn.d_rtab + K1;
    r.cfill = m->wn.d_rtab + 2 * K1;
    r.csub = G * kCoarseSub;
    wr[i] = r;
    tn_bound[i] = std::min<uint64_t>(m->ntot + 1, 4096ull * 1024);
  }
  const uint64_t T_bound = 2048ull * 16384;
  // an in-process group launches each small per-shard kernel once for all its
  // shards (WinGroup; GS_DD_GROUP=0: one launch per shard, the A/B baseline)
  static const bool group_env = [] { const char* e = getenv("GS_DD_GROUP"); return !(e && atoi(e) == 0); }();
  const bool grouped = !rank && M > 1 && group_env;
  std::vector<WinState> wall;
  WinGroup grp{};
  if (grouped) {
    wall.reserve(3 * M);
    wall.insert(wall.end(), ws.begin(), ws.end());
    wall.insert(wall.end(), wr.begin(), wr.end());
    for (uint32_t i = 0; i < M; ++i) {
      wall.push_back(wr[i]);
      wall.back().guard = 1;
    }
    CK(acc, hipMemcpyAsync(acc->dd.wsm, wall.data(), wall.size() * sizeof(WinState), hipMemcpyHostToDevice, st));
    grp.ws = acc->dd.wsm;
    grp.wr = acc->dd.wsm + M;
    grp.wg = acc->dd.wsm + 2 * M;
    grp.M = M;
    for (uint32_t i = 0; i < M; ++i) {
      grp.nfine_max = std::max(grp.nfine_max, ws[i].nfine);
      grp.ncoarse_max = std::max(grp.ncoarse_max, ws[i].ncoarse);
      grp.slots_max = std::max(grp.slots_max, ws[i].slots);
    }
  }
  // ranks whose blocks travel: the block sizes, from the gathered rows
  auto bsize = [&](uint32_t s, uint32_t d) {
    unsigned long long a = 0;
    for (uint32_t r = d * B8; r < (d + 1) * B8; ++r) a += acc->dd.h_lay[(size_t)s * kDDRow + r];
    return a;
  };
  // one window: 0 = enqueued up to its close, 1 = stopped at the block
  // exchange (the window is dead: stopped, or aborted -> *aborted)
  auto enqueue = [&](uint32_t slot, bool* aborted) -> int {
    *aborted = false;
    if (grouped) {
      CK(acc, win_units_g(grp, Lmax, st));
      CK(acc, win_cut_g(grp, budget, st));
      CK(acc, win_unitscan_g(grp, st));
    } else {
      for (uint32_t i = 0; i < M; ++i) CK(acc, win_units(ws[i], 0, Lmax, st));
      if (rank) RC(x_all_gather(m0, acc->dd.gcnt, kMaxWindow * 8));
      for (uint32_t i = 0; i < M; ++i) CK(acc, win_cut(ws[i], budget, st));
      for (uint32_t i = 0; i < M; ++i) CK(acc, win_unitscan(ws[i], st));
    }
    if (grouped) CK(acc, win_expand_g(grp, Lmax, st));
    for (uint32_t i = 0; i < M && !grouped; ++i) CK(acc, win_expand(ws[i], 0, Lmax, tn_bound[i], 1, st));
    if (rank) RC(x_all_gather(m0, acc->dd.glay, kDDRow * 8));
    if (grouped)
      CK(acc, win_rtab_g(grp, (const unsigned long long* const*)d_ccaps, (const uint32_t* const*)d_src, nsrc, st));
    for (uint32_t i = 0; i < M && !solo && !grouped; ++i)
      CK(acc, win_rtab(ws[i], ms[i]->wn.d_rtab, (const unsigned long long* const*)d_ccaps, (const uint32_t* const*)d_src,
                       nsrc, rank ? 1u : 0u, st));
    if (travel) {
      // the window's one host wait: block sizes for the grouped send / receive
      gs_ctx* m = m0;
      const uint32_t me = m->rank;
      CK(acc, hipMemcpyAsync(acc->dd.h_lay, acc->dd.glay, (size_t)G * kDDRow * 8, hipMemcpyDeviceToHost, st));
      CK(acc, hipMemcpyAsync(m->wn.h_err, m->d_err, 4, hipMemcpyDeviceToHost, st));
      CK(acc, hipMemcpyAsync(m->wn.h_misc, acc->dd.ctl, 32, hipMemcpyDeviceToHost, st));
      CK(acc, hipStreamSynchronize(st));
      const uint32_t* hc0 = (const uint32_t*)m->wn.h_misc;  // WinCtl t, L, tnext, tend, poll, pbase, stop, lmax
      if (*m->wn.h_err & kErrAbort) { *aborted = true; return 1; }
      if (hc0[1] == 0 || hc0[6]) return 1;  // stopped or past the end: the same on every rank
      // every rank's send / receive needs against its buffers (their
      // capacities travel in the gathered rows): a rank that must grow them
      // does, and then every rank learns whether every rank could
      std::vector<unsigned long long> ptot(G, 0), rsum(G, 0);
      for (uint32_t s = 0; s < G; ++s)
        for (uint32_t d = 0; d < G; ++d)
          if (s != d) {
            const unsigned long long b = bsize(s, d);
            ptot[s] += b;
            rsum[d] += b;
          }
      bool any_grow = false;
      for (uint32_t s = 0; s < G; ++s) {
        const unsigned long long* row = acc->dd.h_lay + (size_t)s * kDDRow;
        if (ptot[s] > row[kRegions + 2] || rsum[s] > row[kRegions + 3]) any_grow = true;
      }
      if (any_grow) {
        const void* old_recv = m->xc.xrecv.p;
        const bool ok = grow(m->xc.xsend, (ptot[me] + 16) * 4) && grow(m->xc.xrecv, (rsum[me] + 16) * 4);
        unsigned long long* d = m->xc.d_gcounts + (size_t)G * kMaxWindow;  // scratch
        m->wn.h_misc[8] = ok ? 0ull : 1ull;
        CK(acc, hipMemcpyAsync(d, &m->wn.h_misc[8], 8, hipMemcpyHostToDevice, st));
        RC(x_all_reduce(m, d, 1));
        CK(acc, hipMemcpyAsync(&m->wn.h_misc[9], d, 8, hipMemcpyDeviceToHost, st));
        CK(acc, hipStreamSynchronize(st));
        if (m->wn.h_misc[9]) return fail(acc, GS_ENOMEM, "a rank cannot allocate its exchange buffers");
        WinCtl* c = acc->dd.ctl;
        m->wn.h_misc[10] = buf_cap(m->xc.xsend);
        m->wn.h_misc[11] = buf_cap(m->xc.xrecv);
        CK(acc, hipMemcpyAsync(&c->xs_cap, &m->wn.h_misc[10], 16, hipMemcpyHostToDevice, st));
        if (m->xc.xrecv.p != old_recv) {  // the receive layout's source 0 (k_rtab wrote the old address)
          m->wn.h_misc[12] = (unsigned long long)(uintptr_t)m->xc.xrecv.p;
          CK(acc, hipMemcpyAsync(m->wn.d_rtab + 4 * K1, &m->wn.h_misc[12], 8, hipMemcpyHostToDevice, st));
          hp[M] = m->xc.xrecv.p;
          CK(acc, hipMemcpyAsync(&d_src[0], &hp[M], sizeof(void*), hipMemcpyHostToDevice, st));
        }
        CK(acc, hipStreamSynchronize(st));  // the pinned words above are reused next window
      }
      CK(acc, win_pack(ws[0], m->wn.d_rtab + 3 * K1, nreg, (uint32_t*)m->xc.xsend.p, st));
      // block of sender s for destination d: after s's blocks for d' < d (its packed output)
      auto bstart = [&](uint32_t s, uint32_t d) {
        unsigned long long a = 0;
        for (uint32_t d2 = 0; d2 < d; ++d2)
          if (d2 != s) a += bsize(s, d2);
        return a;
      };
      std::vector<unsigned long long> in(G, 0);
      unsigned long long rs = 0;
      for (uint32_t s = 0; s < G; ++s)
        if (s != me) { in[s] = rs; rs += bsize(s, me); }
      uint32_t* xs = (uint32_t*)m->xc.xsend.p;
      uint32_t* xr = (uint32_t*)m->xc.xrecv.p;
      if (m->xc.comm) {
        const Rccl& r = rccl();
        NCK(acc, r.group_start());
        for (uint32_t p = 0; p < G; ++p) {
          if (p == me) continue;
          if (bsize(me, p)) NCK(acc, r.send(xs + bstart(me, p), bsize(me, p), ncclUint32, (int)p, m->xc.comm, st));
          if (bsize(p, me)) NCK(acc, r.recv(xr + in[p], bsize(p, me), ncclUint32, (int)p, m->xc.comm, st));
        }
        NCK(acc, r.group_end());
      } else {
        std::vector<size_t> sb(G, 0), rb(G, 0);
        for (uint32_t p = 0; p < G; ++p)
          if (p != me) { sb[p] = bsize(me, p) * 4; rb[p] = bsize(p, me) * 4; }
        RC(agree_ok(m, grow_pinned(m, (ptot[me] + rs) * 4 + 16), "cannot allocate exchange staging"));
        char* hs = m->xc.h_xbuf;
        char* hr = m->xc.h_xbuf + ptot[me] * 4;
        CK(acc, hipMemcpyAsync(hs, xs, ptot[me] * 4, hipMemcpyDeviceToHost, st));
        CK(acc, hipStreamSynchronize(st));
        if (m->xc.hx.all_to_allv(m->xc.hx.user, hs, sb.data(), hr, rb.data()))
          return fail(acc, GS_EDEVICE, "the exchange's all_to_allv callback failed");
        CK(acc, hipMemcpyAsync(xr, hr, rs * 4, hipMemcpyHostToDevice, st));
        CK(acc, hipStreamSynchronize(st));
      }
    }
    if (grouped) {
      CK(acc, win_recv_g(grp, T_bound, st));
      CK(acc, win_resolve_g(grp, Lmax, st));
      CK(acc, win_stats_dd_g(grp, slot, st));
    } else {
      for (uint32_t i = 0; i < M; ++i) {
        CK(acc, win_plan(wr[i], false, st));
        CK(acc, win_part2(wr[i], T_bound, true, st));
        if (!solo) CK(acc, win_fine_redo(wr[i], T_bound, st));
        CK(acc, win_resolve(wr[i], 0, Lmax, st));
        CK(acc, win_stats_dd(ws[i], slot, st));
      }
    }
    if (rank) RC(x_all_reduce(m0, acc->dd.wstat, kDDWStat));
    if (!solo)  // (one in-process shard: k_stats_dd closed the window)
      CK(acc, win_close_dd(ws[0], (const unsigned long long* const*)d_wst, (WinCtl* const*)d_ctls, M, slot, st));
    CK(acc, hipEventRecord(acc->aw.wev[slot], st));
    return 0;
  };
  bool eoverflow = false;
  // window i-1's results: 0 = go on, 1 = finished
  auto absorb = [&](uint32_t slot, int* what) -> int {
    CK(acc, hipEventSynchronize(acc->aw.wev[slot]));
    const unsigned long long* sg = acc->aw.h_stage + (size_t)slot * kStageWords;
    const uint32_t t0 = (uint32_t)sg[0], L = (uint32_t)sg[1];
    *what = 0;
    if (sg[3] & kErrAbort) {
      if (dd_log()) fprintf(stderr, "[dd] window at t0=%u aborted: redone host-driven\n", t0);
      ++m0->timing.dd_fallbacks;
      *fallback = true;
      *what = 1;
      return GS_OK;
    }
    if (dd_log()) fprintf(stderr, "[dd] t0=%u L=%u stop=%llu redos=%llu\n", t0, L, sg[2], sg[4]);
    m0->timing.exact_redos += sg[4];
    for (uint32_t k = 0; k < L; ++k) on_tick((uint64_t)t0 + k, sg + 8 + (size_t)k * kStatFields);
    if (sg[3] & kErrArrivals) eoverflow = true;
    if (sg[2]) *stop = (uint32_t)sg[2];
    if (sg[2] || L == 0 || (uint64_t)t0 + L >= tend || eoverflow) *what = 1;
    return GS_OK;
  };
  bool ab = false;
  int e0 = 0;
  RC((e0 = enqueue(0, &ab), e0 < 0 ? e0 : 0));
  if (e0 == 1) {
    *fallback = ab;
  } else {
    for (uint32_t i = 1;; ++i) {
      const int e = enqueue(i % kSlots, &ab);
      if (e < 0) return e;
      int what = 0;
      RC(absorb((i - 1) % kSlots, &what));
      if (what) break;
      if (e == 1) {  // window i stopped at its exchange (it staged nothing)
        *fallback = ab;
        break;
      }
    }
  }
  CK(acc, hipStreamSynchronize(st));
  if (*fallback) {  // undo what the stopped window left: its expand's counters, the flags
    for (gs_ctx* m : ms) {
      CK(acc, hipMemsetAsync(m->ws.sstats, 0, (size_t)kStatShards * kMaxWindow * kStatFields * 8, st));
      CK(acc, hipMemcpyAsync(m->wn.h_err, m->d_err, 4, hipMemcpyDeviceToHost, st));
      CK(acc, hipStreamSynchronize(st));
      if (dd_log()) {  // the window's cut and coarse plan (plan 0: k_cut found the buffer too small)
        const size_t i = (size_t)(std::find(ms.begin(), ms.end(), m) - ms.begin());
        WinCtl h1{};
        unsigned long long plan = 0;
        CK(acc, hipMemcpy(&h1, acc->dd.ctl + i, sizeof(WinCtl), hipMemcpyDeviceToHost));
        CK(acc, hipMemcpy(&plan, m->ws.ccap + kRegions, 8, hipMemcpyDeviceToHost));
        fprintf(stderr, "[dd] shard %u flags %#x t=%u L=%u Tn=%llu T=%llu cmsg_cap=%llu plan=%llu\n", m->rank,
                *m->wn.h_err, h1.t, h1.L, h1.Tn, h1.T, h1.cmsg_cap, plan);
      }
      *m->wn.h_err &= ~(kErrCoarse | kErrFine | kErrAbort);
      CK(acc, hipMemcpyAsync(m->d_err, m->wn.h_err, 4, hipMemcpyHostToDevice, st));
    }
    CK(acc, hipStreamSynchronize(st));
  }
  if (eoverflow) return fail(acc, GS_EOVERFLOW, "too many arrivals at one node in one tick");
  return GS_OK;
}

// Sharded step: `acc` keeps the global counters (the group, or the rank).
int shard_step(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint32_t ticks, gs_tick_stats* out) {
  const bool timing = (acc->p.flags & GS_FLAG_TIMING) != 0;
  for (gs_ctx* m : ms) {
    CK(m, hipSetDevice(m->dev));
    RC(expand_view(m));
  }
  if (dd_ok(acc, ms) && ticks > 0) {  // device-driven windows
    uint32_t stop = 0, k = 0;
    bool fallback = false;
    RC(dd_run(acc, ms, acc->t + ticks + 1, 0, ~0ull, step_sink(acc, out, &k), &stop, &fallback));
    if (!fallback) return GS_OK;
    ticks -= k;  // a window overflowed: it and the rest host-driven
    if (out) out += k;
  }
  uint32_t done = 0;
  while (done < ticks) {
    const uint32_t batch = std::min<uint32_t>(ticks - done, kStatSlots);
    const uint64_t t0 = acc->t + 1;
    const StatSpans sp = stat_spans(t0, batch);
    for (gs_ctx* m : ms) {
      CK(m, hipSetDevice(m->dev));
      for (int j = 0; j < sp.n; ++j) CK(m, hipMemsetAsync(m->st.stats + sp.off[j], 0, sp.words[j] * 8, m->stream));
    }
    RC(shard_windows(acc, ms, t0, batch, timing));
    for (gs_ctx* m : ms) {
      CK(m, hipSetDevice(m->dev));
      for (int j = 0; j < sp.n && is_rank(m); ++j)  // the global per-tick counters on every rank
        RC(x_all_reduce(m, m->st.stats + sp.off[j], sp.words[j]));
      for (int j = 0; j < sp.n; ++j)
        CK(m, hipMemcpyAsync(m->h_stats + sp.off[j], m->st.stats + sp.off[j], sp.words[j] * 8, hipMemcpyDeviceToHost,
                             m->stream));
    }
    RC(sync_all(ms));
    account_members(acc, ms, t0, batch, out ? out + done : nullptr);
    done += batch;
  }
  return GS_OK;
}

}  // namespace gs
