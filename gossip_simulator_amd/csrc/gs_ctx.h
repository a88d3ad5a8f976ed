// gs_ctx.h -- the context behind the C ABI, private to csrc/: struct gs_ctx,
// the error macros and the few host functions that cross the engine files
// (gs_ctx.cpp lifetime, gs_peers.cpp tables, gs_windows.cpp / gs_shards.cpp
// the flood engines, gs_pushpull_host.cpp push-pull, gs_rumor_host.cpp rumor
// mongering, gs_median_host.cpp median-counter push-pull, gs_trials_host.cpp
// the batched trials' shared loops, gs_rumorset_host.cpp concurrent push-pull
// rumors, gs_round_host.cpp the shared round loop of those three one-trial
// engines, gs_api.cpp the entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "gossip.h"
#include "gs_comm.h"
#include "gs_internal.h"
#include "gs_mdt16_plan.h"
#include "gs_median.h"
#include "gs_ppt_plan.h"
#include "gs_rmt_plan.h"
#include "gs_rumorset.h"

namespace gs {

struct Buf {
  void* p = nullptr;
  size_t bytes = 0;
};

// One trial's running counters and its stopping snapshot (gs_run's rule).
struct TrialAcc {
  uint64_t fired = 0, sent = 0, msgs = 0, recv = 0, crash = 0, sched = 0, tick99 = 0;
  uint64_t start = 1;  // batched flood: the sender's own Broadcast (0: a failed sender, never scheduled)
  int32_t status = GS_RUN_RUNNING;
  gs_trial_stats snap{};
};

// window engine (gs_win_*.hip): alloc_window / release_window
struct WinEngine {
  void* d_win = nullptr;      // fcount + small per-window buffers
  void* d_flist = nullptr;    // [R][nfine][16384] u16
  void* d_rlmsg = nullptr;    // [nfine][kRolledCap] k_resolve's rolled receipts
  size_t fcount_bytes = 0;
  Buf gmap, cmsg, fmsg, tmp;
  unsigned long long* h_cap = nullptr;  // pinned [257] coarse region plan
  unsigned long long* h_misc = nullptr; // pinned scratch (counts, flags): misc_words words
  size_t misc_words = 0;                // >= kRegions and >= G * kMaxWindow (gathered fire counts)
  uint32_t* h_err = nullptr;            // pinned copy of the error word (shard windows)
  // owner expand: the receive layout of a window ([4][kRegions + 1]: region
  // starts, ends, fills; the pack offsets of this shard's own send blocks),
  // pinned host copy
  unsigned long long* d_rtab = nullptr;
  unsigned long long* h_rtab = nullptr;
};

// device-driven windows (run_async; the staging slots also serve dd_run):
// async_setup, alloc_stage / release_async
struct AsyncWin {
  WinCtl* d_ctl = nullptr;
  unsigned long long* d_stage = nullptr;  // [kSlots][kStageWords]
  unsigned long long* h_stage = nullptr;  // pinned, mapped: d_stage is its device address
  std::vector<hipEvent_t> wev;            // one per staging slot
};

// device-driven shard windows (dd_run; the group's or the rank's): gathered
// fire counts [G][kMaxWindow] and region rows [G][kDDRow], each member's
// window counters [M][kDDWStat] and control block, the pointer tables the
// kernels read (region starts [M], sources [M + 1], counters [M], control
// blocks [M]); pinned copy of the gathered rows for ranks whose blocks travel:
// dd_setup / release_dd
struct DdWin {
  void* mem = nullptr;
  unsigned long long* gcnt = nullptr;
  unsigned long long* glay = nullptr;
  unsigned long long* wstat = nullptr;
  WinCtl* ctl = nullptr;
  void** ptrs = nullptr;
  void** h_ptrs = nullptr;              // pinned staging of ptrs
  WinState* wsm = nullptr;              // in-process group: the members' window states [3][M] (WinGroup)
  unsigned long long* h_lay = nullptr;
};

// push-pull sparse early rounds (PPSparse): reverse table, informed list,
// failed-slot mask, round control; rebuilt when the table (table_ver) or the
// failure mask (fail_ver) changes: pp_prepare / release_sparse
struct PpSparseBufs {
  Buf rend, rsrc, rslot, ilist, fmask, scan, ctlb;
  Buf rfail;  // push-pull: failed-caller bit per in-edge (with fmask)
  Buf dset, dcnt;  // deferred sets of the pull-answer rounds (PPSparse::dset)
  Buf rend16;         // the compact view of rend: rend16 [n] u16, then rbase [n/64 + 1] u64, then a flag
  bool rend16_ok = false;  // the view fits (no 64-node block with more than 65,535 in-edges)
  uint64_t rev_ver = ~0ull, fm_tver = ~0ull, fm_fver = ~0ull;
  // push-pull: live callers and live empty rows of (cl_tver, cl_fver) (pp_seed_ctx)
  uint64_t cl_tver = ~0ull, cl_fver = ~0ull;
  unsigned long long cl_counts[2] = {0, 0};
};

// rumor mongering (gs_rumor.hip): the two hot lists [n] u32 (push modes) or the
// hot, served and vain bitsets [W] (pull modes), the miss counts [n] u8, round
// control (RumorCtl) and, once gs_read_removed asks, the removed bitset [W].
// A batched context (gs_rumor_trials.hip) has none of the lists: hot [W] and
// miss [n] over the padded id space, and per-trial words (tri: the hot counts
// [trials], then the started flags [trials]):
// rumor_alloc / release_rumor
struct RumorBufs {
  Buf list[2], hot, served, vain, miss, ctlb, removed, tri;
  uint32_t cur = 0;   // list[cur] is the next round's read list
  uint32_t grid = 0;  // the round kernel's persistent grid (rumor_begin)
  RumorCtl* h_ctl = nullptr;  // pinned copy of the control block, read once per poll
};

// median-counter push-pull (gs_median.hip): the state bytes [n], the
// own-contribution bytes [n], the tally [n] u64, the gotb / gotc bitsets [W],
// round control (a RumorCtl) and, once gs_read_removed asks, the done bitset
// [W].  A batched context (gs_median_trials.hip) has the state bytes over the
// padded id space and the done bitset only: median_alloc / release_median
struct MedianBufs {
  Buf st, own, tally, gotb, gotc, ctlb, done;
  uint32_t grid = 0;  // the round kernel's persistent grid (median_begin)
  RumorCtl* h_ctl = nullptr;  // pinned copy of the control block, read once per poll
};

// concurrent push-pull rumors (gs_rumorset.hip): the rumor words have, next
// and own [n] u64 each, the count ring [kStatSlots][kRsMax], round control
// (RsCtl) and, once gs_read_rumor_column asks, a column bitset [W]:
// rs_alloc / release_rumorset
struct RsBufs {
  Buf have, next, own, ring, ctlb, col;
  uint32_t grid = 0;  // the persistent grid of the round and the commit (rs_begin)
  RsCtl* h_ctl = nullptr;               // pinned copy of the control block, read once per poll
  unsigned long long* h_ring = nullptr; // pinned copy of the count ring
  int64_t sender[kRsMax] = {};          // where each rumor started (rs_begin)
  uint64_t count[kRsMax] = {};          // nodes that hold each rumor, as of the last row read
  uint64_t tick99[kRsMax] = {};         // first poll at which its float32 rule held, else 0
  uint64_t live = 0;                    // bit j: rumor j started
  // bounded sets (section 4.9.1; gs_rumorset_cap.hip)
  uint32_t payload = 0, pick = 0;       // rumors a message carries at most (0: no cap) and GS_PICK_*; outlive a reset
  uint32_t start[kRsMax] = {};          // the round after whose commit rumor j enters (0: at begin)
  uint32_t last_start = 0;              // the largest of them: no round after it injects
  RsSenders snd = {};                   // the senders as the inject kernel takes them
};

// batched trials' per-trial counter rows (every model) and the push-pull
// trials' stall check: alloc_trial_rows / release_trials
struct TrialRows {
  uint32_t* d_tstat = nullptr;          // [trials][kMaxWindow][kTStatFields]
  uint32_t* h_tstat = nullptr;          // pinned copy
  Buf chk;                              // the stall check's need bytes [trials] (4-aligned), then live u32 [trials]
  // rumor and median trials: every trial's live (hot, active) nodes after the last round run (rumor_alloc, median_alloc)
  std::vector<uint32_t> live;
};

// shard or rank exchange: finish_rank / release_exchange
struct Exchange {
  uint64_t rtotal = 0;                  // messages received in the window
  Buf xsend, xrecv;                     // multi-process: packed send blocks, received blocks
  unsigned long long* d_gcounts = nullptr;  // multi-process: [G][16] gathered fires per tick
  unsigned long long* d_glay = nullptr;     // multi-process: [G][kRegions + 1] gathered region fills + error word
  unsigned long long* h_glay = nullptr;     // pinned copy
  ncclComm_t comm = nullptr;
  // multi-process exchange done by the caller (gs_create_rank_exchange)
  gs_exchange hx{};
  bool has_hx = false;
  char* h_xbuf = nullptr;               // pinned staging of the host exchanges
  size_t h_xbytes = 0;
};

// push-pull node-range shard: the informed / failed sets by global id
// (G * segw words; shared by the members on one device, owned by a rank);
// st.recv / st.crash are this shard's slice of them: alloc_pp_sets / release_sets
struct PpSets {
  bool own_ig = false;
  unsigned long long* d_ig = nullptr;
  unsigned long long* d_fg = nullptr;
  // pull-answer rounds of push-pull shards: the round's informed set being
  // built, by global id (shared like d_ig); a rank's staging for the bits the
  // other ranks set in its range ([G][segw] words)
  unsigned long long* d_gn = nullptr;
  unsigned long long* d_gst = nullptr;
  bool pp_answer = false;               // the current broadcast's sharded rounds still run pull-answer
  bool pp_gn_ok = false;                // d_gn holds the replicated set (set at the first sharded round)
  uint64_t segw = 0;
  // push-pull shards: the replica -- an unsharded push-pull context over the
  // full table on this device (shared by the device's members; owned by the
  // group, or by the rank) whose informed / failed sets ARE the replicated
  // ones: it runs the sparse early rounds, identically on every device and
  // rank, with no exchange (section 6.3 of DESIGN.md)
  gs_ctx* rep = nullptr;
  bool own_rep = false;
  bool rep_live = false;                // the current broadcast's rounds still run on the replicas
  uint32_t rep_rounds = 0;              // rounds run on the replicas since the broadcast began
};

// group (gs_create_multi): create_multi / release_group
struct Group {
  std::vector<gs_ctx*> mem;
  std::vector<int> devs;                // distinct devices, first-use order
  std::vector<int> dev_of;              // member -> index into devs
  std::vector<Buf> buf;                 // per distinct device: its members' send blocks, then blocks from other devices
  std::vector<hipEvent_t> ev_c, ev_x;   // per member: its part of an exchange done; per device: copies done
  std::vector<unsigned long long*> ig, fg, gn;  // push-pull shards: per distinct device, the replicated sets
  std::vector<gs_ctx*> reps;            // push-pull shards: per distinct device, the replica
};

}  // namespace gs

struct gs_ctx {
  gs_params p{};
  int dev = 0;
  hipStream_t stream = nullptr;  // where device work is issued (own, or gs_set_stream's)
  hipStream_t own = nullptr;     // the context's own stream
  std::string err;
  gs::DevState st{};
  // peer table: alloc_table / release_table
  uint8_t* d_deg = nullptr;
  uint32_t* d_ids = nullptr;
  uint32_t tab_stride = 0;  // row stride d_ids was allocated for
  uint32_t* d_pk = nullptr;  // k_expand's packed view of the sealed rows (expand_view)
  size_t pk_bytes = 0;
  uint64_t pk_ver = ~0ull;   // table_ver the packed view was built from
  uint32_t row_slots = 0;   // longest row when rows are padded past it (0: the stride)
  // state block: ctx_setup / release_state
  void* d_state = nullptr;  // one allocation for recv/crash/ring/cflag/clist/ccount/stats
  uint32_t* d_cnt = nullptr;
  uint32_t* d_err = nullptr;
  unsigned long long* d_failed = nullptr;  // pre-failed mask, re-applied by gs_reset
  size_t state_bytes = 0;
  unsigned long long* h_stats = nullptr;  // pinned, kStatSlots * kStatFields
  bool peers = false, begun = false, failed = false;
  uint64_t t = 0, fired = 0, sent = 0, msgs = 0, recv = 0, crashed = 0, pending = 0;
  std::vector<hipEvent_t> ev;
  gs_timing timing{};
  // push-pull extension (gs_pp_*.hip)
  bool pp = false, pp_l2_only = false;
  unsigned long long* d_next = nullptr;  // informed set being built (state block)
  unsigned long long* d_ppsum = nullptr;  // push-pull word summaries (state block)
  uint32_t* d_flag = nullptr;
  uint64_t table_ver = 0, fail_ver = 0;
  gs::PPSparse sp{};
  gs::PpSparseBufs sr;
  // rumor mongering (gs_rumor.hip; d_next is its informed set being built)
  bool rumor = false;
  gs::RumorBufs rm;
  // batched rumor trials (gs_create_trials; gs_rumor_trials.hip): a workgroup per trial
  bool rmt = false;
  gs::RmtPlan rplan{};
  // median-counter push-pull (gs_median.hip)
  bool median = false;
  gs::MedianBufs md;
  // batched median trials (gs_create_batch; gs_median_trials.hip): a workgroup per trial
  bool mdt = false;
  gs::MdtPlan mplan{};
  // GS_FLAG_MEDIAN_PACKED at create: mplan is gs_mdt16_plan.h's.  named_ok: the table in place has
  // passed the in-degree guard (set by the first gs_broadcast_begin after it entered)
  bool mdt16 = false, named_ok = false;
  // concurrent push-pull rumors (gs_create_rumorset; gs_rumorset.hip): `rumors` bits per node
  bool rset = false;
  uint32_t rumors = 0;
  gs::RsBufs rsb;
  // window engine (gs_win_*.hip)
  bool win = false;
  gs::WinState ws{};
  gs::WinEngine wn;
  gs::AsyncWin aw;
  bool async_off = false;                 // GS_SYNC_WINDOWS=1: host-driven windows only (A/B tests)
  bool winlog = false;                    // GS_WINLOG=1: one stderr line per device-driven window
  // trials: `trials` per context (batched when > 1), ids trial << tlog | node
  uint32_t trials = 1, tlog = 32;
  uint64_t ntot = 0;                    // nodes in this context's id space
  std::vector<gs::TrialAcc> tacc;
  gs::TrialRows bt;
  // batched push-pull trials (gs_pushpull_trials.hip): a workgroup per trial
  bool ppt = false;
  gs::PptState pt{};
  // node-range shard (config C4)
  bool shard = false;
  uint32_t G = 1, rank = 0;
  uint64_t lo = 0, hi = 0, seg_per = 0;
  gs::WinState wr{};                    // the receive-side WinState (kept for an exact redo)
  gs::Exchange xc;
  bool pp_shard = false;
  bool aborted = false;                 // a rank whose exchange failed (RCCL communicator aborted)
  gs::PpSets rs;
  // group (gs_create_multi)
  bool group = false, gtrials = false;
  gs::Group gr;
  gs::OverlayWork ovw;                  // overlay builder buffers, kept between builds
  gs::DdWin dd;
};

#define CK(c, expr)                                                                   \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail((c), GS_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define NCK(c, expr)                                                                  \
  do {                                                                                \
    ncclResult_t r_ = (expr);                                                         \
    if (r_ != ncclSuccess)                                                            \
      return fail((c), GS_EDEVICE, std::string(#expr) + ": " + rccl_error((int)r_));  \
  } while (0)

#define RC(expr)              \
  do {                        \
    int rc_ = (expr);         \
    if (rc_) return rc_;      \
  } while (0)

namespace gs {

inline int fail(gs_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

inline bool grow(Buf& b, size_t bytes) {
  if (b.bytes >= bytes) return true;
  const size_t nb = std::max(bytes, b.bytes + b.bytes / 4);
  if (b.p) (void)dev_free(b.p);
  b.p = nullptr;
  b.bytes = 0;
  if (dev_malloc(&b.p, nb) != hipSuccess) return false;
  b.bytes = nb;
  return true;
}

inline void release(Buf& b) {
  if (b.p) (void)dev_free(b.p);
  b = Buf{};
}

// A rank context exchanges through RCCL (gs_create_rank) or the caller's host
// callbacks (gs_create_rank_exchange); both are stream-ordered on c->stream.
inline bool is_rank(const gs_ctx* c) { return c->xc.comm != nullptr || c->xc.has_hx; }

inline std::vector<gs_ctx*> shards_of(gs_ctx* c) { return c->group ? c->gr.mem : std::vector<gs_ctx*>{c}; }

// Runs f(member, index) for every member, one host thread each (members on
// several devices, or several trial batches on one, overlap); first error wins.
template <class F>
int par_members(gs_ctx* g, F f) {
  std::vector<int> rcs(g->gr.mem.size(), 0);
  std::vector<std::thread> th;
  for (size_t i = 0; i < g->gr.mem.size(); ++i)
    th.emplace_back([&, i] {
      (void)hipSetDevice(g->gr.mem[i]->dev);
      rcs[i] = f(g->gr.mem[i], i);
    });
  for (auto& t : th) t.join();
  for (size_t i = 0; i < rcs.size(); ++i)
    if (rcs[i]) return fail(g, rcs[i], "member " + std::to_string(i) + ": " + g->gr.mem[i]->err);
  return GS_OK;
}

// The stats-ring rows of ticks [t0, t0 + batch), batch in [1, kStatSlots]:
// one span of u64 words from slot t0 % kStatSlots, and a second from slot 0
// where the batch wraps.
struct StatSpans {
  size_t off[2], words[2];
  int n;
};
inline StatSpans stat_spans(uint64_t t0, uint32_t batch) {
  const uint32_t i0 = (uint32_t)(t0 % kStatSlots), first = std::min<uint32_t>(batch, kStatSlots - i0);
  return StatSpans{{(size_t)i0 * kStatFields, 0}, {(size_t)first * kStatFields, (size_t)(batch - first) * kStatFields},
                   first < batch ? 2 : 1};
}

// What the device-driven windows (run_async, dd_run) call for every tick, in order.
using OnTick = std::function<void(uint64_t tick, const unsigned long long* row)>;
constexpr uint32_t kSlots = 4;  // staging slots of the device-driven windows

// gs_ctx.cpp
extern thread_local std::string g_create_err;
// rumor_trials: GS_MODEL_RUMOR with trials > 1 makes a batched rumor context
// (gs_create_trials, gs_create_batch); median_trials: GS_MODEL_MEDIAN with
// trials > 1 makes a batched median context (gs_create_batch); every other
// create refuses the combinations
// rumorset: 1..kRsMax makes a rumor set of that many rumors (gs_create_rumorset)
int create_one(const gs_params* params, int device, bool shard, uint32_t G, uint32_t rank, gs_ctx** out,
               bool rumor_trials = false, bool median_trials = false, uint32_t rumorset = 0);
int create_multi(const gs_params* params, const int* devices, int ndev, gs_ctx** out);
int finish_rank(gs_ctx* c, gs_ctx** out);
void destroy_one(gs_ctx* c);
std::string ppt_limit_error(int device, bool masked, uint64_t* lim);
int ppt_masked_plan(const gs_ctx* c, PptPlan* plan, std::string& why);
void refresh_state(gs_ctx* c);
void reset_counters(gs_ctx* c);
void account_tick(gs_ctx* c, uint64_t tick, const unsigned long long* s, gs_tick_stats* o);
bool covered(uint64_t recv, uint64_t n);
void account_members(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint64_t t0, uint32_t batch, gs_tick_stats* out);

// gs_peers.cpp
uint64_t table_n(const gs_ctx* c);
int alloc_table(gs_ctx* c, uint32_t stride);
void release_table(gs_ctx* c);
int validate_table(gs_ctx* c, const uint8_t* deg, const uint32_t* ids, uint64_t n, uint64_t bound);
int seal_rows(gs_ctx* c, const uint8_t* deg, uint32_t* ids, uint64_t n);
int expand_view(gs_ctx* c);
int upload_table(gs_ctx* c, const uint8_t* deg, const uint32_t* ids, uint32_t stride);
int partition_from(gs_ctx* leader, const std::vector<gs_ctx*>& ms);
std::vector<gs_ctx*> on_device(gs_ctx* g, size_t d);
int overlay_into(gs_ctx* c, uint64_t max_ticks, gs_window* win, size_t cap, size_t* nwin, uint64_t* final_tick);
int set_failed(gs_ctx* c, const uint64_t* words, size_t nwords);

// gs_windows.cpp
void refresh_window(gs_ctx* c);
bool async_ok(const gs_ctx* c);
uint64_t cover_threshold(uint64_t n);
int alloc_stage(gs_ctx* c);
void release_async(gs_ctx* c);
int run_async(gs_ctx* c, uint64_t tend, uint32_t poll, uint64_t max_ticks, const OnTick& on_tick, uint32_t* stop,
              bool* fallback);
OnTick step_sink(gs_ctx* acc, gs_tick_stats* out, uint32_t* k);
int plain_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out);

// gs_shards.cpp
bool grow_pinned(gs_ctx* c, size_t bytes);
int x_all_gather(gs_ctx* c, void* dbuf, size_t bytes);
int x_all_reduce(gs_ctx* c, unsigned long long* dbuf, size_t count);
int abort_rank(gs_ctx* c, int rc);
int rank_sum(gs_ctx* c, unsigned long long* v);
bool dd_ok(const gs_ctx* acc, const std::vector<gs_ctx*>& ms);
void release_dd(gs_ctx* c);
int dd_run(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint64_t tend, uint32_t poll, uint64_t max_ticks,
           const OnTick& on_tick, uint32_t* stop, bool* fallback);
int shard_step(gs_ctx* acc, const std::vector<gs_ctx*>& ms, uint32_t ticks, gs_tick_stats* out);

// gs_pushpull_host.cpp
int pp_seed_ctx(gs_ctx* c, unsigned long long* next, uint32_t node, unsigned long long thr, unsigned long long bthr,
                unsigned long long athr);
int pp_prepare(gs_ctx* c);
void release_sparse(gs_ctx* c);
uint32_t pp_shift();
unsigned long long pp_bottom_thr(const gs_ctx* c);
unsigned long long pp_answer_thr(const gs_ctx* c);
int pp_shard_begin(gs_ctx* acc, uint64_t sender);
int pp_shard_step(gs_ctx* acc, uint32_t ticks, gs_tick_stats* out);
int pp_stalled(gs_ctx* c, bool* stalled);
void account_trials(gs_ctx* c, uint64_t t0, uint32_t nt, unsigned long long* sums = nullptr);
int ppt_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out);
int ppt_poll_stops(gs_ctx* c, const std::vector<uint64_t>& r0, uint64_t max_ticks, uint32_t* running);
void snap_trial(gs_ctx* c, uint32_t tr, int32_t status);
bool trials_stopped(const gs_ctx* c, uint32_t running, int32_t* st);

// gs_trials_host.cpp
std::string trial_limit_error(const char* where, int device, hipError_t e);
int trial_device_check(int device, std::string& why);
using TrialLaunch = std::function<int(uint64_t t0, uint32_t batch)>;  // the rounds kernel, `batch` rounds from t0
int trial_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls, const TrialLaunch& launch,
               uint64_t (*row_msgs)(const uint32_t* r));
int trial_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
              int32_t* status, const TrialLaunch& launch, uint64_t (*row_msgs)(const uint32_t* r));
int trial_read_words(gs_ctx* c, uint64_t* words, const unsigned long long* d);

// gs_round_host.cpp
// What a one-trial, self-terminating engine gives the shared round loop: the
// round's two halves (launches on c->stream for round tt; the commit half
// holds whatever else the engine enqueues or flips per round), its control
// block (device, pinned copy, and where the pinned copy keeps the three words
// the loop reads), and for an engine that has them a second ring beside the
// stats ring (`words` per slot; 0: none) and a hook run for every row read
// back (the ring's slot, null without a ring, and whether the tick is a poll),
// which then takes the trial's tick_99 itself.  name: as in "the <name>
// control block ...".
using RoundLaunch = std::function<int(uint32_t tt)>;
struct RoundCtl {
  const void* d;
  void* h;
  size_t bytes;
  const unsigned long long *received, *pending;
  const uint32_t* stop;
};
struct RoundRing {
  const unsigned long long* d;
  unsigned long long* h;
  uint32_t words;
};
struct RoundEngine {
  const char* name;
  RoundLaunch round, commit;
  RoundCtl ctl;
  RoundRing ring;
  std::function<void(uint64_t tick, const unsigned long long* slot, bool poll)> row;
};
int round_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls, const RoundEngine& e);
int round_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
              int32_t* status, const RoundEngine& e);
uint32_t env_grid(const char* name);  // a GS_*_GRID variable clamped to 1..4096; 0: unset
int read_words(gs_ctx* c, uint64_t* words, const unsigned long long* d);  // d's W words to the host, then the sync

// gs_rumor_host.cpp
int rumor_refuse(const gs_params* params, const char* what);
int rumor_alloc(gs_ctx* c);
void release_rumor(gs_ctx* c);
int rumor_begin(gs_ctx* c, uint64_t sender);
int rumor_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls);
int rumor_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
              int32_t* status);
int rumor_read_removed(gs_ctx* c, uint64_t* words, size_t nwords);
std::string rmt_limit_error(int device, uint32_t mode, uint64_t* lim);
int check_rmt_n(const gs_params* p, int device, std::string& why, RmtPlan* pl);

// gs_median_host.cpp
int median_refuse(const gs_params* params, const char* what);
int median_alloc(gs_ctx* c);
void release_median(gs_ctx* c);
int median_begin(gs_ctx* c, uint64_t sender);
int median_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls);
int median_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
               int32_t* status);
int median_read_removed(gs_ctx* c, uint64_t* words, size_t nwords);
int median_read_state(gs_ctx* c, uint8_t* st, size_t n);
std::string mdt_limit_error(int device, bool packed, uint64_t* lim);
int check_mdt_n(const gs_params* p, bool median_trials, int device, std::string& why, MdtPlan* pl, bool* packed);
int mdt_load_device(gs_ctx* c, const void* d_deg, const void* d_ids, uint32_t stride);

// gs_rumorset_host.cpp
int rs_check_create(const gs_params* params, uint32_t rumors);
int rs_alloc(gs_ctx* c);
void release_rumorset(gs_ctx* c);
int rs_begin(gs_ctx* c, const int64_t* senders, const int64_t* starts = nullptr);  // starts NULL: every rumor at begin
int rs_set_payload(gs_ctx* c, uint32_t payload, uint32_t pick);
int rs_traffic(gs_ctx* c, gs_rumorset_traffic* out);
int rs_step(gs_ctx* c, uint32_t ticks, gs_tick_stats* out, bool every_tick_polls);
int rs_run(gs_ctx* c, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out, size_t cap, size_t* nout,
           int32_t* status);
int rs_results(gs_ctx* c, gs_rumor_stats* out, size_t cap, size_t* nout);
int rs_read_words(gs_ctx* c, uint64_t* have, size_t n);
int rs_read_column(gs_ctx* c, uint32_t rumor, uint64_t* words, size_t nwords);

}  // namespace gs
