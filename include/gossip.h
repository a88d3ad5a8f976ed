/*
 * gossip.h -- C ABI of libgossip_hip.so, the MI355X (gfx950) engine for the
 * broadcast round loop of go-distributed/gossip_simulator (simulator.go).
 *
 * The reference has no FFI/plugin seam: it is one Go `package main`.  This ABI
 * is the seam a maintainer adds behind its `main` (simulator.go:207-253); each
 * entry point names the reference code it replaces.  A cgo binding is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *  - return 0 on success, <0 on error (GS_E*); message via gs_last_error().
 *  - all caller buffers are caller-owned and copied during the call; nothing
 *    is retained across calls (cgo pointer rules).
 *  - one gs_ctx is single-threaded.  gs_create gives one HIP device and one
 *    stream; gs_create_multi spreads one context over several devices (or
 *    several shards of one device) and gs_create_rank makes one shard of a
 *    multi-process (RCCL) run -- every other call is the same for all three.
 *  - node ids are uint32 (n <= 2^31-1); friend rows are uint32[stride] with a
 *    uint8 length per node (a friends list is at most 255 long).
 *  - every random decision is drawn from Philox4x32-10 keyed by
 *    (seed; kind, trial, tick, node, slot) -- see DESIGN.md "Tick model".
 */
#ifndef GOSSIP_H
#define GOSSIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 6

enum {
  GS_OK = 0,
  GS_EINVAL = -1,     /* bad parameter or call order                          */
  GS_ELIVELOCK = -2,  /* overlay never stabilised (fanin <= fanout livelock)  */
  GS_EREJECT = -3,    /* replacement-friend rejection exhausted (n <= 2)      */
  GS_ENOMEM = -4,     /* host or device allocation failed                     */
  GS_EDEVICE = -5,    /* HIP runtime error / no gfx950 device                 */
  GS_EOVERFLOW = -6   /* a counter exceeded its range                         */
};

/* Flags (gs_params.flags). */
#define GS_FLAG_TIMING 1u /* time every tick kernel with HIP events (gs_timing) */
#define GS_FLAG_TICK_ENGINE 2u /* force the per-tick atomic engine (default: window engine) */
#define GS_FLAG_PP_L2_ONLY 4u  /* push-pull: skip the LDS-staged second-level summaries (the path
                                * N > ~1.02e9 takes); read at gs_create, for tests */
#define GS_FLAG_PP_DENSE 8u    /* push-pull: every round streams the whole table (no reverse
                                * table, no sparse early rounds); same results, for tests */
#define GS_FLAG_PP_EARLY 16u   /* push-pull: sparse early rounds at any informed count (default:
                                * while |I| <= n/256); same results, for tests */
#define GS_FLAG_PP_TOPDOWN 32u /* push-pull: dense rounds always push by atomics (default: bottom-up,
                                * receivers scan their in-edges, once |I| >= 96n/256); same results */
#define GS_FLAG_PP_BOTTOM 64u  /* push-pull: every dense round bottom-up; same results, for tests */
#define GS_FLAG_PP_ANSWER 128u /* push-pull: every dense round below the bottom-up threshold pull-answer
                                * (informed nodes answer the pulls among their in-edges; the default
                                * does too unless GS_PP_ANSWER256 is set); same results, for tests */
#define GS_FLAG_MEDIAN_PACKED 256u /* gs_create_batch with GS_MODEL_MEDIAN and trials > 1: the batch keeps
                                * 16-bit tallies (208 B per 64 nodes, not 336), so n may reach
                                * gs_median_trials_max_n_packed(), 50,304 on an MI355X; the price is the
                                * in-degree bound checked at gs_broadcast_begin (below, gs_create_batch).
                                * Read at that create only: gs_set_flags does not switch a live context,
                                * and every other create and model never looks at the bit.  Same results */

/* Dissemination model (gs_params.model). */
#define GS_MODEL_FLOOD 0u    /* the reference: every receipt re-broadcasts to all friends (simulator.go:107-149) */
#define GS_MODEL_PUSHPULL 1u /* extension (config C5), no reference counterpart: one synchronous
                              * round per tick; each live node calls one Philox-picked friend,
                              * informed callers push, uninformed callers pull; -droprate loses
                              * calls, -crashrate is unused, gs_set_failed masks nodes
                              * (oracle/gsoracle.h).  With trials > 1:
                              * one workgroup per trial, the trial's informed set in LDS, so
                              * n <= gs_pp_trials_max_n(); the GS_FLAG_PP_* round modes are
                              * accepted and ignored (there is one round kind); gs_set_failed
                              * takes one mask per trial (a third bitset in LDS, so then
                              * n <= gs_pp_trials_max_n_masked()) */
#define GS_MODEL_RUMOR 2u    /* extension, no reference counterpart: rumor mongering with loss of
                              * interest (Demers et al.).  One synchronous round per tick; every HOT
                              * node (informed, live, a friend to call, fewer than rumor_k misses)
                              * calls one Philox-picked friend; a kept call to a live uninformed
                              * friend informs it (hot from the next round), one to a friend that
                              * was informed at the start of the round is a miss, and after
                              * rumor_k misses the caller is REMOVED.  The run ends by itself when
                              * no node is hot.  -droprate loses calls (no feedback either),
                              * -delaylow/-delayhigh/-crashrate are unused, gs_set_failed masks
                              * nodes (a failed callee gives no feedback).  gs_tick_stats.pending =
                              * the hot nodes after the round.  One device: gs_create_multi and
                              * gs_create_rank[_exchange] answer GS_EINVAL, and so does gs_create
                              * with trials > 1; gs_create_trials makes a batch of trials (one
                              * workgroup per trial, the trial's sets and miss counts in LDS, so
                              * n <= gs_rumor_trials_max_n(); gs_set_failed takes one mask per
                              * trial and needs no further LDS)
                              * (DESIGN.md sections 4.7, 4.7.2).  gs_params.rumor_mode (GS_RUMOR_*)
                              * selects the other variants of Demers et al.; 0 is the model
                              * above */
#define GS_MODEL_MEDIAN 3u   /* extension, no reference counterpart: the median-counter push-pull of
                              * Karp, Schindelhauer, Shenker and Voecking, a push-pull that ends by
                              * itself.  One synchronous round per tick; every live node with a
                              * friend that is not done calls one Philox-picked friend, and a kept
                              * call to a live friend is a connection on which the rumor moves both
                              * ways (messages counts the active ends).  A node is uninformed (A),
                              * informed with a counter 1..rumor_k (B), in the final phase of
                              * rumor_k rounds (C) or done (D); a B node advances its counter when
                              * more of the round's partners are B with a counter at least its own
                              * than are A or B with a smaller one, a C partner moves an A or B
                              * node straight to C, and after the counter's rumor_k steps and the
                              * rumor_k rounds of C the node is done and silent.  The run ends by
                              * itself when no node is B or C.  rumor_k must be 1..127; -droprate
                              * loses calls, -delaylow/-delayhigh/-crashrate and rumor_mode are
                              * unused, gs_set_failed masks nodes (no connection reaches them).
                              * gs_tick_stats.pending = the B and C nodes after the round.  An
                              * informed node that nobody connects to, or whose partners are all
                              * done already, stays B, so such a run ends GS_RUN_MAX_TICKS (a
                              * short counter strands some nodes this way: DESIGN.md section 4.8).
                              * One trial on one device through gs_create; gs_create_batch is the
                              * batch of trials (one workgroup per trial, the trial's state in LDS,
                              * so n <= gs_median_trials_max_n(), or with GS_FLAG_MEDIAN_PACKED
                              * n <= gs_median_trials_max_n_packed(); DESIGN.md sections 4.8.1,
                              * 4.8.2).  The
                              * four other creates keep refusing: gs_create with trials > 1,
                              * gs_create_trials, gs_create_multi and gs_create_rank[_exchange]
                              * answer GS_EINVAL */

/* Variants of GS_MODEL_RUMOR (gs_params.rumor_mode, any combination; the other
 * models ignore the field; another bit answers GS_EINVAL). */
#define GS_RUMOR_BLIND 1u /* a hot node has an event every round it is hot, reply or not (a lost
                           * call and a failed callee count too), instead of only when its call
                           * reached an informed peer */
#define GS_RUMOR_COIN 2u  /* an event removes the node with probability 1/rumor_k (a keyed draw)
                           * instead of after rumor_k events; the miss counts stay 0 */
#define GS_RUMOR_PULL 4u  /* every live node with a friend calls every round; a call that reaches
                           * a hot node informs an uninformed caller (the hot node was served) or
                           * was in vain; a hot node's event: asked in vain and not served in the
                           * round (feedback), or every round (blind).  Hot needs no friend here.
                           * A hot node that no live node ever calls stays hot with feedback, so
                           * such a run ends GS_RUN_MAX_TICKS */

/* simulator.go:11-20 (Parameters) + the additive -seed/-trial knobs. */
typedef struct gs_params {
  uint64_t n;          /* -n          simulator.go:187                       */
  int32_t fanout;      /* -fanout     simulator.go:188                       */
  int32_t fanin;       /* -fanin      simulator.go:189 (default 6, see :189) */
  int32_t delay_low;   /* -delaylow   simulator.go:190 (ms = ticks)          */
  int32_t delay_high;  /* -delayhigh  simulator.go:191                       */
  double drop_rate;    /* -droprate   simulator.go:192 -> int(rate*100) %    */
  double crash_rate;   /* -crashrate  simulator.go:193 -> int(rate*100) %    */
  uint64_t seed;       /* Philox key                                          */
  uint32_t trial;      /* Philox counter word 3, low 24 bits                  */
  int32_t device;      /* HIP device ordinal                                  */
  uint32_t flags;      /* GS_FLAG_*                                           */
  uint32_t model;      /* GS_MODEL_* (0 = the reference's push flooding)      */
  /* Batched independent trials (config C3): trials trial .. trial+trials-1 of n
   * nodes each, run at once (one overlay, one broadcast per trial, keyed by
   * its trial number exactly as a one-trial context).  0 or 1 = one trial.
   * Every model (GS_MODEL_RUMOR: through gs_create_trials only);
   * trials << max(14, ceil(log2 n)) must be < 2^31.
   * The reference runs one trial per process (simulator.go:207-253). */
  uint32_t trials;
  uint32_t rumor_k;    /* GS_MODEL_RUMOR: misses after which a node stops calling, 1..255;
                        * GS_MODEL_MEDIAN: the counter steps and the final phase's rounds, 1..127
                        * (the other models ignore it) */
  uint32_t rumor_mode; /* GS_MODEL_RUMOR: GS_RUMOR_* bits, 0 = push with feedback and counter
                        * (the other models ignore it) */
  uint32_t reserved32_;
  uint64_t reserved_[4];
} gs_params;

/* One tick (1 ms) of the broadcast phase; the reference exposes these as the
 * int32 atomics of simulator.go:26-31, read by main's poll loop (:243-253). */
typedef struct gs_tick_stats {
  uint64_t tick;      /* simulated ms since Broadcast() (:239-241)            */
  uint64_t fired;     /* Broadcast goroutines whose delay expired (:142)     */
  uint64_t sent;      /* friend slots not dropped = delivered sends (:144-145)*/
  uint64_t messages;  /* TotalMessage increments (:111)                      */
  uint64_t received;  /* TotalReceived, cumulative (:121)                    */
  uint64_t crashed;   /* TotalCrashed, cumulative (:114)                     */
  uint64_t pending;   /* broadcasts scheduled, not yet fired                  */
} gs_tick_stats;

/* One 10-ms poll window of overlay construction (simulator.go:222-234). */
typedef struct gs_window {
  uint64_t tick;      /* end of the window (ms)                               */
  uint64_t makeups;   /* MakeUps  in the window (:67)                         */
  uint64_t breakups;  /* BreakUps in the window (:77)                         */
} gs_window;

/* Device time spent in the broadcast kernels (GS_FLAG_TIMING), from HIP
 * events on the context's stream.  Tick engine: deliver = the per-tick
 * delivery kernel, resolve = its second (kc > 0) pass.  Window engine:
 * deliver = expand + partition (expand_ms + part_ms), resolve = k_resolve. */
typedef struct gs_timing {
  double deliver_ms;       /* sum over launches of the delivery kernel(s)    */
  double resolve_ms;       /* sum over launches of the resolve kernel        */
  uint64_t deliver_launches;
  uint64_t resolve_launches;
  double overlay_ms;       /* wall time of the last gs_build_overlay          */
  double expand_ms;        /* window engine: k_expand (row gather + coarse partition) */
  double part_ms;          /* window engine: k_plan + k_part2 (fine partition)        */
  uint64_t windows;        /* window engine: windows processed                */
  uint64_t exact_redos;    /* window engine: windows re-partitioned exactly   */
  double prep_ms;          /* push-pull: wall time of the last reverse-table / failed-slot-mask
                            * build (at gs_broadcast_begin, once per table / failure mask) */
  uint64_t pp_early_rounds;  /* push-pull: rounds of this broadcast run sparse (informed list)   */
  uint64_t pp_bottom_rounds; /* push-pull: dense rounds of this broadcast run bottom-up          */
  uint64_t pp_answer_rounds; /* push-pull: dense rounds of this broadcast run pull-answer        */
  uint64_t dd_fallbacks;     /* device-driven shard windows stopped by an overflow and redone
                              * host-driven (cumulative; a buffer that fits makes it stop growing) */
  uint64_t pp_rev_part;      /* push-pull: the passes of the last reverse table's partition build
                              * (>= 1), or 0 if the atomic count + fill built it (GS_PP_REV_ATOMIC, or a
                              * fallback) */
  uint64_t ov_part_ticks;    /* last overlay build: ticks grouped by the destination partition     */
  uint64_t ov_sort_ticks;    /* last overlay build: ticks grouped by the radix sort (sparse ticks,
                              * GS_OV_SORT=1, or a partition fallback)                              */
  uint64_t ov_part_fallbacks; /* last overlay build: partition plans that overflowed (then sorted) */
  /* Device memory, process-wide and cumulative since the library was loaded (every
   * context shares the library's cache of large blocks; see gs_trim).  The reference
   * allocates its nodes once per process (simulator.go:208-212). */
  double alloc_ms;           /* wall time inside hipMalloc                                      */
  double largest_alloc_ms;   /* the longest single hipMalloc                                    */
  double free_ms;            /* wall time inside hipFree and the cache's idle waits             */
  uint64_t alloc_calls;      /* hipMalloc calls                                                 */
  uint64_t alloc_cache_hits; /* device buffers served from the cache (no hipMalloc)             */
  uint64_t cached_bytes;     /* bytes the cache holds free now                                  */
  uint64_t coarse_redos;     /* window engine, host-driven windows: windows whose k_expand overflowed
                              * a coarse region estimate and ran again from exact counts (cumulative) */
} gs_timing;

/* gs_run status */
enum { GS_RUN_COVERED = 0, GS_RUN_QUIESCENT = 1, GS_RUN_MAX_TICKS = 2, GS_RUN_RUNNING = -1 };

/* One trial's outcome (batched trials, or the one trial of any flood context):
 * the counters at the poll that stopped it under gs_run's rule -- what the
 * reference prints at :252-253 -- plus the first tick it was covered. */
typedef struct gs_trial_stats {
  uint64_t trial;     /* trial number (Philox counter word 3)                 */
  uint64_t tick_99;   /* first tick with float32(recv)/float32(n) >= 0.99, else 0 */
  uint64_t tick;      /* tick of the stopping poll (or the last tick run)     */
  uint64_t fired, sent, messages, received, crashed;  /* cumulative at `tick` */
  int32_t status;     /* GS_RUN_* (GS_RUN_RUNNING: not stopped yet)          */
  int32_t reserved_;
} gs_trial_stats;

typedef struct gs_ctx gs_ctx;

int gs_version(void);
const char* gs_strerror(int code);

/* Replaces simulator.go:186-212 (flag globals, GlobalView/NewNode allocation).
 * Validates params exactly as the reference would fail: n == 0 (:240 panics),
 * delay_high <= delay_low (:167 panics).  One device (params.device). */
int gs_create(const gs_params* params, gs_ctx** out);

/* ---- multi-GPU (no reference counterpart: the reference runs every node as
 * a goroutine of one process, simulator.go:214-217) ----
 * One context over ndev devices (entries may repeat: several shards or trial
 * batches on one GPU).  params.trials > 1: the trials are split over the
 * devices and run with no communication.  Otherwise ONE broadcast whose node
 * range is split into ndev shards (config C4): every window each shard
 * expands its own firing nodes and hands every other shard the messages
 * addressed to its nodes (an all-to-all: device-to-device copies), then
 * resolves its own nodes; counters are summed.  Results are bit-identical to
 * gs_create's. */
int gs_create_multi(const gs_params* params, const int* devices, int ndev, gs_ctx** out);
/* Multi-process (one process per GPU): rank 0 calls gs_comm_unique_id and
 * ships the GS_COMM_ID_BYTES bytes to every rank; each rank calls
 * gs_create_rank.  A flood run is then node-range sharded over the ranks with
 * an RCCL all-to-all of each window's messages (grouped send/recv, after an
 * all-gather of the fire counts and the message layout) and an RCCL sum per
 * gs_step (every rank's
 * gs_step/gs_run/gs_totals return the global counters); a push-pull run
 * (rows <= 16 slots) is node-range sharded with an all-gather of the informed
 * set's owned words per round; params.trials > 1 gives each rank its share of
 * the trials (no communication, id may be NULL).  gs_create_multi splits both
 * models the same way over its devices. */
#define GS_COMM_ID_BYTES 128
int gs_comm_unique_id(uint8_t id[GS_COMM_ID_BYTES]);
int gs_create_rank(const gs_params* params, int device, int nranks, int rank,
                   const uint8_t* id, gs_ctx** out);
/* The same with the exchange done by the caller instead of RCCL (MPI, a
 * torch.distributed group, a test harness): every rank calls it with the same
 * nranks and its own rank, and the callbacks move HOST bytes between the
 * ranks -- all_gather: `bytes` from every rank into recv (nranks * bytes,
 * rank-major; send is this rank's part); all_reduce_sum_u64: element-wise sum
 * over the ranks of count uint64, in place; all_to_allv (flood runs): rank r
 * gets send_bytes[r] bytes of send (the blocks lie back to back in rank
 * order) and recv receives recv_bytes[r] bytes from every rank r, back to back
 * in rank order.  All return 0 on success and are called by every rank in the
 * same order.  Unlike every other argument the struct is kept: user and the
 * callbacks must stay valid until gs_destroy. */
typedef struct gs_exchange {
  void* user;
  int (*all_gather)(void* user, const void* send, void* recv, size_t bytes);
  int (*all_reduce_sum_u64)(void* user, uint64_t* buf, size_t count);
  int (*all_to_allv)(void* user, const void* send, const size_t* send_bytes, void* recv,
                     const size_t* recv_bytes);
} gs_exchange;
int gs_create_rank_exchange(const gs_params* params, int device, int nranks, int rank, const gs_exchange* ex,
                            gs_ctx** out);
/* Nodes [lo, hi) owned by shard `index` of a context (index < *nshards);
 * an unsharded context is one shard [0, n). */
int gs_shard_info(const gs_ctx* ctx, uint32_t index, uint32_t* nshards, uint64_t* lo, uint64_t* hi);
void gs_destroy(gs_ctx* ctx);
/* ctx == NULL: why the calling thread's last gs_create* failed (a failed create
 * leaves no context to ask; this is how the limit of a batched push-pull
 * context reaches the caller); "NULL context" if it gave no reason. */
const char* gs_last_error(const gs_ctx* ctx);
/* Largest n a batched push-pull context (trials > 1, GS_MODEL_PUSHPULL) may
 * have on `device`: a trial's two informed bitsets must fit the LDS the
 * device grants one workgroup.  gs_create refuses a larger n with GS_EINVAL.
 * (Where no device is visible gs_create keeps answering GS_EINVAL for
 * trials > 1 with GS_MODEL_PUSHPULL, as it did before the combination
 * existed; every other create, and this query, then fail with GS_EDEVICE.) */
int gs_pp_trials_max_n(int device, uint64_t* n_max);
/* The same for a batched push-pull context that is given failure masks
 * (gs_set_failed): the trial's failed set is a third bitset in LDS, so this
 * limit is about two thirds of gs_pp_trials_max_n's.  A context past it runs
 * unmasked; gs_set_failed refuses it with GS_EINVAL. */
int gs_pp_trials_max_n_masked(int device, uint64_t* n_max);
/* gs_create that also accepts GS_MODEL_RUMOR with params.trials > 1: a batched
 * rumor context on params.device, trials params.trial .. params.trial +
 * trials - 1 run at once, a workgroup each.  Every other parameter set is
 * handled exactly as by gs_create (rumor with trials <= 1 included).
 * Why there are two creates: gs_create has always answered GS_EINVAL for the
 * rumor model with trials > 1, callers were told so and fall back to a loop of
 * one-trial contexts when they see it, and programs test for that answer; it
 * keeps giving it.  This create is the opt-in.  Every parameter check runs
 * before any device call (rumor_k, rumor_mode, the 31-bit id space): bad
 * parameters answer GS_EINVAL with the reason in gs_last_error(NULL) even
 * where no device is visible, valid ones then answer GS_EDEVICE.  n past
 * gs_rumor_trials_max_n() of the mode answers GS_EINVAL and names the limit.
 * The batched context takes the usual calls with the batched layouts of the
 * other models (gs_load_peers: tables back to back; gs_set_failed: one mask
 * per trial; gs_broadcast_begin: a fixed node in every trial, or < 0 each
 * trial's keyed sender; gs_step rows: sums over the trials, pending = their
 * hot nodes; gs_read_received / _crashed / _removed: trials x ceil(n/64)
 * words, trial-major).  Trial i behaves exactly like a one-trial gs_create
 * context with params.trial + i, trial i's table and trial i's mask, round by
 * round, also in rounds stepped after its own end.  gs_run: each trial stops
 * at the first poll at which it has no hot node (GS_RUN_COVERED or
 * GS_RUN_QUIESCENT by the float32 rule at that poll) or at max_ticks; the run
 * ends when all have stopped, with the latest status among them.
 * Trials do not communicate: to use several devices make one such context per
 * device with an offset params.trial (gs_create_multi and gs_create_rank keep
 * refusing the rumor model). */
int gs_create_trials(const gs_params* params, gs_ctx** out);
/* Largest n a batched rumor context of gs_params.rumor_mode `rumor_mode` may
 * have on `device`: three bitsets (five with GS_RUMOR_PULL and feedback) and,
 * unless GS_RUMOR_COIN, a miss byte per node must fit the LDS the device
 * grants one workgroup.  gs_create_trials refuses a larger n with GS_EINVAL.
 * A failure mask does not lower it.  GS_EINVAL for a bad mode bit, GS_EDEVICE
 * where the device cannot be asked. */
int gs_rumor_trials_max_n(int device, uint32_t rumor_mode, uint64_t* n_max);
/* gs_create_trials with one more refusal lifted: GS_MODEL_MEDIAN with
 * params.trials > 1 makes a batched median context on params.device, trials
 * params.trial .. params.trial + trials - 1 run at once, a workgroup each.
 * Every other parameter set is handled exactly as by gs_create_trials (median
 * with trials <= 1: the one-trial context of gs_create).  It is a third create
 * for the reason given above: gs_create and gs_create_trials have always
 * answered GS_EINVAL for a median batch, programs test for that answer, and
 * they keep giving it.  Every parameter check runs before any device call
 * (rumor_k 1..127, the 31-bit id space, n >= 1): bad parameters answer
 * GS_EINVAL with the reason in gs_last_error(NULL) even where no device is
 * visible, valid ones then answer GS_EDEVICE.  n past gs_median_trials_max_n()
 * answers GS_EINVAL and names the limit (31,104 on an MI355X).  The reference's
 * default n = 50,000 needs GS_FLAG_MEDIAN_PACKED in params.flags: the batch
 * then keeps a 16-bit tally per node, two to a word, n may reach
 * gs_median_trials_max_n_packed() (50,304 on an MI355X; a larger n answers
 * GS_EINVAL and names that limit), and every result is the same, at any n.
 * What the flag costs is an in-degree bound: the tallies are exact only while
 * no node has more than 32,767 partners in a round.  With n <= 32,766 that
 * holds for every table.  Past it, the first gs_broadcast_begin after a table
 * entered (gs_load_peers, gs_load_peers_device, gs_build_overlay) counts, on
 * the device, the used slots of each trial's table that name each node --
 * slots, not rows, which is conservative: a row that names a node twice calls
 * it once -- and if some node is named by more than 32,766 it answers
 * GS_EINVAL; gs_last_error names the trial, the node, its count and the
 * bound.  The table is kept and the context stays usable: load another table
 * and begin again.  The overlay's own tables (fanin 6) are far inside the
 * bound.
 * The batched context takes the usual calls with the batched layouts
 * (gs_load_peers and gs_load_peers_device: tables back to back;
 * gs_build_overlay: the batch's own overlays; gs_set_failed: one mask per
 * trial; gs_broadcast_begin: a fixed node in every trial, or < 0 each trial's
 * keyed sender; gs_step rows: sums over the trials, pending = their active
 * nodes; gs_read_received / _crashed / _removed: trials x ceil(n/64) words,
 * trial-major; gs_read_median_state: trials x n bytes, trial-major).  Trial i
 * behaves exactly like a one-trial gs_create context with params.trial + i,
 * trial i's table and trial i's mask, round by round, also in rounds stepped
 * after its own end.  gs_run: each trial stops at the first poll at which it
 * has no active node (GS_RUN_COVERED or GS_RUN_QUIESCENT by the float32 rule
 * at that poll) or at max_ticks; the run ends when all have stopped, with the
 * latest status among them. */
int gs_create_batch(const gs_params* params, gs_ctx** out);
/* Largest n a batched median context may have on `device`: a state byte and a
 * signed tally word per node and two bitsets (336 B per 64 nodes) must fit the
 * LDS the device grants one workgroup.  gs_create_batch refuses a larger n
 * with GS_EINVAL.  A failure mask does not lower it.  GS_EDEVICE where the
 * device cannot be asked. */
int gs_median_trials_max_n(int device, uint64_t* n_max);
/* The same for a batch made with GS_FLAG_MEDIAN_PACKED: a state byte and a
 * 16-bit tally per node and two bitsets (208 B per 64 nodes). */
int gs_median_trials_max_n_packed(int device, uint64_t* n_max);

/* ---- concurrent rumors for push-pull ----
 * Who calls whom in a push-pull round, and which calls are lost, does not
 * depend on who is informed, so `rumors` broadcasts over one table with one
 * seed share every table read and every draw.  A rumor set runs them in one
 * pass: a uint64 per node whose bit j says that the node holds rumor j, and on
 * every kept call to a live friend both ends learn everything the other held
 * at the start of the round.  Column j of the words after round t is bit for
 * bit the informed set of a one-rumor GS_MODEL_PUSHPULL context with the same
 * seed, trial, table and mask after round t from sender j.  The counters are
 * the set's own: fired counts every caller, sent every kept call, messages the
 * ends of a connection that hold a rumor; received is the number of (node,
 * rumor) pairs and pending the started rumors still below 99 %.
 * gs_create_rumorset needs params.model == GS_MODEL_PUSHPULL, rumors in
 * 1..GS_RUMORSET_MAX, trials <= 1 and no flag besides GS_FLAG_TIMING; anything
 * else answers GS_EINVAL before any device call, the reason in
 * gs_last_error(NULL).  crash_rate, delay_*, rumor_k and rumor_mode are
 * unused.  One device.  The context takes gs_load_peers[_device],
 * gs_build_overlay, gs_read_peers, gs_set_failed, gs_set_trial, gs_set_stream,
 * gs_reset, gs_step, gs_run, gs_totals, gs_timing_get (deliver = the round,
 * resolve = commit + publish) and gs_read_crashed like a one-trial push-pull
 * context.  gs_broadcast_begin(ctx, s): s < 0 draws every sender, s >= 0
 * starts rumor j at (s + j) mod n.  gs_run stops at the first poll at which
 * every started rumor satisfies the float32 rule (GS_RUN_COVERED; if no rumor
 * started, GS_RUN_QUIESCENT at the first poll), else at max_ticks: there is no
 * test for "nothing can change any more".  gs_read_received gives the nodes
 * that hold every started rumor; gs_trial_results one row for the set, its
 * tick_99 the first poll with pending == 0; gs_read_removed and
 * gs_read_median_state answer GS_EINVAL. */
#define GS_RUMORSET_MAX 64u
typedef struct gs_rumor_stats {
  int64_t  sender;    /* the node the rumor started at                        */
  uint64_t received;  /* nodes that hold it now                               */
  uint64_t tick_99;   /* first poll at which the float32 rule held, else 0    */
  int32_t  started;   /* 0: its sender was failed                             */
  int32_t  reserved_;
} gs_rumor_stats;
int gs_create_rumorset(const gs_params* params, uint32_t rumors, gs_ctx** out);
/* Rumor j starts at senders[j] (count must equal the set's rumors; an entry
 * >= n: GS_EINVAL); a negative entry draws uniform(Philox{j, 0, 0, SENDER}, n),
 * so rumor 0's keyed sender is the one gs_broadcast_begin(ctx, -1) draws on any
 * context.  A rumor whose sender is failed does not start.  Two rumors may
 * share a sender. */
int gs_rumorset_begin(gs_ctx* ctx, const int64_t* senders, size_t count);
/* One entry per rumor, in order (cap entries; *nout gets the count). */
int gs_rumorset_results(gs_ctx* ctx, gs_rumor_stats* out, size_t cap, size_t* nout);
/* The rumor words, have[n]: bit j of have[v] says that v holds rumor j. */
int gs_read_rumorset(gs_ctx* ctx, uint64_t* have, size_t n);
/* Column `rumor` of the words as a bitset, words[ceil(n/64)]: the informed set
 * of that one broadcast. */
int gs_read_rumor_column(gs_ctx* ctx, uint32_t rumor, uint64_t* words, size_t nwords);

/* ---- bounded rumor sets ----
 * A payload cap: a message carries at most `payload` rumors (1..64; 0 = no
 * cap, the section 4.9 path).  The ends of a connection are taken to exchange
 * digests, so with H the words at the start of the round and v the caller of
 * u, the caller's message carries give = pick(H[v] & ~H[u], o_push) and the
 * reply take = pick(H[u] & ~H[v], o_pull); next[u] |= give, next[v] |= take.
 * The cap is per message: a node that several callers reach receives up to
 * `payload` rumors from each.  pick(x, o) is x if it has at most `payload`
 * bits, else its `payload` lowest set bits (GS_PICK_LOW: with starts in index
 * order, oldest first), its highest (GS_PICK_HIGH: newest first) or the first
 * `payload` met going up from index o, wrapping from R - 1 to 0
 * (GS_PICK_ROTATE; o_push = uniform(r.z, R) and o_pull = uniform(r.w, R) of
 * the draw r the caller already makes).  Rumors compete for the payload, so a
 * column is no longer a one-rumor broadcast; fired, sent, messages, received
 * and pending keep their meaning.  payload >= 1 always runs the capped round
 * kernel, which moves what no cap moves once payload >= rumors.
 * gs_rumorset_set_payload: rumor-set contexts only; payload > 64 or an unknown
 * pick answers GS_EINVAL; refused between a begin and the next gs_reset; kept
 * by gs_reset and gs_set_trial. */
#define GS_PICK_LOW 0u
#define GS_PICK_HIGH 1u
#define GS_PICK_ROTATE 2u
int gs_rumorset_set_payload(gs_ctx* ctx, uint32_t payload, uint32_t pick);
/* gs_rumorset_begin with a start round per rumor, 0 <= starts[j] < 2^31
 * (starts NULL: every rumor at begin, which gs_rumorset_begin and
 * gs_broadcast_begin keep meaning).  Bit j is set at senders[j] after round
 * starts[j]'s commit, so that round's row and per-rumor count include it
 * (count 1) and round starts[j] + 1 is the first that moves it; 0 is at begin.
 * Whether its sender is failed is decided at begin.  started, pending and the
 * holds-every-rumor set refer to every rumor whose sender is not failed from
 * begin on, injected or not: until the last one is in nobody holds all of
 * them, and gs_run cannot stop GS_RUN_COVERED.  tick_99 stays an absolute
 * round. */
int gs_rumorset_begin_at(gs_ctx* ctx, const int64_t* senders, const int64_t* starts, size_t count);
/* Rumor copies, cumulative over the broadcast, as of the last round gs_step or
 * gs_run completed.  GS_EINVAL on a set without a cap (payload 0): its round
 * kernel counts none of them; payload 64 moves the same and counts. */
typedef struct gs_rumorset_traffic {
  uint64_t wanted;   /* rumors the receiving ends lacked, summed over messages  */
  uint64_t carried;  /* rumors the messages carried (<= wanted)                 */
  uint64_t bound;    /* messages that wanted more than `payload` rumors         */
  uint64_t reserved_;
} gs_rumorset_traffic;
int gs_rumorset_traffic_get(gs_ctx* ctx, gs_rumorset_traffic* out);

/* Injects a peer table in place of the overlay (the `friends` slices,
 * simulator.go:45,58).  deg[n] uint8, ids[n*stride] uint32 row-major.
 * Host buffers; copied.  Batched trials: trials tables back to back
 * (deg[trials*n], ids[trials*n*stride], ids local to their trial).  A sharded
 * context keeps only each shard's partition (gs_read_peers then fails).
 * stride 1..255 (a window-engine context without GS_FLAG_TICK_ENGINE: at
 * most 32); slots past a row's deg are never followed and may hold anything.
 * Refused (GS_EINVAL): a deg above the stride ("a friends-list length exceeds
 * the row stride") or a used slot >= n ("a friend id is >= n").  A table
 * with both: the length is reported; batched trials, checked on the host,
 * report whichever comes first in row order.
 * After a refusal the context has NO table: the new table is written over
 * the old one before it is validated, so a load that fails for any reason
 * other than its arguments (a NULL pointer, a stride outside 1..255, a
 * broadcast already begun: these touch nothing and keep the table) leaves the
 * context, every member of a gs_create_multi group and a push-pull shard's
 * replica without one.  Until the next load or overlay build that succeeds,
 * gs_broadcast_begin and gs_run answer GS_EINVAL "load peers or build the
 * overlay first" and gs_read_peers "no peer table". */
int gs_load_peers(gs_ctx* ctx, const uint8_t* deg, const uint32_t* ids, uint32_t stride);
/* Same, from device-resident buffers (copied device-to-device on the
 * context's stream).  One-trial one-device contexts, and a gs_create_batch
 * median batch (tables back to back); stride 2..255.  The same refusals and
 * the same state after one: a refusal of the arguments (NULL, stride, begun,
 * a group or a batched non-median context) keeps the table, any later one
 * leaves the context without a table. */
int gs_load_peers_device(gs_ctx* ctx, const void* d_deg, const void* d_ids, uint32_t stride);
/* Copies the current table out (stride = max(fanout, fanin) after an overlay).
 * Used slots hold the ids loaded or built; unused slots hold 0xFFFFFFFF on a
 * window-engine context (the rows are sealed) and what was loaded elsewhere.
 * "no peer table" before the first load or build and after a refused one. */
int gs_read_peers(gs_ctx* ctx, uint8_t* deg, uint32_t* ids, uint32_t* stride_out);

/* Replaces simulator.go:62-106,127-164 (makeup/breakup handlers, Makeup,
 * Breakup, removeFriend) and the stabilisation loop :214-235, on the GPU.
 * Writes one gs_window per non-final poll (up to cap; *nwin gets the total)
 * and the stabilising poll's tick.  GS_ELIVELOCK after max_ticks.  The build
 * writes into the table's buffers from its first tick: a build that fails
 * (GS_ELIVELOCK included) leaves the context without a table, as a refused
 * gs_load_peers does; only "overlay must be built before gs_broadcast_begin"
 * keeps the table. */
int gs_build_overlay(gs_ctx* ctx, uint64_t max_ticks, gs_window* win, size_t cap,
                     size_t* nwin, uint64_t* final_tick);

/* Pre-failed node mask (extension, config C5): words[ceil(n/64)], set bits
 * are crash-stopped before the broadcast: they never count nor forward, and
 * a failed sender does not broadcast (both models).  Set before
 * gs_broadcast_begin; kept by gs_reset and gs_set_trial.
 * Batched trials (both models): one mask per trial, trials x ceil(n/64)
 * words, trial-major (the layout of gs_read_received / gs_read_crashed; fewer
 * words: GS_EINVAL); bits at or past n in a trial's last word are ignored.
 * Trial i with its mask behaves exactly like a one-trial context of trial
 * params.trial + i given that mask; a trial whose sender is failed never
 * starts and stops at its first poll while the others run on.  A context
 * made by gs_create_multi hands each member its trials' slice; one made by
 * gs_create_rank takes the masks of that rank's trials only.  A push-pull
 * batch needs n <= gs_pp_trials_max_n_masked() (else GS_EINVAL, and the
 * context stays usable without a mask). */
int gs_set_failed(gs_ctx* ctx, const uint64_t* words, size_t nwords);

/* Replaces simulator.go:239-241.  sender < 0 draws it from the keyed stream
 * like rand.Intn(len(GlobalView)) (per trial when batched).  The sender is NOT
 * marked received. */
int gs_broadcast_begin(gs_ctx* ctx, int64_t sender);
/* Advances `ticks` ticks of the receive/broadcast actors (simulator.go:107-123,
 * 140-149, 166-184); out[i] (may be NULL) gets each tick's stats. */
int gs_step(gs_ctx* ctx, uint32_t ticks, gs_tick_stats* out);
/* Replaces the poll loop simulator.go:243-251: steps `poll` ticks at a time
 * until float32(received)/float32(n) >= 0.99 at a poll (GS_RUN_COVERED), no
 * broadcast is pending (GS_RUN_QUIESCENT; the reference would spin forever;
 * push-pull: no call can change the informed set any more -- no live
 * informed node has a live uninformed friend and no live uninformed node has
 * an informed friend, or every call is dropped), or max_ticks.  out (may be
 * NULL) receives one gs_tick_stats per poll.  Batched trials: each trial
 * stops at its own poll (gs_trial_results); the run ends when all have.
 * GS_MODEL_RUMOR runs to its own end: it stops at the first poll with no hot
 * node (pending == 0) -- GS_RUN_COVERED if the float32 rule holds at that poll,
 * else GS_RUN_QUIESCENT -- or at max_ticks; reaching 99 % does not stop it, and
 * gs_trial_stats.tick_99 is the first poll at which the rule held. */
int gs_run(gs_ctx* ctx, uint32_t poll, uint64_t max_ticks, gs_tick_stats* out,
           size_t cap, size_t* nout, int32_t* status);
/* Cumulative totals so far (tick, fired/sent/messages summed). */
int gs_totals(gs_ctx* ctx, gs_tick_stats* out);

/* Per-trial outcomes, trials in order (cap entries; *nout gets the count). */
int gs_trial_results(gs_ctx* ctx, gs_trial_stats* out, size_t cap, size_t* nout);

/* Bitset dumps for per-round parity: words[ceil(n/64)], bit v of word v/64
 * (batched trials: trials x ceil(n/64) words, trial-major).  A rank of a
 * multi-process run fills only the words of the nodes it owns (others 0). */
int gs_read_received(gs_ctx* ctx, uint64_t* words, size_t nwords);
int gs_read_crashed(gs_ctx* ctx, uint64_t* words, size_t nwords);
/* GS_MODEL_RUMOR: the removed nodes -- informed and no longer hot (rumor_k
 * events or a lost coin toss, or in the push modes no friend to call; with
 * GS_RUMOR_PULL an informed live node with no friend is hot, not removed) --
 * in the same layout, words[ceil(n/64)] (a gs_create_trials batch: trials x
 * ceil(n/64) words, trial-major; removed = informed and not hot in every mode).
 * GS_MODEL_MEDIAN: the done nodes (state D).
 * GS_EINVAL on a context of another model. */
int gs_read_removed(gs_ctx* ctx, uint64_t* words, size_t nwords);
/* GS_MODEL_MEDIAN: every node's state byte, st[n]: 0 = uninformed (A), m in
 * 1..rumor_k = informed with counter m (B-m), rumor_k + c = round c of the final
 * phase (C-c, c in 1..rumor_k), 255 = done (D).  gs_read_received gives the
 * nodes whose byte is not 0, gs_read_removed those at 255.  A gs_create_batch
 * batch: trials x n bytes, trial-major (a shorter buffer: GS_EINVAL).
 * GS_EINVAL on a context of another model. */
int gs_read_median_state(gs_ctx* ctx, uint8_t* st, size_t n);

int gs_timing_get(gs_ctx* ctx, gs_timing* out);
/* The same for shard `index` of a sharded (or batched) context's members;
 * index 0 of a one-device context is gs_timing_get. */
int gs_shard_timing(gs_ctx* ctx, uint32_t index, gs_timing* out);
/* Renumber the context's trial(s) to trial .. trial+trials-1 (Philox
 * counter word 3) between runs, keeping its device buffers: the overlay must
 * be built or loaded again before gs_broadcast_begin (config C3 runs batch
 * after batch in one context this way). */
int gs_set_trial(gs_ctx* ctx, uint32_t trial);
/* Replace gs_params.flags (e.g. toggle GS_FLAG_TIMING between runs). */
int gs_set_flags(gs_ctx* ctx, uint32_t flags);
/* Return to the state before gs_broadcast_begin: clears received/crashed,
 * the fire ring and the counters; keeps the peer table and failure mask
 * (a fresh process in the reference, simulator.go:207). */
int gs_reset(gs_ctx* ctx);

/* Run all later device work of a one-device context on `hip_stream` (a
 * hipStream_t owned by the caller); NULL restores the context's own stream. */
int gs_set_stream(gs_ctx* ctx, void* hip_stream);
/* Device-memory cache.  Device buffers of >= 64 MiB come from a process-wide
 * cache: a destroyed context's blocks (or a rebuilt table's temporaries) stay
 * mapped and serve the next context's requests, so a process that creates
 * context after context does not hand tens of GB back to the driver and ask
 * for them again (first allocations after large frees ran seconds slow on
 * some MI355X boxes).  gs_trim returns every free cached
 * block of `device` (-1: all devices) to the driver; *released (may be NULL)
 * gets the bytes.  The cache also trims itself before a hipMalloc the device
 * has no room for.  GS_DEVMEM_CACHE=0 in the environment disables it.  The
 * reference allocates once per process (simulator.go:208-212). */
int gs_trim(int device, size_t* released);
/* The device-memory fields of a gs_timing, alloc_ms .. cached_bytes, without a
 * context; every other field is zero. */
int gs_memory_stats(gs_timing* out);

/* ---- host-only helpers for the reference's stdout contract ------------- */
/* Go fmt %v of a float32 (strconv 'g', -1, 32), e.g. 99.61 or 9.9999994e-08
 * (simulator.go:247).  Returns the length written (NUL-terminated). */
size_t gs_format_float32(float x, char* buf, size_t cap);
/* Go fmt %v of a float64 (flag echo, simulator.go:199). */
size_t gs_format_float64(double x, char* buf, size_t cap);
/* Go time.Duration.String() of `ns` nanoseconds, e.g. 1.5s, 120ms, 1m0s. */
size_t gs_format_duration(int64_t ns, char* buf, size_t cap);
/* Go int(rate*100) (simulator.go:172,180), clamped to [0,100]. */
int32_t gs_threshold(double rate);
/* Philox4x32-10 (for replay tooling and tests). */
void gs_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
