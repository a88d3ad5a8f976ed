"""Python host API over the C ABI: the operator-level mirror of simulator.go.

`Simulator` keeps the reference's parameter names (simulator.go:11-20,
186-193) and phases: `build_overlay()` = main :214-235, `broadcast_begin()` =
:239-241, `step()` / `run()` = the receive/broadcast actors plus the poll loop
:243-251.  All compute runs in libgossip_hip.so on a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import GossipError, Params, TickStats, Timing, TrialStats, Window

STAT_FIELDS = ("tick", "fired", "sent", "messages", "received", "crashed", "pending")
TRIAL_FIELDS = ("trial", "tick_99", "tick", "fired", "sent", "messages", "received", "crashed",
                "status")


@dataclass
class Config:
    """The reference's flags (simulator.go:187-193) plus additive knobs."""
    n: int = 50000
    fanout: int = 5
    fanin: int = 6          # Fanout+1 evaluated before Parse -> always 6 (:189)
    delaylow: int = 10
    delayhigh: int = 20
    droprate: float = 0.1
    crashrate: float = 0.001
    seed: int = 1
    trial: int = 0
    device: int = 0
    timing: bool = False
    engine: str = "window"  # "window" (default) or "tick" (per-tick atomic engine)
    model: str = "flood"    # "flood" (the reference), "pushpull" (extension),
                            # "rumor" (extension, DESIGN.md 4.7: one device; a batch of trials
                            # through Simulator.batch) or "median" (extension, DESIGN.md 4.8:
                            # median-counter push-pull, one trial on one device; a batch of
                            # trials through Simulator.median_batch)
    rumor_k: int = 2        # rumor: a node stops calling after this many calls that reached an
                            # informed peer (1..255); median: the counter steps and the rounds of
                            # the final phase (1..127)
    rumor_blind: bool = False  # rumor: an event every round a node is hot, reply or not (GS_RUMOR_BLIND)
    rumor_coin: bool = False   # rumor: an event removes with probability 1/rumor_k (GS_RUMOR_COIN)
    rumor_pull: bool = False   # rumor: every live node calls; hot nodes answer (GS_RUMOR_PULL)
    trials: int = 1         # batched independent trials trial .. trial+trials-1 (config C3): flood and
                            # push-pull through Simulator(cfg), the rumor model too through
                            # Simulator.batch(cfg), every model through Simulator.median_batch(cfg)
    median_packed: bool = False  # Simulator.median_batch of model "median" with trials > 1: 16-bit
                                 # tallies (GS_FLAG_MEDIAN_PACKED), n up to median_trials_max_n(packed=True);
                                 # same results; a table in which some node is named by more than
                                 # 32,766 used slots is refused at broadcast_begin when n > 32,766
    pp_l2_only: bool = False  # push-pull: force the no-LDS summary path (tests)
    pp_rounds: str = "auto"   # push-pull: "auto" (sparse early rounds while |I| <= n/256, dense
                              # rounds bottom-up once |I| >= 96n/256), "dense" (every round streams the
                              # table top-down), "early" (sparse at any |I|), "topdown" (auto, but
                              # dense rounds never bottom-up nor pull-answer), "bottom" (every dense round
                              # bottom-up), "answer" (every dense round below the bottom-up threshold
                              # pull-answer)

    PP_ROUNDS = ("auto", "dense", "early", "topdown", "bottom", "answer")
    MODELS = {"flood": _lib.GS_MODEL_FLOOD, "pushpull": _lib.GS_MODEL_PUSHPULL, "rumor": _lib.GS_MODEL_RUMOR,
              "median": _lib.GS_MODEL_MEDIAN}

    def flags(self, timing: bool | None = None) -> int:
        if self.pp_rounds not in self.PP_ROUNDS:
            raise ValueError(f"pp_rounds must be one of {self.PP_ROUNDS}, not {self.pp_rounds!r}")
        t = self.timing if timing is None else timing
        return (_lib.GS_FLAG_TIMING if t else 0) | \
            (_lib.GS_FLAG_TICK_ENGINE if self.engine == "tick" else 0) | \
            (_lib.GS_FLAG_PP_L2_ONLY if self.pp_l2_only else 0) | \
            (_lib.GS_FLAG_PP_DENSE if self.pp_rounds == "dense" else 0) | \
            (_lib.GS_FLAG_PP_EARLY if self.pp_rounds == "early" else 0) | \
            (_lib.GS_FLAG_PP_TOPDOWN if self.pp_rounds == "topdown" else 0) | \
            (_lib.GS_FLAG_PP_BOTTOM if self.pp_rounds == "bottom" else 0) | \
            (_lib.GS_FLAG_PP_ANSWER if self.pp_rounds == "answer" else 0) | \
            (_lib.GS_FLAG_MEDIAN_PACKED if self.median_packed else 0)

    def to_params(self) -> Params:
        p = Params()
        p.n, p.fanout, p.fanin = self.n, self.fanout, self.fanin
        p.delay_low, p.delay_high = self.delaylow, self.delayhigh
        p.drop_rate, p.crash_rate = self.droprate, self.crashrate
        p.seed, p.trial, p.device = self.seed, self.trial, self.device
        if self.model not in self.MODELS:
            raise ValueError(f"model must be 'flood', 'pushpull', 'rumor' or 'median', not {self.model!r}")
        p.model = self.MODELS[self.model]
        if self.model == "rumor":
            if not 1 <= int(self.rumor_k) <= 255:
                raise ValueError(f"rumor_k must be in 1..255, not {self.rumor_k!r}")
            p.rumor_k = int(self.rumor_k)
            p.rumor_mode = (_lib.GS_RUMOR_BLIND if self.rumor_blind else 0) | \
                (_lib.GS_RUMOR_COIN if self.rumor_coin else 0) | \
                (_lib.GS_RUMOR_PULL if self.rumor_pull else 0)
        if self.model == "median":
            if not 1 <= int(self.rumor_k) <= 127:
                raise ValueError(f"rumor_k must be in 1..127 for model 'median', not {self.rumor_k!r}")
            p.rumor_k = int(self.rumor_k)
        p.flags = self.flags()
        p.trials = max(1, int(self.trials))
        return p


def _stats_array(buf, k: int) -> np.ndarray:
    return np.array([[getattr(buf[i], f) for f in STAT_FIELDS] for i in range(k)],
                    dtype=np.uint64).reshape(k, len(STAT_FIELDS))


class Simulator:
    """One broadcast (or one batch of trials) behind a gs_ctx.

    devices=None: one GPU (cfg.device), gs_create.  devices=[d0, d1, ...]:
    gs_create_multi -- a node-range-sharded broadcast over those devices
    (entries may repeat), or the trials split over them when cfg.trials > 1.
    Simulator.rank(...): one rank of a multi-process run (gs_create_rank).
    Simulator.batch(cfg): gs_create_trials -- as Simulator(cfg), and also a
    batch of rumor trials (model="rumor", trials > 1), which gs_create refuses.
    Simulator.median_batch(cfg): gs_create_batch -- as Simulator.batch(cfg), and
    also a batch of median trials (model="median", trials > 1), which both
    other creates refuse."""

    def __init__(self, cfg: Config, devices=None, _rank=None, _batch=False, _rumors=None):
        self.cfg = cfg
        self.L = _lib.load()
        self._p = cfg.to_params()
        self.rumors = 0 if _rumors is None else int(_rumors)
        h = C.c_void_p()
        if _rumors is not None:
            rc = self.L.gs_create_rumorset(C.byref(self._p), self.rumors, C.byref(h))
            what = "gs_create_rumorset"
        elif _rank is not None and len(_rank) == 5:  # host exchange: (nranks, rank, all_gather, all_reduce, all_to_allv)
            nranks, rank, ag, ar, av = _rank
            self._xfns = self._exchange_fns(nranks, ag, ar, av)  # kept alive with the context
            rc = self.L.gs_create_rank_exchange(C.byref(self._p), cfg.device, nranks, rank,
                                                C.byref(self._xfns[-1]), C.byref(h))
            what = "gs_create_rank_exchange"
        elif _rank is not None:
            nranks, rank, cid = _rank
            rc = self.L.gs_create_rank(C.byref(self._p), cfg.device, nranks, rank, cid, C.byref(h))
            what = "gs_create_rank"
        elif devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self.L.gs_create_multi(C.byref(self._p), devs, len(devices), C.byref(h))
            what = "gs_create_multi"
        elif _batch == "median":
            rc = self.L.gs_create_batch(C.byref(self._p), C.byref(h))
            what = "gs_create_batch"
        elif _batch:
            rc = self.L.gs_create_trials(C.byref(self._p), C.byref(h))
            what = "gs_create_trials"
        else:
            rc = self.L.gs_create(C.byref(self._p), C.byref(h))
            what = "gs_create"
        if rc != 0:
            why = self.L.gs_last_error(None).decode(errors="replace")  # no context: the create's own reason
            raise GossipError(rc, f"{what} failed: {self.L.gs_strerror(rc).decode()}" +
                              (f" ({why})" if why and why != "NULL context" else ""))
        self.h = h
        self.n = cfg.n
        self.trials = max(1, int(cfg.trials))
        self.words = (cfg.n + 63) // 64

    @classmethod
    def batch(cls, cfg: Config):
        """cfg.trials trials at once on cfg.device through gs_create_trials: what
        Simulator(cfg) makes, and for model="rumor" with trials > 1 a batched
        rumor context (n <= rumor_trials_max_n of its mode).  Every call takes
        the batched layouts: tables back to back, one mask per trial,
        [trials, ceil(n/64)] sets."""
        return cls(cfg, _batch=True)

    @classmethod
    def median_batch(cls, cfg: Config):
        """cfg.trials trials at once on cfg.device through gs_create_batch: what
        Simulator.batch(cfg) makes, and for model="median" with trials > 1 a
        batched median context.  n <= median_trials_max_n() (31,104 on an
        MI355X); with cfg.median_packed n <= median_trials_max_n(packed=True)
        (50,304 there, so the default n = 50,000 fits): the same results from
        16-bit tallies, which take every table of n <= 32,766 nodes and past
        that only tables in which no node is named by more than 32,766 used
        slots (broadcast_begin refuses the others and names the node; the
        overlay's own tables are far inside the bound).  Every call takes the
        batched layouts, and median_state() is [trials, n]."""
        return cls(cfg, _batch="median")

    @classmethod
    def rumor_set(cls, cfg: Config, rumors: int):
        """`rumors` (1..64) push-pull broadcasts over one table, one seed and one
        trial in one pass (gs_create_rumorset): cfg.model must be
        "pushpull", trials 1 and pp_rounds "auto".  begin_rumors(senders) or
        broadcast_begin(s) starts them; step / run / totals count the set
        (received = (node, rumor) pairs, pending = started rumors below 99 %),
        received() gives the nodes that hold every started rumor, and
        rumor_results(), rumor_words() and rumor_column(j) the rumors themselves."""
        return cls(cfg, _rumors=rumors)

    @classmethod
    def rank(cls, cfg: Config, nranks: int, rank: int, comm_id: bytes | None):
        """Rank `rank` of `nranks` processes (gs_create_rank); comm_id from
        comm_unique_id() on rank 0, shipped to every rank by the caller.  With
        cfg.trials > 1 the rank gets its share of the trials (no comm_id)."""
        sim = cls(cfg, _rank=(nranks, rank, comm_id))
        if cfg.trials > 1:  # this rank's trials
            t0 = cfg.trials * rank // nranks
            sim.trials = cfg.trials * (rank + 1) // nranks - t0
        return sim

    @classmethod
    def rank_exchange(cls, cfg: Config, nranks: int, rank: int, all_gather, all_reduce_sum, all_to_allv=None):
        """Rank `rank` of `nranks` processes with the exchange done by the caller
        (gs_create_rank_exchange): all_gather(send: np.uint8 array) -> np.uint8
        array of nranks * len(send) bytes, rank-major; all_reduce_sum(x:
        np.uint64 array) -> the element-wise sum over the ranks;
        all_to_allv(send: np.uint8 array, send_sizes, recv_sizes) -> np.uint8
        array of sum(recv_sizes) bytes (blocks back to back in rank order; a
        flood run needs it)."""
        return cls(cfg, _rank=(nranks, rank, all_gather, all_reduce_sum, all_to_allv))

    @staticmethod
    def _exchange_fns(nranks, all_gather, all_reduce_sum, all_to_allv):
        def ag(_user, send, recv, nbytes):
            try:
                src = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(send))
                out = np.asarray(all_gather(src.copy()), dtype=np.uint8).ravel()
                C.memmove(recv, out.ctypes.data, out.nbytes)
                return 0
            except Exception:  # noqa: BLE001 -- reported to the engine as a failed exchange
                import traceback
                traceback.print_exc()
                return 1

        def ar(_user, buf, count):
            try:
                x = np.ctypeslib.as_array(buf, shape=(count,))
                x[:] = np.asarray(all_reduce_sum(x.copy()), dtype=np.uint64)
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        def av(_user, send, send_bytes, recv, recv_bytes):
            try:
                sb = [int(send_bytes[i]) for i in range(nranks)]
                rb = [int(recv_bytes[i]) for i in range(nranks)]
                src = np.ctypeslib.as_array((C.c_uint8 * sum(sb)).from_address(send)) if sum(sb) else \
                    np.zeros(0, np.uint8)
                out = np.asarray(all_to_allv(src.copy(), sb, rb), dtype=np.uint8).ravel()
                if out.nbytes != sum(rb):
                    raise ValueError(f"all_to_allv returned {out.nbytes} bytes, expected {sum(rb)}")
                if out.nbytes:
                    C.memmove(recv, out.ctypes.data, out.nbytes)
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        f1, f2 = _lib.ALL_GATHER_FN(ag), _lib.ALL_REDUCE_FN(ar)
        f3 = _lib.ALL_TO_ALLV_FN(av) if all_to_allv is not None else _lib.ALL_TO_ALLV_FN()
        return f1, f2, f3, _lib.Exchange(None, f1, f2, f3)

    # -- plumbing --------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.L.gs_last_error(self.h).decode(errors="replace")
            raise GossipError(rc, f"{what}: {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.L.gs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- overlay (simulator.go:62-106, 127-164, 214-235) -------------------
    def load_peers(self, deg: np.ndarray, ids: np.ndarray):
        """deg [n], ids [n, stride]; batched trials: the trials' tables back to
        back (deg [trials*n], ids [trials*n, stride], ids local to the trial)."""
        deg = np.ascontiguousarray(deg, dtype=np.uint8)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        m = self.n * self.trials
        if deg.shape != (m,) or ids.ndim != 2 or ids.shape[0] != m:
            raise ValueError("deg must be [trials*n], ids [trials*n, stride]")
        self._check(self.L.gs_load_peers(self.h, deg.ctypes.data, ids.ctypes.data, ids.shape[1]),
                    "gs_load_peers")

    def load_peers_device(self, deg_ptr: int, ids_ptr: int, stride: int):
        self._check(self.L.gs_load_peers_device(self.h, deg_ptr, ids_ptr, stride),
                    "gs_load_peers_device")

    def build_overlay(self, max_ticks: int = 10_000_000, wcap: int = 1 << 16):
        win = (Window * wcap)()
        nwin = C.c_size_t(0)
        ft = C.c_uint64(0)
        self._check(self.L.gs_build_overlay(self.h, max_ticks, win, wcap, C.byref(nwin),
                                            C.byref(ft)), "gs_build_overlay")
        ws = [(win[i].tick, win[i].makeups, win[i].breakups)
              for i in range(min(nwin.value, wcap))]
        return ws, int(ft.value)

    def read_peers(self):
        stride = C.c_uint32(0)
        self._check(self.L.gs_read_peers(self.h, None, None, C.byref(stride)), "gs_read_peers")
        deg = np.zeros(self.n * self.trials, dtype=np.uint8)
        ids = np.zeros((self.n * self.trials, stride.value), dtype=np.uint32)
        self._check(self.L.gs_read_peers(self.h, deg.ctypes.data, ids.ctypes.data, C.byref(stride)),
                    "gs_read_peers")
        return deg, ids

    def set_failed(self, words: np.ndarray):
        """Pre-failed nodes (gs_set_failed), before broadcast_begin: ceil(n/64)
        words.  Batched trials: one mask per trial, [trials, ceil(n/64)] or the
        same flat, trial-major; a Simulator.rank context takes the masks of its
        own trials only ([self.trials, ceil(n/64)])."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if words.ndim == 2 and words.shape != (self.trials, self.words):
            raise ValueError(f"masks must be [{self.trials}, {self.words}] (or flat), not {list(words.shape)}")
        self._check(self.L.gs_set_failed(self.h, words.ctypes.data, words.size), "gs_set_failed")

    # -- broadcast (simulator.go:107-123, 140-149, 237-253) ----------------
    def broadcast_begin(self, sender: int = -1):
        self._check(self.L.gs_broadcast_begin(self.h, sender), "gs_broadcast_begin")

    def step(self, ticks: int = 1) -> np.ndarray:
        buf = (TickStats * ticks)()
        self._check(self.L.gs_step(self.h, ticks, buf), "gs_step")
        return _stats_array(buf, ticks)

    def run(self, poll: int = 10, max_ticks: int = 10_000_000, cap: int = 1 << 16):
        buf = (TickStats * cap)()
        nout = C.c_size_t(0)
        status = C.c_int32(0)
        self._check(self.L.gs_run(self.h, poll, max_ticks, buf, cap, C.byref(nout),
                                  C.byref(status)), "gs_run")
        return _stats_array(buf, min(nout.value, cap)), int(status.value)

    def totals(self) -> dict:
        t = TickStats()
        self._check(self.L.gs_totals(self.h, C.byref(t)), "gs_totals")
        return {f: int(getattr(t, f)) for f in STAT_FIELDS}

    def received(self) -> np.ndarray:
        """ceil(n/64) words (batched trials: [trials, ceil(n/64)])."""
        w = np.zeros(self.words * self.trials, dtype=np.uint64)
        self._check(self.L.gs_read_received(self.h, w.ctypes.data, w.size), "gs_read_received")
        return w if self.trials == 1 else w.reshape(self.trials, self.words)

    def crashed(self) -> np.ndarray:
        w = np.zeros(self.words * self.trials, dtype=np.uint64)
        self._check(self.L.gs_read_crashed(self.h, w.ctypes.data, w.size), "gs_read_crashed")
        return w if self.trials == 1 else w.reshape(self.trials, self.words)

    def removed(self) -> np.ndarray:
        """Rumor model: the removed nodes (informed, no longer calling), ceil(n/64)
        words (a batch of trials: [trials, ceil(n/64)]).  Median model: the done
        nodes (state D)."""
        w = np.zeros(self.words * self.trials, dtype=np.uint64)
        self._check(self.L.gs_read_removed(self.h, w.ctypes.data, w.size), "gs_read_removed")
        return w if self.trials == 1 else w.reshape(self.trials, self.words)

    def median_state(self) -> np.ndarray:
        """Median model: every node's state byte, [n] uint8 (a median_batch of
        trials: [trials, n]): 0 = uninformed, m in 1..rumor_k = informed with
        counter m, rumor_k + c = round c of the final phase, 255 = done
        (gs_read_median_state)."""
        st = np.zeros(self.n * self.trials, dtype=np.uint8)
        self._check(self.L.gs_read_median_state(self.h, st.ctypes.data, st.size), "gs_read_median_state")
        return st if self.trials == 1 else st.reshape(self.trials, self.n)

    def begin_rumors(self, senders, starts=None):
        """Rumor set: rumor j starts at senders[j] (len(senders) == rumors); a
        negative entry draws that rumor's keyed sender (gs_rumorset_begin).
        starts: rumor j enters after round starts[j]'s commit, 0 = at begin
        (gs_rumorset_begin_at); None: every rumor at begin."""
        s = (C.c_int64 * len(senders))(*[int(x) for x in senders])
        if starts is None:
            self._check(self.L.gs_rumorset_begin(self.h, s, len(senders)), "gs_rumorset_begin")
            return
        if len(starts) != len(senders):
            raise ValueError("starts must have one entry per sender")
        a = (C.c_int64 * len(starts))(*[int(x) for x in starts])
        self._check(self.L.gs_rumorset_begin_at(self.h, s, a, len(senders)), "gs_rumorset_begin_at")

    PICKS = {"low": _lib.GS_PICK_LOW, "high": _lib.GS_PICK_HIGH, "rotate": _lib.GS_PICK_ROTATE}

    def set_payload(self, B: int, pick="low"):
        """Rumor set: a message carries at most B rumors (1..64; 0 = no cap),
        chosen among the wanted ones by pick: "low" (lowest indices), "high" or
        "rotate" (upwards from a keyed offset), or a GS_PICK_* value.  Before a
        begin or after reset(); kept by reset() and set_trial()
        (gs_rumorset_set_payload)."""
        code = self.PICKS[pick] if isinstance(pick, str) else int(pick)
        self._check(self.L.gs_rumorset_set_payload(self.h, int(B), code), "gs_rumorset_set_payload")

    def rumor_traffic(self) -> dict:
        """Capped rumor set: the rumor copies wanted and carried and the
        messages the cap bound, cumulative over the broadcast
        (gs_rumorset_traffic_get; an error on an uncapped set)."""
        t = _lib.RumorTraffic()
        self._check(self.L.gs_rumorset_traffic_get(self.h, C.byref(t)), "gs_rumorset_traffic_get")
        return dict(wanted=int(t.wanted), carried=int(t.carried), bound=int(t.bound))

    def rumor_results(self) -> list:
        """Rumor set: per rumor a dict of sender, received (nodes that hold it),
        tick_99 (first poll at which its float32 rule held, else 0) and started
        (False: its sender was failed) (gs_rumorset_results)."""
        buf = (_lib.RumorStats * max(1, self.rumors))()
        k = C.c_size_t(0)
        self._check(self.L.gs_rumorset_results(self.h, buf, self.rumors, C.byref(k)), "gs_rumorset_results")
        return [dict(sender=int(buf[i].sender), received=int(buf[i].received), tick_99=int(buf[i].tick_99),
                     started=bool(buf[i].started)) for i in range(k.value)]

    def rumor_words(self) -> np.ndarray:
        """Rumor set: [n] uint64, bit j of word v says that v holds rumor j
        (gs_read_rumorset)."""
        w = np.zeros(self.n, dtype=np.uint64)
        self._check(self.L.gs_read_rumorset(self.h, w.ctypes.data, w.size), "gs_read_rumorset")
        return w

    def rumor_column(self, j: int) -> np.ndarray:
        """Rumor set: the nodes that hold rumor j, ceil(n/64) words
        (gs_read_rumor_column)."""
        w = np.zeros(self.words, dtype=np.uint64)
        self._check(self.L.gs_read_rumor_column(self.h, int(j), w.ctypes.data, w.size), "gs_read_rumor_column")
        return w

    def trial_results(self) -> np.ndarray:
        """[trials, len(TRIAL_FIELDS)] int64: per trial its number, first
        covered tick, stopping poll's tick and counters there, and status."""
        buf = (TrialStats * self.trials)()
        k = C.c_size_t(0)
        self._check(self.L.gs_trial_results(self.h, buf, self.trials, C.byref(k)), "gs_trial_results")
        return np.array([[int(getattr(buf[i], f)) for f in TRIAL_FIELDS] for i in range(k.value)],
                        dtype=np.int64).reshape(k.value, len(TRIAL_FIELDS))

    def shard_info(self):
        """[(lo, hi)] node range of every shard."""
        ns = C.c_uint32(0)
        lo, hi = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.gs_shard_info(self.h, 0, C.byref(ns), C.byref(lo), C.byref(hi)), "gs_shard_info")
        out = []
        for i in range(ns.value):
            self._check(self.L.gs_shard_info(self.h, i, None, C.byref(lo), C.byref(hi)), "gs_shard_info")
            out.append((int(lo.value), int(hi.value)))
        return out

    def set_flags(self, timing: bool):
        flags = self.cfg.flags(timing)
        self._check(self.L.gs_set_flags(self.h, flags), "gs_set_flags")

    def reset(self):
        self._check(self.L.gs_reset(self.h), "gs_reset")

    def set_trial(self, trial: int):
        """Renumber the trial(s) (then build_overlay again), keeping the buffers."""
        self._check(self.L.gs_set_trial(self.h, trial), "gs_set_trial")
        self.cfg.trial = trial

    def set_stream(self, hip_stream: int | None):
        self._check(self.L.gs_set_stream(self.h, hip_stream), "gs_set_stream")

    def timing(self) -> dict:
        t = Timing()
        self._check(self.L.gs_timing_get(self.h, C.byref(t)), "gs_timing_get")
        return {f: getattr(t, f) for f, _ in Timing._fields_}

    def shard_timing(self, index: int) -> dict:
        """Kernel timing of shard `index` (GS_FLAG_TIMING)."""
        t = Timing()
        self._check(self.L.gs_shard_timing(self.h, index, C.byref(t)), "gs_shard_timing")
        return {f: getattr(t, f) for f, _ in Timing._fields_}


def comm_unique_id() -> bytes:
    """RCCL unique id for gs_create_rank (rank 0 makes it, every rank uses it)."""
    L = _lib.load()
    b = C.create_string_buffer(_lib.GS_COMM_ID_BYTES)
    rc = L.gs_comm_unique_id(b)
    if rc != 0:
        raise GossipError(rc, "gs_comm_unique_id failed")
    return b.raw


def trim(device: int = -1) -> int:
    """Return the library's free cached device blocks to the driver (gs_trim);
    returns the bytes released."""
    L = _lib.load()
    out = C.c_size_t(0)
    rc = L.gs_trim(int(device), C.byref(out))
    if rc != 0:
        raise GossipError(rc, "gs_trim failed")
    return int(out.value)


def pp_trials_max_n(device: int = 0) -> int:
    """Largest n a batched push-pull context (model="pushpull", trials > 1) may
    have on `device` (gs_pp_trials_max_n): a trial's informed set lives in one
    workgroup's LDS."""
    L = _lib.load()
    out = C.c_uint64(0)
    rc = L.gs_pp_trials_max_n(int(device), C.byref(out))
    if rc != 0:
        why = L.gs_last_error(None).decode(errors="replace")
        raise GossipError(rc, "gs_pp_trials_max_n failed" + (f" ({why})" if why and why != "NULL context" else ""))
    return int(out.value)


def pp_trials_max_n_masked(device: int = 0) -> int:
    """Largest n a batched push-pull context may have on `device` when it is
    given failure masks (gs_pp_trials_max_n_masked): the trial's failed set is
    a third bitset in the workgroup's LDS."""
    L = _lib.load()
    out = C.c_uint64(0)
    rc = L.gs_pp_trials_max_n_masked(int(device), C.byref(out))
    if rc != 0:
        why = L.gs_last_error(None).decode(errors="replace")
        raise GossipError(rc, "gs_pp_trials_max_n_masked failed" + (f" ({why})" if why and why != "NULL context" else ""))
    return int(out.value)


def rumor_trials_max_n(mode=0, device: int = 0) -> int:
    """Largest n a batched rumor context (Simulator.batch, model="rumor",
    trials > 1) may have on `device` (gs_rumor_trials_max_n): the trial's sets
    and miss counts live in one workgroup's LDS, so the limit depends on the
    mode.  `mode`: the GS_RUMOR_* bits, or a Config (its rumor_blind,
    rumor_coin and rumor_pull flags)."""
    if isinstance(mode, Config):
        mode = mode.to_params().rumor_mode
    L = _lib.load()
    out = C.c_uint64(0)
    rc = L.gs_rumor_trials_max_n(int(device), int(mode), C.byref(out))
    if rc != 0:
        why = L.gs_last_error(None).decode(errors="replace")
        raise GossipError(rc, "gs_rumor_trials_max_n failed" + (f" ({why})" if why and why != "NULL context" else ""))
    return int(out.value)


def median_trials_max_n(device: int = 0, packed: bool = False) -> int:
    """Largest n a batched median context (Simulator.median_batch,
    model="median", trials > 1) may have on `device`
    (gs_median_trials_max_n): the trial's state bytes, tallies and flag sets
    live in one workgroup's LDS.  packed: with Config.median_packed
    (gs_median_trials_max_n_packed)."""
    L = _lib.load()
    out = C.c_uint64(0)
    name = "gs_median_trials_max_n_packed" if packed else "gs_median_trials_max_n"
    rc = getattr(L, name)(int(device), C.byref(out))
    if rc != 0:
        why = L.gs_last_error(None).decode(errors="replace")
        raise GossipError(rc, name + " failed" + (f" ({why})" if why and why != "NULL context" else ""))
    return int(out.value)


MEMORY_FIELDS = ("alloc_ms", "largest_alloc_ms", "free_ms", "alloc_calls", "alloc_cache_hits", "cached_bytes")


def memory_stats() -> dict:
    """The library's process-wide device-memory figures (gs_memory_stats)."""
    L = _lib.load()
    t = Timing()
    rc = L.gs_memory_stats(C.byref(t))
    if rc != 0:
        raise GossipError(rc, "gs_memory_stats failed")
    return {f: getattr(t, f) for f in MEMORY_FIELDS}


def covered(recv: int, n: int) -> bool:
    """simulator.go:246-248 in float32."""
    return bool(np.float32(recv) / np.float32(n) >= np.float32(0.99))
