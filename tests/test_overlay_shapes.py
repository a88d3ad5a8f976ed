"""Overlay parity sweep: hub runs, id-space edges, build outcomes and switches.

The overlay builder (gs_overlay.hip) chooses its code by the shape of a tick:
a destination's run of events in k_process (staged in LDS, or replayed from
global memory when it leaves the staged keys), a workgroup's emitted events
(gathered in LDS, or appended one by one past kEmitCap), the destination
partition against the radix sort (the plan's capacity boundary), the id space
of batched trials, and a handful of environment switches.  Every case here is
bit-exact against oracle.overlay: the windows, the final tick, the degrees and
the rows masked by degree (a window context's rows sealed).  The case lists are
module data shared with one CPU test that runs each case through the oracle
alone and shows, from the oracle's degrees and the kernel's constants (mirrored
here and read out of gs_overlay.hip), that the case reaches the path it is
named for.
"""
from __future__ import annotations

import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_flood_shapes import EMPTY, cfg_of, engine_that_ran, flood, oracle_flood, oracle_overlay, overlay_matches
from test_gpu_parity import masked, sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "overlay_shapes_worker.py")
KERNEL = os.path.join(ROOT, "gossip_simulator_amd", "csrc", "gs_overlay.hip")

# gs_overlay.hip's constants, mirrored (test_cases_reach_their_paths reads them out of the source too)
PROC_TILE = 256 * 4     # kProcBlock * kProcIPT: key positions per k_process workgroup
PROC_LOOK = 64          # kProcLook: staged keys past the tile
EMIT_CAP = 1024         # kEmitCap: a workgroup's emitted events gathered in LDS
OVP_TILE = 512 * 16     # kOvpTile: keys per P1 / P2 tile
FINE_LOG = 14           # kOvFineLog
FINE_MAX = 1024 * 16    # kOvFineMax: ids, and keys, per fine region
PLAN_SCALE, PLAN_SIGMAS, PLAN_PAD = 1.04, 6.0, 32.0  # ov_plan: cap = ceil(scale e + sigmas sqrt(e) + pad)
PLAN_MIN = 32           # ov_plan: a tick is partitioned from m >= 32 * fine regions
ENV = ("GS_OV_SORT", "GS_OV_STAGED", "GS_OV_BLOCK", "GS_OV_PART_BATCHED", "GS_OV_PART_SCALE", "GS_OV_ROW8",
       "GS_OV_FILL_STRIDE", "GS_OV_PICK_COUNT", "GS_OV_PICK_SCALE")  # read per build


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


@pytest.fixture
def env(monkeypatch):
    """Sets the given switches and clears every other one the overlay reads per build."""
    def set_(**kv):
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
        for var, val in kv.items():
            assert var in ENV
            if val is not None:
                monkeypatch.setenv(var, str(val))
    set_()
    return set_


def kw_of(n, fanout, fanin, delay_low=10, delay_high=20, trial=1):
    return dict(n=n, fanout=fanout, fanin=fanin, delay_low=delay_low, delay_high=delay_high, drop_rate=0.1,
                crash_rate=0.01, seed=5, trial=trial)


# ---- the cases ------------------------------------------------------------------
# A. hub runs: (n, fanout, delay_low, delay_high); a delay span of 1 puts the whole
# burst (n * fanout makeups) into tick delay_low
HUBS = {"H1": (11, 100, 10, 11), "H2": (16, 110, 3, 4), "H3": (90, 100, 10, 11), "H4": (150, 100, 10, 11),
        "H5": (160, 100, 10, 11)}
HUB_FANINS = ("+1", "+20", "255")
HUB_FINAL_PLUS1 = {"H1": 850, "H2": 260, "H3": 380, "H4": 350, "H5": 340}
HUB_FINAL_PLUS20 = {"H1": 70, "H2": 30, "H3": 60, "H4": 60, "H5": 60}
HUB_PARTITIONED = ("H1", "H2", "H3", "H4")  # the burst tick's plan is accepted
A_CASES = [(h, f) for h in HUBS for f in HUB_FANINS]
A_STAGED = [(h, st, srt) for h in ("H1", "H3") for st in ("0", "1") for srt in (None, "1")]
A_BLOCKS = [("H1", "10", f) for f in HUB_FANINS] + [("H2", "2", f) for f in HUB_FANINS]


def hub_kw(name, fanin):
    n, fo, dl, dh = HUBS[name]
    return kw_of(n, fo, {"+1": fo + 1, "+20": fo + 20, "255": 255}[fanin], dl, dh)


# B. batched id space: (n, fanout, fanin, delay_low, delay_high, T, model); trial t of a context is
# the oracle's trial 1 + t.  A batched flood context runs on the window engine (rows of at most 32
# slots), so H1's 101-slot rows are built in a batched push-pull context: the overlay is the same
# code and the same keys under either model.
B_HUB = ("H1", "+1", 5)
B_CASES = [(777, 5, 6, 10, 20, 4, "flood"), (777, 5, 6, 10, 20, 5, "flood"), (16384, 5, 6, 10, 20, 3, "flood"),
           (16385, 5, 6, 10, 20, 3, "flood"), (11, 31, 32, 10, 11, 5, "flood"), (11, 100, 101, 10, 11, 5, "pushpull")]
B_GROUPINGS = ("sort", "partition")

# C. one trial, ragged fine buckets
C_N = [16383, 16384, 16385, 32769]
C_FINAL = {16383: 270, 16384: 290, 16385: 220, 32769: 250}

# D. outcomes
D_REJECT_N, D_REJECT_TRIALS = (1, 2), (0, 1, 2, 3)
D_TICKS_KW, D_TICKS_FINAL, D_TICKS_REFUSED = kw_of(3000, 5, 6), 220, (219, 211, 210, 209)
D_EQUAL_KW, D_EQUAL_FINAL = kw_of(100, 3, 3), 6960
D_WIDE_KW = kw_of(3000, 5, 255)

# E. switches: the (5, 6) row shape of the flood sweep, and H1 at fanout + 1
E_BASES = {"C56": kw_of(3000, 5, 6), "H1": hub_kw("H1", "+1")}
E_SWITCHES = [dict(GS_OV_ROW8="0"), dict(GS_OV_FILL_STRIDE="2"), dict(GS_OV_FILL_STRIDE="16")]
E_CASES = [(b, s) for b in E_BASES for s in E_SWITCHES] + \
          [("C56", dict(GS_OV_ROW8="0", GS_OV_STAGED=st)) for st in ("0", "1", "2")]

# F. GS_OV_STAGGER is read once per process
F_VALUES = ("0", "1")
F_BASES = ("C56", "H1")


def ceil_log2(n):
    return max(0, (n - 1).bit_length())


def tlog_of(n):
    return max(FINE_LOG, ceil_log2(n))


def node_bits(ntot):
    b = 1
    while b < 31 and (1 << b) < ntot:
        b += 1
    return b


def plan_cap(e):
    return math.ceil(PLAN_SCALE * e + PLAN_SIGMAS * math.sqrt(e) + PLAN_PAD)


def batched_overlay(oracle, kw, T):
    """The oracle's side of a batched build: the trials' tables, and the windows
    and final tick of overlay_build's one loop over the joint id space -- the
    window ending at a tick sums the trials' windows there (a trial already
    stable adds nothing), the loop ends with the last trial."""
    tabs = [oracle_overlay(oracle, dict(kw, trial=kw["trial"] + t)) for t in range(T)]
    final = max(f for _, _, _, f in tabs)
    wins = []
    for tick in range(10, final, 10):
        each = [dict((w[0], w[1:]) for w in ws).get(tick, (0, 0)) for _, _, ws, _ in tabs]
        wins.append((tick, sum(m for m, _ in each), sum(b for _, b in each)))
    return tabs, wins, final


# ---- non-vacuity, on the CPU ----------------------------------------------------
def source_constants():
    """The constants above, as gs_overlay.hip states them."""
    with open(KERNEL) as f:
        src = f.read()

    def num(pattern):
        m = re.search(pattern, src)
        assert m, f"gs_overlay.hip no longer states {pattern!r}"
        return [float(g) if "." in g else int(g) for g in m.groups()]

    pb, = num(r"constexpr uint32_t kProcBlock = (\d+);")
    pi, = num(r"constexpr uint32_t kProcIPT = (\d+);")
    ob, oi = num(r"constexpr uint32_t kOvpBlock = (\d+), kOvpIPT = (\d+), kOvpTile = kOvpBlock \* kOvpIPT;")
    fb, fi = num(r"constexpr uint32_t kOvFineBlock = (\d+), kOvFineIPT = (\d+);")
    assert re.search(r"constexpr uint32_t kOvFineMax = kOvFineBlock \* kOvFineIPT;", src)
    assert re.search(r"if \(cap > kOvFineMax\) return false;", src)
    sig, pad = num(r"e \* scale \+ ([\d.]+) \* std::sqrt\(e\) \+ ([\d.]+)")
    return dict(PROC_TILE=pb * pi, PROC_LOOK=num(r"constexpr uint32_t kProcLook = (\d+);")[0],
                EMIT_CAP=num(r"constexpr uint32_t kEmitCap = (\d+);")[0], OVP_TILE=ob * oi,
                FINE_LOG=num(r"constexpr uint32_t kOvFineLog = (\d+);")[0], FINE_MAX=fb * fi,
                PLAN_SCALE=num(r'getenv\("GS_OV_PART_SCALE"\)\) : ([\d.]+);')[0], PLAN_SIGMAS=sig, PLAN_PAD=pad,
                PLAN_MIN=num(r"m < (\d+) \* nfb\) return false;")[0])


def hub_layout(oracle, name, trials=1):
    """The burst tick of a hub size, from its fanin = 255 twin (picks and delay
    draws do not depend on fanin, and nothing is evicted there): node v's run is
    deg[v] - fanout makeups, the runs lie in node order -- in a batched id
    space trial after trial.  Returns (run lengths, runs that leave their tile's
    staged keys, the most events one tile's owned runs emit at fanin = fanout + 1)."""
    n, fo, _, _ = HUBS[name]
    each = []
    for t in range(trials):
        kw = hub_kw(name, "255")
        deg, _, wins, final = oracle_overlay(oracle, dict(kw, trial=kw["trial"] + t))
        assert final == 20 and all(b == 0 for _, _, b in wins), (name, t, final, wins)
        assert int(deg.max()) < 255
        each.append(deg.astype(np.int64) - fo)
        assert int(each[-1].min()) >= 0 and int(each[-1].sum()) == n * fo
    runs = np.concatenate(each)
    start = np.cumsum(runs) - runs
    heads = runs > 0
    tile = start // PROC_TILE
    leaves = heads & (start + runs > tile * PROC_TILE + PROC_TILE + PROC_LOOK)
    # fanin = fanout + 1: a run's first makeup fills the row, each further one evicts a friend
    emitted = np.bincount(tile[heads], weights=(runs[heads] - 1)).astype(np.int64)
    return runs, int(leaves.sum()), int(emitted.max())


def test_cases_reach_their_paths(oracle):
    """Every case above, through the oracle alone: that it ends as the sweep
    expects and that its shape reaches the path it is there for."""
    assert source_constants() == dict(PROC_TILE=PROC_TILE, PROC_LOOK=PROC_LOOK, EMIT_CAP=EMIT_CAP, OVP_TILE=OVP_TILE,
                                      FINE_LOG=FINE_LOG, FINE_MAX=FINE_MAX, PLAN_SCALE=PLAN_SCALE,
                                      PLAN_SIGMAS=PLAN_SIGMAS, PLAN_PAD=PLAN_PAD, PLAN_MIN=PLAN_MIN)
    assert FINE_MAX == 1 << FINE_LOG
    # A: hub runs
    for name, (n, fo, dl, dh) in HUBS.items():
        assert dh == dl + 1 and n < FINE_MAX
        m = n * fo
        assert m >= PLAN_MIN  # one fine region: the plan is tried
        runs, leaving, emitted = hub_layout(oracle, name)
        assert int(runs.max()) >= 100  # the ordinal k of a tick reaches the hundreds
        if name in HUB_PARTITIONED:
            assert leaving >= 1, name               # a GlobalRun
            assert emitted > EMIT_CAP, (name, emitted)  # the emit spill
            assert plan_cap(m) <= FINE_MAX, name
        deg, _, wins, final = oracle_overlay(oracle, hub_kw(name, "+1"))
        assert final == HUB_FINAL_PLUS1[name], (name, final)
        assert int(deg.min()) >= fo and int(deg.max()) == fo + 1
        assert sum(b for _, _, b in wins) > m  # evictions, found breakups and replacements
        deg, _, wins, final = oracle_overlay(oracle, hub_kw(name, "+20"))
        assert final == HUB_FINAL_PLUS20[name], (name, final)
        assert fo + 1 < int(deg.max()) <= fo + 20 and sum(b for _, _, b in wins) > 0
    assert [hub_layout(oracle, h)[1] for h in HUB_PARTITIONED] == [1, 1, 1, 3]
    assert [hub_layout(oracle, h)[2] for h in HUB_PARTITIONED] == [1089, 1093, 1081, 1078]
    for name in ("H3", "H4"):  # P1 has two tiles
        assert OVP_TILE < HUBS[name][0] * HUBS[name][1] <= 2 * OVP_TILE
    # the plan's refusal boundary lies between H4 and H5
    assert plan_cap(150 * 100) == 16367 and plan_cap(160 * 100) == 17431
    assert plan_cap(HUBS["H4"][0] * HUBS["H4"][1]) <= FINE_MAX < plan_cap(HUBS["H5"][0] * HUBS["H5"][1])
    for h, _, _ in A_STAGED:
        assert h in HUB_PARTITIONED
    for h, block, _ in A_BLOCKS:  # L = block: L | 10, L <= delay_low
        assert 10 % int(block) == 0 and 1 < int(block) <= HUBS[h][2]
    # the broadcast over H1's fanout + 20 rows spreads
    kw = hub_kw("H1", "+20")
    deg, ids, _, _ = oracle_overlay(oracle, kw)
    assert ids.shape[1] == 120
    assert oracle_flood(oracle, kw, deg, ids, 10)[1] >= 9
    # B: the id-space edges, and trials that end at different ticks (a stable
    # trial adds nothing to the later windows)
    assert [(tlog_of(n), node_bits(T << tlog_of(n))) for n, _, _, _, _, T, _ in B_CASES] == \
        [(14, 16), (14, 17), (14, 16), (15, 17), (14, 17), (14, 17)]
    assert 16385 - FINE_MAX == 1  # the trial's second fine bucket holds one valid id
    spread = 0
    for n, fo, fi, dl, dh, T, model in B_CASES:
        assert fi <= 32 or model == "pushpull"
        tabs, wins, final = batched_overlay(oracle, kw_of(n, fo, fi, dl, dh), T)
        assert len(wins) == final // 10 - 1 and all(f % 10 == 0 for _, _, _, f in tabs)
        assert any(tuple(w) != (w[0], 0, 0) for w in wins)
        spread += len({f for _, _, _, f in tabs}) > 1
        # dense ticks: the opt-in batched partition has something to group
        assert max(m + b for _, m, b in wins) >= 10 * PLAN_MIN * (T << tlog_of(n) >> FINE_LOG)
    assert spread >= 3
    # the batched hub case is H1 at fanout + 1: in the joint id space a run leaves
    # its tile's staged keys, a tile's runs spill, the ordinal passes 100
    name, fanin, T = B_HUB
    kw = hub_kw(name, fanin)
    assert B_CASES[-1] == (kw["n"], kw["fanout"], kw["fanin"], kw["delay_low"], kw["delay_high"], T, "pushpull")
    runs, leaving, emitted = hub_layout(oracle, name, T)
    assert len(runs) == T * kw["n"] and int(runs.max()) >= 100
    assert leaving >= 1 and emitted > EMIT_CAP, (leaving, emitted)
    # C: ragged fine buckets; dense windows
    assert [(n + FINE_MAX - 1) >> FINE_LOG for n in C_N] == [1, 1, 2, 3]
    for n in C_N:
        deg, _, wins, final = oracle_overlay(oracle, kw_of(n, 5, 6))
        assert final == C_FINAL[n], (n, final)
        assert int(deg.min()) == 5 and int(deg.max()) == 6
    # D: outcomes
    for n in D_REJECT_N:
        for trial in D_REJECT_TRIALS:
            with pytest.raises(oracle.OverlayError, match="-3"):
                oracle.overlay(oracle.make_params(**kw_of(n, 5, 6, trial=trial)))
    assert oracle_overlay(oracle, D_TICKS_KW)[3] == D_TICKS_FINAL
    assert max(D_TICKS_REFUSED) == D_TICKS_FINAL - 1 and {211, 210, 209} <= set(D_TICKS_REFUSED)
    for T in (1, 3):
        for t in range(T):
            deg, _, wins, final = oracle_overlay(oracle, kw_of(10, 0, 6, trial=1 + t))
            assert final == 10 and wins == [] and int(deg.sum()) == 0
    deg, _, wins, final = oracle_overlay(oracle, D_EQUAL_KW)
    assert final == D_EQUAL_FINAL and int(deg.min()) == int(deg.max()) == 3
    deg, ids, _, _ = oracle_overlay(oracle, D_WIDE_KW)
    assert ids.shape[1] == 255 and int(deg.min()) == 5 and 6 < int(deg.max()) < 255  # nothing is ever evicted
    assert oracle_flood(oracle, D_WIDE_KW, deg, ids, 10)[1] >= 0.95 * D_WIDE_KW["n"]


# ---- the GPU's side ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,fanin", A_CASES, ids=[f"{h}{f}" for h, f in A_CASES])
def test_hub_runs(gs, oracle, env, name, fanin):
    """A. A few nodes with a large fanout: runs of a hundred events and more
    (some replayed from global memory), a workgroup emitting past kEmitCap, the
    one-region partition up to its plan's capacity boundary."""
    kw = hub_kw(name, fanin)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        overlay_matches(sim, oracle, kw, sealed=False)
        tm = sim.timing()
    if name in HUB_PARTITIONED:
        assert tm["ov_part_ticks"] >= 1 and tm["ov_part_fallbacks"] == 0, tm
    else:  # H5's burst tick is past the plan: sorted
        assert tm["ov_sort_ticks"] >= 1 and tm["ov_part_fallbacks"] == 0, tm


@pytest.mark.gpu
@pytest.mark.parametrize("name,staged,sort", A_STAGED,
                         ids=[f"{h}-staged{st}-{'sort' if s else 'partition'}" for h, st, s in A_STAGED])
def test_hub_runs_staging(gs, oracle, env, name, staged, sort):
    """A. The hub runs with a thread's rows loaded together (GS_OV_STAGED=1) and
    with every key read from global memory (0), grouped by the partition and by
    the radix sort."""
    env(GS_OV_STAGED=staged, GS_OV_SORT=sort)
    kw = hub_kw(name, "+1")
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        overlay_matches(sim, oracle, kw, sealed=False)
        tm = sim.timing()
    if sort:
        assert tm["ov_part_ticks"] == 0 and tm["ov_sort_ticks"] >= 1, tm
    else:
        assert tm["ov_part_ticks"] >= 1, tm


@pytest.mark.gpu
@pytest.mark.parametrize("name,block,fanin", A_BLOCKS, ids=[f"{h}{f}-block{b}" for h, b, f in A_BLOCKS])
def test_hub_runs_tick_blocks(gs, oracle, env, name, block, fanin):
    """A. Blocks of several ticks: a hub's run spans the block's ticks and the
    ordinal restarts with each tag."""
    env(GS_OV_BLOCK=block)
    kw = hub_kw(name, fanin)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        overlay_matches(sim, oracle, kw, sealed=False)


@pytest.mark.gpu
def test_hub_rows_broadcast(gs, oracle, env):
    """A. One broadcast over the 120-slot rows the build left on the device: the
    context falls to the tick engine."""
    kw = hub_kw("H1", "+20")
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        deg, ids = overlay_matches(sim, oracle, kw, sealed=False)
        rows = flood(sim, oracle, kw, deg, ids, 10)
        assert engine_that_ran(sim, rows) == "tick"


@pytest.mark.gpu
@pytest.mark.parametrize("grouping", B_GROUPINGS)
@pytest.mark.parametrize("n,fo,fi,dl,dh,T,model", B_CASES, ids=[f"n{c[0]}-{c[1]}-{c[2]}-T{c[5]}" for c in B_CASES])
def test_batched_id_space(gs, oracle, env, n, fo, fi, dl, dh, T, model, grouping):
    """B. T trials in one id space (trial t at t << tlog): each trial's table is
    the oracle's for trial + t, the windows are the trials' windows summed tick
    by tick and the final tick is the last trial's; sorted (the default for
    batched builds) and partitioned with per-trial plans.  The last case is H1
    at fanout + 1: hub runs in five 11-id fine buckets (a push-pull context:
    batched flood contexts take rows of at most 32 slots)."""
    env(GS_OV_PART_BATCHED="1" if grouping == "partition" else None)
    kw = kw_of(n, fo, fi, dl, dh)
    tabs, wins, final = batched_overlay(oracle, kw, T)
    with gs.Simulator(cfg_of(gs, kw, trials=T, model=model)) as sim:
        gw, gf = sim.build_overlay()
        tm = sim.timing()
        gdeg, gids = sim.read_peers()
    assert gf == final
    assert [tuple(w) for w in gw] == wins
    assert gids.shape == (T * n, fi)
    for t, (deg, ids, _, _) in enumerate(tabs):
        d, r = gdeg[t * n:(t + 1) * n], gids[t * n:(t + 1) * n]
        assert np.array_equal(d, deg), f"trial {t}"
        assert np.array_equal(masked(d, r), masked(deg, ids)), f"trial {t}"
    if model == "flood":  # a window context's rows are sealed
        pad = np.arange(fi)[None, :] >= gdeg.astype(np.int64)[:, None]
        assert np.all(gids[pad] == EMPTY)
    if grouping == "partition":
        assert tm["ov_part_ticks"] >= 1, tm
    else:
        assert tm["ov_part_ticks"] == 0 and tm["ov_sort_ticks"] >= 1, tm


@pytest.mark.gpu
def test_batched_hub_rows_are_refused(gs):
    """B. H1's 101-slot rows in a batched flood context: those run on the
    window engine (rows of at most 32 slots), so the context is refused when it
    is created -- which is why the batched hub case above is a push-pull one."""
    from gossip_simulator_amd import _lib
    name, fanin, T = B_HUB
    with pytest.raises(_lib.GossipError) as e:
        gs.Simulator(cfg_of(gs, hub_kw(name, fanin), trials=T))
    assert e.value.code == _lib.GS_EINVAL and "window engine" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [None, "0.5"], ids=["partition", "fallback"])
@pytest.mark.parametrize("n", C_N)
def test_ragged_fine_buckets(gs, oracle, env, n, scale):
    """C. One trial whose last fine bucket holds all but one, all, or one of its
    16,384 ids; plans at half the expected counts overflow and fall back."""
    env(GS_OV_PART_SCALE=scale)
    kw = kw_of(n, 5, 6)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        overlay_matches(sim, oracle, kw)
        tm = sim.timing()
    if scale is None:
        assert tm["ov_part_ticks"] >= 1 and tm["ov_part_fallbacks"] == 0, tm
    else:
        assert tm["ov_part_fallbacks"] >= 1, tm


@pytest.mark.gpu
@pytest.mark.parametrize("n", D_REJECT_N)
def test_rejection_exhausted(gs, oracle, env, n):
    """D. n = 1, 2: no replacement friend exists (GS_EREJECT, the oracle's -3),
    and a context created afterwards builds as if nothing had happened."""
    from gossip_simulator_amd import _lib
    for trial in D_REJECT_TRIALS:
        with gs.Simulator(cfg_of(gs, kw_of(n, 5, 6, trial=trial))) as sim:
            with pytest.raises(_lib.GossipError) as e:
                sim.build_overlay()
            assert e.value.code == _lib.GS_EREJECT, str(e.value)
    kw = kw_of(3, 5, 6)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        overlay_matches(sim, oracle, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [None, "10"], ids=["block1", "block10"])
def test_max_ticks_boundary(gs, oracle, env, block):
    """D. The overlay stabilises at tick 220: max_ticks = 220 builds it, anything
    less is a livelock -- also where a 10-tick block straddles the limit -- and
    the same context then builds the oracle's overlay with the default limit."""
    from gossip_simulator_amd import _lib
    env(GS_OV_BLOCK=block)
    kw = D_TICKS_KW
    deg, ids, wins, final = oracle_overlay(oracle, kw)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        for limit in D_TICKS_REFUSED:
            with pytest.raises(_lib.GossipError) as e:
                sim.build_overlay(max_ticks=limit)
            assert e.value.code == _lib.GS_ELIVELOCK, (limit, str(e.value))
        gw, gf = sim.build_overlay(max_ticks=D_TICKS_FINAL)
        assert gf == final and [tuple(w) for w in gw] == wins
        gdeg, gids = sim.read_peers()
        assert np.array_equal(gdeg, deg) and np.array_equal(masked(gdeg, gids), masked(deg, ids))
        with pytest.raises(_lib.GossipError) as e:
            sim.build_overlay(max_ticks=D_TICKS_REFUSED[0])
        assert e.value.code == _lib.GS_ELIVELOCK
        overlay_matches(sim, oracle, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3])
def test_no_friends(gs, oracle, env, T):
    """D. fanout = 0: no picks, no events; final tick 10, no windows, every
    degree 0 and every slot empty."""
    kw = kw_of(10, 0, 6)
    if T == 1:
        with gs.Simulator(cfg_of(gs, kw)) as sim:
            deg, _ = overlay_matches(sim, oracle, kw)
        assert int(deg.sum()) == 0
        return
    with gs.Simulator(cfg_of(gs, kw, trials=T)) as sim:
        gw, gf = sim.build_overlay()
        gdeg, gids = sim.read_peers()
    assert gf == 10 and gw == []
    assert gdeg.shape == (T * 10,) and int(gdeg.sum()) == 0
    assert gids.shape == (T * 10, 6) and np.all(gids == EMPTY)


@pytest.mark.gpu
def test_fanout_equals_fanin(gs, oracle, env):
    """D. fanout = fanin: a found breakup never removes, every one replaces
    (6960 overlay ticks of a few events each)."""
    with gs.Simulator(cfg_of(gs, D_EQUAL_KW)) as sim:
        overlay_matches(sim, oracle, D_EQUAL_KW)


@pytest.mark.gpu
def test_wide_rows_with_headroom(gs, oracle, env):
    """D. fanin = 255 over fanout 5: 255-slot rows, the u8 degree far from its
    end, and a broadcast over them on the tick engine."""
    with gs.Simulator(cfg_of(gs, D_WIDE_KW)) as sim:
        deg, ids = overlay_matches(sim, oracle, D_WIDE_KW, sealed=False)
        rows = flood(sim, oracle, D_WIDE_KW, deg, ids, 10)
        assert engine_that_ran(sim, rows) == "tick"


@pytest.mark.gpu
@pytest.mark.parametrize("base,switches", E_CASES,
                         ids=[f"{b}-" + "-".join(f"{k[6:].lower()}{v}" for k, v in s.items()) for b, s in E_CASES])
def test_switches(gs, oracle, env, base, switches):
    """E. Rows of 8 slots replayed in memory (GS_OV_ROW8=0; with each staging of
    k_process), and the per-bucket counters 2 and 16 words apart (copied with
    strided 2-D copies)."""
    env(**switches)
    kw = E_BASES[base]
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        overlay_matches(sim, oracle, kw, sealed=kw["fanin"] <= 32)


@pytest.mark.gpu
@pytest.mark.parametrize("value", F_VALUES)
def test_stagger_in_a_fresh_process(oracle, value):
    """F. GS_OV_STAGGER (read once per process): a child process per value
    builds the (5, 6) overlay and H1's and prints their hashes."""
    kws = [E_BASES[b] for b in F_BASES]
    child_env = {k: v for k, v in os.environ.items() if k not in ENV}
    child_env["GS_OV_STAGGER"] = value
    r = subprocess.run([sys.executable, WORKER, json.dumps(kws)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=180, env=child_env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["stagger"] == value and len(got["overlays"]) == len(kws)
    for kw, o in zip(kws, got["overlays"]):
        deg, ids, wins, final = oracle_overlay(oracle, kw)
        assert o["final"] == final and [tuple(w) for w in o["windows"]] == wins
        assert o["shape"] == list(ids.shape)
        assert o["deg_sha256"] == sha(deg) and o["rows_sha256"] == sha(masked(deg, ids))
        assert o["sealed"] is (True if kw["fanin"] <= 32 else None)
