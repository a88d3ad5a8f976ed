"""Flood parity sweep over row shapes, window lengths, rings and the packed view.

The window engine chooses its code from the table's row shape (the k_expand
instance, load_row's fetch branch, the packed view of GPU-built 5- and 6-slot
rows), from the delay range (window length L = min(delaylow, 10), ring length
delayhigh, tick engine past 256) and from the context (one trial, batched,
sharded).  Every case here is bit-exact against oracle.Engine / oracle.overlay:
every per-tick stats row, the received bitset after every step call and the
crashed bitset at the end.  The case lists are module data shared with one CPU
test that runs each case through the oracle alone and asserts it is worth
running (the flood spreads, nodes crash, dense ticks occur).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import BASE, masked, random_table, sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "flood_shapes_worker.py")
EMPTY = 0xFFFFFFFF
WIN_MAX_STRIDE, WIN_MAX_RING = 32, 256  # kWinMaxStride, kWinMaxRing: wider rows / longer rings -> tick engine


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def cfg_of(gs, kw, engine="window", **extra):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], engine=engine, **extra)


# ---- the cases ------------------------------------------------------------------
# A. injected row strides: (stride, engine asked for, engine that must run)
A_N = 3001
A_CASES = [(s, "window", "window") for s in range(2, WIN_MAX_STRIDE + 1)] + \
          [(s, "tick", "tick") for s in (5, 7, 13, 32)] + \
          [(s, "window", "tick") for s in (33, 64, 255)]


def a_kw(s):
    return dict(n=A_N, fanout=max(1, s - 1), fanin=s, delay_low=3, delay_high=8, drop_rate=0.1,
                crash_rate=0.02, seed=11, trial=0)


_TABLES = {}


def a_table(s):
    if s not in _TABLES:
        deg, ids = random_table(A_N, s, 1, s, seed=1000 + s)
        deg[::97] = 0
        _TABLES[s] = frozen(deg, ids)
    return _TABLES[s]


# B. window lengths and rings: (delay_low, delay_high)
B_N, B_STEP = 5000, 37
B_DELAYS = [(d, d + 1) for d in range(1, 17)] + [(2, 7), (4, 9), (6, 13), (9, 40), (12, 30)] + \
           [(16, 256), (200, 256), (200, 257), (250, 300)]
B_POLLS = [(dl, dh, poll) for dl, dh in ((10, 20), (4, 9)) for poll in (1, 3, 10)]


def b_kw(dl, dh):
    return dict(BASE, n=B_N, crash_rate=0.02, delay_low=dl, delay_high=dh)


def b_table():
    if "b" not in _TABLES:
        _TABLES["b"] = frozen(*random_table(B_N, 6, 5, 6, seed=77))
    return _TABLES["b"]


# C. GPU-built overlays: (fanout, fanin)
C_PAIRS = [(2, 3), (3, 4), (4, 5), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10), (9, 12), (10, 13), (12, 14), (14, 17),
           (15, 16), (18, 19), (18, 20), (20, 21), (20, 24), (25, 27), (28, 31), (30, 32), (33, 34), (40, 64)]


def c_kw(fo, fi):
    # (2, 3): the flood dies at once under drops, so that pair broadcasts without them
    return dict(n=3000, fanout=fo, fanin=fi, delay_low=10, delay_high=20, drop_rate=0.0 if (fo, fi) == (2, 3) else 0.1,
                crash_rate=0.01, seed=5, trial=1)


# D. the packed view (GPU-built rows of 5 or 6 slots, stride 8) at its edges
D_KW = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.02, seed=5, trial=1)
D_SMALL_N = [3, 5, 6, 7, 11, 64, 65, 777, 4099]
D_SMALL = [(n, fo, fi) for fo, fi in ((5, 6), (4, 5)) for n in D_SMALL_N]
D_HARD_N = [777, 4099]
D_VARIANTS = {  # name: (parameter overrides, failure mask?, sender, second sender after reset)
    "base": ({}, False, -1, None),
    "heavy-crash": (dict(drop_rate=0.29, crash_rate=0.57), False, -1, None),
    "delays-1-2": (dict(delay_low=1, delay_high=2), False, -1, None),
    "delays-0-3": (dict(delay_low=0, delay_high=3), False, -1, None),
    "mask-crash0": (dict(crash_rate=0.0), True, "live", None),
    "mask-crash3": (dict(crash_rate=0.03), True, "live", None),
    "sender": ({}, False, "n//3", None),
    "reset": ({}, False, -1, "n-1"),
}
D_HARD = [(n, v) for n in D_HARD_N for v in D_VARIANTS]
D_SHARDS = [(2, 20000), (3, 33000)]
D_BATCH_N, D_BATCH_T = 777, 3


def d_kw(n, fo=5, fi=6, **over):
    return dict(D_KW, n=n, fanout=fo, fanin=fi, **over)


def d_variant(n, name):
    over, mask, sender, second = D_VARIANTS[name]
    failed = failure_mask(n) if mask else None
    at = {"n//3": n // 3, "n-1": n - 1, -1: -1, None: None}
    if mask:  # a sender the mask leaves alive (the keyed sender of n = 4099 is a failed node)
        bits = np.unpackbits(failed.view(np.uint8), bitorder="little")[:n]
        at["live"] = int(np.flatnonzero(bits == 0)[n // 2])
    return d_kw(n, **over), failed, at[sender], at[second]


def failure_mask(n, rate=0.05, seed=2):
    bits = np.random.default_rng(seed).random(n) < rate
    b = np.packbits(bits, bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 8, np.uint8)]).view(np.uint64)


# ---- the oracle's side, computed once per input -----------------------------------
def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


_OVERLAYS = {}


def oracle_overlay(oracle, kw):
    """(deg, ids, windows, final tick) of the oracle's overlay; it depends on n,
    fanout, fanin, the delays, the seed and the trial only."""
    key = tuple(kw[k] for k in ("n", "fanout", "fanin", "delay_low", "delay_high", "seed", "trial"))
    if key not in _OVERLAYS:
        deg, ids, wins, final = oracle.overlay(oracle.make_params(**kw))
        frozen(deg, ids)
        _OVERLAYS[key] = (deg, ids, [tuple(w) for w in wins], final)
    return _OVERLAYS[key]


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def oracle_flood(oracle, kw, deg, ids, chunk, sender=-1, failed=None, cap=8000):
    """The oracle alone, stepped like the GPU tests step: (rows, received, crashed)."""
    e = oracle.Engine(oracle.make_params(**kw), deg, ids)
    if failed is not None:
        e.set_failed(failed)
    e.begin(sender)
    rows = []
    for _ in range(0, cap, chunk):
        rows.append(e.step(chunk))
        if int(rows[-1][-1][6]) == 0:
            break
    else:
        raise AssertionError(f"still pending after {cap} ticks")
    return np.concatenate(rows), popcount(e.received()), popcount(e.crashed())


# ---- E. non-vacuity, on the CPU ---------------------------------------------------
def test_cases_spread_in_the_oracle(oracle):
    """Every case above, through the oracle alone: a broadcast that dies at the
    sender, never crashes a node or never fills a tick proves nothing."""
    # A: the flood reaches a third of the nodes, nodes crash, and from 4 slots
    # on some tick carries more than 256 messages (the large resolve path runs
    # beside k_resolve_small)
    for s in sorted({s for s, _, _ in A_CASES}):
        deg, ids = a_table(s)
        assert ids.shape == (A_N, s) and int(deg.max()) == s and int(deg.min()) == 0
        rows, recv, crashed = oracle_flood(oracle, a_kw(s), deg, ids, 5)
        assert recv * 3 >= A_N, (s, recv)
        assert crashed > 0, s
        if s >= 4:
            assert int(rows[:, 3].max()) > 256, (s, int(rows[:, 3].max()))
    # B: near-full coverage with hundreds of crashes at every delay range; the
    # rings up to 256 slots stay on the window engine's side of the boundary
    deg, ids = b_table()
    for dl, dh in B_DELAYS:
        rows, recv, crashed = oracle_flood(oracle, b_kw(dl, dh), deg, ids, B_STEP)
        assert recv >= 0.95 * B_N and crashed >= 400, (dl, dh, recv, crashed)
        assert len(rows) > dh  # the ring wraps
    assert sorted(dh for _, dh in B_DELAYS if dh > 250) == [WIN_MAX_RING, WIN_MAX_RING, WIN_MAX_RING + 1, 300]
    for dl, dh, _ in B_POLLS:
        assert (dl, dh) in B_DELAYS or (dl, dh) == (10, 20)
    # C: the overlay keeps fanout <= degree <= fanin with both ends met, does not
    # depend on the drop rate, and its broadcast reaches 95 % of the nodes
    for fo, fi in C_PAIRS:
        assert fo < fi  # fanout = fanin needs about 6e5 overlay ticks in the oracle
        kw = c_kw(fo, fi)
        deg, ids, wins, final = oracle_overlay(oracle, kw)
        assert ids.shape == (kw["n"], fi)
        assert int(deg.min()) == fo and fo < int(deg.max()) <= fi, (fo, fi, deg.min(), deg.max())
        if fi <= WIN_MAX_STRIDE:  # some row uses its last slot
            assert int(deg.max()) == fi, (fo, fi, deg.max())
        assert len(wins) > 0 and final > 0
        rows, recv, _ = oracle_flood(oracle, kw, deg, ids, 10)
        assert recv >= 0.95 * kw["n"], (fo, fi, recv)
    d2, i2, w2, f2 = oracle.overlay(oracle.make_params(**dict(c_kw(2, 3), drop_rate=0.1)))
    deg, ids, wins, final = oracle_overlay(oracle, c_kw(2, 3))
    assert np.array_equal(d2, deg) and np.array_equal(i2, ids) and [tuple(w) for w in w2] == wins and f2 == final
    # D: degrees within [fanout, fanin] at every n, full rows from n = 64; the base
    # broadcasts of the larger sizes spread, the masks fail nodes, the second
    # sender of the reset case is another node
    for n, fo, fi in D_SMALL:
        deg, ids, _, _ = oracle_overlay(oracle, d_kw(n, fo, fi))
        assert fo <= int(deg.min()) and int(deg.max()) <= fi, (n, fo, fi, deg.min(), deg.max())
        if n >= 64:
            assert int(deg.max()) == fi, (n, fo, fi, deg.max())
        rows, recv, _ = oracle_flood(oracle, d_kw(n, fo, fi), deg, ids, 1)
        if n >= 64:
            assert recv >= 0.9 * n, (n, fo, fi, recv)
    for n, name in D_HARD:
        kw, failed, sender, second = d_variant(n, name)
        deg, ids, _, _ = oracle_overlay(oracle, kw)
        rows, recv, crashed = oracle_flood(oracle, kw, deg, ids, 1, sender, failed)
        if failed is not None:
            assert popcount(failed) >= n // 40 and crashed >= popcount(failed)
        if name == "heavy-crash":
            assert crashed >= 2  # the flood dies young, by crashes
        else:
            assert recv >= 0.8 * n, (n, name, recv)
        if second is not None:
            p = oracle.make_params(**kw)
            assert second != oracle.pick_sender(p)
            assert oracle_flood(oracle, kw, deg, ids, 3, second)[1] >= 0.8 * n
    for G, n in D_SHARDS:  # shards of 16384 nodes: the last one ragged
        assert (G - 1) * 16384 < n < G * 16384
        deg, ids, _, _ = oracle_overlay(oracle, d_kw(n))
        assert oracle_flood(oracle, d_kw(n), deg, ids, 10)[1] >= 0.95 * n
    for t in range(D_BATCH_T):
        kw = d_kw(D_BATCH_N, trial=D_KW["trial"] + t)
        deg, ids, _, _ = oracle_overlay(oracle, kw)
        assert oracle_flood(oracle, kw, deg, ids, 1)[1] >= 0.9 * D_BATCH_N


# ---- the GPU's side ---------------------------------------------------------------
def flood(sim, oracle, kw, deg, ids, chunk, sender=-1, failed=None, cap=8000):
    """One broadcast on sim against oracle.Engine on (deg, ids): every stats row
    and the received bitset per step call, the crashed bitset at the end.
    Returns the per-tick rows."""
    e = oracle.Engine(oracle.make_params(**kw), deg, ids)
    if failed is not None:
        e.set_failed(failed)
    e.begin(sender)
    sim.broadcast_begin(sender)
    rows = []
    for done in range(0, cap, chunk):
        a, b = e.step(chunk), sim.step(chunk)
        assert np.array_equal(a, b), f"stats differ in ticks {done + 1}..{done + chunk}:\n{a}\n{b}"
        assert np.array_equal(e.received(), sim.received()), f"received differs after tick {done + chunk}"
        rows.append(a)
        if int(a[-1][6]) == 0:
            break
    else:
        pytest.fail(f"still pending after {cap} ticks")
    assert np.array_equal(e.crashed(), sim.crashed()), "crashed differs"
    return np.concatenate(rows)


def engine_that_ran(sim, rows, sender=-1):
    """Which engine the context runs.  gs_timing's `windows` counts the window
    engine's windows, but only with GS_FLAG_TIMING (which also keeps the
    windows host-driven), so the broadcast is started again with the flag set:
    the first ticks must repeat `rows`, and then windows > 0 means the window
    engine, windows == 0 with timed per-tick launches the tick engine."""
    k = min(12, len(rows))
    sim.set_flags(True)
    sim.reset()
    sim.broadcast_begin(sender)
    assert np.array_equal(sim.step(k), rows[:k]), "the timed, host-driven run differs"
    tm = sim.timing()
    if tm["windows"] > 0:
        return "window"
    assert tm["deliver_launches"] >= k, tm  # the tick engine's timed launches: the flag was honoured
    return "tick"


def overlay_matches(sim, oracle, kw, sealed=True):
    """sim builds the oracle's overlay (windows, final tick, degrees, rows; a
    window context's rows sealed).  Returns the oracle's table."""
    deg, ids, wins, final = oracle_overlay(oracle, kw)
    gw, gf = sim.build_overlay()
    assert gf == final
    assert [tuple(w) for w in gw] == wins
    gdeg, gids = sim.read_peers()
    assert np.array_equal(gdeg, deg)
    assert gids.shape == ids.shape
    assert np.array_equal(masked(gdeg, gids), masked(deg, ids))
    if sealed:  # every slot past a node's degree holds the empty id
        pad = np.arange(gids.shape[1])[None, :] >= gdeg.astype(np.int64)[:, None]
        assert np.all(gids[pad] == EMPTY)
    return deg, ids


@pytest.mark.gpu
@pytest.mark.parametrize("s,engine,runs_on", A_CASES, ids=[f"s{s}-{e}" for s, e, _ in A_CASES])
def test_injected_strides(gs, oracle, s, engine, runs_on):
    """A. Every row stride the window engine takes (each k_expand instance and
    load_row branch), windows of 3 and 2 ticks; four strides on the tick engine;
    rows past 32 slots pick the tick engine on their own."""
    deg, ids = a_table(s)
    with gs.Simulator(cfg_of(gs, a_kw(s), engine)) as sim:
        sim.load_peers(deg, ids)
        rows = flood(sim, oracle, a_kw(s), deg, ids, 5)
        assert engine_that_ran(sim, rows) == runs_on


@pytest.mark.gpu
@pytest.mark.parametrize("dl,dh", B_DELAYS, ids=[f"d{a}-{b}" for a, b in B_DELAYS])
def test_window_lengths_and_rings(gs, oracle, dl, dh):
    """B. Window lengths 1..10 (and delaylow past 10), each cut again at the end
    of a 37-tick call; rings up to the window engine's 256, and the tick engine
    past it."""
    deg, ids = b_table()
    with gs.Simulator(cfg_of(gs, b_kw(dl, dh))) as sim:
        sim.load_peers(deg, ids)
        rows = flood(sim, oracle, b_kw(dl, dh), deg, ids, B_STEP)
        assert engine_that_ran(sim, rows) == ("window" if dh <= WIN_MAX_RING else "tick")


@pytest.mark.gpu
@pytest.mark.parametrize("dl,dh,poll", B_POLLS, ids=[f"d{a}-{b}-poll{p}" for a, b, p in B_POLLS])
def test_run_cuts_windows_at_polls(gs, oracle, dl, dh, poll):
    """B. gs_run: the device-driven windows cut at poll boundaries; every poll's
    row, the stop and the final bitsets equal the oracle polled the same way."""
    deg, ids = b_table()
    p = oracle.make_params(**b_kw(dl, dh))
    rows, e = oracle.run_to_coverage(p, deg, ids, poll=poll)
    g = rows.reshape(-1, poll, 7)
    want = g[:, -1, :].copy()
    want[:, 1:4] = g[:, :, 1:4].sum(axis=1)
    with gs.Simulator(cfg_of(gs, b_kw(dl, dh))) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(-1)
        polls, status = sim.run(poll=poll)
        assert status == (0 if oracle.covered(int(rows[-1][4]), B_N) else 1)  # GS_RUN_COVERED / _QUIESCENT
        assert np.array_equal(polls, want), f"\n{polls}\n{want}"
        assert np.array_equal(sim.received(), e.received())
        assert np.array_equal(sim.crashed(), e.crashed())


@pytest.mark.gpu
@pytest.mark.parametrize("fo,fi", C_PAIRS, ids=[f"{a}-{b}" for a, b in C_PAIRS])
def test_overlay_row_shapes(gs, oracle, fo, fi):
    """C. The overlay's row shapes (row8, the staged variants, rows padded to a
    multiple of 4) and the broadcast over the rows it left on the device."""
    kw = c_kw(fo, fi)
    runs_on = "window" if fi <= WIN_MAX_STRIDE else "tick"
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        deg, ids = overlay_matches(sim, oracle, kw, sealed=runs_on == "window")
        rows = flood(sim, oracle, kw, deg, ids, 10)
        assert engine_that_ran(sim, rows) == runs_on


@pytest.mark.gpu
@pytest.mark.parametrize("n,fo,fi", D_SMALL, ids=[f"n{n}-{a}-{b}" for n, a, b in D_SMALL])
def test_packed_view_small_n(gs, oracle, n, fo, fi):
    """D. The packed view where its last 128-B line is partly filled, lanes have
    no node and a wave holds one node: per tick, then again in 10-tick steps."""
    kw = d_kw(n, fo, fi)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        deg, ids = overlay_matches(sim, oracle, kw)
        flood(sim, oracle, kw, deg, ids, 1)
        sim.reset()
        flood(sim, oracle, kw, deg, ids, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("xpair", [None, "0"], ids=["lane-pairs", "per-lane"])
@pytest.mark.parametrize("n,name", D_HARD, ids=[f"n{n}-{v}" for n, v in D_HARD])
def test_packed_view_hard_parameters(gs, oracle, monkeypatch, n, name, xpair):
    """D. The packed view under a heavy crash rate, 1-tick windows, a failure
    mask, an explicit sender and a second broadcast after gs_reset; with the
    rows fetched by lane pairs (the default) and per lane (GS_XPAIR=0)."""
    if xpair is None:
        monkeypatch.delenv("GS_XPAIR", raising=False)
    else:
        monkeypatch.setenv("GS_XPAIR", xpair)
    kw, failed, sender, second = d_variant(n, name)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        deg, ids = overlay_matches(sim, oracle, kw)
        if failed is not None:
            sim.set_failed(failed)
        flood(sim, oracle, kw, deg, ids, 1, sender, failed)
        sim.reset()
        if second is None:
            flood(sim, oracle, kw, deg, ids, 10, sender, failed)
        else:
            flood(sim, oracle, kw, deg, ids, 3, second, failed)


@pytest.mark.gpu
def test_no_packed_view_in_a_fresh_process(oracle):
    """D. GS_NO_PACK (read once per process) makes k_expand read the padded table
    itself -- also what runs when the view cannot be allocated.  A child process
    sets it, builds the n = 4099 overlay and steps a broadcast."""
    kw = d_kw(4099)
    deg, ids, wins, final = oracle_overlay(oracle, kw)
    r = subprocess.run([sys.executable, WORKER, json.dumps(kw)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["no_pack"] == "1"
    assert got["final"] == final and [tuple(w) for w in got["windows"]] == wins
    assert got["deg_sha256"] == sha(deg) and got["rows_sha256"] == sha(masked(deg, ids))
    assert got["sealed"] is True
    assert [run["chunk"] for run in got["runs"]] == [1, 10]
    for run in got["runs"]:
        chunk = run["chunk"]
        e = oracle.Engine(oracle.make_params(**kw), deg, ids)
        e.begin(-1)
        assert len(run["rows"]) == len(run["received_sha256"]) > 0
        for i, (rows, rsha) in enumerate(zip(run["rows"], run["received_sha256"])):
            want = e.step(chunk)
            assert want.tolist() == rows, f"step({chunk}) call {i}:\n{want}\n{rows}"
            assert sha(e.received()) == rsha, f"step({chunk}) call {i}: received"
        assert int(want[-1][6]) == 0, "the child stopped while messages were pending"
        assert sha(e.crashed()) == run["crashed_sha256"]


@pytest.mark.gpu
def test_packed_view_batched(gs, oracle):
    """D. Three trials in one context over GPU-built rows: each trial's table is
    the oracle's for trial + t, every per-tick row is the sum of the three
    oracle engines' rows (the tick from the first), each trial's bitsets are its
    engine's."""
    n, T = D_BATCH_N, D_BATCH_T
    kws = [d_kw(n, trial=D_KW["trial"] + t) for t in range(T)]
    tabs = [oracle_overlay(oracle, kw) for kw in kws]
    es = [oracle.Engine(oracle.make_params(**kw), deg, ids) for kw, (deg, ids, _, _) in zip(kws, tabs)]
    with gs.Simulator(cfg_of(gs, kws[0], trials=T)) as sim:
        sim.build_overlay()
        gdeg, gids = sim.read_peers()
        for t, (deg, ids, _, _) in enumerate(tabs):
            assert np.array_equal(gdeg[t * n:(t + 1) * n], deg), f"trial {t}"
            assert np.array_equal(masked(gdeg, gids)[t * n:(t + 1) * n, :ids.shape[1]], masked(deg, ids)), f"trial {t}"
        for e in es:
            e.begin(-1)
        sim.broadcast_begin(-1)
        for tick in range(1, 2000):
            each = [e.step(1).astype(np.int64) for e in es]
            want = np.sum(each, axis=0)
            want[:, 0] = each[0][:, 0]
            got = sim.step(1).astype(np.int64)
            assert np.array_equal(got, want), f"tick {tick}:\n{got}\n{want}"
            assert np.array_equal(sim.received(), np.stack([e.received() for e in es])), f"tick {tick}"
            if int(want[-1][6]) == 0:
                break
        else:
            pytest.fail("still pending")
        assert np.array_equal(sim.crashed(), np.stack([e.crashed() for e in es]))


@pytest.mark.gpu
@pytest.mark.parametrize("G,n", D_SHARDS, ids=[f"G{g}-n{n}" for g, n in D_SHARDS])
def test_packed_view_sharded(gs, oracle, G, n):
    """D. Node-range shards over rows the shards built themselves (shards of
    16384 nodes, the last ragged), per tick against the oracle on its own
    overlay (a sharded context cannot hand its table back)."""
    kw = d_kw(n)
    deg, ids, wins, final = oracle_overlay(oracle, kw)
    with gs.Simulator(cfg_of(gs, kw), devices=[0] * G) as sim:
        info = sim.shard_info()
        assert [hi - lo for lo, hi in info] == [16384] * (G - 1) + [n - 16384 * (G - 1)]
        gw, gf = sim.build_overlay()
        assert gf == final and [tuple(w) for w in gw] == wins
        flood(sim, oracle, kw, deg, ids, 1)
