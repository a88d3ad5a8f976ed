"""The later loop passes of the flood's persistent kernels, against the oracle.

k_expand loops over rounds, k_part2 over tiles, k_resolve over buckets, and each
carries state from one pass to the next (prefetched words, LDS counters that are
reset per pass, 16-bit per-tick sums).  The default grids are sized for 256 CUs,
so at test sizes every workgroup runs its loop body at most once.  Three knobs,
read once per process, shrink the grids:
  GS_RESOLVE_GRID  workgroups of k_resolve / k_resolve2 (and _m, per shard)
  GS_PART2_GRID    workgroups of every k_part2 launch, the exact redo's included
  GS_XGRID         k_expand's grid cap, in 256-thread workgroups, every row width
Each knob setting runs in one child process (this file, run as a script) that
runs all of its cases in sequence and prints one JSON line; children run one
after another.

Every case is one broadcast over an injected table, bit for bit against
oracle.Engine through test_flood_shapes.flood (every stats row, the received
bitset per step call, the crashed bitset), stepped one window per call:
device-driven first, then host-driven and timed, where gs_timing counts the
windows (one per call, so a call's figures are one window's).

test_cases_reach_pass_two runs every case through the oracle alone and asserts
that some workgroup runs its loop at least twice under each setting
(reaches_pass_two; figures from the oracle only).  What the oracle gives:
  chain          n = 81957, 10-slot rows, crash 0.02, 5 % failed: the window of
                 ticks 71..80 informs 6,242..6,392 nodes in each of the five
                 full buckets (12 in the ragged one, which a skipped bucket
                 leaves to k_resolve_small); 34,513 nodes fire in the next one.
                 With 13-slot rows the densest window exceeds the window cut
                 (65,536 friend slots per bucket) and a call is two windows
  chain-flood    the same without crashes: no bucket goes to the large path
  dead-flush     every friend below 16384, delays 10..11 (a hop fires in one
                 tick), 32-slot rows, 75 % of bucket 0 failed: 78,112 receipts
                 in the window of ticks 41..50, three quarters of them uncounted
  large-between  three buckets, 90 % of the targets in the middle one, crash
                 0.5: the window of ticks 71..80 lists 829 and 746 receipts in
                 buckets 0 and 2 and crashes 4,883 nodes of bucket 1
  rows6 .. 32    28,351 / 34,824 / 14,860 / 7,576 nodes fire in one window
                 (k_expand's grid takes 8,192 / 8,192 / 2,048 / 2,048 per pass
                 with GS_XGRID=8, twice that with 16); batch3 20,047, overlay6
                 over 16,384
  dense3, skewed 185,743 and 409,824 delivered sends in one window: 12 and 26
                 tiles of 16,384
A 90 % failure mask cannot meet dead-flush's receipt bound: only live nodes of
bucket 0 ever fire, 1,638 of them with at most 32 slots each send 52,416
messages in the whole broadcast.  The bound stands and the mask is 75 %: a
lane's 6-bit field takes up to 45 of its 63 between two flushes, and more than
63 in the window if the flush in the loop is left out.  k_resolve2 flushes its
8-bit fields every 31 batches of 4,096 receipts; no bucket of 16,384 nodes with
rows of 32 slots reaches 255 uncounted receipts per lane, so that flush is not
covered here.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINE, SMALL_MAX, ROLLED_CAP, TILE = 16384, 256, 1024, 16384  # kFineNodes, kSmallMax, kRolledCap, kPartTile
SLOT_BUDGET = 1 << 16  # kWinSlotsPerBucket: a window of more friend slots per bucket is cut short
N6, N3 = 5 * FINE + 37, 2 * FINE + 37  # six / three fine buckets, the last one ragged

DENSE = dict(fanout=12, fanin=13, delay_low=10, delay_high=20, drop_rate=0.0, seed=11, trial=0)
KNOBS = ("GS_RESOLVE_GRID", "GS_RESOLVE_OCC3", "GS_RESOLVE_PER_CU", "GS_PART2_GRID", "GS_PART2_NOXCD", "GS_XGRID")


def rows_kw(s, n, **over):
    """Parameters for rows of s slots (fanout s - 1, fanin s)."""
    return dict(dict(DENSE, n=n, fanout=s - 1, fanin=s, crash_rate=0.0), **over)


# name: parameters, table (kind, stride, ...), failure mask (None, ("all", rate), ("bucket0", rate)), shards
# (0: one context), kind (flood: one trial; batch: T trials in one context; overlay: rows built on the GPU)
CASES = {
    "chain": dict(kw=rows_kw(10, N6, crash_rate=0.02), table=("random", 10, 9, 10), mask=("all", 0.05)),
    "chain-flood": dict(kw=rows_kw(10, N6), table=("random", 10, 9, 10), mask=("all", 0.05)),
    "dead-flush": dict(kw=rows_kw(32, N6, delay_high=11), table=("hot0", 32), mask=("bucket0", 0.75)),
    "large-between": dict(kw=dict(DENSE, n=3 * FINE - 11, crash_rate=0.5), table=("mix3", 13, 0.9)),
    # k_expand's four instances (rows <= 6, <= 8, <= 20, <= 32 slots)
    "rows6": dict(kw=rows_kw(6, N6), table=("random", 6, 5, 6)),
    "rows8": dict(kw=rows_kw(8, N6), table=("random", 8, 7, 8)),
    "rows13": dict(kw=rows_kw(13, N3), table=("random", 13, 12, 13)),
    "rows32": dict(kw=rows_kw(32, N6, delay_high=120), table=("random", 32, 31, 32)),
    "batch3": dict(kw=rows_kw(6, 20000), table=("random", 6, 5, 6), kind="batch", trials=3),
    "overlay6": dict(kw=dict(n=N6, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.0, crash_rate=0.01,
                             seed=5, trial=1), kind="overlay"),
    # k_part2: the dense table, and every target in bucket 0 (the estimates overflow: exact redo)
    "dense3": dict(kw=dict(DENSE, n=N3, crash_rate=0.0), table=("random", 13, 12, 13)),
    "skewed": dict(kw=rows_kw(32, N3, delay_low=1, delay_high=2, crash_rate=0.02), table=("hot0", 32), chunk=1,
                   sender=10, redo=True),
    "chain-shards": dict(kw=rows_kw(10, N6, crash_rate=0.02), table=("random", 10, 9, 10), mask=("all", 0.05),
                         shards=2),
    "skewed-shards": dict(kw=rows_kw(32, N3, delay_low=1, delay_high=2, crash_rate=0.02), table=("hot0", 32), chunk=1,
                          sender=10, redo=True, shards=2),
}
RESOLVE_CASES = ["chain", "chain-flood", "dead-flush"]
EXPAND_CASES = ["rows6", "rows8", "rows13", "rows32", "batch3", "overlay6"]
# setting: (environment, cases)
SETTINGS = {}
for _g in (1, 2, 4):
    for _occ, _tag in ((None, "occ3"), ("0", "occ2")):
        _env = {"GS_RESOLVE_GRID": str(_g)}
        if _occ is not None:
            _env["GS_RESOLVE_OCC3"] = _occ
        SETTINGS[f"resolve{_g}-{_tag}"] = (_env, RESOLVE_CASES + (["large-between"] if _g == 1 else []))
SETTINGS["xgrid8"] = ({"GS_XGRID": "8"}, EXPAND_CASES)
SETTINGS["xgrid16"] = ({"GS_XGRID": "16"}, EXPAND_CASES)
SETTINGS["part8"] = ({"GS_PART2_GRID": "8"}, ["dense3", "skewed"])
SETTINGS["part3"] = ({"GS_PART2_GRID": "3"}, ["dense3", "skewed"])
SETTINGS["part8-noxcd"] = ({"GS_PART2_GRID": "8", "GS_PART2_NOXCD": "1"}, ["dense3", "skewed"])
SETTINGS["all-min"] = ({"GS_RESOLVE_GRID": "1", "GS_PART2_GRID": "1", "GS_XGRID": "8"},
                       ["chain", "chain-shards", "skewed-shards"])


# ---- inputs -----------------------------------------------------------------------
_MEMO = {}


def table(name):
    if ("table", name) not in _MEMO:
        from test_flood_shapes import frozen
        from test_gpu_parity import random_table
        c = CASES[name]
        n, t = c["kw"]["n"], c["table"]
        T = c.get("trials", 1)
        if t[0] == "random":
            tabs = [random_table(n, t[1], t[2], t[3], seed=1 + i) for i in range(T)]
            deg, ids = np.concatenate([d for d, _ in tabs]), np.concatenate([i for _, i in tabs])
        elif t[0] == "hot0":  # every friend in fine bucket 0, full rows
            rng = np.random.default_rng(7)
            deg = np.full(n, t[1], np.uint8)
            ids = rng.integers(0, FINE, size=(n, t[1])).astype(np.uint32)
        else:  # mix3: three buckets, a share t[2] of the targets in the middle one
            rng = np.random.default_rng(7)
            deg = rng.integers(t[1] - 1, t[1] + 1, size=n).astype(np.uint8)
            b = rng.choice(3, size=(n, t[1]), p=[(1 - t[2]) / 2, t[2], (1 - t[2]) / 2])
            lo = b * FINE
            hi = np.minimum(lo + FINE, n)
            ids = (lo + rng.integers(0, FINE, size=(n, t[1])) % (hi - lo)).astype(np.uint32)
        _MEMO["table", name] = frozen(deg, ids)
    return _MEMO["table", name]


def mask_and_sender(name):
    """(failed words or None, sender): a masked case starts at a live node of bucket 0."""
    c = CASES[name]
    n, m = c["kw"]["n"], c.get("mask")
    if m is None:
        return None, c.get("sender", -1)
    rng = np.random.default_rng(2)
    bits = np.zeros(n, bool)
    span = n if m[0] == "all" else FINE
    bits[:span] = rng.random(span) < m[1]
    b = np.packbits(bits, bitorder="little")
    words = np.concatenate([b, np.zeros((-len(b)) % 8, np.uint8)]).view(np.uint64)
    return words, int(np.flatnonzero(~bits)[100])


def per_bucket(words, n):
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n]
    return np.add.reduceat(bits.astype(np.int64), np.arange(0, n, FINE))


def oracle_trace(oracle, name):
    """The oracle alone, one step call per window.  Per call: fired and delivered
    sends (the stats rows' columns, summed over the call's ticks), nodes informed
    and crashed per fine bucket, receipts per fine bucket (drop rate 0: every slot
    of every node scheduled for the call's ticks is a receipt at its target)."""
    if ("trace", name) in _MEMO:
        return _MEMO["trace", name]
    from test_flood_shapes import oracle_overlay
    c = CASES[name]
    kw, chunk, T = c["kw"], c.get("chunk", 10), c.get("trials", 1)
    n = kw["n"]
    assert kw["drop_rate"] == 0.0
    if c.get("kind") == "overlay":
        deg, ids = oracle_overlay(oracle, kw)[:2]
    else:
        deg, ids = table(name)
    failed, sender = mask_and_sender(name)
    out = dict(fired=[], sent=[], inf=[], crash=[], rcpt=[])
    live = []
    for t in range(T):
        e = oracle.Engine(oracle.make_params(**dict(kw, trial=kw["trial"] + t)), deg[t * n:(t + 1) * n],
                          ids[t * n:(t + 1) * n])
        if failed is not None:
            e.set_failed(failed)
        e.begin(sender)
        live.append((e, deg[t * n:(t + 1) * n].astype(np.int64), ids[t * n:(t + 1) * n]))
    call = 0
    while live:
        tot = dict(fired=0, sent=0, inf=0, crash=0, rcpt=0)
        for e, d, i in list(live):
            r0, c0 = per_bucket(e.received(), n), per_bucket(e.crashed(), n)
            rcpt = np.zeros(len(r0), np.int64)
            for tick in range(call * chunk + 1, (call + 1) * chunk + 1):
                v = np.flatnonzero(np.unpackbits(e.get_slot(tick).view(np.uint8), bitorder="little")[:n])
                tg = i[v][np.arange(i.shape[1])[None, :] < d[v][:, None]]
                rcpt += np.bincount(tg >> 14, minlength=len(r0))
            rows = e.step(chunk)
            assert int(rows[:, 2].sum()) == int(rcpt.sum()), (name, call)  # the tick model: a kept send is a receipt
            tot["fired"] += int(rows[:, 1].sum())
            tot["sent"] += int(rows[:, 2].sum())
            tot["inf"] = tot["inf"] + per_bucket(e.received(), n) - r0
            tot["crash"] = tot["crash"] + per_bucket(e.crashed(), n) - c0
            tot["rcpt"] = tot["rcpt"] + rcpt
            if int(rows[-1][6]) == 0:
                live.remove((e, d, i))
        for k in out:
            out[k].append(tot[k])
        call += 1
        assert call < 800, name
    _MEMO["trace", name] = out
    return out


# ---- what "pass two" needs, per kernel ----------------------------------------------
def expand_grid(xgrid, slots):
    """(workgroups, firing nodes per round) of win_expand_geometry under GS_XGRID."""
    if slots <= 6:
        return xgrid * 256 // 512, 512 * 4
    if slots <= 8:
        return xgrid, 256 * 4
    return xgrid, 256


def reaches_pass_two(setting, name, tr):
    """Asserts from the oracle's trace that some workgroup of each knobbed kernel
    loops at least twice in the case's densest window; returns the figures."""
    env, c = SETTINGS[setting][0], CASES[name]
    n, G = c["kw"]["n"], c.get("shards", 0)
    nf = (n + FINE - 1) // FINE
    per_shard = (nf + G - 1) // G if G else nf  # fine buckets per shard (ranges are whole buckets)
    fig = {}
    if "GS_RESOLVE_GRID" in env and name != "dead-flush" and not name.startswith("skewed"):
        g = int(env["GS_RESOLVE_GRID"])
        owner = lambda f: (f // per_shard, (f % per_shard) % g)  # noqa: E731
        if name == "large-between":
            # buckets 0 and 2 are listed (> kSmallMax receipts) and stay on the bit path (<= kRolledCap
            # receipts in all), bucket 1 between them lists more than kRolledCap rolled receipts (a
            # node crashes by a rolled receipt at a node live when the window starts)
            assert g == 1
            ok = [w for w, (r, cr) in enumerate(zip(tr["rcpt"], tr["crash"]))
                  if SMALL_MAX < r[0] <= ROLLED_CAP and SMALL_MAX < r[2] <= ROLLED_CAP and cr[1] > ROLLED_CAP]
            assert ok, (name, [list(r) for r in tr["rcpt"]], [list(x) for x in tr["crash"]])
            fig["resolve"] = dict(window=ok[0], receipts=[int(x) for x in tr["rcpt"][ok[0]]],
                                  crashed_bucket1=int(tr["crash"][ok[0]][1]))
        else:
            best = None
            for w, inf in enumerate(tr["inf"]):
                dense = [f for f in range(nf) if inf[f] > SMALL_MAX]
                owned = {}
                for f in dense:
                    owned.setdefault(owner(f), []).append(f)
                most = max((len(v) for v in owned.values()), default=0)
                if best is None or (most, int(inf.sum())) > best[:2]:
                    best = (most, int(inf.sum()), w, [int(x) for x in inf])
            assert best[0] >= 2, (setting, name, best)
            fig["resolve"] = dict(window=best[2], buckets_of_one_workgroup=best[0], informed=best[3])
    if name == "dead-flush":
        # every friend lies in bucket 0: the delivered sends of a window are that bucket's receipts
        assert all(int(r[1:].sum()) == 0 for r in tr["rcpt"])
        fig["dead_flush_receipts"] = max(tr["sent"])
        assert fig["dead_flush_receipts"] > 2 * 15 * 2048, fig
    if "GS_XGRID" in env and not G:
        blocks, per_round = expand_grid(int(env["GS_XGRID"]), c["kw"]["fanin"])
        fig["expand"] = dict(fired=max(tr["fired"]), bound=blocks * per_round)
        assert fig["expand"]["fired"] > fig["expand"]["bound"], (setting, name, fig)
    if "GS_PART2_GRID" in env:
        g = int(env["GS_PART2_GRID"])
        by_xcd = g % 8 == 0 and "GS_PART2_NOXCD" not in env and not G
        # tiles dealt by XCD: the one coarse bin's tiles all go to XCD 0's g / 8 workgroups; else the
        # grid strides the list, a shard's its own (some shard gets 1 / G of the window's messages)
        bound = TILE * g // 8 if by_xcd else TILE * g * max(G, 1)
        fig["part2"] = dict(sent=max(tr["sent"]), bound=bound)
        assert fig["part2"]["sent"] > bound, (setting, name, fig)
    if not G and c.get("chunk", 10) > 1:  # no window is cut short: one window per step call
        slots = c["table"][1] if "table" in c else c["kw"]["fanin"]
        slots = 8 if c.get("kind") == "overlay" else slots  # GPU-built rows of <= 8 slots: stride 8
        nfine = nf if c.get("kind") != "batch" else c["trials"] * (1 << 15) // FINE
        assert max(tr["fired"]) * slots <= nfine * SLOT_BUDGET, (name, max(tr["fired"]))
    assert fig, (setting, name)
    return fig


def test_cases_reach_pass_two(oracle):
    """The oracle alone: under every setting, every case makes some workgroup of
    the knobbed kernels run its loop at least twice (the module docstring)."""
    for setting, (_, names) in SETTINGS.items():
        for name in names:
            reaches_pass_two(setting, name, oracle_trace(oracle, name))
    # the window that fills a lane's 6-bit fields: one tick carries all of it
    tr = oracle_trace(oracle, "dead-flush")
    assert max(tr["sent"]) * 0.75 / 512 > 63  # without the mid-loop flush a field would overflow


# ---- the GPU's side -----------------------------------------------------------------
def timed_again(sim, rows, chunk, sender, step):
    """The same broadcast host-driven and timed: the same rows, one window per call."""
    sim.set_flags(True)
    sim.reset()
    sim.broadcast_begin(sender)
    calls = (len(rows) + chunk - 1) // chunk
    again = np.concatenate([step() for _ in range(calls)])
    assert np.array_equal(again, rows), "the timed, host-driven run differs"
    tm = sim.timing()
    return dict(calls=calls, windows=int(tm["windows"]), exact_redos=int(tm["exact_redos"]),
                coarse_redos=int(tm["coarse_redos"]))


def child_case(gs, oracle, name):
    from test_flood_shapes import cfg_of, flood, overlay_matches
    c = CASES[name]
    kw, chunk, G, kind = c["kw"], c.get("chunk", 10), c.get("shards", 0), c.get("kind", "flood")
    n = kw["n"]
    failed, sender = mask_and_sender(name)
    if kind == "batch":
        T = c["trials"]
        deg, ids = table(name)
        es = [oracle.Engine(oracle.make_params(**dict(kw, trial=kw["trial"] + t)), deg[t * n:(t + 1) * n],
                            ids[t * n:(t + 1) * n]) for t in range(T)]
        with gs.Simulator(cfg_of(gs, kw, trials=T)) as sim:
            sim.load_peers(deg, ids)
            for e in es:
                e.begin(-1)
            sim.broadcast_begin(-1)
            rows = []
            for call in range(800):
                each = [e.step(chunk).astype(np.int64) for e in es]
                want = np.sum(each, axis=0)
                want[:, 0] = each[0][:, 0]
                got = sim.step(chunk).astype(np.int64)
                assert np.array_equal(got, want), f"call {call}:\n{got}\n{want}"
                assert np.array_equal(sim.received(), np.stack([e.received() for e in es])), f"call {call}"
                rows.append(got)
                if int(want[-1][6]) == 0:
                    break
            else:
                raise AssertionError("still pending")
            assert np.array_equal(sim.crashed(), np.stack([e.crashed() for e in es]))
            rows = np.concatenate(rows)
            return timed_again(sim, rows, chunk, -1, lambda: sim.step(chunk).astype(np.int64))
    sim = gs.Simulator(cfg_of(gs, kw), devices=[0] * G) if G else gs.Simulator(cfg_of(gs, kw))
    with sim:
        if kind == "overlay":
            deg, ids = overlay_matches(sim, oracle, kw)
        else:
            deg, ids = table(name)
            sim.load_peers(deg, ids)
        if G:
            nf = (n + FINE - 1) // FINE
            per = (nf + G - 1) // G * FINE
            assert sim.shard_info() == [(i * per, min(n, (i + 1) * per)) for i in range(G)], sim.shard_info()
        if failed is not None:
            sim.set_failed(failed)
        rows = flood(sim, oracle, kw, deg, ids, chunk, sender, failed)
        if G:
            return dict(exact_redos=int(sim.timing()["exact_redos"]))
        return timed_again(sim, rows, chunk, sender, lambda: sim.step(chunk))


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gossip_simulator_amd as gs
    from oracle import pyoracle as oracle
    oracle.build()
    gs.load()
    setting = sys.argv[1]
    out = {"env": {k: os.environ[k] for k in KNOBS if k in os.environ}, "cases": {}}
    for name in SETTINGS[setting][1]:
        try:
            out["cases"][name] = child_case(gs, oracle, name)
        except BaseException as e:  # (pytest.fail raises outside Exception)
            out["cases"][name] = {"error": f"{type(e).__name__}: {e}"[:4000]}
    print(json.dumps(out))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS), ids=list(SETTINGS))
def test_later_passes_match_the_oracle(setting):
    knobs, names = SETTINGS[setting]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), setting], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["env"] == knobs
    assert list(got["cases"]) == names
    for name, fig in got["cases"].items():
        assert "error" not in fig, f"{name}: {fig['error']}"
        c = CASES[name]
        if not c.get("shards", 0):
            assert fig["windows"] == fig["calls"], f"{name}: {fig}"
        if c.get("redo"):
            assert fig["exact_redos"] > 0, f"{name}: {fig}"
        if c.get("kind") == "batch":  # plan_coarse_trials saw k_expand's grid
            assert fig["coarse_redos"] == 0, f"{name}: {fig}"


if __name__ == "__main__":
    main()
