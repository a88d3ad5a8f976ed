"""k_resolve at three workgroups per CU: the branches the smaller budget adds.

k_resolve keeps its infection list in 6,656 LDS entries (kInfCap) and drains it
in rounds when a bucket informs more nodes in one window; a bucket that lists
more than 1,024 rolled receipts (kRolledCap) is handed to k_resolve_large
(k_resolve_large_m for an in-process shard group), launched between k_resolve
and the rolled replay.  GS_RESOLVE_OCC3=0 (read once per process) selects the
two-per-CU kernel with its own large path instead.

Every case is one broadcast over an injected random table, bit for bit against
oracle.Engine through test_flood_shapes.flood (every stats row, the received
bitset per step call, the crashed bitset), stepped one window per call; the
unsharded cases run again host-driven and timed, where gs_timing counts the
windows: one per call, so a call's stats are one window's.  Both switch
settings run every case, each in a child process (this file, run as a script).

What the oracle gives for the cases (test_cases_reach_the_new_branches checks
the bounds on the CPU):
  rounds        n = 32805: the window of ticks 51..60 informs 17,483 nodes, at
                least 8,723 of them in one of the two full buckets: two rounds
  large         n = 16385: the window of ticks 71..80 crashes 5,466 nodes, each
                by a rolled receipt at a node live when the window starts; all
                but at most one in bucket 0
  large-shards  n = 32805 over two shards: the densest window's crashes exceed
                2 * 1,024 + 37, so a full bucket lists more than 1,024
  ring          n = 16385, delays 3..4: ring of 4 slots, windows of 3 ticks
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF_CAP, ROLLED_CAP, FINE = 6656, 1024, 16384  # kInfCap, kRolledCap, kFineNodes

DENSE = dict(fanout=12, fanin=13, delay_low=10, delay_high=20, drop_rate=0.0, seed=11, trial=0)
# name: (parameters, row stride, degrees, shards (0: one context), ticks per step call = window)
CASES = {
    "rounds": (dict(DENSE, n=2 * FINE + 37, crash_rate=0.0), 13, (12, 13), 0, 10),
    "large": (dict(DENSE, n=FINE + 1, crash_rate=0.5), 13, (12, 13), 0, 10),
    "large-shards": (dict(DENSE, n=2 * FINE + 37, crash_rate=0.5), 13, (12, 13), 2, 10),
    "ring": (dict(fanout=5, fanin=6, delay_low=3, delay_high=4, drop_rate=0.1, crash_rate=0.02, seed=11, trial=0,
                  n=FINE + 1), 6, (5, 6), 0, 3),
}
SWITCHES = {"three-per-cu": None, "two-per-cu": "0"}


def table(name):
    from test_gpu_parity import random_table
    kw, stride, (lo, hi), _, _ = CASES[name]
    return random_table(kw["n"], stride, lo, hi, seed=1)


def densest_windows(rows, chunk):
    """(most nodes informed, most nodes crashed) in one step call's ticks."""
    recv = np.concatenate([[0], rows[:, 4].astype(np.int64)])
    crashed = np.concatenate([[0], rows[:, 5].astype(np.int64)])
    ends = list(range(chunk, len(rows), chunk)) + [len(rows)]
    starts = [0] + ends[:-1]
    return (max(int(recv[b] - recv[a]) for a, b in zip(starts, ends)),
            max(int(crashed[b] - crashed[a]) for a, b in zip(starts, ends)))


def reaches_its_branch(name, informed, crashed):
    n = CASES[name][0]["n"]
    full, rest = divmod(n, FINE)
    if name == "rounds":  # some full bucket informs more than the list holds
        assert informed > full * INF_CAP + rest, informed
    elif name.startswith("large"):  # some full bucket lists more rolled receipts than kRolledCap
        assert crashed > full * ROLLED_CAP + rest, crashed
    else:  # the dense path: more receipts than k_resolve_small takes
        assert informed > 256 * (full + 1), informed


def test_cases_reach_the_new_branches(oracle):
    """The oracle alone: the densest window of every case is past the bound its
    branch needs (the figures in the module docstring)."""
    from test_flood_shapes import oracle_flood
    for name, (kw, _, _, _, chunk) in CASES.items():
        deg, ids = table(name)
        rows, _, _ = oracle_flood(oracle, kw, deg, ids, chunk)
        reaches_its_branch(name, *densest_windows(rows, chunk))
    rows, _, _ = oracle_flood(oracle, CASES["rounds"][0], *table("rounds"), 10)
    assert densest_windows(rows, 10)[0] == 17483


def child(name):
    """One case in this process; returns its figures."""
    import gossip_simulator_amd as gs
    from oracle import pyoracle as oracle
    from test_flood_shapes import cfg_of, flood
    oracle.build()
    gs.load()
    kw, _, _, G, chunk = CASES[name]
    deg, ids = table(name)
    out = {}
    sim = gs.Simulator(cfg_of(gs, kw), devices=[0] * G) if G else gs.Simulator(cfg_of(gs, kw))
    with sim:
        sim.load_peers(deg, ids)
        rows = flood(sim, oracle, kw, deg, ids, chunk)
        out["informed"], out["crashed"] = densest_windows(rows, chunk)
        if not G:  # host-driven and timed: the same rows, one window per call
            sim.set_flags(True)
            sim.reset()
            sim.broadcast_begin(-1)
            calls = (len(rows) + chunk - 1) // chunk
            again = np.concatenate([sim.step(chunk) for _ in range(calls)])
            assert np.array_equal(again, rows), "the timed, host-driven run differs"
            out["calls"], out["windows"] = calls, int(sim.timing()["windows"])
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    out = {"switch": os.environ.get("GS_RESOLVE_OCC3"), "cases": {}}
    for name in CASES:
        try:
            out["cases"][name] = child(name)
        except BaseException as e:  # (pytest.fail raises outside Exception)
            out["cases"][name] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(out))


@pytest.mark.gpu
@pytest.mark.parametrize("switch", list(SWITCHES), ids=list(SWITCHES))
def test_resolve_kernels_match_the_oracle(switch):
    env = dict(os.environ)
    env.pop("GS_RESOLVE_OCC3", None)
    env.pop("GS_RESOLVE_PER_CU", None)
    if SWITCHES[switch] is not None:
        env["GS_RESOLVE_OCC3"] = SWITCHES[switch]
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["switch"] == SWITCHES[switch]
    assert list(got["cases"]) == list(CASES)
    for name, fig in got["cases"].items():
        assert "error" not in fig, f"{name}: {fig['error']}"
        reaches_its_branch(name, fig["informed"], fig["crashed"])
        if not CASES[name][3]:
            assert fig["windows"] == fig["calls"], f"{name}: {fig}"


if __name__ == "__main__":
    main()
