"""Rumor set (R = 64) against 64 one-rumor push-pull broadcasts from the same 64
keyed senders on one context: walls of begin + run(poll=10),
alternating, then per-round kernel times of a stepped run of each.
Usage: python scripts/rumorset_measure.py <n> [output file]; one JSON line per figure."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import gossip_simulator_amd as gs  # noqa: E402

N = int(float(sys.argv[1]))
R = 64
out = open(sys.argv[2] if len(sys.argv) > 2 else os.devnull, "w")


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


cfg = gs.Config(n=N, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=1, model="pushpull")
t0 = time.time()
rs = gs.Simulator.rumor_set(cfg, R)
rs.build_overlay()
pp = gs.Simulator(cfg)
pp.build_overlay()
say(what="setup", n=N, seconds=round(time.time() - t0, 2))
rs.broadcast_begin(-1)
senders = [r["sender"] for r in rs.rumor_results()]
rs.reset()
for i in range(4):
    t0 = time.perf_counter()
    rs.begin_rumors(senders)
    rows, st = rs.run(poll=10)
    w_rs = time.perf_counter() - t0
    res = rs.rumor_results()
    t99 = [r["tick_99"] for r in res]
    tot = rs.totals()
    rs.reset()
    w_pp, pp_ticks, pp_msgs = 0.0, [], 0
    for s in senders:
        t0 = time.perf_counter()
        pp.broadcast_begin(s)
        prow, pst = pp.run(poll=10)
        w_pp += time.perf_counter() - t0
        pp_ticks.append(int(prow[-1][0]))
        pp_msgs += pp.totals()["messages"]
        pp.reset()
    say(what="run", i=i, warmup=i == 0, rumorset_ms=round(w_rs * 1e3, 2), pushpull64_ms=round(w_pp * 1e3, 2),
        ratio=round(w_pp / w_rs, 3), status=st, rs_tick=tot["tick"], rs_tick99_min=min(t99), rs_tick99_max=max(t99),
        pp_tick_min=min(pp_ticks), pp_tick_max=max(pp_ticks), rs_messages=tot["messages"], pp_messages=pp_msgs)
# a stepped run: per-round kernel times and per-rumor round of 99 %
rs.set_flags(True)
rs.begin_rumors(senders)
last = rs.timing()
while True:
    row = rs.step(1)[0]
    tm = rs.timing()
    say(what="round", t=int(row[0]), round_ms=round(tm["deliver_ms"] - last["deliver_ms"], 3),
        commit_ms=round(tm["resolve_ms"] - last["resolve_ms"], 3), pairs=int(row[4]), pending=int(row[6]),
        messages=int(row[3]))
    last = tm
    if int(row[6]) == 0 or int(row[0]) >= 100:
        break
t99 = sorted(r["tick_99"] for r in rs.rumor_results())
say(what="tick99_by_round", spread=[t99[0], t99[len(t99) // 2], t99[-1]], all=t99)
pp.set_flags(True)
pp.broadcast_begin(senders[0])
last = pp.timing()
while True:
    t0 = time.perf_counter()
    row = pp.step(1)[0]
    wall = time.perf_counter() - t0
    tm = pp.timing()
    say(what="pp_round", t=int(row[0]), kernels_ms=round(tm["deliver_ms"] + tm["resolve_ms"] - last["deliver_ms"] - last["resolve_ms"], 3),
        wall_ms=round(wall * 1e3, 3), received=int(row[4]))
    last = tm
    if gs.covered(int(row[4]), N) or int(row[0]) >= 100:
        break
rs.close()
pp.close()
