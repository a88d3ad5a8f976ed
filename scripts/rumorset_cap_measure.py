"""Bounded rumor sets, R = 64 keyed senders over section
4.9's set-up (fanout 5, fanin 6, drop 0.1, seed 1).
  cost:  walls of begin + run(poll=10) with every start 0, the uncapped set
         (payload 0, k_rs_round) against payload 64 under each policy
         (k_rsc_round, never binds), alternating; one warm-up, three runs.
  sweep: a stream of updates, rumor j enters at round j (-every 1), B in
         {1, 2, 4, 8, 64} under each policy, stepped so that every round is a
         poll: rounds from start to 99 % per update, carried / wanted, bound.
Usage: python scripts/rumorset_cap_measure.py <n> <output file> [cost] [sweep]; one JSON line per figure."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gossip_simulator_amd as gs  # noqa: E402

N = int(float(sys.argv[1]))
R = 64
out = open(sys.argv[2] if len(sys.argv) > 2 else os.devnull, "w")
parts = sys.argv[3:] or ["cost", "sweep"]
PICKS = ("low", "high", "rotate")


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


cfg = gs.Config(n=N, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=1, model="pushpull")
t0 = time.time()
rs = gs.Simulator.rumor_set(cfg, R)
rs.build_overlay()
say(what="setup", n=N, seconds=round(time.time() - t0, 2))
rs.broadcast_begin(-1)
senders = [r["sender"] for r in rs.rumor_results()]
rs.reset()

if "cost" in parts:
    for i in range(4):
        for payload, pick in [(0, "low")] + [(R, p) for p in PICKS]:
            rs.set_payload(payload, pick)
            t0 = time.perf_counter()
            rs.begin_rumors(senders)
            rows, st = rs.run(poll=10)
            wall = time.perf_counter() - t0
            tot = rs.totals()
            tr = rs.rumor_traffic() if payload else {}
            rs.reset()
            say(what="cost", i=i, warmup=i == 0, payload=payload, pick=pick, ms=round(wall * 1e3, 2), status=st,
                tick=tot["tick"], received=tot["received"], messages=tot["messages"], **tr)

if "sweep" in parts:
    starts = list(range(R))
    for pick in PICKS:
        for B in (1, 2, 4, 8, 64):
            rs.set_payload(B, pick)
            t0 = time.perf_counter()
            rs.begin_rumors(senders, starts)
            while True:
                row = rs.step(10)[-1]
                if int(row[6]) == 0 or int(row[0]) >= 5000:
                    break
            wall = time.perf_counter() - t0
            res, tr, tot = rs.rumor_results(), rs.rumor_traffic(), rs.totals()
            rs.reset()
            took = sorted(r["tick_99"] - s for r, s in zip(res, starts) if r["tick_99"])
            say(what="sweep", payload=B, pick=pick, covered=len(took), rounds=tot["tick"], ms=round(wall * 1e3, 1),
                from_start_min=took[0] if took else None, from_start_median=took[len(took) // 2] if took else None,
                from_start_max=took[-1] if took else None, last_tick99=max(r["tick_99"] for r in res),
                carried_over_wanted=round(tr["carried"] / max(1, tr["wanted"]), 4), messages=tot["messages"], **tr)
rs.close()
