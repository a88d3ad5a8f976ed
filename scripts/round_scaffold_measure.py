"""The host round loop of the one-trial rumor, median and rumor-set engines, one
library build against another:
  one <label> [output file]   this process's library (GS_LIB_PATH, else the package's): wall time per round of one
                              non-timing gs_step(2000) at n = 4,133 for the rumor set (R = 64, uncapped and payload 8),
                              rumor push, rumor pull and median (these three end early and keep stepping: the loop's
                              own cost), then one begin + run(poll=10) of each at n = 1,000,000; a JSON line per figure;
  ab <library A> <library B> <processes per build> <output file>
                              `one` in fresh processes, A and B alternating; then per row median [min, max] of each
                              build and whether B's median lies inside A's range.
Every figure is the host clock around calls that end in a stream synchronise, after one untimed pass of the same
calls (drop 0.1, seed 1, keyed senders, the context's own overlay)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["rumor_set", "rumor_set_payload8", "rumor_push", "rumor_pull", "median"]
R, SMALL_N, BIG_N, ROUNDS = 64, 4133, 1_000_000, 2000


def one(label, path):
    sys.path.insert(0, ROOT)
    import gossip_simulator_amd as gs
    out = open(path, "a") if path else open(os.devnull, "w")

    def say(**kw):
        line = json.dumps(dict(lib=label, **kw))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def make(row, n):
        kw = dict(n=n, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=1)
        if row.startswith("rumor_set"):
            sim = gs.Simulator.rumor_set(gs.Config(model="pushpull", **kw), R)
            if row.endswith("payload8"):
                sim.set_payload(8, "rotate")
        elif row == "median":
            sim = gs.Simulator(gs.Config(model="median", rumor_k=3, **kw))
        else:
            sim = gs.Simulator(gs.Config(model="rumor", rumor_k=2, rumor_pull=row == "rumor_pull", **kw))
        return sim

    for n in (SMALL_N, BIG_N):
        table = None
        for row in ROWS:
            with make(row, n) as sim:
                if table is None:
                    sim.build_overlay()
                    table = sim.read_peers()
                else:
                    sim.load_peers(*table)
                for _ in range(2):   # the first pass warms up: the second pass's wall and totals are reported
                    t0 = time.perf_counter()
                    sim.broadcast_begin(-1)
                    if n == SMALL_N:
                        t0 = time.perf_counter()   # the step rows time gs_step alone
                        sim.step(ROUNDS)
                    else:
                        sim.run(poll=10, max_ticks=10_000)
                    wall = time.perf_counter() - t0
                    tot = sim.totals()
                    sim.reset()
                if n == SMALL_N:
                    say(row=row + "_step", n=n, us_per_round=round(wall / ROUNDS * 1e6, 3), totals=tot)
                else:
                    say(row=row + "_run", n=n, run_ms=round(wall * 1e3, 3), totals=tot)


def ab(lib_a, lib_b, reps, path):
    open(path, "w").close()
    for rep in range(reps):
        for label, lib in (("A", lib_a), ("B", lib_b)):
            env = dict(os.environ, GS_LIB_PATH=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "one", label, path], env=env, check=True,
                           timeout=300)   # a failed or hung process ends the measurement: nothing runs after it
    vals, totals = {}, {}
    with open(path) as f:
        for line in f:
            d = json.loads(line)
            v = d.get("us_per_round", d.get("run_ms"))
            vals.setdefault(d["row"], {}).setdefault(d["lib"], []).append(v)
            totals.setdefault(d["row"], set()).add(json.dumps(d["totals"], sort_keys=True))
    with open(path, "a") as f:
        for row, by in vals.items():
            a, b = sorted(by["A"]), sorted(by["B"])
            line = json.dumps(dict(summary=row, unit="us/round" if row.endswith("_step") else "ms",
                                   A=[a[len(a) // 2], a[0], a[-1]], B=[b[len(b) // 2], b[0], b[-1]],
                                   B_median_inside_A_range=a[0] <= b[len(b) // 2] <= a[-1],
                                   totals_equal=len(totals[row]) == 1))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "one":
        one(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    elif len(sys.argv) == 6 and sys.argv[1] == "ab":
        ab(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
    else:
        sys.exit(__doc__)
