"""Batched push-pull trials against a loop of one-trial contexts (DESIGN.md
section 6.1): is a batch the faster way to get T push-pull trials?

One 2000-trial overlay at n = 1e5 (default flags, crash rate 0), tables read
back.  Timed legs, three repeats each after one untimed pass:
  (a) reset + broadcast_begin + run(poll=10) of the 2000-trial batch;
  (b) the same broadcasts for the first 50 tables on ONE reused one-trial
      push-pull context with the default round selection: per trial
      set_trial + load_peers + begin + run (the reverse-table build included:
      a user pays it per table);
  (c) as (b) with pp_rounds="dense" (no reverse table).
Reports ms per trial for every repeat, checks that the batch's trial_results
rows equal the looped ones for the 50 trials both ran, and requires the slowest
batched repeat per trial to be below the fastest repeat per trial of the
better of (b) and (c).

Usage (on the GPU box): python scripts/pp_trials_ab.py [out.txt] [n] [trials] [looped]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gossip_simulator_amd as gs  # noqa: E402

REPEATS = 3


def batch_pass(sim):
    t0 = time.perf_counter()
    sim.reset()
    sim.broadcast_begin(-1)
    _, status = sim.run(poll=10)
    return time.perf_counter() - t0, status


def loop_pass(sim, tabs):
    rows = []
    t0 = time.perf_counter()
    for t, (deg, ids) in enumerate(tabs):
        sim.reset()
        sim.set_trial(t)
        sim.load_peers(deg, ids)
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        rows.append(sim.trial_results()[0])
    return time.perf_counter() - t0, np.array(rows)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 100_000
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    K = int(sys.argv[4]) if len(sys.argv) > 4 else 50
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"pp_trials_ab: n={n} trials={T} looped={K} repeats={REPEATS} pp_trials_max_n={gs.pp_trials_max_n()}")
    base = dict(n=n, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=0x5EED, model="pushpull")
    with gs.Simulator(gs.Config(**base, trials=T)) as sim:
        t0 = time.perf_counter()
        sim.build_overlay()
        say(f"overlay of {T} trials: {time.perf_counter() - t0:.2f} s")
        deg, ids = sim.read_peers()
        m = np.arange(ids.shape[1])[None, :] < deg[:K * n, None]
        tabs = [(deg[t * n:(t + 1) * n].copy(), np.where(m[t * n:(t + 1) * n], ids[t * n:(t + 1) * n], 0)
                 .astype(np.uint32)) for t in range(K)]
        del deg, ids, m
        batch_pass(sim)  # untimed
        a = []
        for r in range(REPEATS):
            dt, status = batch_pass(sim)
            a.append(dt * 1e3 / T)
            say(f"(a) batch repeat {r}: {dt * 1e3:9.2f} ms = {a[-1]:.4f} ms per trial  (status {status}, "
                f"rounds {sim.totals()['tick']})")
        brow = sim.trial_results()
    legs = {}
    for leg, rounds in (("b", "auto"), ("c", "dense")):
        with gs.Simulator(gs.Config(**base, pp_rounds=rounds)) as one:
            loop_pass(one, tabs)  # untimed
            legs[leg] = []
            for r in range(REPEATS):
                dt, rows = loop_pass(one, tabs)
                legs[leg].append(dt * 1e3 / K)
                say(f"({leg}) loop pp_rounds={rounds} repeat {r}: {dt * 1e3:9.2f} ms = {legs[leg][-1]:.4f} ms per trial")
                same = np.array_equal(rows, brow[:K])
                say(f"({leg}) looped rows equal the batch's first {K}: {same}")
                if not same:
                    say(f"{rows[:3]}\n{brow[:3]}")
    best_loop = min(min(legs["b"]), min(legs["c"]))
    worst_batch = max(a)
    ok = worst_batch < best_loop
    say(f"covered trials in the batch: {int((brow[:, 8] == 0).sum())} of {T}; "
        f"stopping ticks {sorted(set(int(x) for x in brow[:, 2]))}")
    say(f"slowest batched repeat {worst_batch:.4f} ms per trial; fastest looped repeat {best_loop:.4f} ms per trial "
        f"(b {min(legs['b']):.4f}, c {min(legs['c']):.4f}); ratio {best_loop / worst_batch:.1f}x; "
        f"requirement {'met' if ok else 'NOT met'}")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
