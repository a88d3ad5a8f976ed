"""Per-trial failure masks on a batch of push-pull trials (DESIGN.md section
4.5.2): what does the masked batch cost against a loop of one-trial masked
contexts, and does the unmasked batch still run at its old speed?

One 2000-trial overlay at n = 1e5 (default flags, crash rate 0), tables read
back; every trial gets its own mask of 1 % of the nodes.
  (a) masked batch against the loop: reset + broadcast_begin + run(poll=10) of
      the masked 2000-trial batch, three repeats after one untimed pass,
      against the first 50 trials on ONE reused one-trial push-pull context
      (per trial set_trial + load_peers + set_failed + begin + run: the
      reverse-table and failed-slot-mask builds included, a user pays them per
      table and mask).  Rows must be equal; the ratio is recorded, there is no
      target.
  (b) unmasked batch against the parent commit: `--parent TREE` runs the
      parent's own command, `python scripts/pp_trials_ab.py`, in TREE (a built
      checkout of the parent commit) and in this tree, five fresh processes
      each, interleaved, and compares the medians of the batch's ms per
      trial: this build must not be slower than the parent by more than the
      spread (max - min) between the parent's own runs.
  (u) the default run also times this build's unmasked batch (REPEATS_B
      repeats) beside the masked one, for the masked / unmasked ratio.

Usage (on the GPU box): python scripts/pp_trials_mask_ab.py [out.txt] [n] [trials] [looped]
                        python scripts/pp_trials_mask_ab.py [out.txt] --parent TREE"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gossip_simulator_amd as gs  # noqa: E402

REPEATS, REPEATS_B, RUNS_AB, FRAC = 3, 5, 5, 0.01


def batch_pass(sim):
    t0 = time.perf_counter()
    sim.reset()
    sim.broadcast_begin(-1)
    _, status = sim.run(poll=10)
    return time.perf_counter() - t0, status


def loop_pass(sim, tabs, masks):
    rows = []
    t0 = time.perf_counter()
    for t, (deg, ids) in enumerate(tabs):
        sim.reset()
        sim.set_trial(t)
        sim.load_peers(deg, ids)
        sim.set_failed(masks[t])
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        rows.append(sim.trial_results()[0])
    return time.perf_counter() - t0, np.array(rows)


def make_masks(n, T, frac, seed=7):
    """[T, ceil(n/64)]: round(frac * n) failed nodes per trial, each trial its own."""
    rng = np.random.default_rng(seed)
    W, k = (n + 63) // 64, int(round(frac * n))
    out = np.zeros((T, W), dtype=np.uint64)
    for t in range(T):
        idx = rng.choice(n, size=k, replace=False)
        np.bitwise_or.at(out[t], idx // 64, np.left_shift(np.uint64(1), (idx % 64).astype(np.uint64)))
    return out


def parent_ab(parent_tree, out):
    """(b): `python scripts/pp_trials_ab.py` (the parent's own command, no
    arguments) in a built checkout of the parent commit and in this tree,
    RUNS_AB fresh processes each, interleaved.  A run's figure is the median
    of its three "(a) batch repeat" lines, ms per trial."""
    import re
    import subprocess
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = {"parent": os.path.abspath(parent_tree), "this": here}
    figs = {"parent": [], "this": []}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"(b) unmasked batch, parent build against this build: {RUNS_AB} interleaved runs each of "
        f"`python scripts/pp_trials_ab.py`")
    for r in range(RUNS_AB):
        for who in ("parent", "this"):
            p = subprocess.run([sys.executable, os.path.join("scripts", "pp_trials_ab.py")], cwd=trees[who],
                               capture_output=True, text=True, timeout=600)
            reps = [float(x) for x in re.findall(r"^\(a\) batch repeat \d+:.*= ([0-9.]+) ms per trial", p.stdout, re.M)]
            if len(reps) < 3:
                say(f"{who} run {r}: no figures (exit {p.returncode})\n{p.stdout[-400:]}\n{p.stderr[-400:]}")
                return 1
            figs[who].append(float(np.median(reps)))
            say(f"(b) {who:6s} run {r}: repeats {reps} -> {figs[who][-1]:.4f} ms per trial")
    mp, mt = float(np.median(figs["parent"])), float(np.median(figs["this"]))
    spread = max(figs["parent"]) - min(figs["parent"])
    ok = mt - mp <= spread
    say(f"(b) parent median {mp:.4f} ms per trial (min {min(figs['parent']):.4f}, max {max(figs['parent']):.4f}, "
        f"spread {spread:.4f}); this build median {mt:.4f} (min {min(figs['this']):.4f}, max {max(figs['this']):.4f}); "
        f"difference {mt - mp:+.4f}: {'within' if ok else 'NOT within'} the parent's spread")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def main():
    if "--parent" in sys.argv:
        i = sys.argv.index("--parent")
        rest = [a for a in sys.argv[1:i] + sys.argv[i + 2:] if not a.startswith("--")]
        return parent_ab(sys.argv[i + 1], rest[0] if rest else None)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    unmasked_only = "--unmasked-only" in sys.argv
    out = args[0] if len(args) > 0 else None
    n = int(float(args[1])) if len(args) > 1 else 100_000
    T = int(args[2]) if len(args) > 2 else 2000
    K = int(args[3]) if len(args) > 3 else 50
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"pp_trials_mask_ab: n={n} trials={T} looped={K} failed={FRAC:.0%} per trial")
    base = dict(n=n, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=0x5EED, model="pushpull")
    ok = True
    with gs.Simulator(gs.Config(**base, trials=T)) as sim:
        t0 = time.perf_counter()
        sim.build_overlay()
        say(f"overlay of {T} trials: {time.perf_counter() - t0:.2f} s")
        batch_pass(sim)  # untimed
        b = []
        for r in range(REPEATS_B):
            dt, status = batch_pass(sim)
            b.append(dt * 1e3 / T)
            say(f"(u) unmasked batch repeat {r}: {dt * 1e3:9.2f} ms = {b[-1]:.4f} ms per trial  (status {status}, "
                f"rounds {sim.totals()['tick']})")
        say(f"(u) unmasked batch: median {np.median(b):.4f} ms per trial, min {min(b):.4f}, max {max(b):.4f}, "
            f"spread {max(b) - min(b):.4f}")
        if not unmasked_only:
            say(f"pp_trials_max_n_masked={gs.pp_trials_max_n_masked()}")
            deg, ids = sim.read_peers()
            m = np.arange(ids.shape[1])[None, :] < deg[:K * n, None]
            tabs = [(deg[t * n:(t + 1) * n].copy(), np.where(m[t * n:(t + 1) * n], ids[t * n:(t + 1) * n], 0)
                     .astype(np.uint32)) for t in range(K)]
            del deg, ids, m
            masks = make_masks(n, T, FRAC)
            sim.reset()
            t0 = time.perf_counter()
            sim.set_failed(masks)
            say(f"set_failed of {T} masks: {(time.perf_counter() - t0) * 1e3:.2f} ms")
            batch_pass(sim)  # untimed
            a = []
            for r in range(REPEATS):
                dt, status = batch_pass(sim)
                a.append(dt * 1e3 / T)
                say(f"(a) masked batch repeat {r}: {dt * 1e3:9.2f} ms = {a[-1]:.4f} ms per trial  (status {status}, "
                    f"rounds {sim.totals()['tick']})")
            brow = sim.trial_results()
    if not unmasked_only:
        with gs.Simulator(gs.Config(**base)) as one:
            loop_pass(one, tabs, masks)  # untimed
            loop = []
            for r in range(REPEATS):
                dt, rows = loop_pass(one, tabs, masks)
                loop.append(dt * 1e3 / K)
                same = np.array_equal(rows, brow[:K])
                ok = ok and same
                say(f"(a) masked loop repeat {r}: {dt * 1e3:9.2f} ms = {loop[-1]:.4f} ms per trial; "
                    f"rows equal the batch's first {K}: {same}")
                if not same:
                    say(f"{rows[:3]}\n{brow[:3]}")
        say(f"statuses in the masked batch: covered {int((brow[:, 8] == 0).sum())}, quiescent "
            f"{int((brow[:, 8] == 1).sum())} of {T}; stopping ticks {sorted(set(int(x) for x in brow[:, 2]))}")
        say(f"(a) masked batch median {np.median(a):.4f} ms per trial; masked loop median {np.median(loop):.4f}; "
            f"ratio {np.median(loop) / np.median(a):.1f}x; masked / unmasked batch "
            f"{np.median(a) / np.median(b):.3f}; rows {'equal' if ok else 'DIFFER'}")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
