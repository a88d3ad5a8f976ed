"""Packed median batches (GS_FLAG_MEDIAN_PACKED) on one device:
  ab     packed against unpacked batch at n = 20,000, T = 2,048 (section 4.8.1's workload), legs alternating;
  loop   the packed batch at n = 50,000, T = 256 and 2,048, against section 4.8.1's sequential leg: one-trial
         runs on one context with reset, set_trial and load_peers outside the timed part;
  sweep  k = 2..6 at n = 50,000, T = 2,048, poll 1: ended share, stranded nodes, messages per node, rounds to 99 %.
Walls are the host clock around broadcast_begin + run (drop 0.1, seed 1, keyed senders, the batch's own overlays,
max_ticks 150).  Usage: python scripts/median_packed_measure.py [output file] [ab,loop,sweep]; one JSON line per figure."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import gossip_simulator_amd as gs  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
PARTS = (sys.argv[2] if len(sys.argv) > 2 else "ab,loop,sweep").split(",")
MAX_TICKS, COVERED, QUIESCENT, MAX = 150, 0, 1, 2


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def config(n, k, trials=1, trial=0, packed=False):
    return gs.Config(n=n, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=1, trial=trial, model="median",
                     rumor_k=k, trials=trials, median_packed=packed)


def timed_run(sim, poll):
    t0 = time.perf_counter()
    sim.broadcast_begin(-1)
    sim.run(poll=poll, max_ticks=MAX_TICKS)
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    s = sorted(ms)
    return [round(s[len(s) // 2], 3), round(s[0], 3), round(s[-1], 3)]   # median, min, max


say(max_n=gs.median_trials_max_n(), max_n_packed=gs.median_trials_max_n(packed=True))

if "ab" in PARTS:
    n, T, k = 20_000, 2048, 5
    sims = {"unpacked": gs.Simulator.median_batch(config(n, k, T)),
            "packed": gs.Simulator.median_batch(config(n, k, T, packed=True))}
    for s in sims.values():
        s.build_overlay()
    ms, res = {leg: [] for leg in sims}, {}
    for run in range(-1, 5):   # run -1: the warm-up
        for leg, s in sims.items():
            w = timed_run(s, 10)
            r = s.trial_results()
            assert leg not in res or np.array_equal(res[leg], r)
            res[leg] = r
            s.reset()
            if run >= 0:
                ms[leg].append(w)
                say(leg=leg, n=n, T=T, k=k, run=run, ms=round(w, 3))
    say(summary="ab", n=n, T=T, k=k, unpacked_ms=spread(ms["unpacked"]), packed_ms=spread(ms["packed"]),
        results_identical=bool(np.array_equal(res["unpacked"], res["packed"])))
    for s in sims.values():
        s.close()

if "loop" in PARTS:
    n, k = 50_000, 5
    one = gs.Simulator(config(n, k))
    for T, seq_runs in ((256, 5), (2048, 3)):
        batch = gs.Simulator.median_batch(config(n, k, T, packed=True))
        batch.build_overlay()
        deg, ids = batch.read_peers()

        def sequential(count):
            total, rows = 0.0, []
            for i in range(count):
                one.reset()
                one.set_trial(i)
                one.load_peers(deg[i * n:(i + 1) * n], ids[i * n:(i + 1) * n])
                total += timed_run(one, 10)
                rows.append(one.trial_results()[0])
            return total, np.array(rows)

        timed_run(batch, 10)   # warm-up of both legs
        batch.reset()
        sequential(8)
        bms, sms, identical = [], [], True
        for run in range(5):
            w = timed_run(batch, 10)
            bres = batch.trial_results()
            batch.reset()
            bms.append(w)
            say(leg="batch", n=n, T=T, k=k, run=run, ms=round(w, 3))
            if run < seq_runs:
                w, sres = sequential(T)
                sms.append(w)
                identical &= bool(np.array_equal(bres, sres))
                say(leg="sequential", n=n, T=T, k=k, run=run, ms=round(w, 3))
        say(summary="loop", n=n, T=T, k=k, batch_ms=spread(bms), seq_ms=spread(sms), results_identical=identical,
            every_batch_below_every_seq=max(bms) < min(sms))
        batch.close()
        del deg, ids
    one.close()

if "sweep" in PARTS:
    n, T = 50_000, 2048
    for k in range(2, 7):
        batch = gs.Simulator.median_batch(config(n, k, T, packed=True))
        batch.build_overlay()
        w = timed_run(batch, 1)
        r = batch.trial_results()
        st = batch.median_state()
        stranded = ((st != 0) & (st != 255)).sum(1)
        ended = r[:, 8] != MAX
        t99 = r[:, 1][r[:, 1] > 0]
        mpn = r[:, 5] / n
        say(summary="sweep", k=k, T=T, n=n, ended_share=float(ended.mean()), stranded_mean=float(stranded.mean()),
            stranded_max=int(stranded.max()), msgs_per_node_mean=float(mpn.mean()),
            msgs_per_node_sd=float(mpn.std(ddof=1)), never_99=int((r[:, 1] == 0).sum()),
            rounds_to_99_mean=float(t99.mean()), rounds_to_99_min=int(t99.min()), rounds_to_99_max=int(t99.max()),
            stop_round_mean_of_ended=float(r[:, 2][ended].mean()) if ended.any() else None,
            residue_mean=float((1.0 - r[:, 6] / n).mean()), wall_ms=round(w, 1))
        batch.close()
