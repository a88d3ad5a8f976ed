"""A fresh process with GS_NO_PACK set (the library reads it once per process):
k_expand reads the padded table itself instead of the packed view.  Builds the
overlay of the given parameters, runs one broadcast per tick and one in 10-tick
steps, and prints one JSON line: the overlay's windows, final tick and hashes,
and per step call the stats rows and the received bitset's hash.  Launched by
tests/test_flood_shapes.py, which compares the line with the oracle.

Usage: python tests/flood_shapes_worker.py '<parameters as JSON>'"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAP = 8000  # ticks


def main():
    os.environ["GS_NO_PACK"] = "1"  # before the library's first window run
    kw = json.loads(sys.argv[1])
    import gossip_simulator_amd as gs
    from test_gpu_parity import masked, sha
    gs.load()
    cfg = gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                    delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                    seed=kw["seed"], trial=kw["trial"])
    out = {"no_pack": os.environ["GS_NO_PACK"], "runs": []}
    with gs.Simulator(cfg) as sim:
        wins, final = sim.build_overlay()
        deg, ids = sim.read_peers()
        pad = np.arange(ids.shape[1])[None, :] >= deg.astype(np.int64)[:, None]
        out.update(windows=[list(w) for w in wins], final=final, deg_sha256=sha(deg),
                   rows_sha256=sha(masked(deg, ids)), sealed=bool(np.all(ids[pad] == 0xFFFFFFFF)))
        for chunk in (1, 10):
            sim.reset()
            sim.broadcast_begin(-1)
            run = {"chunk": chunk, "rows": [], "received_sha256": []}
            for _ in range(0, CAP, chunk):
                rows = sim.step(chunk)
                run["rows"].append(rows.tolist())
                run["received_sha256"].append(sha(sim.received()))
                if int(rows[-1][6]) == 0:
                    break
            run["crashed_sha256"] = sha(sim.crashed())
            out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
