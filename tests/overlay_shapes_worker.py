"""A fresh process for GS_OV_STAGGER (the library reads it once per process: the
ring's buckets start at staggered offsets, or with 0 at their allocation's
base).  Builds the overlay of each given parameter set and prints one JSON
line: per overlay its windows, final tick, row shape and hashes.  Launched by
tests/test_overlay_shapes.py with the variable set, which compares the line
with the oracle.

Usage: GS_OV_STAGGER=<0|1> python tests/overlay_shapes_worker.py '<list of parameters as JSON>'"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    kws = json.loads(sys.argv[1])
    import gossip_simulator_amd as gs
    from test_flood_shapes import EMPTY
    from test_gpu_parity import masked, sha
    gs.load()
    out = {"stagger": os.environ["GS_OV_STAGGER"], "overlays": []}
    for kw in kws:
        cfg = gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                        delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                        seed=kw["seed"], trial=kw["trial"])
        with gs.Simulator(cfg) as sim:
            wins, final = sim.build_overlay()
            deg, ids = sim.read_peers()
        pad = np.arange(ids.shape[1])[None, :] >= deg.astype(np.int64)[:, None]
        out["overlays"].append(dict(windows=[list(w) for w in wins], final=final, shape=list(ids.shape),
                                    deg_sha256=sha(deg), rows_sha256=sha(masked(deg, ids)),
                                    sealed=bool(np.all(ids[pad] == EMPTY)) if kw["fanin"] <= 32 else None))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
