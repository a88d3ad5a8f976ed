"""A fresh process with GS_DD_GROUP=0 (the library reads it once per process):
the device-driven shard windows launch each per-shard kernel once per shard
instead of once for the group.  Builds case D (n, G) of
tests/test_shard_shapes.py, runs one broadcast in 10-tick steps, resets and
runs it again, and prints one JSON line: the value of the switch it saw, the
shard ranges, and per broadcast the stats rows and the received bitset's hash
of every step call, the crashed bitset's hash and dd_fallbacks.  Launched by
tests/test_shard_shapes.py, which compares the line with the oracle.

Usage: python tests/shard_shapes_worker.py '{"n": ..., "G": ...}'"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAP = 8000  # ticks


def main():
    os.environ["GS_DD_GROUP"] = "0"  # before the library's first device-driven shard window
    arg = json.loads(sys.argv[1])
    import gossip_simulator_amd as gs
    from test_flood_shapes import cfg_of
    from test_gpu_parity import sha
    from test_shard_shapes import build_d
    gs.load()
    c = build_d(arg["n"], arg["G"])
    out = {"dd_group": os.environ["GS_DD_GROUP"], "runs": []}
    with gs.Simulator(cfg_of(gs, c.kw), devices=[0] * c.G) as sim:
        out["shard_info"] = sim.shard_info()
        sim.load_peers(c.deg, c.ids)
        for _ in range(2):
            sim.reset()
            sim.broadcast_begin(c.sender)
            run = {"rows": [], "received_sha256": []}
            for _ in range(0, CAP, c.chunk):
                rows = sim.step(c.chunk)
                run["rows"].append(rows.tolist())
                run["received_sha256"].append(sha(sim.received()))
                if int(rows[-1][6]) == 0:
                    break
            run["crashed_sha256"] = sha(sim.crashed())
            run["dd_fallbacks"] = int(sim.timing()["dd_fallbacks"])
            out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
