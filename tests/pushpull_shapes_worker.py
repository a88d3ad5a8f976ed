"""A fresh process with push-pull A/B switches set (the library reads them once
per process): GS_PPB_WORDS, GS_PPB_WORD_MAXU, GS_PPA_WORD_MAXI,
GS_PPB_PULLFIRST, GS_PP_NODEG, GS_PP_NORFAIL, GS_PP_NODEFER.  Sets the given
switches before the library loads, rebuilds each case's table from its key
(tests/test_pushpull_shapes.py: case_data), runs it per round in a fresh
context and prints one JSON line: the switches as set, and per case the stats
rows, the informed bitset's hash after every round, the crashed hash and the
mode counters.  A case in mode "answer-all" also sets GS_PP_BOTTOM256=256
around its own broadcast (gpu_rounds; the library reads it at every
broadcast_begin): no bottom-up rounds, pull-answer to the end.  Launched by
tests/test_pushpull_shapes.py, which compares the line with the oracle.

Usage: python tests/pushpull_shapes_worker.py '{"env": {...}, "cases": [[key, mode], ...]}'"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCHES = ("GS_PPB_WORDS", "GS_PPB_WORD_MAXU", "GS_PPA_WORD_MAXI", "GS_PPB_PULLFIRST", "GS_PP_NODEG",
            "GS_PP_NORFAIL", "GS_PP_NODEFER")


def main():
    arg = json.loads(sys.argv[1])
    for k in SWITCHES:  # only what the parent asks for
        os.environ.pop(k, None)
    for k, v in arg["env"].items():
        if k not in SWITCHES:
            raise SystemExit(f"unknown switch {k}")
        os.environ[k] = v  # before the library's first push-pull broadcast
    import gossip_simulator_amd as gs
    from test_pushpull_shapes import gpu_rounds
    gs.load()
    out = {"env": {k: os.environ[k] for k in SWITCHES if k in os.environ},
           "results": [gpu_rounds(gs, key, mode) for key, mode in arg["cases"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
