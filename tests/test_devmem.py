"""The library's device-memory cache (gs_devmem.cpp, DESIGN.md section 9;
verdict r05 item 2).

A hipMalloc right after tens of GB of hipFree waited for seconds on this
pool, so the product must not free and re-allocate large buffers in its
steady state.  Pinned here on the GPU:

* after a context's first broadcast, further broadcasts (gs_reset +
  gs_broadcast_begin + gs_run) make no device allocation at all -- neither a
  hipMalloc nor a block from the cache -- for the flood (window engine) and
  for push-pull, whose first broadcast builds the reverse table;
* a destroyed context's large blocks serve the next context of the same
  shape from the cache (no hipMalloc), and gs_trim gives them back;
* results do not depend on the cache: the same broadcast with
  GS_DEVMEM_CACHE=0 (every buffer a plain hipMalloc) gives the same counters
  and bitsets (a subprocess: the switch is read once per process), also for
  contexts of different shapes whose lifetimes overlap, so that blocks are
  split out of other contexts' extents and merged back while a neighbour is
  in use;
* the members of a multi-member batched context, whose regrows free and reuse
  blocks while the other members' streams run, give the results of fresh
  contexts through two renumberings;
* gs_trim's return value is the cache's own account, to the byte.

The bookkeeping itself (splits, merges, best fit, trimming, double frees, a
device without room) is pinned on the CPU against a model:
tests/test_devmem_model.py.

The reference allocates its nodes once per process (simulator.go:208-212).
"""
from __future__ import annotations

import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def allocs(gs):
    m = gs.memory_stats()
    return int(m["alloc_calls"]), int(m["alloc_cache_hits"])


@pytest.mark.parametrize("model", ["flood", "pushpull"])
def test_no_device_allocation_after_the_first_broadcast(gs, model):
    cfg = gs.Config(n=4_000_000, fanout=5, fanin=6, droprate=0.1, crashrate=0.01 if model == "flood" else 0.0,
                    seed=0x5EED, model=model)
    with gs.Simulator(cfg) as sim:
        sim.build_overlay()
        sim.broadcast_begin(-1)
        first = sim.run(poll=10)
        before = allocs(gs)
        for _ in range(3):
            sim.reset()
            sim.broadcast_begin(-1)
            again = sim.run(poll=10)
            assert np.array_equal(again[0], first[0]) and again[1] == first[1]
        assert allocs(gs) == before, f"device allocations in a later broadcast: {before} -> {allocs(gs)}"


def test_destroyed_context_blocks_serve_the_next(gs):
    cfg = gs.Config(n=8_000_000, fanout=5, fanin=6, droprate=0.1, crashrate=0.01, seed=0x5EED)
    with gs.Simulator(cfg) as sim:
        sim.build_overlay()
        sim.broadcast_begin(-1)
        a = sim.run(poll=10)
    _, hits0 = allocs(gs)
    assert gs.memory_stats()["cached_bytes"] > 0
    with gs.Simulator(cfg) as sim:
        sim.build_overlay()
        sim.broadcast_begin(-1)
        b = sim.run(poll=10)
    _, hits1 = allocs(gs)
    assert hits1 > hits0, "the second context took no block from the cache"
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    # gs_trim hands back whole free slabs: exactly that many cached bytes go
    cached = int(gs.memory_stats()["cached_bytes"])
    released = gs.trim()
    assert released > 0
    assert int(gs.memory_stats()["cached_bytes"]) == cached - released


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gossip_simulator_amd as gs
out = {}
for model in ("flood", "pushpull"):
    cfg = gs.Config(n=2_000_000, fanout=5, fanin=6, droprate=0.1, crashrate=0.01 if model == "flood" else 0.0,
                    seed=0x5EED, model=model)
    with gs.Simulator(cfg) as sim:
        sim.build_overlay()
        sim.broadcast_begin(-1)
        rows, status = sim.run(poll=10)
        out[model] = {"rows": np.asarray(rows).tolist(), "status": int(status),
                      "recv": int(np.unpackbits(sim.received().view(np.uint8)).sum())}
out["cached"] = int(gs.memory_stats()["cached_bytes"])
print("JSON" + json.dumps(out))
"""


def test_results_do_not_depend_on_the_cache():
    runs = {}
    for mode in ("1", "0"):
        env = dict(os.environ, GS_DEVMEM_CACHE=mode)
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        line = next(ln for ln in p.stdout.splitlines() if ln.startswith("JSON"))
        runs[mode] = json.loads(line[4:])
    assert runs["0"]["cached"] == 0 and runs["1"]["cached"] > 0
    for model in ("flood", "pushpull"):
        assert runs["0"][model] == runs["1"][model], model


_CHILD_OVERLAP = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gossip_simulator_amd as gs
out = {}
def run(sim, key, first):
    if first:
        sim.build_overlay()
    else:
        sim.reset()
    sim.broadcast_begin(-1)
    rows, status = sim.run(poll=10)
    out[key] = {"rows": np.asarray(rows).tolist(), "status": int(status),
                "recv": int(np.unpackbits(sim.received().view(np.uint8)).sum())}
a = gs.Simulator(gs.Config(n=4_000_000, fanout=5, fanin=6, droprate=0.1, crashrate=0.01, seed=0x5EED))
run(a, "A", True)
b = gs.Simulator(gs.Config(n=3_000_000, fanout=5, fanin=6, droprate=0.1, crashrate=0.0, seed=0x5EED,
                           model="pushpull"))
run(b, "B", True)
a.close()
hits = int(gs.memory_stats()["alloc_cache_hits"])
c = gs.Simulator(gs.Config(n=2_000_000, fanout=18, fanin=19, droprate=0.1, crashrate=0.01, seed=0x5EED))
run(c, "C", True)
run(b, "B again", False)
b.close()
c.close()
out["hits_after_a"] = int(gs.memory_stats()["alloc_cache_hits"]) - hits
out["cached"] = int(gs.memory_stats()["cached_bytes"])
print("JSON" + json.dumps(out))
"""


def test_overlapping_contexts_of_different_shapes_do_not_depend_on_the_cache():
    """A flood context (N = 4e6), a push-pull context (N = 3e6) created while
    it lives, a wide-row flood context (N = 2e6, fanout 18) created after the
    first was destroyed -- its blocks come out of the first's extents, beside
    the second's live ones -- and the second run again: every run's rows,
    status and informed count equal the same script's with every buffer a
    plain hipMalloc.  A block handed out twice or a bad split shows here."""
    runs = {}
    for mode in ("1", "0"):
        env = dict(os.environ, GS_DEVMEM_CACHE=mode)
        p = subprocess.run([sys.executable, "-c", _CHILD_OVERLAP, ROOT], capture_output=True, text=True, timeout=300,
                           env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        line = next(ln for ln in p.stdout.splitlines() if ln.startswith("JSON"))
        runs[mode] = json.loads(line[4:])
    for key in ("A", "B", "C", "B again"):
        assert runs["0"][key] == runs["1"][key], key
        assert runs["1"][key]["recv"] > 0
    assert runs["1"]["B"] == runs["1"]["B again"]
    assert runs["1"]["hits_after_a"] > 0, "nothing came from the cache after the first context was destroyed"
    assert runs["0"]["hits_after_a"] == 0 and runs["0"]["cached"] == 0 and runs["1"]["cached"] > 0


def _batch(sim):
    sim.build_overlay()
    sim.broadcast_begin(-1)
    sim.run(poll=10)
    return sim.trial_results()


def test_four_member_batch_renumbered_matches_fresh_contexts(gs):
    """400 trials of N = 1e5 over four members on device 0 (1e7 node slots a
    member), renumbered twice with gs_reset + gs_set_trial: each batch equals
    a fresh four-member context and a one-member context of the same trials.
    The members regrow their buffers while the others' streams run -- the
    path gs_dev_free's device-wide wait protects.  The device allocations of
    each renumbered batch are printed (DESIGN.md section 9 quotes them); that
    they are not zero is known and not asserted here."""
    n, T = 100_000, 400
    c = dict(n=n, fanout=5, fanin=6, droprate=0.1, crashrate=0.001, seed=0x5EED)
    with gs.Simulator(gs.Config(trial=0, trials=T, **c), devices=[0, 0, 0, 0]) as sim:
        first = _batch(sim)
        assert list(first[:, 0]) == list(range(T))
        for b in (T, 2 * T):
            before = allocs(gs)
            sim.reset()
            sim.set_trial(b)
            got = _batch(sim)
            after = allocs(gs)
            print(f"four members, batch at trial {b}: alloc_calls +{after[0] - before[0]}, "
                  f"alloc_cache_hits +{after[1] - before[1]}")
            assert list(got[:, 0]) == list(range(b, b + T))
            with gs.Simulator(gs.Config(trial=b, trials=T, **c), devices=[0, 0, 0, 0]) as fresh:
                assert np.array_equal(got, _batch(fresh)), f"batch at trial {b} vs a fresh four-member context"
            with gs.Simulator(gs.Config(trial=b, trials=T, **c)) as one:
                assert np.array_equal(got, _batch(one)), f"batch at trial {b} vs a one-member context"
    with gs.Simulator(gs.Config(trial=0, trials=T, **c)) as one:
        assert np.array_equal(first, _batch(one))


def test_trim_accounting(gs):
    """With no context alive every slab is fully free: gs_trim returns exactly
    the cached bytes, leaves none, and a second trim returns 0; a context
    created afterwards maps its blocks anew and computes the same."""
    cfg = gs.Config(n=2_000_000, fanout=5, fanin=6, droprate=0.1, crashrate=0.01, seed=0x5EED)

    def run():
        with gs.Simulator(cfg) as sim:
            sim.build_overlay()
            sim.broadcast_begin(-1)
            rows, status = sim.run(poll=10)
            return np.asarray(rows), status, sim.received()

    a = run()
    gc.collect()  # a context an earlier test dropped without closing
    cached = int(gs.memory_stats()["cached_bytes"])
    assert cached > 0
    assert gs.trim() == cached
    assert int(gs.memory_stats()["cached_bytes"]) == 0
    assert gs.trim() == 0
    calls0, _ = allocs(gs)
    b = run()
    assert allocs(gs)[0] > calls0, "no hipMalloc after everything was trimmed"
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
