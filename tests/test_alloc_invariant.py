"""The product allocates device memory with hipMalloc only -- never from the
stream-ordered pool (verdict r04, Weak 5 / item 3).

Round 4 moved the overlay's event buckets (gs_overlay.hip overlay_build:
one multi-GB bucket per ring block, regrown by allocate -> hipMemcpyAsync of
the filled prefix -> free) to hipMallocAsync / hipFreeAsync.  The N = 1e9
build then failed with "too many overlay events at one node in one tick":
k_process (gs_overlay.hip, err bit 2) met a run of > 2^26 events with one
destination, i.e. bucket words no scatter had written.  The builder's
buffer lifetimes are stream-ordered and correct (every pointer the device
reads is refreshed after a regrow or the sort's double-buffer swap, and the
host arrays are rewritten only after a stream sync); the cause is the pool
itself: scripts/micro/pool_repro.hip replays only the allocation pattern
(six buckets, 1.5x regrows with a hipMemcpyAsync of the filled prefix, a
swapped scratch buffer) and checks every word.  On an MI355X with ROCm 7.2
(profiles/r05a_pool_repro.txt, profiles/r05c_pool_repro.txt):

* hipMalloc / hipFree, 5 GiB buckets: every word intact;
* pool, 1 GiB buckets: every word intact;
* pool, 5 GiB buckets: after the first regrow round three of six regrown
  buckets read back zeros or ANOTHER bucket's earlier contents (bucket 3
  held bucket 0's generation-3 pattern): pool allocations of several GiB
  alias memory that is still live, or the copy into them is lost.

So the invariant is: no product source uses the stream-ordered allocator.
(The reproducer under scripts/micro/ is not product code.)
"""
from __future__ import annotations

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = [os.path.join(ROOT, "gossip_simulator_amd", "csrc"), os.path.join(ROOT, "include")]
POOL_APIS = re.compile(r"\b(hipMallocAsync|hipFreeAsync|hipMallocFromPoolAsync|hipMemPoolCreate|"
                       r"hipDeviceGetDefaultMemPool|hipDeviceSetMemPool|hipMemPoolSetAttribute)\b")


def _sources():
    for d in PRODUCT:
        for dirpath, _dirs, files in os.walk(d):
            for f in files:
                if f.endswith((".hip", ".cpp", ".h", ".hpp", ".cc")):
                    yield os.path.join(dirpath, f)


def _code(text):
    """The text without comments (a comment may name the pool APIs)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_product_never_uses_the_stream_ordered_pool():
    hits = []
    for path in _sources():
        with open(path, encoding="utf-8", errors="replace") as f:
            for m in POOL_APIS.finditer(_code(f.read())):
                hits.append(f"{os.path.relpath(path, ROOT)}: {m.group(1)}")
    assert not hits, "stream-ordered pool allocations in the product:\n" + "\n".join(hits)


def test_the_scan_sees_every_product_source():
    names = {os.path.basename(p) for p in _sources()}
    for must in ("gs_overlay.hip", "gs_win_units.hip", "gs_win_expand.hip", "gs_win_part.hip", "gs_win_resolve.hip",
                 "gs_win_shard.hip", "gs_win_dev.h", "gs_wave.h", "gs_pp_dev.h", "gs_pp_dense.hip", "gs_pp_early.hip",
                 "gs_pp_round.hip", "gs_pp_defer.hip", "gs_pp_rev.hip", "gs_pp_fmask.hip", "gs_api.cpp", "gossip.h", "gs_ctx.h",
                 "gs_ctx.cpp", "gs_peers.cpp", "gs_windows.cpp", "gs_shards.cpp", "gs_pushpull_host.cpp"):
        assert must in names


def test_the_reproducer_is_committed():
    src = os.path.join(ROOT, "scripts", "micro", "pool_repro.hip")
    with open(src) as f:
        text = f.read()
    assert "hipMallocAsync" in text and "hipMemcpyAsync" in text and "POOL DEFECT REPRODUCED" in text
