"""The device-block cache's bookkeeping (gs_devmem.cpp) and the reverse-table
pass planner (gs_rev_plan.h), on the CPU, against plain models.

tests/devmem_harness.cpp is compiled together with the product's
gs_devmem.cpp, unchanged, and defines the eight HIP entry points that file
calls itself (hipMemset among them, for GS_DEVMEM_POISON): a fake driver with
three devices of 288 GB, a table of live allocations and a log of every call.  Nothing backs the addresses, so every
path can be driven exactly, including the ones whose failure on a device is a
fault: double frees, a device with no room, trimming.

One sanitized executable (-fsanitize=address,undefined) runs every scenario,
each in a fresh process (GS_DEVMEM_CACHE is read once per process); a second
one (-fsanitize=thread) runs the threaded scenario.  They are ordinary
programs: nothing is preloaded.

* random:<seed> -- 2,000 random malloc / free / device switch / trim / largest
  operations; before each request a naive model predicts the class of the
  outcome (plain, hit and the extent's size, new slab, which slabs are trimmed
  first, failure) and after it the driver's log, gs_devmem_stats,
  gs_devmem_largest and the blocks' placement are checked; at the end one
  trim returns every mapped byte;
* the directed scenarios are named after what they pin (see the harness).
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip_simulator_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "devmem_harness.cpp")

SEEDS = list(range(1, 21))
DIRECTED = ["double_free", "picky_best_fit", "no_room", "trim_to_fit", "margin", "bypass_small", "devices",
            "split_coalesce", "planner"]


def _rocm_include():
    for base in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if base and os.path.exists(os.path.join(base, "include", "hip", "hip_runtime.h")):
            return os.path.join(base, "include")
    return None


def _command(out, sanitize):
    inc = _rocm_include()
    assert inc, "no ROCm headers (hip/hip_runtime.h) under ROCM_PATH or /opt/rocm"
    return ["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={sanitize}", "-fno-omit-frame-pointer",
            "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", CSRC, "-o", out, HARNESS,
            os.path.join(CSRC, "gs_devmem.cpp"), "-pthread"]


def _runtime_missing(returncode, err):
    """A link that fails for want of the sanitizer's runtime library."""
    return returncode != 0 and ("cannot find" in err or "unsupported option" in err or "unrecognized" in err)


@pytest.fixture(scope="session")
def _builds(tmp_path_factory):
    """Both executables, compiled side by side (the compile is most of this
    module's time).  The sanitizer's runtime is linked into the executable
    where the toolchain has the static one -- the program then does not care
    what else the loader brings in -- else the shared one."""
    assert shutil.which("g++"), "g++ is needed to build the allocator harness"
    d = tmp_path_factory.mktemp("devmem")
    jobs = {"asan": (str(d / "devmem_harness"), "address,undefined", ["-static-libasan", "-static-libubsan"]),
            "tsan": (str(d / "devmem_harness_tsan"), "thread", ["-static-libtsan"])}
    procs = {k: subprocess.Popen(_command(out, san) + static, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, (out, san, static) in jobs.items()}
    res = {}
    for k, (out, san, static) in jobs.items():
        _, err = procs[k].communicate(timeout=600)
        rc = procs[k].returncode
        if _runtime_missing(rc, err):  # no static runtime: the shared one
            p = subprocess.run(_command(out, san), capture_output=True, text=True, timeout=600)
            rc, err = p.returncode, p.stderr
        res[k] = (out, rc, err)
    return res


@pytest.fixture(scope="session")
def harness(_builds):
    out, rc, err = _builds["asan"]
    assert rc == 0, err[-4000:]
    return out


@pytest.fixture(scope="session")
def harness_tsan(_builds):
    out, rc, err = _builds["tsan"]
    if _runtime_missing(rc, err):
        pytest.skip("the toolchain has no ThreadSanitizer runtime: " + err.strip().splitlines()[-1])
    assert rc == 0, err[-4000:]
    return out


def run(exe, scenario, cache=None, poison=None):
    env = {k: v for k, v in os.environ.items() if k not in ("GS_DEVMEM_CACHE", "GS_DEVMEM_LOG", "GS_DEVMEM_POISON")}
    if cache is not None:
        env["GS_DEVMEM_CACHE"] = cache
    if poison is not None:
        env["GS_DEVMEM_POISON"] = poison
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"  # the cache and the fake driver live until exit
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    env["TSAN_OPTIONS"] = "halt_on_error=1"
    p = subprocess.run([exe, scenario], capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, f"{scenario}: no result line (exit {p.returncode})\n{p.stderr[-4000:]}"
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res["ok"], f"{scenario}: exit {p.returncode}: {res}\n{p.stderr[-4000:]}"
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    res["stderr"] = p.stderr
    return res


_seen: dict = {}


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequence_matches_the_model(harness, seed):
    res = run(harness, f"random:{seed}")
    for k, v in res["seen"].items():
        _seen[k] = _seen.get(k, 0) + v


def test_random_sequences_met_every_class_of_outcome(harness):
    """The 20 sequences together take every path the model distinguishes, so
    none of them is pinned by the directed scenarios alone."""
    if len(_seen) == 0:  # run alone: the sequences have not run in this session
        for seed in SEEDS:
            for k, v in run(harness, f"random:{seed}")["seen"].items():
                _seen[k] = _seen.get(k, 0) + v
    for cls in ("plain", "plain_fail", "hit", "hit_relaxed", "new_slab", "new_slab_after_trim", "fail",
                "free_headroom_trim", "largest_cached", "largest_new"):
        assert _seen.get(cls, 0) > 0, f"no {cls} in {sorted(_seen.items())}"


@pytest.mark.parametrize("seed", [1, 2])
def test_random_sequence_with_the_cache_off(harness, seed):
    res = run(harness, f"random:{seed}", cache="0")
    assert set(res["seen"]) <= {"plain", "plain_fail", "largest_new"}, res


@pytest.mark.parametrize("scenario", DIRECTED)
def test_directed(harness, scenario):
    run(harness, scenario)


def test_bypass_with_the_cache_off(harness):
    run(harness, "bypass_off", cache="0")


@pytest.mark.parametrize("byte", ["0xFF", "1", "0x7f"])
def test_poison_fills_every_block_handed_out(harness, byte):
    """GS_DEVMEM_POISON: plain, hit after a split, new slab and both fallbacks
    are each followed by one fill of the whole block and one sync; a failed
    fill is the request's error and leaves no block behind."""
    res = run(harness, "poison", poison=byte)
    assert res["stderr"].count("[devmem] poison 0x%02X\n" % int(byte, 0)) == 1, res["stderr"][-2000:]


@pytest.mark.parametrize("seed", [1, 2])
def test_random_sequence_poisoned(harness, seed):
    """The same sequences with the switch on: every block handed out is
    filled, whatever path served it."""
    res = run(harness, f"random:{seed}", poison="0x01")
    assert res["seen"].get("hit", 0) and res["seen"].get("new_slab", 0) and res["seen"].get("plain", 0)


@pytest.mark.parametrize("value", [None, "0", "256", "-1", "0x100", "ff", "1x", ""])
def test_poison_off_logs_no_fill(harness, value):
    """Unset, or out of range, or not a number: no fill on any path, in the
    directed requests and in a random run."""
    for scenario in ("poison_off", "random:3", "no_room", "split_coalesce") if value is None else ("poison_off",):
        res = run(harness, scenario, poison=value)
        assert "[devmem] poison" not in res["stderr"]


def test_threads_asan(harness):
    res = run(harness, "threads")
    assert res["seen"]["cache_hits"] > 0


def test_threads_tsan(harness_tsan):
    res = run(harness_tsan, "threads")
    assert res["seen"]["cache_hits"] > 0
