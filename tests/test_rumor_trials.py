"""Batched Monte Carlo trials of the rumor model (gs_create_trials; DESIGN.md
section 4.7.2; gs_rumor_trials.hip), the part that needs no GPU: the LDS plan
of gs_rmt_plan.h under the host compiler, the two new symbols, what
gs_create_trials answers before it reaches a device, and the CLI's way to it.
The rounds themselves are pinned in tests/test_rumor_trials_gpu.py.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

from test_rumor import ROOT, cli

CSRC = os.path.join(ROOT, "gossip_simulator_amd", "csrc")
NEW = ("gs_create_trials", "gs_rumor_trials_max_n")

PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "gs_rmt_plan.h"
using namespace gs;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  const unsigned long long big = 1ull << 40;
  const unsigned BLIND = 1, COIN = 2, PULL = 4;
  CHECK(kRmtScratchBytes == 320);
  // bitsets of ceil(n / 64) 8-byte words + 320 B of reduction scratch + 64 miss bytes per word
  CHECK(rmt_plan(1, 0, big).lds_bytes == 3 * 8 + 320 + 64);              // push, counter: cur, next, hot, miss
  CHECK(rmt_plan(1, BLIND, big).lds_bytes == 3 * 8 + 320 + 64);
  CHECK(rmt_plan(1, COIN, big).lds_bytes == 3 * 8 + 320);                // push, coin: no miss
  CHECK(rmt_plan(1, COIN | BLIND, big).lds_bytes == 3 * 8 + 320);
  CHECK(rmt_plan(1, PULL, big).lds_bytes == 5 * 8 + 320 + 64);           // feedback pull: + served, vain
  CHECK(rmt_plan(1, PULL | COIN, big).lds_bytes == 5 * 8 + 320);
  CHECK(rmt_plan(1, PULL | BLIND, big).lds_bytes == 3 * 8 + 320 + 64);   // blind pull: cur, next, hot
  CHECK(rmt_plan(1, PULL | BLIND | COIN, big).lds_bytes == 3 * 8 + 320);
  CHECK(rmt_plan(64, 0, big).lds_bytes == 88 + 320 && rmt_plan(65, 0, big).lds_bytes == 2 * 88 + 320);
  CHECK(rmt_plan(16385, PULL, big).lds_bytes == 257 * 104 + 320);
  CHECK(!rmt_plan(0, 0, big).fits);
  for (unsigned mode = 0; mode < 8; ++mode) {
    const unsigned long long per = rmt_word_bytes(mode);
    CHECK(per == rmt_bitsets(mode) * 8ull + (rmt_has_miss(mode) ? 64 : 0));
    CHECK(rmt_bitsets(mode) == ((mode & PULL) && !(mode & BLIND) ? 5u : 3u) && rmt_has_miss(mode) == !(mode & COIN));
    const unsigned long long limits[] = {65536, 163840, 320 + per, 1000};
    for (unsigned long long lim : limits) {
      const unsigned long long m = rmt_max_n(mode, lim);
      CHECK(m >= 64 && m % 64 == 0);
      CHECK(rmt_plan(m, mode, lim).fits && rmt_plan(m, mode, lim).lds_bytes <= lim);
      CHECK(!rmt_plan(m + 1, mode, lim).fits && !rmt_plan(m + 64, mode, lim).fits);
      CHECK(rmt_plan(m + 64, mode, lim).lds_bytes > lim);
    }
    CHECK(rmt_max_n(mode, 320 + per - 1) == 0 && rmt_max_n(mode, 0) == 0);  // not even one word
    // every n: the bytes, the fit and the limit agree
    for (int q = 0; q < 2; ++q) {
      const unsigned long long lim = limits[q];
      const unsigned long long m = rmt_max_n(mode, lim);
      for (unsigned long long n = 1; n <= 200000; ++n) {
        const RmtPlan p = rmt_plan(n, mode, lim);
        CHECK(p.words == (n + 63) / 64 && p.bitsets == rmt_bitsets(mode));
        CHECK(p.miss_bytes == (rmt_has_miss(mode) ? 64 * p.words : 0));
        CHECK(p.lds_bytes == p.words * per + 320);
        CHECK(p.fits == (p.lds_bytes <= lim) && p.fits == (n <= m));
        CHECK(p.miss_bytes == 0 || p.miss_bytes >= n);  // a byte per node
      }
    }
  }
  CHECK(rmt_max_n(0, 163840) == (163840 - 320) / 88 * 64 && rmt_max_n(PULL, 65536) == (65536 - 320) / 104 * 64);
  // blocks: ppt_plan's rule -- whole waves, smaller for small n, at most 1024 threads
  unsigned prev = 0;
  for (unsigned long long n = 1; n <= 200000; ++n) {
    const RmtPlan p = rmt_plan(n, 0, big);
    CHECK(p.block >= 64 && p.block <= 1024 && (p.block & (p.block - 1)) == 0);
    CHECK(p.block >= prev);
    CHECK(p.block == 1024 || (unsigned long long)p.block * 16 >= n);
    CHECK(p.block == 64 || (unsigned long long)(p.block / 2) * 16 < n);  // the smallest such
    CHECK(p.block == rmt_plan(n, PULL | COIN, big).block);               // the same in every mode
    prev = p.block;
  }
  CHECK(rmt_plan(1, 0, big).block == 64 && rmt_plan(1024, 0, big).block == 64 && rmt_plan(1025, 0, big).block == 128);
  CHECK(rmt_plan(8192, 0, big).block == 512 && rmt_plan(8193, 0, big).block == 1024);
  CHECK(rmt_plan(16385, 0, big).block == 1024 && rmt_plan(20000, 0, big).block == 1024);
  std::printf("ok\n");
  return 0;
}
"""


def test_plan_header_on_the_host(tmp_path):
    """gs_rmt_plan.h alone under the host compiler, as a stand-alone sanitized program."""
    assert shutil.which("g++"), "g++ is needed to build the plan check"
    src = tmp_path / "rmt_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "rmt_plan_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr or "unsupported" in r.stderr):
        r = subprocess.run(base, capture_output=True, text=True)  # no sanitizer runtime on this toolchain
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_plan_header_includes_no_hip():
    """No HIP header is reachable: <cstdint>, and the shared plan header, which includes <cstdint> only."""
    with open(os.path.join(CSRC, "gs_rmt_plan.h")) as f:
        includes = re.findall(r"^#include\s+(\S+)", f.read(), re.M)
    assert includes == ["<cstdint>", '"gs_trial_plan.h"']
    with open(os.path.join(CSRC, "gs_trial_plan.h")) as f:
        includes = re.findall(r"^#include\s+(\S+)", f.read(), re.M)
    assert includes == ["<cstdint>"]


def test_new_symbols_are_declared_bound_and_exported():
    from gossip_simulator_amd import _lib
    with open(os.path.join(ROOT, "include", "gossip.h")) as f:
        hdr = f.read()
    L = _lib.load()
    for name in NEW:
        assert re.search(rf"^int {name}\(", hdr, re.M), name
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert all(name in doc for name in NEW)
    import gossip_simulator_amd as gs
    assert callable(gs.Simulator.batch) and callable(gs.rumor_trials_max_n)


BASE = dict(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, model=2)


def create_trials(**kw):
    from gossip_simulator_amd import _lib
    L = _lib.load()
    p = _lib.Params(**dict(BASE, **kw))
    h = C.c_void_p()
    rc = L.gs_create_trials(C.byref(p), C.byref(h))
    why = L.gs_last_error(None).decode()
    if rc == _lib.GS_OK:
        L.gs_destroy(h)
    else:
        assert not h.value
    return rc, why


def test_create_trials_checks_the_parameters_before_the_device():
    from gossip_simulator_amd import _lib
    for kw, word in ((dict(rumor_k=0, trials=3), "rumor_k"), (dict(rumor_k=256, trials=3), "rumor_k"),
                     (dict(rumor_k=2, rumor_mode=8, trials=3), "rumor_mode"),
                     (dict(rumor_k=2, trials=1 << 17), "2^31"),              # 2^17 << 14
                     (dict(n=70_000, rumor_k=2, trials=1 << 14), "2^31"),    # 2^14 << 17
                     (dict(rumor_k=0, trials=1), "rumor_k")):                # one trial: gs_create's checks
        rc, why = create_trials(**kw)
        assert rc == _lib.GS_EINVAL and word in why, (kw, rc, why)
    # valid parameters get past the checks: with no device visible that is GS_EDEVICE, never GS_EINVAL
    for kw in (dict(rumor_k=2, trials=3), dict(rumor_k=2, rumor_mode=7, trials=3), dict(rumor_k=2, trials=1)):
        rc, why = create_trials(**kw)
        assert rc != _lib.GS_EINVAL, (kw, why)
        if rc != _lib.GS_OK:
            assert rc == _lib.GS_EDEVICE and why and "trials > 1" not in why, (kw, rc, why)


def test_gs_create_keeps_its_refusal():
    """The opt-in is the new create: gs_create still answers GS_EINVAL, and says where the batch is."""
    from gossip_simulator_amd import _lib
    L = _lib.load()
    p = _lib.Params(**dict(BASE, rumor_k=2, trials=3))
    h = C.c_void_p()
    assert L.gs_create(C.byref(p), C.byref(h)) == _lib.GS_EINVAL and not h.value
    why = L.gs_last_error(None).decode()
    assert "trials" in why and "gs_create_trials" in why


def test_max_n_query_checks_its_arguments():
    from gossip_simulator_amd import _lib
    L = _lib.load()
    out = C.c_uint64(7)
    assert L.gs_rumor_trials_max_n(0, 8, C.byref(out)) == _lib.GS_EINVAL and out.value == 0
    assert "rumor_mode" in L.gs_last_error(None).decode()
    assert L.gs_rumor_trials_max_n(0, 0, None) == _lib.GS_EINVAL
    assert L.gs_rumor_trials_max_n(-1, 0, C.byref(out)) == _lib.GS_EDEVICE and out.value == 0


def test_cli_rumor_trials_reach_the_device():
    """With no device visible the run fails at the device, not with the refusal of trials > 1."""
    r = cli("-n", "4133", "-model", "rumor", "-k", "2", "-trials", "4")
    assert r.returncode == 1, r.stderr
    assert "HIP device" in r.stderr and "no HIP device visible" in r.stderr
    assert "trials > 1" not in r.stderr and "one trial per context" not in r.stderr
    assert r.stdout.startswith("=== Parameters ===\n") and "Constructing Overlay" not in r.stdout
