"""Batched Monte Carlo trials of the median-counter model (gs_create_batch;
DESIGN.md section 4.8.1; gs_median_trials.hip), the part that needs no GPU:
the LDS plan of gs_mdt_plan.h under the host compiler, the two new symbols,
what gs_create_batch answers before it reaches a device, and the CLI's way to
it.  The rounds themselves are pinned in tests/test_median_trials_gpu.py.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from test_rumor import ROOT, cli

CSRC = os.path.join(ROOT, "gossip_simulator_amd", "csrc")
NEW = ("gs_create_batch", "gs_median_trials_max_n")

PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "gs_mdt_plan.h"
using namespace gs;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  const unsigned long long big = 1ull << 40;
  CHECK(kMdtScratchBytes == 320 && kMdtWordBytes == 336 && kMdtCounters == 5 && kMdtMaxBlock == 1024);
  // per 64 nodes: 64 state bytes, 64 signed words, two bitset words; then 320 B of reduction scratch
  CHECK(mdt_plan(1, big).lds_bytes == 336 + 320 && mdt_plan(64, big).lds_bytes == 336 + 320);
  CHECK(mdt_plan(65, big).lds_bytes == 2 * 336 + 320 && mdt_plan(4133, big).lds_bytes == 65 * 336 + 320);
  CHECK(!mdt_plan(0, big).fits);
  const unsigned long long limits[] = {65536, 163840, 320 + 336, 1000};
  for (unsigned long long lim : limits) {
    const unsigned long long m = mdt_max_n(lim);
    CHECK(m >= 64 && m % 64 == 0);
    CHECK(mdt_plan(m, lim).fits && mdt_plan(m, lim).lds_bytes <= lim);
    CHECK(!mdt_plan(m + 1, lim).fits && !mdt_plan(m + 64, lim).fits);
    CHECK(mdt_plan(m + 64, lim).lds_bytes > lim);
  }
  CHECK(mdt_max_n(320 + 336 - 1) == 0 && mdt_max_n(0) == 0);  // not even one word
  CHECK(mdt_max_n(65536) == (65536 - 320) / 336 * 64 && mdt_max_n(163840) == (163840 - 320) / 336 * 64);
  CHECK(mdt_max_n(65536) == 12416 && mdt_max_n(163840) == 31104);
  CHECK(mdt_max_n(163840) < 50000);  // the reference's default n does not fit
  // every n at both limits: the bytes, the fit, the limit and the layout agree
  for (int q = 0; q < 2; ++q) {
    const unsigned long long lim = limits[q], m = mdt_max_n(lim);
    for (unsigned long long n = 1; n <= 200000; ++n) {
      const MdtPlan p = mdt_plan(n, lim);
      const unsigned long long W = (n + 63) / 64;
      CHECK(p.words == W && p.lds_bytes == W * 336 + 320);
      CHECK(p.fits == (p.lds_bytes <= lim) && p.fits == (n <= m));
      // the arrays: [offset, offset + bytes), in ascending order, back to back, none overlapping
      const unsigned long long off[5] = {p.off_diff, p.off_gotb, p.off_gotc, p.off_scratch, p.off_st};
      const unsigned long long len[5] = {256 * W, 8 * W, 8 * W, 320, 64 * W};
      CHECK(off[0] == 0);
      for (int i = 0; i < 4; ++i) CHECK(off[i] + len[i] <= off[i + 1]);
      CHECK(off[4] + len[4] <= p.lds_bytes);
      CHECK(p.off_diff % 4 == 0 && p.off_scratch % 4 == 0);
      CHECK(p.off_gotb % 8 == 0 && p.off_gotc % 8 == 0);
      CHECK(p.off_st % 8 == 0);   // the state bytes are loaded and stored as 8-byte words
      CHECK(64 * W >= n);         // a byte and a word per node
      CHECK(p.block >= 64 && p.block <= 1024 && (p.block & (p.block - 1)) == 0);
      CHECK(p.block == 1024 || (unsigned long long)p.block * 16 >= n);
      CHECK(p.block == 64 || (unsigned long long)(p.block / 2) * 16 < n);  // the smallest such
    }
  }
  CHECK(mdt_plan(1, big).block == 64 && mdt_plan(1024, big).block == 64 && mdt_plan(1025, big).block == 128);
  CHECK(mdt_plan(8192, big).block == 512 && mdt_plan(8193, big).block == 1024 && mdt_plan(31104, big).block == 1024);
  std::printf("ok\n");
  return 0;
}
"""


def test_plan_header_on_the_host(tmp_path):
    """gs_mdt_plan.h alone under the host compiler, as a stand-alone sanitized program."""
    assert shutil.which("g++"), "g++ is needed to build the plan check"
    src = tmp_path / "mdt_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "mdt_plan_main")
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
    with open(os.path.join(CSRC, "gs_mdt_plan.h")) as f:
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
    assert L.gs_version() == 6 and "#define GS_ABI_VERSION 6" in hdr
    assert C.sizeof(_lib.Params) == 112          # gs_params got no new field
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert all(name in doc for name in NEW + ("median_batch", "-batch"))
    import gossip_simulator_amd as gs
    assert callable(gs.Simulator.median_batch) and callable(gs.median_trials_max_n)


BASE = dict(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1)


def create(fn, **kw):
    from gossip_simulator_amd import _lib
    L = _lib.load()
    p = _lib.Params(**dict(BASE, **kw))
    h = C.c_void_p()
    rc = getattr(L, fn)(C.byref(p), C.byref(h))
    why = L.gs_last_error(None).decode()
    if rc == _lib.GS_OK:
        L.gs_destroy(h)
    else:
        assert not h.value
    return rc, why


def test_create_batch_checks_the_parameters_before_the_device():
    from gossip_simulator_amd import _lib
    for kw, word in ((dict(model=3, rumor_k=0, trials=3), "rumor_k"), (dict(model=3, rumor_k=128, trials=3), "rumor_k"),
                     (dict(model=3, rumor_k=2, trials=1 << 17), "2^31"),             # 2^17 << 14
                     (dict(model=3, n=70_000, rumor_k=2, trials=1 << 14), "2^31"),   # 2^14 << 17
                     (dict(model=3, n=0, rumor_k=2, trials=3), "n must be >= 1"),
                     (dict(model=3, rumor_k=0, trials=1), "rumor_k")):               # one trial: gs_create's checks
        rc, why = create("gs_create_batch", **kw)
        assert rc == _lib.GS_EINVAL and word in why, (kw, rc, why)
    # valid parameters get past the checks: with no device visible that is GS_EDEVICE, never GS_EINVAL
    for kw in (dict(model=3, rumor_k=2, trials=3), dict(model=3, rumor_k=127, trials=2), dict(model=3, rumor_k=2)):
        rc, why = create("gs_create_batch", **kw)
        assert rc != _lib.GS_EINVAL, (kw, why)
        if rc != _lib.GS_OK:
            assert rc == _lib.GS_EDEVICE and why and "trials > 1" not in why, (kw, rc, why)


def test_create_batch_is_create_trials_for_the_other_models():
    """A rumor batch, a flood config and their bad parameters: the same answers from both creates."""
    for kw in (dict(model=2, rumor_k=2, trials=3), dict(model=2, rumor_k=0, trials=3),
               dict(model=2, rumor_k=2, rumor_mode=8, trials=3), dict(model=0), dict(model=0, trials=3),
               dict(model=0, delay_high=5), dict(model=1, trials=2), dict(model=4)):
        a, b = create("gs_create_trials", **kw), create("gs_create_batch", **kw)
        assert a == b, (kw, a, b)


def test_the_other_creates_keep_their_refusals():
    from gossip_simulator_amd import _lib
    for fn in ("gs_create", "gs_create_trials"):
        rc, why = create(fn, model=3, rumor_k=2, trials=2)
        assert rc == _lib.GS_EINVAL and "GS_MODEL_MEDIAN" in why, (fn, rc, why)
    rc, why = create("gs_create_trials", model=3, rumor_k=2, trials=1)
    assert rc == _lib.GS_EINVAL and "GS_MODEL_MEDIAN" in why


def test_max_n_query_checks_its_arguments():
    from gossip_simulator_amd import _lib
    L = _lib.load()
    out = C.c_uint64(7)
    assert L.gs_median_trials_max_n(0, None) == _lib.GS_EINVAL
    assert L.gs_median_trials_max_n(-1, C.byref(out)) == _lib.GS_EDEVICE and out.value == 0
    assert L.gs_last_error(None).decode()
    out = C.c_uint64(7)
    rc = L.gs_median_trials_max_n(0, C.byref(out))   # no device here: it cannot be asked
    assert rc in (_lib.GS_OK, _lib.GS_EDEVICE) and (out.value == 0) == (rc != _lib.GS_OK)


@pytest.mark.parametrize("args,word", [(("-batch", "4", "-model", "rumor"), "needs -model median"),
                                       (("-batch", "4"), "needs -model median"),
                                       (("-batch", "0", "-model", "median"), 'invalid value "0" for flag -batch'),
                                       (("-batch", "x", "-model", "median"), 'invalid value "x" for flag -batch')])
def test_cli_rejects_a_bad_batch_before_any_device_call(args, word):
    r = cli("-n", "4133", *args)
    assert r.returncode == 2 and word in r.stderr, r.stderr
    assert r.stdout == ""  # not even the parameter echo


def test_cli_keeps_refusing_trials_with_the_median_model():
    r = cli("-n", "1000", "-model", "median", "-trials", "2")
    assert r.returncode == 2 and "-trials" in r.stderr and "GS_MODEL_MEDIAN" in r.stderr and r.stdout == ""


def test_cli_batch_reaches_the_create():
    """With no device visible (cli hides them) the run fails at the device, after the parameter echo,
    which has no -batch."""
    r = cli("-n", "4133", "-model", "median", "-batch", "4")
    assert r.returncode == 1 and "failed" in r.stderr, r.stderr
    assert "one trial" not in r.stderr and "needs -model" not in r.stderr
    assert r.stdout.startswith("=== Parameters ===\n") and "batch" not in r.stdout
    assert "Constructing Overlay" not in r.stdout
    r = cli("-h")
    assert re.search(r"^  -batch int$", r.stderr, re.M)
