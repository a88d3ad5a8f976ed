"""Packed median batches (GS_FLAG_MEDIAN_PACKED; DESIGN.md section 4.8.2;
k_mdt16_rounds in gs_median_trials.hip), the part that needs no GPU: the LDS
plan and the 16-bit field arithmetic of gs_mdt16_plan.h under the host
compiler -- the same functions the kernel compiles -- the new symbol, what
gs_create_batch answers with the flag before it reaches a device, and the
CLI's -packed.  The rounds are pinned in tests/test_median_packed_gpu.py.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

from test_median_trials import CSRC, create
from test_rumor import ROOT, cli

PACKED = 256   # GS_FLAG_MEDIAN_PACKED

PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "gs_mdt16_plan.h"
using namespace gs;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// `count` adds of `up` on node a and of the opposite sign on node b, its mate in word 0, interleaved.
static int ramp(uint32_t a, bool up, int count) {
  const uint32_t b = a ^ 1;
  uint32_t w[2] = {kMdt16Init, kMdt16Init};   // w[1]: a neighbour that nothing may reach
  CHECK(mdt16_word(a) == 0 && mdt16_word(b) == 0);
  for (int i = 1; i <= count; ++i) {
    w[0] += mdt16_delta(a, up);
    CHECK(mdt16_diff(w[0], a) == (up ? i : -i) && mdt16_diff(w[0], b) == (up ? 1 - i : i - 1));
    w[0] += mdt16_delta(b, !up);
    CHECK(mdt16_diff(w[0], a) == (up ? i : -i) && mdt16_diff(w[0], b) == (up ? -i : i));
  }
  const uint32_t fa = (w[0] >> (16 * (a & 1))) & 0xFFFF, fb = (w[0] >> (16 * (b & 1))) & 0xFFFF;
  CHECK(fa == (up ? 0x8000u + count : 0x8000u - count) && fb == (up ? 0x8000u - count : 0x8000u + count));
  CHECK(w[1] == kMdt16Init);
  // the commit's read-and-clear of one half leaves the other as it is
  const uint32_t before = w[0];
  CHECK(mdt16_take(w, a) == (up ? count : -count));
  CHECK(mdt16_diff(w[0], a) == 0 && mdt16_diff(w[0], b) == (up ? -count : count));
  CHECK((w[0] ^ before) >> (16 * (b & 1)) << 16 == 0);   // b's 16 bits untouched
  CHECK(mdt16_take(w, a) == 0 && mdt16_take(w, b) == (up ? -count : count));
  CHECK(w[0] == kMdt16Init && w[1] == kMdt16Init);
  return 0;
}

int main() {
  const unsigned long long big = 1ull << 40;
  CHECK(kMdt16WordBytes == 208 && kMdtScratchBytes == 320 && kMdt16MaxDiff == 32767 && kMdt16MaxNamed == 32766);
  CHECK(kMdt16Init == 0x80008000u && kMdt16Bias == 0x8000 && kMdt16MaxN == 50304);
  CHECK(kMdtWordBytes == 336 && mdt_max_n(163840) == 31104);   // the unpacked plan is as it was
  CHECK(mdt16_plan(1, big).lds_bytes == 208 + 320 && mdt16_plan(64, big).lds_bytes == 208 + 320);
  CHECK(mdt16_plan(65, big).lds_bytes == 2 * 208 + 320 && mdt16_plan(4133, big).lds_bytes == 65 * 208 + 320);
  CHECK(!mdt16_plan(0, big).fits);
  CHECK(mdt16_max_n(65536) == 20032 && mdt16_max_n(163840) == 50304 && mdt16_max_n(163840) >= 50000);
  CHECK(mdt16_max_n(320 + 208 - 1) == 0 && mdt16_max_n(320 + 208) == 64 && mdt16_max_n(0) == 0);
  const unsigned long long limits[] = {65536, 163840};
  for (unsigned long long lim : limits) {
    const unsigned long long m = mdt16_max_n(lim);
    for (unsigned long long n = 1; n <= 200000; ++n) {   // every n around both limits
      const MdtPlan p = mdt16_plan(n, lim);
      const unsigned long long W = (n + 63) / 64;
      CHECK(p.words == W && p.lds_bytes == W * 208 + 320);
      CHECK(p.fits == (p.lds_bytes <= lim) && p.fits == (n <= m));
      const unsigned long long off[5] = {p.off_diff, p.off_gotb, p.off_gotc, p.off_scratch, p.off_st};
      const unsigned long long len[5] = {128 * W, 8 * W, 8 * W, 320, 64 * W};
      CHECK(off[0] == 0);
      for (int i = 0; i < 4; ++i) CHECK(off[i] + len[i] == off[i + 1]);
      CHECK(off[4] + len[4] == p.lds_bytes);
      for (int i = 0; i < 5; ++i) CHECK(off[i] % 8 == 0);
      CHECK(2 * 64 * W >= 2 * n);   // a 16-bit field per node
      const MdtPlan q = mdt_plan(n, big);
      CHECK(p.block == q.block);    // the block rule is gs_trial_plan.h's
      CHECK(p.block >= 64 && p.block <= 1024 && (p.block & (p.block - 1)) == 0);
      CHECK(p.block == 1024 || (unsigned long long)p.block * 16 >= n);
      CHECK(p.block == 64 || (unsigned long long)(p.block / 2) * 16 < n);
    }
  }
  CHECK(mdt16_plan(1024, big).block == 64 && mdt16_plan(1025, big).block == 128 && mdt16_plan(50304, big).block == 1024);

  // the fields: +-32,767 on either half with the opposite sign on the other, interleaved
  for (uint32_t a = 0; a < 2; ++a)
    for (int up = 0; up < 2; ++up)
      if (ramp(a, up != 0, 32767)) return 1;
  // a delta is one add to the node's own word; node v is the u16 at index v
  uint32_t w[4] = {kMdt16Init, kMdt16Init, kMdt16Init, kMdt16Init};
  for (uint32_t v = 0; v < 8; ++v) w[mdt16_word(v)] += mdt16_delta(v, (v & 2) != 0);
  for (uint32_t v = 0; v < 8; ++v) CHECK(mdt16_diff(w[v >> 1], v) == ((v & 2) ? 1 : -1));
  for (uint32_t v = 0; v < 8; ++v) {
    CHECK(((const mdt16_half_t*)w)[v] == ((v & 2) ? 0x8001 : 0x7FFF));
    CHECK(mdt16_take(w, v) == ((v & 2) ? 1 : -1));
  }
  for (int i = 0; i < 4; ++i) CHECK(w[i] == kMdt16Init);
  std::printf("ok\n");
  return 0;
}
"""


def test_plan_and_fields_on_the_host(tmp_path):
    """gs_mdt16_plan.h alone under the host compiler, as a stand-alone sanitized program."""
    assert shutil.which("g++"), "g++ is needed to build the plan check"
    src = tmp_path / "mdt16_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "mdt16_plan_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr or "unsupported" in r.stderr):
        r = subprocess.run(base, capture_output=True, text=True)  # no sanitizer runtime on this toolchain
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_plan_header_includes_no_hip():
    with open(os.path.join(CSRC, "gs_mdt16_plan.h")) as f:
        text = f.read()
    assert re.findall(r"^#include\s+(\S+)", text, re.M) == ["<cstdint>", '"gs_mdt_plan.h"']
    # the kernel file compiles these very functions
    with open(os.path.join(CSRC, "gs_median_trials.hip")) as f:
        hip = f.read()
    assert '#include "gs_mdt16_plan.h"' in hip
    assert all(name in hip for name in ("mdt16_word(", "mdt16_delta(", "mdt16_take(", "kMdt16Init"))
    assert "asm" not in hip


def test_new_symbol_is_declared_bound_and_exported():
    from gossip_simulator_amd import _lib
    import gossip_simulator_amd as gs
    with open(os.path.join(ROOT, "include", "gossip.h")) as f:
        hdr = f.read()
    L = _lib.load()
    name = "gs_median_trials_max_n_packed"
    assert re.search(rf"^int {name}\(int device, uint64_t\* n_max\);", hdr, re.M)
    assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert re.search(r"#define GS_FLAG_MEDIAN_PACKED 256u\b", hdr) and _lib.GS_FLAG_MEDIAN_PACKED == PACKED
    assert L.gs_version() == 6 and "#define GS_ABI_VERSION 6" in hdr and C.sizeof(_lib.Params) == 112
    assert gs.Config().median_packed is False and gs.Config().flags() & PACKED == 0
    assert gs.Config(median_packed=True).flags() & PACKED and gs.Config(median_packed=True).to_params().flags == PACKED
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert all(w in doc for w in (name, "GS_FLAG_MEDIAN_PACKED", "median_packed", "-packed"))
    with open(os.path.join(ROOT, "go", "simulator_hip.go")) as f:
        assert name in f.read()


def test_max_n_packed_query_checks_its_arguments():
    from gossip_simulator_amd import _lib
    L = _lib.load()
    out = C.c_uint64(7)
    assert L.gs_median_trials_max_n_packed(0, None) == _lib.GS_EINVAL
    assert L.gs_median_trials_max_n_packed(-1, C.byref(out)) == _lib.GS_EDEVICE and out.value == 0
    assert L.gs_last_error(None).decode()
    out = C.c_uint64(7)
    rc = L.gs_median_trials_max_n_packed(0, C.byref(out))   # no device here: it cannot be asked
    assert rc in (_lib.GS_OK, _lib.GS_EDEVICE) and (out.value == 0) == (rc != _lib.GS_OK)


def test_create_batch_with_the_flag_checks_the_parameters_before_the_device():
    from gossip_simulator_amd import _lib
    for k in (0, 128):
        rc, why = create("gs_create_batch", model=3, rumor_k=k, trials=3, flags=PACKED)
        assert rc == _lib.GS_EINVAL and "rumor_k" in why, (k, rc, why)
    for kw in (dict(model=3, rumor_k=2, trials=3), dict(model=3, n=50_000, rumor_k=5, trials=2)):
        rc, why = create("gs_create_batch", flags=PACKED, **kw)
        assert rc != _lib.GS_EINVAL, (kw, why)
        if rc != _lib.GS_OK:
            assert rc == _lib.GS_EDEVICE and why, (kw, rc, why)


def test_the_other_creates_and_models_do_not_look_at_the_flag():
    from gossip_simulator_amd import _lib
    for fn in ("gs_create", "gs_create_trials"):
        rc, why = create(fn, model=3, rumor_k=2, trials=2, flags=PACKED)
        assert rc == _lib.GS_EINVAL and "GS_MODEL_MEDIAN" in why, (fn, rc, why)
    # the same answers with the bit as without it
    for fn, kw in (("gs_create", dict(model=0)), ("gs_create", dict(model=3, rumor_k=2)),
                   ("gs_create_trials", dict(model=2, rumor_k=2, trials=3)),
                   ("gs_create_trials", dict(model=2, rumor_k=0, trials=3)),
                   ("gs_create_batch", dict(model=2, rumor_k=2, trials=3)), ("gs_create_batch", dict(model=1, trials=2)),
                   ("gs_create_batch", dict(model=3, rumor_k=2, trials=1)), ("gs_create_batch", dict(model=4))):
        assert create(fn, **kw) == create(fn, flags=PACKED, **kw), (fn, kw)


def test_cli_packed_needs_batch():
    for args in (("-model", "median", "-packed"), ("-packed",), ("-model", "rumor", "-packed")):
        r = cli("-n", "4133", *args)
        assert r.returncode == 2 and "-packed needs -batch" in r.stderr, r.stderr
        assert r.stdout == ""   # not even the parameter echo
    r = cli("-n", "4133", "-model", "median", "-batch", "4", "-packed")   # reaches the create: no device here
    assert r.returncode == 1 and "failed" in r.stderr and "needs -" not in r.stderr, r.stderr
    assert r.stdout.startswith("=== Parameters ===\n") and "packed" not in r.stdout
    r = cli("-h")
    assert re.search(r"^  -packed$", r.stderr, re.M) and re.search(r"^  -batch int$", r.stderr, re.M)
