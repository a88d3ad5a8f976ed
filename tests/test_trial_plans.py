"""The three trial-resident LDS plans over their shared arithmetic
(gs_trial_plan.h), on the CPU: gs_ppt_plan.h,
gs_rmt_plan.h and gs_mdt_plan.h together in one stand-alone host program.
Each plan alone is pinned beside its engine (test_pushpull_trials.py,
test_rumor_trials.py, test_median_trials.py).
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

from test_rumor import ROOT

CSRC = os.path.join(ROOT, "gossip_simulator_amd", "csrc")

PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "gs_ppt_plan.h"
#include "gs_rmt_plan.h"
#include "gs_mdt_plan.h"
using namespace gs;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  const unsigned long long big = 1ull << 40;
  CHECK(kTrialMaxBlock == 1024 && kPptMaxBlock == 1024 && kRmtMaxBlock == 1024 && kMdtMaxBlock == 1024);
  CHECK(trial_scratch_bytes(4) == 256 && trial_scratch_bytes(5) == 320);
  CHECK(kPptScratchBytes == 256 && kRmtScratchBytes == 320 && kMdtScratchBytes == 320);
  // one block and one word count for the three engines
  const unsigned long long ns[] = {1, 64, 65, 1024, 1025, 8192, 8193, 16384, 16385, 100000};
  for (unsigned long long n : ns) {
    const PptPlan p = ppt_plan(n, big), pm = ppt_plan_masked(n, big);
    const MdtPlan m = mdt_plan(n, big);
    CHECK(p.block == trial_block(n) && pm.block == p.block && m.block == p.block);
    CHECK(p.words == (n + 63) / 64 && pm.words == p.words && m.words == p.words);
    for (unsigned mode = 0; mode < 8; ++mode) {
      const RmtPlan r = rmt_plan(n, mode, big);
      CHECK(r.block == p.block && r.words == p.words);
    }
  }
  // the block doubles exactly at 16 * block + 1, and not past 1024
  for (unsigned b = 64; b <= 1024; b *= 2) {
    CHECK(trial_block(16ull * b) == b && trial_block(16ull * b - 1) == b);
    CHECK(trial_block(16ull * b + 1) == (b < 1024 ? 2 * b : 1024));
  }
  CHECK(trial_block(0) == 64 && trial_block(1) == 64 && trial_block(big) == 1024);
  unsigned prev = 64;
  for (unsigned long long n = 1; n <= 20000; ++n) {
    const unsigned b = trial_block(n);
    CHECK(b == prev || (b == 2 * prev && n == 16ull * prev + 1));
    prev = b;
  }
  // the largest n fits and the next does not: every engine, every rumor mode
  const unsigned long long limits[] = {65536, 163840};
  for (unsigned long long lim : limits) {
    unsigned long long m = ppt_max_n(lim);
    CHECK(m > 0 && ppt_plan(m, lim).fits && !ppt_plan(m + 1, lim).fits);
    m = ppt_max_n_masked(lim);
    CHECK(m > 0 && ppt_plan_masked(m, lim).fits && !ppt_plan_masked(m + 1, lim).fits);
    m = mdt_max_n(lim);
    CHECK(m > 0 && mdt_plan(m, lim).fits && !mdt_plan(m + 1, lim).fits);
    for (unsigned mode = 0; mode < 8; ++mode) {
      m = rmt_max_n(mode, lim);
      CHECK(m > 0 && rmt_plan(m, mode, lim).fits && !rmt_plan(m + 1, mode, lim).fits);
      CHECK(m == trial_max_n(lim, kRmtScratchBytes, rmt_word_bytes(mode)));
    }
    CHECK(ppt_max_n(lim) == trial_max_n(lim, 256, 16) && ppt_max_n_masked(lim) == trial_max_n(lim, 256, 24));
    CHECK(mdt_max_n(lim) == trial_max_n(lim, 320, 336));
  }
  // the fit: n >= 1 and the bytes within the limit, the limit itself included
  CHECK(!trial_fits(0, 0, big) && trial_fits(1, 100, 100) && !trial_fits(1, 101, 100));
  CHECK(trial_max_n(256 + 16 - 1, 256, 16) == 0 && trial_max_n(256 + 16, 256, 16) == 64 && trial_max_n(0, 256, 16) == 0);
  // the values the engines' own tests pin
  CHECK(ppt_max_n(65536) == 261120 && ppt_max_n_masked(65536) == 174080);
  CHECK(mdt_max_n(65536) == 12416 && mdt_max_n(163840) == 31104);
  std::printf("ok\n");
  return 0;
}
"""


def test_the_three_plans_agree_on_the_host(tmp_path):
    """The three plan headers together under the host compiler, as a stand-alone sanitized program."""
    assert shutil.which("g++"), "g++ is needed to build the plan check"
    src = tmp_path / "trial_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "trial_plan_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr or "unsupported" in r.stderr):
        r = subprocess.run(base, capture_output=True, text=True)  # no sanitizer runtime on this toolchain
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_plan_headers_include_no_hip():
    """No HIP header is reachable from a plan: <cstdint>, and the shared header, which includes <cstdint> only."""
    for name in ("gs_ppt_plan.h", "gs_rmt_plan.h", "gs_mdt_plan.h"):
        with open(os.path.join(CSRC, name)) as f:
            includes = re.findall(r"^#include\s+(\S+)", f.read(), re.M)
        assert includes == ["<cstdint>", '"gs_trial_plan.h"'], name
    with open(os.path.join(CSRC, "gs_trial_plan.h")) as f:
        includes = re.findall(r"^#include\s+(\S+)", f.read(), re.M)
    assert includes == ["<cstdint>"]
