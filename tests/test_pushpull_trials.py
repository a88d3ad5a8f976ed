"""Batched Monte Carlo trials of the push-pull model (DESIGN.md section 4.5,
"trial-resident rounds"; gs_pushpull_trials.hip): one workgroup per trial with
the trial's informed set in LDS.  Trial t of a batch is keyed exactly like a
one-trial context with trial = base + t, so the specification is the oracle
pinned by tests/test_pushpull.py: oracle.Engine / oracle.run_to_coverage per
trial with make_params(trial=base + t, model=1).  Every GPU test here needs a
push-pull context with trials > 1.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_parity import masked, random_table, sha
from test_pushpull import words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip_simulator_amd", "csrc")
CLI = os.path.join(ROOT, "gossip_simulator_amd", "bin", "gossip_sim")

PP = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.0,
          seed=0x5EED, trial=0, model=1)
COVERED, QUIESCENT, MAX_TICKS = 0, 1, 2


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def config(gs, **kw):
    base = dict(n=5000, fanout=5, fanin=6, delaylow=10, delayhigh=20, droprate=0.1, crashrate=0.0,
                seed=0x5EED, trial=0, model="pushpull")
    base.update(kw)
    return gs.Config(**base)


def tables(n, T, stride, dlo, dhi, seed0):
    return [random_table(n, stride, dlo, dhi, seed=seed0 + t) for t in range(T)]


def stacked(tabs):
    return np.concatenate([d for d, _ in tabs]), np.concatenate([i for _, i in tabs])


def popcount(words):
    return int(sum(bin(int(x)).count("1") for x in words))


def oracle_trial(oracle, n, deg, ids, drop, trial, sender=-1, poll=10, max_ticks=100000):
    """One trial's gs_trial_results row from the oracle: gs_run's rule per
    trial -- covered; else the stopping poll informed nobody new and no call
    can change the informed set (QUIESCENT); else max_ticks.  Also returns the
    engine, left at the stopping poll."""
    p = oracle.make_params(**dict(PP, n=n, drop_rate=drop, trial=trial))
    rows, e = oracle.run_to_coverage(p, deg, ids, sender=sender, poll=poll, max_ticks=max_ticks)
    tick99 = next((int(r[0]) for r in rows if oracle.covered(int(r[4]), n)), 0)
    last = rows[-1]
    before = int(rows[-poll - 1][4]) if len(rows) > poll else 1  # informed before the stopping poll
    if oracle.covered(int(last[4]), n):
        st = COVERED
    elif int(last[4]) == before and oracle.pp_stalled(p, deg, ids, e.received(), e.crashed()):
        st = QUIESCENT
    else:
        assert int(last[0]) >= max_ticks
        st = MAX_TICKS
    row = [trial, tick99, int(last[0]), *[int(x) for x in rows[:, 1:4].sum(0)], int(last[4]), 0, st]
    return row, e


# ---- 1. per round, bit-exact --------------------------------------------------
SHAPES = [
    (1, 3, 2, 1, 2, 0.1, 0),
    (2, 2, 3, 0, 3, 0.0, 0),
    (777, 5, 6, 0, 6, 0.1, 0),           # ragged last word, zero degrees
    (16384, 3, 6, 5, 6, 0.1, 0),         # tlog = 14 exactly
    (16385, 3, 6, 5, 6, 0.29, 5),        # tlog = 15: a slot almost half padding, nonzero base trial
    (9000, 4, 19, 18, 19, 0.05, 0),      # wide rows
    (20000, 2, 6, 5, 6, 1.0, 0),         # every call lost
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,T,stride,dlo,dhi,drop,base", SHAPES)
def test_per_round_bit_exact(gs, oracle, n, T, stride, dlo, dhi, drop, base):
    tabs = tables(n, T, stride, dlo, dhi, seed0=7 * n)
    engines = []
    for t in range(T):
        e = oracle.Engine(oracle.make_params(**dict(PP, n=n, drop_rate=drop, trial=base + t)), *tabs[t])
        e.begin(-1)
        engines.append(e)
    with gs.Simulator(config(gs, n=n, droprate=drop, trial=base, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(-1)
        assert sim.totals()["received"] == T  # every trial's sender is informed at begin
        for r in range(60):
            rows = np.array([e.step(1)[0] for e in engines]).astype(np.int64)
            want = rows.sum(0)
            want[0] = rows[0][0]
            got = sim.step(1)[0].astype(np.int64)
            assert np.array_equal(got, want), f"round {r + 1}:\n{got}\n{want}"
            rec = sim.received()
            assert rec.shape == (T, (n + 63) // 64)
            for t in range(T):
                assert sha(rec[t]) == sha(engines[t].received()), f"round {r + 1}, trial {base + t}"
            if all(oracle.covered(int(x[4]), n) for x in rows):
                break
        assert not sim.crashed().any()


@pytest.mark.gpu
def test_one_step_call_crosses_chunk_boundaries(gs):
    """step(37) = the first 37 single-round rows (two 16-round chunk boundaries)."""
    n, T = 777, 5
    deg, ids = stacked(tables(n, T, 6, 0, 6, seed0=11))
    with gs.Simulator(config(gs, n=n, trials=T)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(-1)
        single = np.concatenate([sim.step(1) for _ in range(37)])
        rec1 = sim.received()
    with gs.Simulator(config(gs, n=n, trials=T)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(-1)
        assert np.array_equal(sim.step(37), single)
        assert np.array_equal(sim.received(), rec1)


# ---- 2. run against the oracle ------------------------------------------------
def halves_table(n, seed):
    """Two disconnected halves: a broadcast stays in its sender's half."""
    deg, ids = random_table(n, 6, 5, 6, seed=seed)
    h = n // 2
    ids = ids.copy()
    ids[:h] %= h
    ids[h:] = h + ids[h:] % (n - h)
    return deg, ids


@pytest.mark.gpu
@pytest.mark.parametrize("poll", [10, 1])
@pytest.mark.parametrize("sender", [-1, 7])
def test_run_matches_oracle_mixed_outcomes(gs, oracle, poll, sender):
    n, T = 3000, 4
    tabs = [random_table(n, 6, 5, 6, seed=21), halves_table(n, 22), random_table(n, 6, 5, 6, seed=23),
            halves_table(n, 24)]
    want = [oracle_trial(oracle, n, *tabs[t], 0.1, t, sender=sender, poll=poll)[0] for t in range(T)]
    assert [w[-1] for w in want] == [COVERED, QUIESCENT, COVERED, QUIESCENT]
    assert all(w[6] < 0.99 * n for w in want if w[-1] == QUIESCENT)
    with gs.Simulator(config(gs, n=n, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(sender)
        _, status = sim.run(poll=poll)
        got = sim.trial_results()
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"
    assert status == gs.GS_RUN_QUIESCENT


@pytest.mark.gpu
def test_run_max_ticks(gs, oracle):
    """max_ticks = 20 at a 90 % loss rate: nothing is covered by then.  Trial 0's
    nodes only know themselves, so it stalls at its first poll; the others are
    still spreading and report GS_RUN_MAX_TICKS."""
    n, T, drop = 3000, 4, 0.9
    tabs = tables(n, T, 6, 5, 6, seed0=31)
    tabs[0] = (tabs[0][0], np.repeat(np.arange(n, dtype=np.uint32)[:, None], 6, axis=1))
    want = [oracle_trial(oracle, n, *tabs[t], drop, t, max_ticks=20)[0] for t in range(T)]
    assert [w[-1] for w in want] == [QUIESCENT, MAX_TICKS, MAX_TICKS, MAX_TICKS]
    assert [w[2] for w in want] == [10, 20, 20, 20]
    with gs.Simulator(config(gs, n=n, droprate=drop, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(-1)
        _, status = sim.run(poll=10, max_ticks=20)
        got = sim.trial_results()
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"
    assert status == gs.GS_RUN_MAX_TICKS


# ---- 3. many trials -------------------------------------------------------------
@pytest.mark.gpu
def test_many_trials(gs, oracle):
    """More trials than workgroups resident at once.  Every trial keeps running
    until the run ends, so totals() counts each trial through the run's last
    tick F while its trial_results row stops at its own poll:
    totals().messages == sum over trials of the oracle's messages in rounds
    1..F >= the sum of the rows' messages, with equality iff every trial
    stopped at F; received likewise."""
    n, T = 300, 1500
    tabs = tables(n, T, 6, 5, 6, seed0=100_000)
    want, engines = [], []
    for t in range(T):
        row, e = oracle_trial(oracle, n, *tabs[t], 0.1, t)
        want.append(row)
        engines.append(e)
    want = np.array(want)
    with gs.Simulator(config(gs, n=n, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        got = sim.trial_results()
        tot = sim.totals()
    assert np.array_equal(got, want), f"{np.nonzero((got != want).any(1))[0][:10]}"
    F = int(want[:, 2].max())
    assert tot["tick"] == F
    late_msgs = late_recv = 0
    for t in range(T):
        k = F - int(want[t, 2])
        if k:
            rows = engines[t].step(k)
            late_msgs += int(rows[:, 3].sum())
            late_recv += int(rows[-1, 4]) - int(want[t, 6])
    assert tot["messages"] == int(want[:, 5].sum()) + late_msgs
    assert tot["received"] == int(want[:, 6].sum()) + late_recv
    assert (late_msgs == 0) == bool((want[:, 2] == F).all())


# ---- 4. against the one-trial GPU engine ---------------------------------------
@pytest.mark.gpu
def test_batch_matches_one_trial_contexts(gs):
    n, T, base = 20000, 12, 3
    with gs.Simulator(config(gs, n=n, trial=base, trials=T)) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        got = sim.trial_results()
    with gs.Simulator(config(gs, n=n, trial=base, trials=T, model="flood")) as flood:
        flood.build_overlay()
        fdeg, fids = flood.read_peers()
    assert np.array_equal(deg, fdeg)  # the batched overlay is model-independent
    assert np.array_equal(masked(deg, ids), masked(fdeg, fids))
    want = []
    for t in range(T):
        with gs.Simulator(config(gs, n=n, trial=base + t)) as one:
            one.load_peers(deg[t * n:(t + 1) * n], masked(deg, ids)[t * n:(t + 1) * n])
            one.broadcast_begin(-1)
            one.run(poll=10)
            want.append(one.trial_results()[0])
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"


# ---- 5. renumbering, 6. members -------------------------------------------------
def batch_run(sim):
    sim.build_overlay()
    sim.broadcast_begin(-1)
    sim.run(poll=10)
    return sim.trial_results()


@pytest.mark.gpu
def test_reset_and_set_trial(gs):
    n, T = 5000, 6
    with gs.Simulator(config(gs, n=n, trials=T)) as sim:
        first = batch_run(sim)
        sim.reset()
        sim.broadcast_begin(-1)  # no renumbering: the same table, the same run
        sim.run(poll=10)
        assert np.array_equal(sim.trial_results(), first)
        sim.reset()
        sim.set_trial(T)
        got = batch_run(sim)
    with gs.Simulator(config(gs, n=n, trial=T, trials=T)) as fresh:
        want = batch_run(fresh)
    assert list(got[:, 0]) == list(range(T, 2 * T))
    assert np.array_equal(got, want), f"\n{got}\n{want}"
    assert not np.array_equal(got[:, 1:], first[:, 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [9, 3])
def test_trials_split_over_members(gs, T):
    """Two members on device 0 = one batch.  T = 3 splits into one trial and two:
    the member with a single trial is a one-trial push-pull context (reverse
    table, sparse and dense rounds), keyed identically."""
    c = config(gs, n=5000, trials=T)
    with gs.Simulator(c) as one:
        want = batch_run(one)
    with gs.Simulator(c, devices=[0, 0]) as two:
        got = batch_run(two)
        assert two.received().shape == (T, (5000 + 63) // 64)
    assert np.array_equal(got, want), f"\n{got}\n{want}"


# ---- 7. the limit -----------------------------------------------------------------
@pytest.mark.gpu
def test_limit(gs, oracle):
    m = gs.pp_trials_max_n()
    assert m >= 65536 and m % 64 == 0
    T = 2
    tabs = tables(m, T, 6, 5, 6, seed0=41)
    want = [oracle_trial(oracle, m, *tabs[t], 0.1, t)[0] for t in range(T)]
    with gs.Simulator(config(gs, n=m, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        with pytest.raises(gs.GossipError):
            sim.set_failed(np.zeros((m + 63) // 64, dtype=np.uint64))  # failure masks stay refused on a batch
        sim.broadcast_begin(-1)
        _, status = sim.run(poll=10)
        got = sim.trial_results()
    assert status == gs.GS_RUN_COVERED
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator(config(gs, n=m + 1, trials=T))
    assert ei.value.code == -1 and str(m) in str(ei.value)  # GS_EINVAL, naming the limit


# ---- 8. CLI on the GPU --------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("model", ["pushpull", "flood"])
def test_cli_trials(gs, model):
    from gossip_simulator_amd import _lib
    n, T = 5000, 6
    r = subprocess.run([CLI, "-model", model, "-n", str(n), "-trials", str(T), "-seed", "9"],
                       capture_output=True, text=True, timeout=300)
    lines = re.findall(r"^trial (\d+): (\S+)% covered, took (\S+), Total message (\d+) Total Crashed (\d+)$",
                       r.stdout, re.M)
    assert len(lines) == T, r.stdout + r.stderr
    with gs.Simulator(gs.Config(n=n, seed=9, trials=T, model=model)) as sim:
        res = batch_run(sim)
    want = [(str(int(x[0])), _lib.format_float32(float(np.float32(int(x[6])) / np.float32(n) * np.float32(100))),
             _lib.format_duration(int(x[2]) * 1_000_000), str(int(x[5])), str(int(x[7]))) for x in res]
    assert lines == want
    k = int((res[:, 8] == COVERED).sum())
    assert f"--- {k} of {T} trials got 99% ---\n" in r.stdout
    assert r.returncode == (0 if k == T else 3)
    assert "=== Constructing Overlay ===" in r.stdout and "=== Broadcast one message ===" in r.stdout


# ---- 9. CPU ---------------------------------------------------------------------------
def test_cli_trials_flag_usage():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    names = re.findall(r"^  -(\w+)", r.stderr, flags=re.M)
    assert "trials" in names and names == sorted(names)
    for bad in ("0", "-1"):
        r = subprocess.run([CLI, "-trials", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "-trials" in r.stderr
    r = subprocess.run([CLI, "-n=1000"], capture_output=True, text=True, timeout=60)
    assert "trials" not in r.stdout  # additive: not echoed


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "gs_ppt_plan.h"
using namespace gs;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  // two bitsets of ceil(n / 64) 8-byte words + 256 B of reduction scratch
  const unsigned long long big = 1ull << 40;
  CHECK(ppt_plan(1, big).lds_bytes == 2 * 8 + 256);
  CHECK(ppt_plan(64, big).lds_bytes == 2 * 8 + 256);
  CHECK(ppt_plan(65, big).lds_bytes == 4 * 8 + 256);
  CHECK(ppt_plan(16384, big).lds_bytes == 2 * 256 * 8 + 256);
  CHECK(ppt_plan(16385, big).lds_bytes == 2 * 257 * 8 + 256);
  CHECK(!ppt_plan(0, big).fits);
  const unsigned long long limits[] = {65536, 163840, 272, 300};
  for (unsigned long long lim : limits) {
    const unsigned long long m = ppt_max_n(lim);
    CHECK(m >= 64 && m % 64 == 0);
    CHECK(ppt_plan(m, lim).fits && ppt_plan(m, lim).lds_bytes <= lim);
    CHECK(!ppt_plan(m + 1, lim).fits && ppt_plan(m + 1, lim).lds_bytes > lim);
  }
  CHECK(ppt_max_n(65536) == 261120 && ppt_max_n(163840) == 654336);
  CHECK(ppt_max_n(271) == 0 && ppt_max_n(0) == 0);
  // blocks: whole waves, smaller for small n, at most 1024 threads
  unsigned prev = 0;
  for (unsigned long long n = 1; n <= 700000; n += (n < 4096 ? 1 : 997)) {
    const PptPlan p = ppt_plan(n, big);
    CHECK(p.block >= 64 && p.block <= 1024 && p.block % 64 == 0 && (p.block & (p.block - 1)) == 0);
    CHECK(p.block >= prev);
    CHECK(p.block == 1024 || (unsigned long long)p.block * 16 >= n);
    CHECK(p.words == (n + 63) / 64);
    prev = p.block;
  }
  CHECK(ppt_plan(1, big).block == 64 && ppt_plan(1025, big).block == 128 && ppt_plan(100000, big).block == 1024);
  std::printf("ok\n");
  return 0;
}
"""


def test_plan_header_on_the_host(tmp_path):
    """gs_ppt_plan.h alone under the host compiler, as a stand-alone sanitized program."""
    assert shutil.which("g++"), "g++ is needed to build the plan check"
    src = tmp_path / "ppt_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "ppt_plan_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr or "unsupported" in r.stderr):
        r = subprocess.run(base, capture_output=True, text=True)  # no sanitizer runtime on this toolchain
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
