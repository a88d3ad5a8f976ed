"""Batched Monte Carlo trials of the rumor model on the GPU (gs_create_trials,
Simulator.batch; gs_rumor_trials.hip): one workgroup
per trial with the trial's sets and miss counts in LDS.  Trial i of a batch is
a one-trial context with trial = base + i, trial i's table and trial i's mask,
so the truth is one PyRumorModes restatement (tests/test_rumor_modes.py) per
trial: bit-exact per round in all eight modes -- the summed stats row, every
trial's informed and removed sets -- then gs_run's per-trial stop rule, failure
masks, the lifecycle calls, the LDS limit and the CLI.
"""
from __future__ import annotations

import re
import subprocess

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumor import RUMOR, words_of
from test_rumor_modes import BLIND, COIN, PULL, PyRumorModes
from test_rumor_modes_gpu import cfg_of, mode_id, ring_table

pytestmark = pytest.mark.gpu

COVERED, QUIESCENT, MAX_TICKS, RUNNING = 0, 1, 2, -1


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def tables(n, T, seed0, dlo=0, table=None):
    if table is not None:
        return [table(n, seed0 + i) for i in range(T)]
    return [random_table(n, 6, dlo, 6, seed=seed0 + i) for i in range(T)]


def stacked(tabs):
    return np.concatenate([d for d, _ in tabs]), np.concatenate([i for _, i in tabs])


def restatements(oracle, kw, tabs, sender, k, mode, failed=None):
    """One restatement per trial, keyed trial = kw['trial'] + i."""
    return [PyRumorModes(oracle, oracle.make_params(**dict(kw, trial=kw["trial"] + i)), deg, masked(deg, ids), sender,
                         k, None if failed is None else failed[i], mode) for i, (deg, ids) in enumerate(tabs)]


def summed(rows):
    r = np.array(rows, dtype=np.int64)
    return [int(r[0, 0])] + [int(x) for x in r[:, 1:].sum(0)]


def check_sets(sim, es, what):
    rec, rem = sim.received(), sim.removed()
    T, W = len(es), (es[0].n + 63) // 64
    assert rec.shape == (T, W) and rem.shape == (T, W)
    for i, e in enumerate(es):
        assert np.array_equal(rec[i], words_of(e.inf)), f"{what}: trial {i}: informed set differs"
        assert np.array_equal(rem[i], words_of(e.removed)), f"{what}: trial {i}: removed set differs"


def begin(sim, es, sender):
    sim.broadcast_begin(sender)
    tot = sim.totals()
    assert (tot["received"], tot["pending"]) == (sum(e.received for e in es), sum(e.pending for e in es))
    check_sets(sim, es, "after begin")


def step_all(sim, es, rounds, what=""):
    """gs_step(1) x rounds: the summed row and every trial's sets after every round."""
    for _ in range(rounds):
        want = summed([e.step() for e in es])
        got = [int(x) for x in sim.step(1)[0]]
        assert got == want, f"{what} round {es[0].t}:\n{got}\n{want}"
        check_sets(sim, es, f"{what} round {es[0].t}")


# ---- 1. word and slot edges ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 777, 4133])
@pytest.mark.parametrize("mode", range(8), ids=mode_id)
def test_word_and_slot_edges(gs, oracle, mode, n):
    T, kw = 3, dict(RUMOR, n=n, trial=2)
    tabs = tables(n, T, seed0=10 * n, dlo=0 if n > 2 else 1)
    for deg, _ in tabs:
        deg[n // 2] = max(deg[n // 2], 1)   # the sender has a friend to call (the other rows may be empty)
    es = restatements(oracle, kw, tabs, n // 2, 2, mode)
    with gs.Simulator.batch(cfg_of(gs, kw, 2, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, n // 2)
        rows = []
        for _ in range(40):
            rows.append([e.step() for e in es])
            got = [int(x) for x in sim.step(1)[0]]
            assert got == summed(rows[-1]), f"round {es[0].t}:\n{got}\n{summed(rows[-1])}"
            check_sets(sim, es, f"round {es[0].t}")
        tot = sim.totals()
        r = np.array(rows, dtype=np.int64)  # [round, trial, field]
        assert tot == dict(tick=40, fired=int(r[:, :, 1].sum()), sent=int(r[:, :, 2].sum()),
                           messages=int(r[:, :, 3].sum()), received=sum(e.received for e in es), crashed=0,
                           pending=sum(e.pending for e in es))
    if n == 4133 and not mode & BLIND:  # (blind with k = 2 dies out early; a pull sender may have no caller)
        assert any(e.received > n // 2 for e in es)


# ---- 2. slot padding and big blocks -------------------------------------------------
@pytest.mark.parametrize("n", [16385, 20000])   # tlog = 15, a slot half padding; a block of 1,024, words per wave
@pytest.mark.parametrize("mode", [0, COIN | BLIND, PULL, PULL | BLIND | COIN], ids=mode_id)
def test_slot_padding_and_big_blocks(gs, oracle, mode, n):
    T, kw = 2, dict(RUMOR, n=n, trial=5)
    tabs = tables(n, T, seed0=n, dlo=1)
    es = restatements(oracle, kw, tabs, -1, 3, mode)
    cum = np.zeros((T, 3), dtype=np.int64)
    tick99 = [0] * T
    with gs.Simulator.batch(cfg_of(gs, kw, 3, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, -1)
        for call in (16, 17, 1):  # a launch boundary falls inside the second call
            want = []
            for _ in range(call):
                rows = [e.step() for e in es]
                want.append(summed(rows))
                cum += np.array(rows, dtype=np.int64)[:, 1:4]
                for i, e in enumerate(es):
                    if not tick99[i] and oracle.covered(e.received, n):
                        tick99[i] = e.t
            got = sim.step(call)
            assert got.astype(np.int64).tolist() == want, f"step({call}) ending at round {es[0].t}"
            check_sets(sim, es, f"after round {es[0].t}")
            res = sim.trial_results()
            for i, e in enumerate(es):
                assert res[i].tolist() == [5 + i, tick99[i], e.t, *cum[i].tolist(), e.received, 0, RUNNING], i
    assert any(e.received > n // 4 for e in es)   # (a pull sender may have no caller)


# ---- 3. trials differ and are keyed by number ----------------------------------------
def test_trials_have_their_own_senders(gs, oracle):
    n, T = 4133, 5
    kw = dict(RUMOR, n=n, trial=7)
    tabs = tables(n, T, seed0=70, dlo=1)
    es = restatements(oracle, kw, tabs, -1, 2, 0)
    senders = [int(np.nonzero(e.inf)[0][0]) for e in es]
    assert len(set(senders)) == T
    with gs.Simulator.batch(cfg_of(gs, kw, 2, 0, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, -1)   # every trial's informed set is its own keyed sender
        rec = sim.received()
        for i, s in enumerate(senders):
            assert np.array_equal(rec[i], words_of(np.arange(n) == s)), i
        step_all(sim, es, 12)
    assert len({e.received for e in es}) > 1


@pytest.mark.parametrize("mode", [0, PULL], ids=mode_id)
def test_batch_equals_one_trial_contexts(gs, mode):
    """trial = 7, T = 5: trials 7..11 of five one-trial GPU contexts, round by round and under gs_run."""
    n, T = 4133, 5
    kw = dict(RUMOR, n=n, trial=7)
    tabs = tables(n, T, seed0=80, table=ring_table)
    ones = []
    for i, (deg, ids) in enumerate(tabs):
        with gs.Simulator(cfg_of(gs, dict(kw, trial=7 + i), 2, mode)) as one:
            one.load_peers(deg, ids)
            one.broadcast_begin(-1)
            rows = one.step(25).astype(np.int64)
            sets = (one.received(), one.removed())
            one.reset()
            one.broadcast_begin(-1)
            _, st = one.run(poll=10)
            ones.append((rows, sets, one.trial_results()[0], st))
    with gs.Simulator.batch(cfg_of(gs, kw, 2, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(-1)
        got = sim.step(25).astype(np.int64)
        want = sum(o[0] for o in ones)
        want[:, 0] = ones[0][0][:, 0]
        assert np.array_equal(got, want)
        rec, rem = sim.received(), sim.removed()
        for i, o in enumerate(ones):
            assert np.array_equal(rec[i], o[1][0]) and np.array_equal(rem[i], o[1][1]), i
        sim.reset()
        sim.broadcast_begin(-1)
        _, st = sim.run(poll=10)
        assert np.array_equal(sim.trial_results(), np.array([o[2] for o in ones]))
        assert st == max(o[3] for o in ones)


# ---- 4. gs_run ---------------------------------------------------------------------------
def reference_trial(oracle, kw, deg, ids, sender, k, mode, poll, max_ticks):
    """gs_run's rule on one restatement (test_rumor_modes_gpu.reference_run's),
    with the cumulative counters: the trial's gs_trial_results row."""
    e = PyRumorModes(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, k, None, mode)
    tick_99, cum = 0, np.zeros(3, dtype=np.int64)
    while True:
        for _ in range(poll):
            cum += np.array(e.step()[1:4], dtype=np.int64)
        cov = oracle.covered(e.received, e.n)
        if cov and not tick_99:
            tick_99 = e.t
        if e.pending == 0:
            st = COVERED if cov else QUIESCENT
            break
        if e.t >= max_ticks:
            st = MAX_TICKS
            break
    return [kw["trial"], tick_99, e.t, *cum.tolist(), e.received, 0, st]


RUN_CASES = [(BLIND, 16), (BLIND, 1), (COIN, 16), (COIN, 1), (PULL, 2), (PULL, 1)]


@pytest.fixture(scope="module")
def run_truth(oracle):
    """Each case's tables and, per poll length, the trials' rows (computed once)."""
    n, T, out = 4133, 4, {}
    for mode, k in RUN_CASES:
        tabs = tables(n, T, seed0=n + 100 * k + mode, dlo=5, table=ring_table if mode & PULL else None)
        for poll in (10, 1):
            kw = dict(RUMOR, n=n, trial=3)
            out[mode, k, poll] = (tabs, [reference_trial(oracle, dict(kw, trial=3 + i), *tabs[i], 3, k, mode, poll,
                                                         10_000) for i in range(T)])
    return out


@pytest.mark.parametrize("mode,k", RUN_CASES)
@pytest.mark.parametrize("poll", [10, 1])
def test_run_stops_each_trial_at_its_own_poll(gs, run_truth, mode, k, poll):
    n, T = 4133, 4
    kw = dict(RUMOR, n=n, trial=3)
    tabs, want = run_truth[mode, k, poll]
    with gs.Simulator.batch(cfg_of(gs, kw, k, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(3)
        rows, st = sim.run(poll=poll, max_ticks=10_000)
        got = sim.trial_results()
        assert got.tolist() == want, f"\n{got}\n{np.array(want)}"
        last = max(w[2] for w in want)
        assert st == max(w[8] for w in want) and len(rows) * poll == last == sim.totals()["tick"]
        assert sim.totals()["pending"] == 0
    if (mode, k, poll) == (PULL, 2, 1):
        assert len({w[2] for w in want}) > 1   # trials of one run stop at different polls


def test_run_max_ticks_with_an_unasked_hot_sender(gs, oracle):
    """Trial 0: nobody's row names the sender (feedback pull): hot, never asked, no event ever.
    It runs to max_ticks; the others stop at their own polls long before."""
    n, T = 777, 4
    kw = dict(RUMOR, n=n, trial=0)
    tabs = tables(n, T, seed0=40, table=ring_table)
    rng = np.random.default_rng(4)
    tabs[0] = (np.full(n, 6, np.uint8), rng.integers(1, n, size=(n, 6)).astype(np.uint32))
    want = [reference_trial(oracle, dict(kw, trial=i), *tabs[i], 0, 2, PULL, 10, 200) for i in range(T)]
    assert want[0][8] == MAX_TICKS and want[0][2] == 200 and want[0][6] == 1
    assert all(w[8] != MAX_TICKS and w[2] < 200 for w in want[1:])
    with gs.Simulator.batch(cfg_of(gs, kw, 2, PULL, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(0)
        rows, st = sim.run(poll=10, max_ticks=200)
        assert st == MAX_TICKS and len(rows) == 20
        assert sim.trial_results().tolist() == want
        assert sim.totals()["pending"] == 1 and not sim.removed()[0].any()


# ---- 5. failure masks ----------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.05, 0.5])
@pytest.mark.parametrize("mode", [BLIND, PULL, PULL | BLIND], ids=mode_id)
def test_failure_masks_per_trial(gs, oracle, mode, frac):
    n, T = 4133, 3
    kw = dict(RUMOR, n=n, drop_rate=0.0, trial=1)
    tabs = tables(n, T, seed0=9, dlo=1)
    dead = [np.random.default_rng(30 + i).random(n) < frac for i in range(T)]
    dead[0][100] = dead[2][100] = False
    dead[1][100] = True   # trial 1's sender is failed: it stays empty
    masks = np.stack([words_of(d) for d in dead])
    assert not np.array_equal(masks[0], masks[2])
    es = restatements(oracle, kw, tabs, 100, 6, mode, dead)
    with gs.Simulator.batch(cfg_of(gs, kw, 6, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(masks)
        begin(sim, es, 100)
        step_all(sim, es, 40)
        assert es[1].received == 0 and not sim.received()[1].any()
        assert es[0].received > (1000 if frac < 0.5 else 0) and not any((e.inf & d).any() for e, d in zip(es, dead))
        sim.reset()     # keeps the masks
        assert np.array_equal(sim.crashed(), masks) and not sim.received().any() and not sim.removed().any()
        es = restatements(oracle, kw, tabs, 100, 6, mode, dead)
        begin(sim, es, 100)
        step_all(sim, es, 12, "after reset")


# ---- 6. lifecycle ----------------------------------------------------------------------------
def step_rows(sim, rounds):
    return sim.step(rounds).astype(np.int64).tolist()


@pytest.mark.parametrize("mode", [0, PULL], ids=mode_id)
def test_lifecycle(gs, oracle, mode):
    n, T = 4133, 3
    kw = dict(RUMOR, n=n, trial=0)
    tabs, tabs2 = tables(n, T, seed0=21, dlo=1), tables(n, T, seed0=61, dlo=1)
    kw7 = dict(kw, trial=7)
    with gs.Simulator.batch(cfg_of(gs, kw, 2, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(9)
        first = step_rows(sim, 30)
        sets = (sim.received(), sim.removed())
        sim.reset()                      # a second broadcast equals the first
        assert not sim.received().any() and not sim.removed().any()
        sim.broadcast_begin(9)
        assert step_rows(sim, 30) == first
        assert np.array_equal(sim.received(), sets[0]) and np.array_equal(sim.removed(), sets[1])
        sim.reset()                      # set_trial plus a new table equals a fresh batch
        sim.set_trial(7)
        sim.load_peers(*stacked(tabs2))
        sim.broadcast_begin(-1)
        a = step_rows(sim, 30)
        a_sets = (sim.received(), sim.removed())
    es = restatements(oracle, kw7, tabs2, -1, 2, mode)
    with gs.Simulator.batch(cfg_of(gs, kw7, 2, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs2))
        sim.broadcast_begin(-1)
        assert step_rows(sim, 30) == a == [summed([e.step() for e in es]) for _ in range(30)]
        assert np.array_equal(sim.received(), a_sets[0]) and np.array_equal(sim.removed(), a_sets[1])
    assert a != first


def test_overlay_on_the_batch_feeds_the_restatement(gs, oracle):
    n, T = 5000, 3
    kw = dict(RUMOR, n=n, trial=4)
    with gs.Simulator.batch(cfg_of(gs, kw, 2, PULL, trials=T)) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        assert deg.shape == (T * n,) and not np.array_equal(deg[:n], deg[n:2 * n])
        tabs = [(deg[i * n:(i + 1) * n], ids[i * n:(i + 1) * n]) for i in range(T)]
        es = restatements(oracle, kw, tabs, -1, 2, PULL)
        begin(sim, es, -1)
        step_all(sim, es, 30)
    assert all(e.received > n // 2 for e in es)


# ---- 7. the limit -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, PULL], ids=mode_id)
def test_limit(gs, oracle, mode):
    m = gs.rumor_trials_max_n(mode)   # from the query, never a constant
    assert m >= 64 and m % 64 == 0 and m == gs.rumor_trials_max_n(gs.Config(model="rumor", rumor_pull=bool(mode & PULL)))
    assert gs.rumor_trials_max_n(PULL) < gs.rumor_trials_max_n(0) < gs.rumor_trials_max_n(COIN)
    T, kw = 2, dict(RUMOR, n=m, trial=0)
    tabs = tables(m, T, seed0=41, dlo=5)
    es = restatements(oracle, kw, tabs, -1, 2, mode)
    with gs.Simulator.batch(cfg_of(gs, kw, 2, mode, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, -1)
        want = [summed([e.step() for e in es]) for _ in range(20)]
        assert step_rows(sim, 20) == want
        check_sets(sim, es, "round 20")
    assert all(e.received > 1000 for e in es)
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator.batch(cfg_of(gs, dict(kw, n=m + 64), 2, mode, trials=T))
    assert ei.value.code == -1 and str(m) in str(ei.value) and "gs_rumor_trials_max_n" in str(ei.value)
    with pytest.raises(gs.GossipError) as ei:   # gs_create keeps its own refusal
        gs.Simulator(cfg_of(gs, dict(kw, n=1000), 2, mode, trials=T))
    assert ei.value.code == -1 and "trials" in str(ei.value)


# ---- 8. CLI --------------------------------------------------------------------------------------
def test_cli_prints_the_trials_and_their_statistics(gs):
    from gossip_simulator_amd import _lib
    n, T, seed = 4133, 4, 9
    r = subprocess.run([_lib.CLI_PATH, "-n", str(n), "-model", "rumor", "-k", "2", "-trials", str(T), "-seed",
                        str(seed)], capture_output=True, text=True, timeout=300)
    lines = re.findall(r"^trial (\d+): Residue (\S+), (\S+) messages per node after (\S+), (\w+)$", r.stdout, re.M)
    assert len(lines) == T, r.stdout + r.stderr
    with gs.Simulator.batch(gs.Config(n=n, seed=seed, trials=T, model="rumor", rumor_k=2)) as sim:
        sim.build_overlay()
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        res = sim.trial_results()
    names = {COVERED: "covered", QUIESCENT: "quiescent", MAX_TICKS: "maxticks"}
    want = [(str(int(x[0])), _lib.format_float32(float(np.float32(1) - np.float32(int(x[6])) / np.float32(n))),
             _lib.format_float32(float(np.float32(int(x[5])) / np.float32(n))),
             _lib.format_duration(int(x[2]) * 1_000_000), names[int(x[8])]) for x in res]
    assert lines == want
    m = re.search(r"^--- 4 trials: residue mean (\S+) sd (\S+), messages per node mean (\S+) sd (\S+), "
                  r"rounds mean (\S+) sd (\S+) ---$", r.stdout, re.M)
    assert m, r.stdout
    got = [float(x) for x in m.groups()]
    cols = [1.0 - res[:, 6] / n, res[:, 5] / n, res[:, 2].astype(np.float64)]
    want = [f(c) for c in cols for f in (np.mean, lambda c: np.std(c, ddof=1))]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-15), (got, want)
    assert r.returncode == 0 and all(int(x[8]) != MAX_TICKS for x in res)
    assert "=== Constructing Overlay ===" in r.stdout and "=== Broadcast one message ===" in r.stdout
