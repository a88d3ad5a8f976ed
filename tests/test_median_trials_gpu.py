"""Batched Monte Carlo trials of the median-counter model on the GPU
(gs_create_batch, Simulator.median_batch; gs_median_trials.hip; DESIGN.md
section 4.8.1): one workgroup per trial with the trial's state in LDS.  Trial i
of a batch is a one-trial context with trial = base + i, trial i's table and
trial i's mask, so the truth is one PyMedian restatement (tests/test_median.py)
per trial: bit-exact per round and per trial -- the state bytes, the informed
and done sets, the per-trial counters -- and the summed stats row; then
gs_run's per-trial stop rule, failure masks, the lifecycle calls, the LDS limit,
the CLI, and a check that the sweep would catch a dropped own end.
"""
from __future__ import annotations

import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_median import MEDIAN, PyMedian, reference_run, words_of

pytestmark = pytest.mark.gpu

COVERED, QUIESCENT, MAX_TICKS, RUNNING = 0, 1, 2, -1
LIMIT_64K = (65536 - 320) // 336 * 64   # gs_mdt_plan.h restated: 336 B per 64 nodes and 320 B of scratch


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def cfg_of(gs, kw, k=2, **more):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], model="median", rumor_k=k, **more)


def ring_table(n, seed, stride=6, lo=5):
    """A random table whose first slot is a ring, so every node has a caller."""
    deg, ids = random_table(n, stride, max(lo, 1), stride, seed=seed)
    ids[:, 0] = (np.arange(n) + 1) % n
    return deg, ids


def hub_table(n, seed):
    """Every row names node 0 (twice in every third row): all adds and flag ORs of a round meet in node 0's words."""
    rng = np.random.default_rng(seed)
    deg = np.full(n, 4, np.uint8)
    ids = rng.integers(1, n, size=(n, 4)).astype(np.uint32)
    ids[:, 1] = 0
    ids[::3, 3] = 0
    return deg, ids


def tables(n, T, seed0, table=ring_table):
    return [table(n, seed0 + i) for i in range(T)]


def stacked(tabs):
    return np.concatenate([d for d, _ in tabs]), np.concatenate([i for _, i in tabs])


def restatements(oracle, kw, tabs, sender, k, failed=None, wrong=None):
    """One restatement per trial, keyed trial = kw['trial'] + i."""
    return [PyMedian(oracle, oracle.make_params(**dict(kw, trial=kw["trial"] + i)), deg, masked(deg, ids), sender, k,
                     None if failed is None else failed[i], wrong) for i, (deg, ids) in enumerate(tabs)]


def summed(rows):
    r = np.array(rows, dtype=np.int64)
    return [int(r[0, 0])] + [int(x) for x in r[:, 1:].sum(0)]


class Truth:
    """The restatements of a batch with their cumulative per-trial counters."""

    def __init__(self, oracle, es, base):
        self.oracle, self.es, self.base = oracle, es, base
        self.cum = np.zeros((len(es), 3), dtype=np.int64)
        self.tick99 = [0] * len(es)

    def step(self):
        rows = [e.step() for e in self.es]
        self.cum += np.array(rows, dtype=np.int64)[:, 1:4]
        for i, e in enumerate(self.es):   # every stepped tick is a poll
            if not self.tick99[i] and self.oracle.covered(e.received, e.n):
                self.tick99[i] = e.t
        return summed(rows)

    def results(self, status=RUNNING):
        return [[self.base + i, self.tick99[i], e.t, *self.cum[i].tolist(), e.received, 0, status]
                for i, e in enumerate(self.es)]


def check_state(sim, es, what):
    st, rec, rem = sim.median_state(), sim.received(), sim.removed()
    T, n = len(es), es[0].n
    W = (n + 63) // 64
    assert st.shape == (T, n) and st.dtype == np.uint8 and rec.shape == (T, W) and rem.shape == (T, W)
    for i, e in enumerate(es):
        assert np.array_equal(st[i], e.st), f"{what}: trial {i}: state bytes differ"
        assert np.array_equal(rec[i], words_of(e.inf)), f"{what}: trial {i}: informed set differs"
        assert np.array_equal(rem[i], words_of(e.removed)), f"{what}: trial {i}: done set differs"


def begin(sim, es, sender):
    sim.broadcast_begin(sender)
    tot = sim.totals()
    assert (tot["received"], tot["pending"]) == (sum(e.received for e in es), sum(e.pending for e in es))
    check_state(sim, es, "after begin")


def step_all(sim, tr, rounds, what=""):
    """gs_step(1) x rounds: the summed row, every trial's state and sets and its counters after every round."""
    for _ in range(rounds):
        want = tr.step()
        got = [int(x) for x in sim.step(1)[0]]
        t = tr.es[0].t
        assert got == want, f"{what} round {t}:\n{got}\n{want}"
        check_state(sim, tr.es, f"{what} round {t}")
        assert sim.trial_results().tolist() == tr.results(), f"{what} round {t}: per-trial counters"


def parity(gs, oracle, kw, tabs, sender, k=2, rounds=30, failed=None, load=None):
    T = len(tabs)
    es = restatements(oracle, kw, tabs, sender, k, failed)
    tr = Truth(oracle, es, kw["trial"])
    with gs.Simulator.median_batch(cfg_of(gs, kw, k, trials=T)) as sim:
        (load or (lambda s: s.load_peers(*stacked(tabs))))(sim)
        if failed is not None:
            sim.set_failed(np.stack([words_of(f) for f in failed]))
        begin(sim, es, sender)
        step_all(sim, tr, rounds)
        tot = sim.totals()
        assert tot == dict(tick=rounds, fired=int(tr.cum[:, 0].sum()), sent=int(tr.cum[:, 1].sum()),
                           messages=int(tr.cum[:, 2].sum()), received=sum(e.received for e in es), crashed=0,
                           pending=sum(e.pending for e in es))
    return es


# ---- 1. sizes -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4133])
def test_word_edges(gs, oracle, n):
    """Word edges, a partial last word, one wave and several; rows with duplicates, self entries and
    (n > 2) empty rows."""
    T, kw = 3, dict(MEDIAN, n=n, trial=2)
    tabs = [random_table(n, 6, 0 if n > 2 else 1, 6, seed=10 * n + i) for i in range(T)]
    for deg, _ in tabs:
        deg[n // 2] = max(deg[n // 2], 1)
    es = parity(gs, oracle, kw, tabs, n // 2, rounds=30)
    if n == 4133:
        assert any(e.received > n // 2 and e.removed.sum() > n // 2 for e in es)


@pytest.mark.parametrize("n", [LIMIT_64K, LIMIT_64K + 64])
def test_the_64_kib_opt_in_boundary(gs, oracle, n):
    """The largest n whose plan needs no opt-in to more than 64 KiB of dynamic LDS, and the first that does."""
    W = (n + 63) // 64
    assert (W * 336 + 320 <= 65536) == (n == LIMIT_64K) and LIMIT_64K == 12416
    es = parity(gs, oracle, dict(MEDIAN, n=n, trial=1), tables(n, 2, seed0=n), -1, k=3, rounds=22)
    assert all(e.received > n // 2 for e in es)


def test_limit(gs, oracle):
    m = gs.median_trials_max_n()   # from the query, never a constant
    assert m >= LIMIT_64K and m % 64 == 0
    kw = dict(MEDIAN, n=m, trial=0)
    es = parity(gs, oracle, kw, tables(m, 2, seed0=41), -1, k=3, rounds=20)
    assert all(e.received > 1000 for e in es)
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator.median_batch(cfg_of(gs, dict(kw, n=m + 64), 3, trials=2))
    assert ei.value.code == -1 and str(m) in str(ei.value) and "gs_median_trials_max_n" in str(ei.value)
    with gs.Simulator.median_batch(cfg_of(gs, dict(kw, n=m + 64), 3)) as one:   # one trial: no such limit
        assert one.median_state().shape == (m + 64,)


# ---- 2. counter lengths, drop rates -------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(1, 4133), (3, 4133), (127, 4133), (127, 65)])
def test_counter_lengths(gs, oracle, k, n):
    es = parity(gs, oracle, dict(MEDIAN, n=n, trial=3), tables(n, 3, seed0=k + n), 5, k=k, rounds=36)
    assert all(e.received > 0.99 * n for e in es)
    if k == 127:   # the counters are still running
        assert all(20 < e.st.max() <= 127 and not e.removed.any() for e in es)


@pytest.mark.parametrize("drop", [0.0, 0.1, 0.57])
def test_drop_rates(gs, oracle, drop):
    n = 4133
    es = parity(gs, oracle, dict(MEDIAN, n=n, drop_rate=drop, trial=1), tables(n, 3, seed0=11), 9, rounds=40)
    assert all(e.received > 0.9 * n for e in es)


def test_every_call_lost_reaches_max_ticks(gs, oracle):
    n, T = 777, 3
    kw = dict(MEDIAN, n=n, drop_rate=1.0, trial=0)
    tabs = tables(n, T, seed0=1)
    parity(gs, oracle, kw, tabs, 0, rounds=5)
    with gs.Simulator.median_batch(cfg_of(gs, kw, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(0)
        rows, st = sim.run(poll=10, max_ticks=30)
        assert st == MAX_TICKS and len(rows) == 3
        res = sim.trial_results()
        assert res[:, 8].tolist() == [MAX_TICKS] * T and res[:, 2].tolist() == [30] * T
        assert res[:, 3].tolist() == [30 * n] * T and not res[:, 4].any() and res[:, 6].tolist() == [1] * T
        assert sim.totals()["pending"] == T


# ---- 3. launch boundaries ---------------------------------------------------------------------
def test_launch_boundaries(gs, oracle):
    """gs_step(16), gs_step(1), gs_step(17): a full launch, a one-round launch and a call split into two
    launches equal 34 single steps; every read works between the calls."""
    n, T = 4133, 3
    kw = dict(MEDIAN, n=n, trial=5)
    tabs = tables(n, T, seed0=16)
    es = restatements(oracle, kw, tabs, -1, 2)
    tr = Truth(oracle, es, 5)
    with gs.Simulator.median_batch(cfg_of(gs, kw, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, -1)
        for call in (16, 1, 17):
            want = [tr.step() for _ in range(call)]
            got = sim.step(call)
            assert got.astype(np.int64).tolist() == want, f"step({call}) ending at round {es[0].t}"
            check_state(sim, es, f"after round {es[0].t}")
            assert sim.trial_results().tolist() == tr.results()
    assert es[0].t == 34 and all(e.removed.sum() > n // 2 for e in es)


# ---- 4. table shapes ------------------------------------------------------------------------------
def test_hub_takes_every_add_of_a_round(gs, oracle):
    """n = 20,000: about a third of the callers pick node 0.  While it is in B its signed word takes
    several thousand adds of both signs in one round, and its flag bits that many requests."""
    n, T = 20_000, 2
    kw = dict(MEDIAN, n=n, fanout=4, fanin=4, drop_rate=0.0, trial=0)
    tabs = tables(n, T, seed0=5, table=hub_table)
    es = restatements(oracle, kw, tabs, 7, 3)
    tr = Truth(oracle, es, 0)
    most, both = 0, False
    with gs.Simulator.median_batch(cfg_of(gs, kw, 3, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, 7)
        for _ in range(30):
            before = [e.state.copy() for e in es]
            step_all(sim, tr, 1)
            for e, S in zip(es, before):
                if 1 <= S[0] <= 3:
                    callers = e.last[0][e.last[1] == 0]
                    most = max(most, callers.size)
                    both |= bool((S[callers] >= S[0]).any() and (S[callers] < S[0]).any())
    assert most > 5000 and both and all(e.removed[0] for e in es)


def test_self_calls(gs, oracle):
    """Every row holds v itself twice: a self-call is one connection with two ends."""
    n, T = 2049, 3
    tabs = tables(n, T, seed0=33)
    for _, ids in tabs:
        ids[:, 2] = ids[:, 4] = np.arange(n)
    es = parity(gs, oracle, dict(MEDIAN, n=n, trial=0), tabs, 17, rounds=36)
    assert all((e.last[0] == e.last[1]).any() for e in es) and all(e.received > n // 2 for e in es)


@pytest.mark.parametrize("stride", [1, 255])
def test_row_lengths_1_and_255(gs, oracle, stride):
    n, T = 3001, 2
    tabs = []
    for i in range(T):
        deg = np.full(n, stride, np.uint8)
        ids = np.random.default_rng(stride + i).integers(0, n, size=(n, stride)).astype(np.uint32)
        ids[:, 0] = (np.arange(n) + 1) % n
        if stride == 1:
            deg[::7] = 0   # empty rows sprinkled in
        tabs.append((deg, ids))
    es = parity(gs, oracle, dict(MEDIAN, n=n, fanout=stride, fanin=stride, trial=0), tabs, 17, rounds=36)
    assert all(e.received > 1 for e in es)


@pytest.mark.parametrize("fanout,fanin", [(5, 6), (3, 4)])
def test_overlay_built_tables(gs, oracle, fanout, fanin):
    n, T = 5000, 3
    kw = dict(MEDIAN, n=n, fanout=fanout, fanin=fanin, trial=4)
    with gs.Simulator.median_batch(cfg_of(gs, kw, 2, trials=T, timing=True)) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        assert deg.shape == (T * n,) and not np.array_equal(deg[:n], deg[n:2 * n])
        tabs = [(deg[i * n:(i + 1) * n], ids[i * n:(i + 1) * n]) for i in range(T)]
        es = restatements(oracle, kw, tabs, -1, 2)
        begin(sim, es, -1)
        step_all(sim, Truth(oracle, es, 4), 32)
        tm = sim.timing()
        assert tm["deliver_launches"] == 32 and tm["deliver_ms"] > 0
    assert all(e.received > 0.9 * n for e in es)


# ---- 5. senders and masks -----------------------------------------------------------------------
def test_trials_have_their_own_senders(gs, oracle):
    n, T = 4133, 5
    kw = dict(MEDIAN, n=n, trial=7)
    tabs = tables(n, T, seed0=70)
    es = restatements(oracle, kw, tabs, -1, 2)
    senders = [int(np.nonzero(e.inf)[0][0]) for e in es]
    assert len(set(senders)) == T
    with gs.Simulator.median_batch(cfg_of(gs, kw, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, -1)
        st = sim.median_state()
        for i, s in enumerate(senders):
            assert np.array_equal(st[i], (np.arange(n) == s).astype(np.uint8)), i
        step_all(sim, Truth(oracle, es, 7), 12)


@pytest.mark.parametrize("mask", ["one_percent", "all_but_sender", "per_trial"])
def test_failure_masks(gs, oracle, mask):
    n, T = 4133, 3
    kw = dict(MEDIAN, n=n, drop_rate=0.0, trial=1)
    tabs = tables(n, T, seed0=9)
    if mask == "one_percent":
        dead = [np.random.default_rng(3).random(n) < 0.01 for _ in range(T)]
    elif mask == "all_but_sender":
        dead = [np.ones(n, bool) for _ in range(T)]
    else:
        dead = [np.random.default_rng(30 + i).random(n) < (0.02, 0.3, 0.6)[i] for i in range(T)]
    for d in dead:
        d[100] = False
    es = parity(gs, oracle, kw, tabs, 100, rounds=36, failed=dead)
    assert not any((e.inf & d).any() for e, d in zip(es, dead))
    if mask == "one_percent":
        assert all(e.received > 0.9 * n for e in es)
    elif mask == "all_but_sender":   # it calls a failed friend every round: sent, never a connection
        assert all(e.received == 1 and e.pending == 1 for e in es)
    else:
        assert len({e.received for e in es}) == T


def test_a_sender_failed_in_one_trial_only(gs, oracle):
    """Trial 1's fixed sender is failed: it never starts and its first poll is quiescent; the others run on."""
    n, T = 4133, 3
    kw = dict(MEDIAN, n=n, trial=0)
    tabs = tables(n, T, seed0=90)
    dead = [np.zeros(n, bool) for _ in range(T)]
    dead[1][100] = True
    masks = np.stack([words_of(d) for d in dead])
    es = parity(gs, oracle, kw, tabs, 100, k=5, rounds=12, failed=dead)
    assert es[1].received == 0 and es[1].pending == 0 and es[0].received > 100
    want = [reference_trial(oracle, dict(kw, trial=i), *tabs[i], 100, 5, dead[i], 10, 300) for i in range(T)]
    assert want[1][8] == QUIESCENT and want[1][2] == 10 and want[1][6] == 0 and want[1][3] > 0
    assert all(w[2] > 10 for w in (want[0], want[2]))
    with gs.Simulator.median_batch(cfg_of(gs, kw, 5, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(masks)
        sim.broadcast_begin(100)
        assert sim.totals()["pending"] == 2 and not sim.received()[1].any()
        rows, st = sim.run(poll=10, max_ticks=300)
        assert sim.trial_results().tolist() == want
        assert st == max(w[8] for w in want) and not sim.received()[1].any() and not sim.median_state()[1].any()
        sim.reset()   # keeps the masks
        assert np.array_equal(sim.crashed(), masks) and not sim.received().any() and not sim.median_state().any()


# ---- 6. against the GPU's own one-trial engine ------------------------------------------------------
def test_batch_equals_one_trial_contexts(gs):
    """trial = 7, T = 5: trials 7..11 of five one-trial gs_create contexts, round by round and under gs_run."""
    n, T, k = 4133, 5, 5
    kw = dict(MEDIAN, n=n, trial=7)
    tabs = tables(n, T, seed0=80)
    ones = []
    for i, (deg, ids) in enumerate(tabs):
        with gs.Simulator(cfg_of(gs, dict(kw, trial=7 + i), k)) as one:
            one.load_peers(deg, ids)
            one.broadcast_begin(-1)
            rows = one.step(25).astype(np.int64)
            sets = (one.median_state(), one.received(), one.removed())
            one.reset()
            one.broadcast_begin(-1)
            _, st = one.run(poll=10, max_ticks=200)
            ones.append((rows, sets, one.trial_results()[0], st, one.median_state()))
    with gs.Simulator.median_batch(cfg_of(gs, kw, k, trials=T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(-1)
        got = sim.step(25).astype(np.int64)
        want = sum(o[0] for o in ones)
        want[:, 0] = ones[0][0][:, 0]
        assert np.array_equal(got, want)
        st, rec, rem = sim.median_state(), sim.received(), sim.removed()
        for i, o in enumerate(ones):
            assert np.array_equal(st[i], o[1][0]) and np.array_equal(rec[i], o[1][1]), i
            assert np.array_equal(rem[i], o[1][2]), i
        sim.reset()
        sim.broadcast_begin(-1)
        _, status = sim.run(poll=10, max_ticks=200)
        assert np.array_equal(sim.trial_results(), np.array([o[2] for o in ones]))
        assert status == max(o[3] for o in ones)
        # a trial that stopped before the last poll went on like the one-trial context: A nodes still
        # call, nothing changes
        for i, o in enumerate(ones):
            if o[3] != MAX_TICKS:
                assert np.array_equal(sim.median_state()[i], o[4]), i


# ---- 7. gs_run ---------------------------------------------------------------------------------------
def reference_trial(oracle, kw, deg, ids, sender, k, failed, poll, max_ticks):
    """reference_run (tests/test_median.py) on one restatement, with the cumulative counters: the
    trial's gs_trial_results row."""
    e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, k, failed)
    cum = np.zeros(3, dtype=np.int64)
    plain = e.step

    def counted():
        row = plain()
        cum[:] += np.array(row[1:4], dtype=np.int64)
        return row
    e.step = counted
    status, tick_99 = reference_run(oracle, e, poll, max_ticks)
    return [kw["trial"], tick_99, e.t, *cum.tolist(), e.received, 0, status]


def default_k(n):
    """The CLI's rule for -model median without -k."""
    return min(127, math.ceil(math.log2(math.log2(max(4, n)))) + 1)


RUN_N, RUN_T, RUN_MAX = 4133, 4, 120


def run_truth_of(oracle, k, poll):
    kw = dict(MEDIAN, n=RUN_N, trial=3)
    tabs = tables(RUN_N, RUN_T, seed0=RUN_N + 100 * k)
    return tabs, [reference_trial(oracle, dict(kw, trial=3 + i), *tabs[i], 3, k, None, poll, RUN_MAX)
                  for i in range(RUN_T)]


@pytest.fixture(scope="module")
def run_truth(oracle):
    """Per (k, poll) the tables and the trials' rows (computed once)."""
    return {(k, poll): run_truth_of(oracle, k, poll) for k in (default_k(RUN_N), 1) for poll in (1, 3, 10, 64)}


@pytest.mark.parametrize("poll", [1, 3, 10, 64])
@pytest.mark.parametrize("k", [default_k(RUN_N), 1])
def test_run_stops_each_trial_at_its_own_poll(gs, run_truth, k, poll):
    kw = dict(MEDIAN, n=RUN_N, trial=3)
    tabs, want = run_truth[k, poll]
    with gs.Simulator.median_batch(cfg_of(gs, kw, k, trials=RUN_T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(3)
        rows, st = sim.run(poll=poll, max_ticks=RUN_MAX)
        got = sim.trial_results()
        assert got.tolist() == want, f"\n{got}\n{np.array(want)}"
        last = max(w[2] for w in want)
        assert st == max(w[8] for w in want) and len(rows) * poll == last == sim.totals()["tick"]
        stopped = [w[8] != MAX_TICKS for w in want]
        active = ((sim.median_state() != 0) & (sim.median_state() != 255)).sum(1)
        assert [a == 0 for a in active.tolist()] == stopped
        assert sim.totals()["pending"] == int(active.sum())
    if k == 1:      # a counter this short strands B nodes: those trials go to max_ticks
        assert any(w[8] == MAX_TICKS and w[2] >= RUN_MAX for w in want)
    else:           # with the CLI's default k a trial ends by itself
        assert any(w[8] == COVERED and w[2] < RUN_MAX for w in want)
        if poll == 1:
            assert len({w[2] for w in want}) > 1   # trials of one run stop at different polls
    assert all(w[1] % poll == 0 for w in want)


# ---- 8. lifecycle ----------------------------------------------------------------------------------------
def step_rows(sim, rounds):
    return sim.step(rounds).astype(np.int64).tolist()


def test_lifecycle(gs, oracle):
    n, T = 4133, 3
    kw, kw7 = dict(MEDIAN, n=n, trial=0), dict(MEDIAN, n=n, trial=3)
    tabs, tabs2 = tables(n, T, seed0=21), tables(n, T, seed0=61)
    with gs.Simulator.median_batch(cfg_of(gs, kw, trials=T)) as sim, \
            gs.Simulator.median_batch(cfg_of(gs, kw, trials=T)) as other:   # two batches alive at once
        sim.load_peers(*stacked(tabs))
        other.load_peers(*stacked(tabs2))
        sim.broadcast_begin(9)
        other.broadcast_begin(11)
        first, second = [], []
        for _ in range(30):   # side by side, a round each in turn
            first += step_rows(sim, 1)
            second += step_rows(other, 1)
        es, es2 = restatements(oracle, kw, tabs, 9, 2), restatements(oracle, kw, tabs2, 11, 2)
        assert first == [summed([e.step() for e in es]) for _ in range(30)]
        assert second == [summed([e.step() for e in es2]) for _ in range(30)]
        check_state(sim, es, "first batch")
        check_state(other, es2, "second batch")
        sets = (sim.median_state(), sim.received(), sim.removed())
        sim.reset()                      # a second broadcast equals the first
        assert not sim.received().any() and not sim.removed().any() and not sim.median_state().any()
        sim.broadcast_begin(9)
        assert step_rows(sim, 30) == first
        for a, b in zip(sets, (sim.median_state(), sim.received(), sim.removed())):
            assert np.array_equal(a, b)
        sim.reset()                      # set_trial(base + T) plus a new table: parity with the new numbers
        sim.set_trial(T)
        sim.load_peers(*stacked(tabs2))
        es7 = restatements(oracle, kw7, tabs2, -1, 2)
        begin(sim, es7, -1)
        step_all(sim, Truth(oracle, es7, T), 30, "after set_trial")


def test_load_peers_device(gs, oracle):
    """Tables back to back in device memory, as gs_load_peers takes them from the host."""
    n, T = 4133, 3
    kw = dict(MEDIAN, n=n, trial=2)
    tabs = tables(n, T, seed0=41)
    deg, ids = stacked(tabs)
    with open("/proc/self/maps") as f:   # the HIP runtime the library itself loaded
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    bufs = []
    try:
        for a in (deg, ids):
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), a.nbytes) == 0
            bufs.append(d)
            assert hip.hipMemcpy(d, a.ctypes.data, a.nbytes, 1) == 0   # hipMemcpyHostToDevice
        es = parity(gs, oracle, kw, tabs, 8, rounds=25,
                    load=lambda sim: sim.load_peers_device(bufs[0].value, bufs[1].value, ids.shape[1]))
        assert all(e.received > n // 2 for e in es)
        bad = ids.copy()
        bad[n + 5, 0] = n   # a friend id of trial 1 that is no node
        assert hip.hipMemcpy(bufs[1], bad.ctypes.data, bad.nbytes, 1) == 0
        with gs.Simulator.median_batch(cfg_of(gs, kw, trials=T)) as sim:
            with pytest.raises(gs.GossipError) as ei:
                sim.load_peers_device(bufs[0].value, bufs[1].value, ids.shape[1])
            assert ei.value.code == -1 and ">= n" in str(ei.value)
    finally:
        for d in bufs:
            hip.hipFree(d)


# ---- 9. the pinned refusals ----------------------------------------------------------------------------
def test_pinned_refusals_still_hold(gs, oracle):
    from test_rumor import RUMOR
    kw = dict(MEDIAN, n=4133)
    for make in (lambda: gs.Simulator.batch(cfg_of(gs, kw)), lambda: gs.Simulator.batch(cfg_of(gs, kw, trials=2)),
                 lambda: gs.Simulator(cfg_of(gs, kw, trials=2)),
                 lambda: gs.Simulator(cfg_of(gs, kw), devices=[0, 0])):
        with pytest.raises(gs.GossipError) as ei:
            make()
        assert ei.value.code == -1 and "GS_MODEL_MEDIAN" in str(ei.value)
    with gs.Simulator.median_batch(cfg_of(gs, kw, trials=2)) as sim:
        with pytest.raises(gs.GossipError) as ei:   # a shorter buffer than trials * n bytes
            sim._check(sim.L.gs_read_median_state(sim.h, np.zeros(2 * 4133 - 1, np.uint8).ctypes.data, 2 * 4133 - 1),
                       "gs_read_median_state")
        assert ei.value.code == -1
    # median_batch of a rumor config is batch of it
    n, T = 2000, 3
    rk = dict(RUMOR, n=n, trial=1)
    rcfg = gs.Config(n=n, droprate=rk["drop_rate"], crashrate=0.0, seed=rk["seed"], trial=1, model="rumor", rumor_k=2,
                     trials=T)
    deg, ids = stacked(tables(n, T, seed0=3))
    got = []
    for make in (gs.Simulator.batch, gs.Simulator.median_batch):
        with make(rcfg) as sim:
            sim.load_peers(deg, ids)
            sim.broadcast_begin(-1)
            got.append((sim.step(20).tolist(), sim.received().tolist(), sim.removed().tolist()))
    assert got[0] == got[1] and got[0][0][-1][4] > T


# ---- 10. CLI -------------------------------------------------------------------------------------------
def test_cli_prints_the_trials_and_their_statistics(gs):
    from gossip_simulator_amd import _lib
    n, T, seed = 4133, 4, 9
    r = subprocess.run([_lib.CLI_PATH, "-n", str(n), "-model", "median", "-batch", str(T), "-seed", str(seed),
                        "-maxticks", "3000"], capture_output=True, text=True, timeout=300)   # (the overlay's limit too)
    lines = re.findall(r"^trial (\d+): Residue (\S+), (\S+) messages per node after (\S+), (\w+), stranded (\d+)$",
                       r.stdout, re.M)
    assert len(lines) == T, r.stdout + r.stderr
    with gs.Simulator.median_batch(gs.Config(n=n, seed=seed, trials=T, model="median", rumor_k=default_k(n))) as sim:
        sim.build_overlay()
        sim.broadcast_begin(-1)
        sim.run(poll=10, max_ticks=3000)
        res = sim.trial_results()
        st = sim.median_state()
    stranded = ((st != 0) & (st != 255)).sum(1)
    names = {COVERED: "covered", QUIESCENT: "quiescent", MAX_TICKS: "maxticks"}
    want = [(str(int(x[0])), _lib.format_float32(float(np.float32(1) - np.float32(int(x[6])) / np.float32(n))),
             _lib.format_float32(float(np.float32(int(x[5])) / np.float32(n))),
             _lib.format_duration(int(x[2]) * 1_000_000), names[int(x[8])], str(int(s)))
            for x, s in zip(res, stranded)]
    assert lines == want
    m = re.search(r"^--- 4 trials: residue mean (\S+) sd (\S+), messages per node mean (\S+) sd (\S+), "
                  r"rounds mean (\S+) sd (\S+), stranded mean (\S+) sd (\S+) ---$", r.stdout, re.M)
    assert m, r.stdout
    got = [float(x) for x in m.groups()]
    cols = [1.0 - res[:, 6] / n, res[:, 5] / n, res[:, 2].astype(np.float64), stranded.astype(np.float64)]
    want = [f(c) for c in cols for f in (np.mean, lambda c: np.std(c, ddof=1))]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-15), (got, want)
    ended = all(int(x[8]) != MAX_TICKS for x in res)
    assert r.returncode == (0 if ended else 3)
    assert [int(s) == 0 for s in stranded] == [int(x[8]) != MAX_TICKS for x in res]
    assert "=== Constructing Overlay ===" in r.stdout and "=== Broadcast one message ===" in r.stdout


# ---- 11. non-vacuity -------------------------------------------------------------------------------------
NV = dict(n=4133, T=3, k=2, rounds=30, seed0=11, sender=9)


def wrong_diverges(oracle, true_states, wrong):
    """Per trial the first round (0-based) at which the wrong restatement's state bytes differ from
    true_states[round][trial]; from there on they must differ in every round."""
    kw = dict(MEDIAN, n=NV["n"], trial=1)
    es = restatements(oracle, kw, tables(NV["n"], NV["T"], NV["seed0"]), NV["sender"], NV["k"], wrong=wrong)
    firsts = []
    for i, e in enumerate(es):
        diff = []
        for r in range(NV["rounds"]):
            e.step()
            diff.append(not np.array_equal(e.st, true_states[r][i]))
        assert any(diff), f"{wrong}: trial {i} never diverges"
        first = diff.index(True)
        assert all(diff[first:]), f"{wrong}: trial {i} agrees again after round {first + 1}"
        firsts.append(first)
    return firsts


def test_the_sweep_would_catch_a_dropped_own_end(gs, oracle):
    """The caller's own end is what this kernel folds into diff and the flag sets.  Against the GPU's own
    states of a sweep case (equal to the true restatement's), a restatement that drops the own end and one
    that counts a C partner as B both differ from some early round on."""
    kw = dict(MEDIAN, n=NV["n"], trial=1)
    tabs = tables(NV["n"], NV["T"], NV["seed0"])
    es = restatements(oracle, kw, tabs, NV["sender"], NV["k"])
    gpu = []
    with gs.Simulator.median_batch(cfg_of(gs, kw, NV["k"], trials=NV["T"])) as sim:
        sim.load_peers(*stacked(tabs))
        sim.broadcast_begin(NV["sender"])
        for r in range(NV["rounds"]):
            sim.step(1)
            gpu.append(sim.median_state())
            for i, e in enumerate(es):
                e.step()
                assert np.array_equal(gpu[-1][i], e.st), f"round {r + 1}: trial {i}"
    for wrong in ("no_own", "c_as_b"):
        firsts = wrong_diverges(oracle, gpu, wrong)
        assert all(f < NV["rounds"] // 2 for f in firsts), (wrong, firsts)
