"""The HIP rumor engine (gs_rumor.hip) against the Python restatement of
tests/test_rumor.py: bit-exact per round -- the stats rows, the informed set
and the removed set after every gs_step(1) -- over the shapes at which the
kernels can go wrong, then gs_run's stop rule, the lifecycle calls and the
combinations the model refuses.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumor import RUMOR, PyRumor, words_of

pytestmark = pytest.mark.gpu

RUN_NAMES = {0: "COVERED", 1: "QUIESCENT", 2: "MAX_TICKS"}


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def cfg_of(gs, kw, k=2, **more):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], model="rumor", rumor_k=k, **more)


def check_round(sim, e, got, row, t):
    assert [int(x) for x in got] == row, f"round {t}:\n{got}\n{row}"
    assert np.array_equal(sim.received(), words_of(e.inf)), f"informed set differs at round {t}"
    assert np.array_equal(sim.removed(), words_of(e.removed)), f"removed set differs at round {t}"


def parity(gs, oracle, kw, deg, ids, sender, k=2, rounds=40, failed=None):
    """gs_step(1) x rounds against the restatement; returns the last row."""
    p = oracle.make_params(**kw)
    e = PyRumor(oracle, p, deg, masked(deg, ids), sender, k, failed)
    with gs.Simulator(cfg_of(gs, kw, k)) as sim:
        sim.load_peers(deg, ids)
        if failed is not None:
            sim.set_failed(words_of(failed))
        sim.broadcast_begin(sender)
        tot = sim.totals()
        assert (tot["received"], tot["pending"]) == (e.received, e.pending)
        assert np.array_equal(sim.received(), words_of(e.inf))
        assert np.array_equal(sim.removed(), words_of(e.removed))
        if failed is not None:
            assert np.array_equal(sim.crashed(), words_of(failed))
        row = None
        for t in range(1, rounds + 1):
            row = e.step()
            check_round(sim, e, sim.step(1)[0], row, t)
        tot = sim.totals()
        assert tot["tick"] == rounds and tot["received"] == e.received and tot["pending"] == e.pending
    return row


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 777, 4133])
def test_word_edges(gs, oracle, n):
    deg, ids = random_table(n, 6, 0 if n > 2 else 1, 6, seed=n)
    parity(gs, oracle, dict(RUMOR, n=n), deg, ids, sender=n // 2)


@pytest.mark.parametrize("k", [1, 255])
def test_k_extremes(gs, oracle, k):
    n = 777
    deg, ids = random_table(n, 6, 1, 6, seed=k)
    row = parity(gs, oracle, dict(RUMOR, n=n), deg, ids, sender=5, k=k)
    # k = 1 has fallen quiet within 40 rounds; with k = 255 nobody has cooled off yet
    assert (row[6] == 0) == (k == 1)


@pytest.mark.parametrize("stride", [1, 8, 32])
def test_row_shapes(gs, oracle, stride):
    n = 3001
    deg, ids = random_table(n, stride, 0, stride, seed=stride)  # degrees 0..stride: informed nodes with no friend
    deg[17] = stride
    kw = dict(RUMOR, n=n, fanout=stride, fanin=stride)
    row = parity(gs, oracle, kw, deg, ids, sender=17, rounds=40 if stride > 1 else 60)
    assert row[4] > 1


@pytest.mark.parametrize("frac,sender_failed", [(0.05, False), (0.5, False), (0.05, True)])
def test_failure_masks(gs, oracle, frac, sender_failed):
    n = 4133
    deg, ids = random_table(n, 6, 1, 6, seed=9)
    dead = np.random.default_rng(3).random(n) < frac
    dead[100] = sender_failed
    kw = dict(RUMOR, n=n, drop_rate=0.0)
    p = oracle.make_params(**kw)
    e = PyRumor(oracle, p, deg, masked(deg, ids), 100, 2, dead)
    rows = e.run(40)
    if sender_failed:
        assert not rows[:, 1:].any()
    else:  # calls to failed callees: sent without messages (drop 0: sent = fired)
        assert (rows[:, 2] == rows[:, 1]).all() and int(rows[:, 3].sum()) < int(rows[:, 2].sum())
    parity(gs, oracle, kw, deg, ids, 100, failed=dead)


@pytest.mark.parametrize("leaves", [32, 20_000])
def test_star_duplicate_suppression(gs, oracle, leaves):
    """A star: every leaf's only friend is node 0, node 0 has 32 friends, the
    sender is a leaf.  Node 0 must enter a list exactly once however many
    leaves push into its one bit (pending and received equal the
    restatement's), and every later push into it is a miss of the leaf.
    (With one sender the model cannot make thousands of leaves hot while node
    0 is still uninformed -- node 0 is every leaf's only way to anyone -- so
    same-round pushes into one fresh bit are exercised by the random tables
    here and in test_list_growth_past_one_grid_pass, where several callers
    pick the same fresh node in one round; this star pins the hub's single
    entry and the leaves' misses at 20,000 rows of one slot.)"""
    n = leaves + 1
    deg = np.ones(n, np.uint8)
    ids = np.zeros((n, 32), np.uint32)
    deg[0] = 32
    ids[0] = 1 + (np.arange(32) * 617) % leaves
    kw = dict(RUMOR, n=n, fanout=32, fanin=32, drop_rate=0.0)
    row = parity(gs, oracle, kw, deg, ids, sender=7, k=2, rounds=40)
    assert row[4] > 2


def test_same_round_pushes_into_fresh_bits(gs, oracle):
    """A dense funnel: 20,000 callers whose rows name only 50 targets, so at
    the growth rounds many lanes push into the same fresh bit in one round;
    each target must be listed once (pending equals the restatement's)."""
    n, targets = 20_050, 50
    rng = np.random.default_rng(8)
    deg = np.full(n, 6, np.uint8)
    ids = rng.integers(targets, n, size=(n, 6)).astype(np.uint32)   # callers name callers ...
    ids[targets:, 5] = rng.integers(0, targets, size=n - targets)   # ... and one target each
    ids[:targets] = rng.integers(targets, n, size=(targets, 6))
    kw = dict(RUMOR, n=n)
    e = PyRumor(oracle, oracle.make_params(**kw), deg, ids, 4000, 255)
    with gs.Simulator(cfg_of(gs, kw, 255)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(4000)
        writers = 0
        for t in range(1, 26):
            check_round(sim, e, sim.step(1)[0], e.step(), t)
            if e.last_fresh.size:  # the most callers that reached one fresh node in this round
                writers = max(writers, int(np.bincount(e.last_fresh).max()))
    assert writers >= 3


@pytest.fixture(scope="module")
def big(oracle):
    """n = 300,000 to quiescence, k = 3: the restatement's rows, and its sets
    after rounds 1..5 and at the end (computed once, shared)."""
    n = 300_000
    deg, ids = random_table(n, 6, 5, 6, seed=300)
    kw = dict(RUMOR, n=n)
    e = PyRumor(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 12345, 3)
    rows, sets = [], {}
    while True:
        rows.append(e.step())
        if e.t <= 5:
            sets[e.t] = (words_of(e.inf), words_of(e.removed))
        if e.pending == 0:
            break
        assert e.t < 500
    sets[e.t] = (words_of(e.inf), words_of(e.removed))
    return kw, deg, ids, rows, sets


@pytest.mark.parametrize("grid", [None, "16"])
def test_list_growth_past_one_grid_pass(gs, big, grid, monkeypatch):
    """The hot list peaks above 180,000 entries: dozens of passes of a 16-block
    grid (4,096 lanes; GS_RUMOR_GRID), and one pass of the default grid, which
    has a lane per node at this n."""
    kw, deg, ids, rows, sets = big
    if grid:
        monkeypatch.setenv("GS_RUMOR_GRID", grid)
    peak = max(r[6] for r in rows)
    assert peak > 16 * 256 * 4
    with gs.Simulator(cfg_of(gs, kw, 3)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(12345)
        for t, row in enumerate(rows, 1):
            got = sim.step(1)[0]
            assert [int(x) for x in got] == row, f"round {t}"
            if t in sets:
                assert np.array_equal(sim.received(), sets[t][0]), t
                assert np.array_equal(sim.removed(), sets[t][1]), t
        assert sim.totals()["pending"] == 0
        assert [int(x) for x in sim.step(1)[0]] == [len(rows) + 1, 0, 0, 0, rows[-1][4], 0, 0]


def reference_run(oracle, kw, deg, ids, sender, k, poll, max_ticks):
    """gs_run's rule on the restatement: polls every `poll` rounds; stops at
    the first poll with nobody hot, or at max_ticks."""
    e = PyRumor(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, k)
    tick_99 = 0
    while True:
        for _ in range(poll):
            e.step()
        cov = oracle.covered(e.received, e.n)
        if cov and not tick_99:
            tick_99 = e.t
        if e.pending == 0:
            return e, (0 if cov else 1), tick_99
        if e.t >= max_ticks:
            return e, 2, tick_99


@pytest.mark.parametrize("n,k,expect", [(4133, 8, "COVERED"), (4133, 1, "QUIESCENT")])
@pytest.mark.parametrize("poll", [10, 1])
def test_run_stops_where_stepping_does(gs, oracle, n, k, expect, poll):
    deg, ids = random_table(n, 6, 5, 6, seed=n + k)
    kw = dict(RUMOR, n=n)
    e, status, tick_99 = reference_run(oracle, kw, deg, ids, 3, k, poll, 10_000)
    assert RUN_NAMES[status] == expect
    with gs.Simulator(cfg_of(gs, kw, k)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(3)
        rows, st = sim.run(poll=poll, max_ticks=10_000)
        assert st == status and len(rows) * poll == e.t
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (e.t, e.received, 0)
        assert np.array_equal(sim.received(), words_of(e.inf))
        assert np.array_equal(sim.removed(), words_of(e.removed))
        tr = dict(zip(gs.engine.TRIAL_FIELDS, sim.trial_results()[0]))
        assert tr["tick_99"] == tick_99 and tr["status"] == status and tr["tick"] == e.t
        assert tr["received"] == e.received and tr["messages"] == tot["messages"]
    # the same state as stepping to that tick
    e2 = PyRumor(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 3, k)
    r2 = e2.run(e.t)
    assert int(r2[:, 3].sum()) == tot["messages"] and int(r2[:, 1].sum()) == tot["fired"]


def test_run_every_call_lost_reaches_max_ticks(gs, oracle):
    n = 777
    deg, ids = random_table(n, 6, 1, 6, seed=1)
    kw = dict(RUMOR, n=n, drop_rate=1.0)
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(0)
        rows, st = sim.run(poll=10, max_ticks=30)
        assert RUN_NAMES[st] == "MAX_TICKS" and len(rows) == 3
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"], tot["sent"]) == (30, 1, 1, 0)


def steps(sim, rounds):
    return [[int(x) for x in sim.step(1)[0]] for _ in range(rounds)]


def test_lifecycle_reset_trial_and_mask(gs, oracle):
    n = 4133
    deg, ids = random_table(n, 6, 1, 6, seed=21)
    deg2, ids2 = random_table(n, 6, 1, 6, seed=22)
    dead = np.random.default_rng(5).random(n) < 0.1
    dead[9] = False
    kw = dict(RUMOR, n=n)
    ref = PyRumor(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 9, 2).run(30).tolist()
    ref_masked = PyRumor(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 9, 2, dead).run(30).tolist()
    kw7 = dict(kw, trial=7)
    ref7 = PyRumor(oracle, oracle.make_params(**kw7), deg2, masked(deg2, ids2), -1, 2).run(30).tolist()
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(9)
        assert steps(sim, 30) == ref
        sim.reset()                      # a second broadcast equals the first
        assert not sim.received().any() and not sim.removed().any()
        sim.broadcast_begin(9)
        assert steps(sim, 30) == ref
        sim.reset()
        sim.set_failed(words_of(dead))   # set_failed, then reset keeps the mask
        sim.broadcast_begin(9)
        assert steps(sim, 30) == ref_masked
        sim.reset()
        assert np.array_equal(sim.crashed(), words_of(dead))
        sim.broadcast_begin(9)
        assert steps(sim, 30) == ref_masked
    with gs.Simulator(cfg_of(gs, kw)) as sim:   # set_trial plus a new table equals a fresh context
        sim.load_peers(deg, ids)
        sim.broadcast_begin(9)
        sim.step(5)
        sim.reset()
        sim.set_trial(7)
        sim.load_peers(deg2, ids2)
        sim.broadcast_begin(-1)
        a = steps(sim, 30)
    with gs.Simulator(cfg_of(gs, kw7)) as sim:
        sim.load_peers(deg2, ids2)
        sim.broadcast_begin(-1)
        assert steps(sim, 30) == a == ref7


def test_overlay_then_rumor(gs, oracle):
    kw = dict(RUMOR, n=5000)
    with gs.Simulator(cfg_of(gs, kw, timing=True)) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        e = PyRumor(oracle, oracle.make_params(**kw), deg, masked(deg, ids), -1, 2)
        sim.broadcast_begin(-1)
        for t in range(1, 41):
            check_round(sim, e, sim.step(1)[0], e.step(), t)
        tm = sim.timing()
        assert tm["deliver_launches"] == 40 and tm["deliver_ms"] > 0


def test_refusals(gs):
    kw = dict(RUMOR, n=20000)
    for make, word in ((lambda: gs.Simulator(cfg_of(gs, kw, trials=2)), "trials"),
                       (lambda: gs.Simulator(cfg_of(gs, kw), devices=[0, 0]), "gs_create_multi"),
                       (lambda: gs.Simulator.rank(cfg_of(gs, kw), 2, 0, None), "gs_create_rank")):
        with pytest.raises(gs.GossipError) as ei:
            make()
        assert ei.value.code == -1 and word in str(ei.value) and "GS_MODEL_RUMOR" in str(ei.value)
    with gs.Simulator(gs.Config(n=1000, model="pushpull")) as sim:
        with pytest.raises(gs.GossipError) as ei:
            sim.removed()
        assert ei.value.code == -1 and "GS_MODEL_RUMOR" in str(ei.value)


@pytest.mark.parametrize("model", [0, 1])
def test_other_models_unchanged(gs, oracle, model):
    n = 4133
    deg, ids = random_table(n, 6, 1, 6, seed=4)
    kw = dict(RUMOR, n=n, model=model, crash_rate=0.0)
    e = oracle.Engine(oracle.make_params(**kw), deg, ids)
    e.begin(5)
    cfg = gs.Config(n=n, droprate=0.1, crashrate=0.0, seed=kw["seed"], model="pushpull" if model else "flood")
    with gs.Simulator(cfg) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(5)
        for _ in range(6):
            assert np.array_equal(e.step(10), sim.step(10))
        assert np.array_equal(e.received(), sim.received())
