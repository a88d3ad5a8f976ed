"""The HIP rumor engines in every mode of gs_params.rumor_mode (gs_rumor.hip:
the list engine's blind and coin instantiations, and the pull modes' dense
engine) against the Python restatement of tests/test_rumor_modes.py: bit-exact
per round -- the stats row, the informed set and the removed set after every
gs_step(1) -- over the shapes at which the kernels can go wrong, then gs_run's
stop rule, the lifecycle calls, the timing counters and a bad mode word.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumor import RUMOR, words_of
from test_rumor_gpu import RUN_NAMES, check_round, steps
from test_rumor_modes import BLIND, COIN, PULL, PyRumorModes

pytestmark = pytest.mark.gpu

MODE_NAMES = {m: "+".join(w for b, w in ((PULL, "pull"), (BLIND, "blind"), (COIN, "coin")) if m & b) or "mode0"
              for m in range(8)}


def mode_id(m):
    return MODE_NAMES[m]


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def cfg_of(gs, kw, k=2, mode=0, **more):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], model="rumor", rumor_k=k,
                     rumor_blind=bool(mode & BLIND), rumor_coin=bool(mode & COIN), rumor_pull=bool(mode & PULL),
                     **more)


def parity(gs, oracle, kw, deg, ids, sender, mode, k=2, rounds=40, failed=None):
    """gs_step(1) x rounds against the restatement; returns the restatement and its last row."""
    p = oracle.make_params(**kw)
    e = PyRumorModes(oracle, p, deg, masked(deg, ids), sender, k, failed, mode)
    with gs.Simulator(cfg_of(gs, kw, k, mode)) as sim:
        sim.load_peers(deg, ids)
        if failed is not None:
            sim.set_failed(words_of(failed))
        sim.broadcast_begin(sender)
        tot = sim.totals()
        assert (tot["received"], tot["pending"]) == (e.received, e.pending)
        assert np.array_equal(sim.received(), words_of(e.inf))
        assert np.array_equal(sim.removed(), words_of(e.removed))
        row = None
        for t in range(1, rounds + 1):
            row = e.step()
            check_round(sim, e, sim.step(1)[0], row, t)
        tot = sim.totals()
        assert tot["tick"] == rounds and tot["received"] == e.received and tot["pending"] == e.pending
    return e, row


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 777, 4133])
@pytest.mark.parametrize("mode", range(1, 8), ids=mode_id)
def test_word_edges(gs, oracle, mode, n):
    deg, ids = random_table(n, 6, 0 if n > 2 else 1, 6, seed=n)
    e, row = parity(gs, oracle, dict(RUMOR, n=n), deg, ids, sender=n // 2, mode=mode)
    if n == 4133 and not mode & BLIND:  # (blind with k = 2 dies out early; test_k_extremes spreads it)
        assert row[4] > n // 2


def test_mode_0_through_the_new_arguments(gs, oracle):
    n = 4133
    deg, ids = random_table(n, 6, 0, 6, seed=n)
    from test_rumor import PyRumor
    e, row = parity(gs, oracle, dict(RUMOR, n=n), deg, ids, sender=n // 2, mode=0)
    ref = PyRumor(oracle, oracle.make_params(**dict(RUMOR, n=n)), deg, masked(deg, ids), n // 2, 2)
    assert ref.run(40)[-1].tolist() == row and np.array_equal(ref.hot, e.hot)


@pytest.mark.parametrize("k", [1, 255])
@pytest.mark.parametrize("mode", [COIN, COIN | BLIND, PULL, PULL | BLIND, PULL | COIN, PULL | COIN | BLIND],
                         ids=mode_id)
def test_k_extremes(gs, oracle, mode, k):
    n = 777
    deg, ids = random_table(n, 6, 1, 6, seed=k)
    e, row = parity(gs, oracle, dict(RUMOR, n=n), deg, ids, sender=5, mode=mode, k=k)
    if k == 1:  # every event removes: quiet within 40 rounds
        # (feedback pull: the informed nodes that nobody's row names stay hot)
        assert row[6] == 0 or (mode & PULL and not mode & BLIND)
    elif mode & BLIND:
        assert row[4] > 700
    elif not mode & COIN:  # 255 misses take more than 40 rounds
        assert row[6] == row[4]


@pytest.mark.parametrize("stride", [1, 8, 32])
@pytest.mark.parametrize("mode", [BLIND | COIN, PULL, PULL | BLIND], ids=mode_id)
def test_row_shapes(gs, oracle, mode, stride):
    n = 3001
    deg, ids = random_table(n, stride, 0, stride, seed=stride)  # degrees 0..stride: informed nodes with no friend
    deg[17] = stride
    kw = dict(RUMOR, n=n, fanout=stride, fanin=stride)
    e, row = parity(gs, oracle, kw, deg, ids, sender=17, mode=mode, k=6, rounds=40 if stride > 1 else 60)
    assert row[4] > 1 or stride == 1
    if not mode & PULL and stride > 1:  # informed nodes with an empty row: removed at once
        assert (e.inf & (e.deg == 0)).any()
    if mode & PULL:  # a node with an empty row never calls, so it never learns the rumor
        assert not (e.inf & (e.deg == 0)).any()


@pytest.mark.parametrize("n", [1, 3001])
@pytest.mark.parametrize("mode", [PULL, PULL | BLIND], ids=mode_id)
def test_pull_hot_sender_with_no_friend(gs, oracle, mode, n):
    """In pull only the sender can be informed with an empty row (a node that
    never calls never learns the rumor).  It is hot all the same: it answers
    the callers whose rows name it and never calls itself.  (The push rule --
    no friend: removed at once -- would leave received at 1 here.)"""
    deg, ids = random_table(n, 6, 0, 6, seed=n + 1)
    sender = 17 % n
    deg[sender] = 0
    named = np.arange(3, n, 7)           # every seventh row names the sender in its first slot
    named = named[named != sender]
    deg[named] = np.maximum(deg[named], 1)
    ids[named, 0] = sender
    e, row = parity(gs, oracle, dict(RUMOR, n=n, drop_rate=0.0), deg, ids, sender=sender, mode=mode, k=6)
    if n == 1:  # nobody can call it: feedback stays hot for ever, blind cools off after k rounds
        assert row == [40, 0, 0, 0, 1, 0, 0 if mode & BLIND else 1]
        return
    assert e.deg[sender] == 0 and e.inf[sender] and row[4] > 1000   # it served its callers
    assert e.removed[sender]                                        # and cooled off in the end
    assert not (e.inf & (e.deg == 0))[np.arange(n) != sender].any()


@pytest.mark.parametrize("frac,sender_failed", [(0.05, False), (0.5, False), (0.05, True)])
@pytest.mark.parametrize("mode", [BLIND, PULL, PULL | BLIND], ids=mode_id)
def test_failure_masks(gs, oracle, mode, frac, sender_failed):
    n = 4133
    deg, ids = random_table(n, 6, 1, 6, seed=9)
    dead = np.random.default_rng(3).random(n) < frac
    dead[100] = sender_failed
    kw = dict(RUMOR, n=n, drop_rate=0.0)
    e, row = parity(gs, oracle, kw, deg, ids, 100, mode, k=6, failed=dead)
    if sender_failed:
        assert row[4] == 0 and row[6] == 0
    else:
        assert row[4] > (1000 if frac < 0.5 else 0) and not (e.inf & dead).any()


def test_pull_funnel_contention(gs, oracle):
    """The 20,050-node funnel: 20,000 callers whose sixth slot names one of 50
    targets, all in word 0.  About 3,000 callers a round ask a target, some 60
    each, so once the targets are hot one word of `served`, then of `vain`,
    takes thousands of requests in a round and each of its bits dozens; the
    events must be the restatement's (pending, removed)."""
    n, targets = 20_050, 50
    rng = np.random.default_rng(8)
    deg = np.full(n, 6, np.uint8)
    ids = rng.integers(targets, n, size=(n, 6)).astype(np.uint32)
    ids[targets:, 5] = rng.integers(0, targets, size=n - targets)
    ids[:targets] = rng.integers(targets, n, size=(targets, 6))
    kw = dict(RUMOR, n=n)
    e = PyRumorModes(oracle, oracle.make_params(**kw), deg, ids, 7, 4, None, PULL)
    with gs.Simulator(cfg_of(gs, kw, 4, PULL)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(7)
        served = vain = 0
        for t in range(1, 31):
            check_round(sim, e, sim.step(1)[0], e.step(), t)
            for got, name in ((e.last_served, "served"), (e.last_vain, "vain")):
                if got.size:
                    most = int(np.bincount(got).max())
                    served, vain = (max(served, most), vain) if name == "served" else (served, max(vain, most))
    assert served >= 50 and vain >= 50, (served, vain)


def ring_table(n, seed):
    """A random table whose first slot is a ring, so every node has a caller:
    with feedback a hot node that nobody ever asks stays hot for ever."""
    deg, ids = random_table(n, 6, 5, 6, seed=seed)
    ids[:, 0] = (np.arange(n) + 1) % n
    return deg, ids


@pytest.fixture(scope="module")
def big(oracle):
    """n = 300,000 in feedback pull, k = 2, to quiescence (80 rounds): the
    restatement's rows and its sets after every round (computed once; 2 x 37 KB
    per round)."""
    n = 300_000
    deg, ids = ring_table(n, 300)
    kw = dict(RUMOR, n=n)
    e = PyRumorModes(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 12345, 2, None, PULL)
    rows, sets = [], []
    while True:
        rows.append(e.step())
        sets.append((words_of(e.inf), words_of(e.removed)))
        if e.pending == 0:
            break
        assert e.t < 200
    return kw, deg, ids, rows, sets


def test_pull_word_range_in_many_grid_passes(gs, big, monkeypatch):
    """4,688 words through a 16-block grid (64 waves; GS_RUMOR_GRID): 74 passes."""
    kw, deg, ids, rows, sets = big
    monkeypatch.setenv("GS_RUMOR_GRID", "16")
    assert rows[-1][4] > 0.99 * kw["n"]
    with gs.Simulator(cfg_of(gs, kw, 2, PULL)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(12345)
        assert np.array_equal(sim.received(), words_of(np.arange(kw["n"]) == 12345)) and not sim.removed().any()
        for t, (row, (inf, removed)) in enumerate(zip(rows, sets), 1):
            got = sim.step(1)[0]
            assert [int(x) for x in got] == row, f"round {t}"
            assert np.array_equal(sim.received(), inf), f"informed set differs at round {t}"
            assert np.array_equal(sim.removed(), removed), f"removed set differs at round {t}"
        assert sim.totals()["pending"] == 0


@pytest.mark.parametrize("mode", [PULL, PULL | BLIND | COIN, BLIND], ids=mode_id)
def test_grid_of_one_block(gs, oracle, mode, monkeypatch):
    monkeypatch.setenv("GS_RUMOR_GRID", "1")
    n = 4133
    deg, ids = random_table(n, 6, 1, 6, seed=77)
    parity(gs, oracle, dict(RUMOR, n=n), deg, ids, sender=4132, mode=mode, k=3)


def reference_run(oracle, kw, deg, ids, sender, k, mode, poll, max_ticks):
    """gs_run's rule on the restatement: polls every `poll` rounds; stops at
    the first poll with nobody hot, or at max_ticks."""
    e = PyRumorModes(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, k, None, mode)
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


@pytest.mark.parametrize("mode,k,expect", [(BLIND, 16, "COVERED"), (BLIND, 1, "QUIESCENT"), (COIN, 16, "QUIESCENT"),
                                           (COIN, 1, "QUIESCENT"), (PULL, 2, "COVERED"), (PULL, 1, "QUIESCENT")],
                         ids=lambda x: x if isinstance(x, str) else None)
@pytest.mark.parametrize("poll", [10, 1])
def test_run_stops_where_stepping_does(gs, oracle, mode, k, expect, poll):
    n = 4133
    deg, ids = ring_table(n, n + k) if mode & PULL else random_table(n, 6, 5, 6, seed=n + k)
    kw = dict(RUMOR, n=n)
    e, status, tick_99 = reference_run(oracle, kw, deg, ids, 3, k, mode, poll, 10_000)
    assert RUN_NAMES[status] == expect
    with gs.Simulator(cfg_of(gs, kw, k, mode)) as sim:
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
    e2 = PyRumorModes(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 3, k, None, mode)
    r2 = e2.run(e.t)
    assert int(r2[:, 3].sum()) == tot["messages"] and int(r2[:, 1].sum()) == tot["fired"]


def test_run_feedback_pull_with_an_unasked_hot_node_reaches_max_ticks(gs, oracle):
    """Nobody's row names the sender: it is hot, nobody asks it, no event ever."""
    n = 777
    rng = np.random.default_rng(4)
    deg = np.full(n, 6, np.uint8)
    ids = rng.integers(1, n, size=(n, 6)).astype(np.uint32)
    kw = dict(RUMOR, n=n)
    with gs.Simulator(cfg_of(gs, kw, 2, PULL)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(0)
        rows, st = sim.run(poll=10, max_ticks=30)
        assert RUN_NAMES[st] == "MAX_TICKS" and len(rows) == 3
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"], tot["fired"]) == (30, 1, 1, 30 * n)
        assert not sim.removed().any()
    # the blind node loses interest by itself
    with gs.Simulator(cfg_of(gs, kw, 2, PULL | BLIND)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(0)
        rows, st = sim.run(poll=10, max_ticks=30)
        assert RUN_NAMES[st] == "QUIESCENT" and len(rows) == 1
        assert np.array_equal(sim.removed(), sim.received())


def test_lifecycle_reset_trial_and_mask(gs, oracle):
    n = 4133
    deg, ids = random_table(n, 6, 1, 6, seed=21)
    deg2, ids2 = random_table(n, 6, 1, 6, seed=22)
    dead = np.random.default_rng(5).random(n) < 0.1
    dead[9] = False
    kw = dict(RUMOR, n=n)

    def ref_of(kw, deg, ids, sender, failed=None):
        return PyRumorModes(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, 2, failed,
                            PULL).run(30).tolist()
    ref, ref_masked = ref_of(kw, deg, ids, 9), ref_of(kw, deg, ids, 9, dead)
    kw7 = dict(kw, trial=7)
    ref7 = ref_of(kw7, deg2, ids2, -1)
    with gs.Simulator(cfg_of(gs, kw, 2, PULL)) as sim:
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
    with gs.Simulator(cfg_of(gs, kw, 2, PULL)) as sim:   # set_trial plus a new table equals a fresh context
        sim.load_peers(deg, ids)
        sim.broadcast_begin(9)
        sim.step(5)
        sim.reset()
        sim.set_trial(7)
        sim.load_peers(deg2, ids2)
        sim.broadcast_begin(-1)
        a = steps(sim, 30)
    with gs.Simulator(cfg_of(gs, kw7, 2, PULL)) as sim:
        sim.load_peers(deg2, ids2)
        sim.broadcast_begin(-1)
        assert steps(sim, 30) == a == ref7


def test_timing_counts_one_deliver_launch_per_round(gs, oracle):
    kw = dict(RUMOR, n=5000)
    with gs.Simulator(cfg_of(gs, kw, 2, PULL, timing=True)) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        e = PyRumorModes(oracle, oracle.make_params(**kw), deg, masked(deg, ids), -1, 2, None, PULL)
        sim.broadcast_begin(-1)
        for t in range(1, 41):
            check_round(sim, e, sim.step(1)[0], e.step(), t)
        tm = sim.timing()
        assert tm["deliver_launches"] == 40 and tm["deliver_ms"] > 0


def test_bad_mode_bits(gs):
    @dataclasses.dataclass
    class Bad(gs.Config):
        def to_params(self):
            p = super().to_params()
            p.rumor_mode = 8 | PULL
            return p
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator(Bad(n=1000, model="rumor"))
    assert ei.value.code == -1 and "rumor_mode" in str(ei.value)
    with gs.Simulator(Bad(n=1000, model="pushpull")) as sim:   # the other models ignore the word
        assert sim.totals()["received"] == 0
