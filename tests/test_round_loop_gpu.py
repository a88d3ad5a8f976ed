"""The round loop that rumor mongering, median-counter push-pull and the rumor
set share (gs_round_host.cpp), at the places no other suite reaches: a batch
whose rows straddle the end of the stats ring (slot 4096: two spans to read
back, in the stats ring and in the rumor set's count ring), the split of a
gs_step call into batches of 256 rounds under GS_FLAG_TIMING, and gs_run's
stop word with a poll that divides nothing.  Bit-exact against the Python
restatements of the models' own suites.
"""
from __future__ import annotations

import numpy as np
import pytest

import test_median_gpu as median_gpu
import test_rumor_gpu as rumor_gpu
import test_rumor_modes_gpu as modes_gpu
import test_rumorset_gpu as set_gpu
from test_gpu_parity import masked
from test_median import MEDIAN, PyMedian
from test_median import reference_run as median_reference_run
from test_rumor import RUMOR, PyRumor, words_of
from test_rumor_modes import PULL, PyRumorModes
from test_rumorset import RS
from test_rumorset import reference_run as set_reference_run
from test_rumorset_cap import ROTATE, PyCappedSet

pytestmark = pytest.mark.gpu

RING_SLOTS = 4096    # kStatSlots: round t's row is in slot t % 4096
N = 4133
ENGINES = ["rumor_push", "rumor_pull", "median", "rumor_set"]
SENDER, K_RUMOR, K_MEDIAN = 3, 2, 3
SET_SENDERS = [7, 7, 4000, 4132, 63, 64]


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


@pytest.fixture(scope="module")
def table():
    return set_gpu.ring_table(N, seed=70)


def trial_row(gs, sim):
    return dict(zip(gs.engine.TRIAL_FIELDS, sim.trial_results()[0]))


# ---- ring wrap ---------------------------------------------------------------------------

@pytest.mark.parametrize("payload", [0, 2], ids=["uncapped", "payload2"])
def test_rumor_set_batch_straddles_the_ring_wrap(gs, oracle, payload):
    """Three rumors enter after rounds 4090, 4096 and 4100, so nothing moves
    before the wrap and the rows change on both sides of it (the restatement's
    rows of rounds 4090..4107 all differ from their predecessors; checked below).
    gs_step(4080) is one batch of one span; gs_step(40) is rounds 4081..4120:
    slots 4081..4095, then 0..24.  Uncapped it is k_rs_round that crosses the
    wrap, with a payload of 2 k_rsc_round (three staggered rumors never want
    more than two at once: the cap does not bind), and both times the inject
    launch of rounds 4090, 4096 and 4100."""
    n, senders, starts = 65, [3, 40, 64], [4090, 4096, 4100]
    deg, ids = set_gpu.ring_table(n, seed=65)
    kw = dict(RS, n=n, drop_rate=0.0)
    e = PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, starts, payload, ROTATE)
    with gs.Simulator.rumor_set(set_gpu.cfg_of(gs, kw), len(senders)) as sim:
        sim.load_peers(deg, ids)
        sim.set_payload(payload, ROTATE)
        sim.begin_rumors(senders, starts)
        for ticks in (4080, 40):
            want = []
            for _ in range(ticks):    # gs_step: every tick is a poll
                want.append(e.step())
                e.poll()
            got = sim.step(ticks).tolist()
            bad = [i for i in range(ticks) if got[i] != want[i]]
            assert not bad, f"round {want[bad[0]][0]}:\n{got[bad[0]]}\n{want[bad[0]]}"
            set_gpu.check_state(sim, e, e.t)
            assert trial_row(gs, sim)["tick_99"] == e.set_tick_99
            if payload:
                assert sim.rumor_traffic() == e.traffic
        assert e.t == 4120 > RING_SLOTS > 4080
        moved = [i for i in range(1, 40) if want[i][1:] != want[i - 1][1:]]
        assert len(moved) >= 5 and want[moved[0]][0] < RING_SLOTS < want[moved[-1]][0]
        assert all(4080 < t <= 4120 for t in e.tick_99) and e.set_tick_99 == max(e.tick_99)


# ---- the engines at n = 4133 ---------------------------------------------------------------

def restatement(oracle, engine, deg, ids):
    m = masked(deg, ids)
    if engine == "rumor_push":
        return PyRumor(oracle, oracle.make_params(**dict(RUMOR, n=N)), deg, m, SENDER, K_RUMOR)
    if engine == "rumor_pull":
        return PyRumorModes(oracle, oracle.make_params(**dict(RUMOR, n=N)), deg, m, SENDER, K_RUMOR, None, PULL)
    if engine == "median":
        return PyMedian(oracle, oracle.make_params(**dict(MEDIAN, n=N)), deg, m, SENDER, K_MEDIAN)
    return PyCappedSet(oracle, oracle.make_params(**dict(RS, n=N)), deg, m, SET_SENDERS)


def begun(gs, engine, deg, ids, **more):
    """A context of `engine` over the table, its broadcast begun."""
    if engine == "rumor_set":
        sim = gs.Simulator.rumor_set(set_gpu.cfg_of(gs, dict(RS, n=N), **more), len(SET_SENDERS))
    elif engine == "median":
        sim = gs.Simulator(median_gpu.cfg_of(gs, dict(MEDIAN, n=N), K_MEDIAN, **more))
    else:
        mode = PULL if engine == "rumor_pull" else 0
        sim = gs.Simulator(modes_gpu.cfg_of(gs, dict(RUMOR, n=N), K_RUMOR, mode, **more))
    try:
        sim.load_peers(deg, ids)
        if engine == "rumor_set":
            sim.begin_rumors(SET_SENDERS)
        else:
            sim.broadcast_begin(SENDER)
    except Exception:
        sim.close()
        raise
    return sim


def check_sets(sim, e, engine):
    if engine == "rumor_set":
        set_gpu.check_state(sim, e, e.t)
    elif engine == "median":
        median_gpu.check_state(sim, e, e.t)
    else:
        assert np.array_equal(sim.received(), words_of(e.inf)) and np.array_equal(sim.removed(), words_of(e.removed))


@pytest.mark.parametrize("engine", ENGINES)
def test_timing_splits_a_step_into_batches_of_256(gs, oracle, table, engine):
    """One gs_step(300) with GS_FLAG_TIMING: a batch of 256 rounds and one of
    44, three events a round.  Rumor and median end long before round 300 and
    the device keeps stepping; so do the restatements (their rows past the end
    are not all zero: the pull mode's uninformed nodes go on asking), so all
    300 rows are compared."""
    deg, ids = table
    e = restatement(oracle, engine, deg, ids)
    want = []
    for _ in range(300):
        want.append(e.step())
        if engine == "rumor_set":
            e.poll()
    assert any(r[6] for r in want[:10]) and (engine == "rumor_set" or want[-1][6] == 0)
    with begun(gs, engine, deg, ids, timing=True) as sim:
        got = sim.step(300).tolist()
        bad = [i for i in range(300) if got[i] != want[i]]
        assert not bad, f"round {bad[0] + 1}:\n{got[bad[0]]}\n{want[bad[0]]}"
        tm = sim.timing()
        assert tm["deliver_launches"] == 300 and tm["resolve_launches"] == 300
        assert tm["deliver_ms"] > 0 and tm["resolve_ms"] > 0
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (300, e.received, e.pending)
        check_sets(sim, e, engine)


@pytest.mark.parametrize("engine", ENGINES)
def test_run_with_a_poll_of_7(gs, oracle, table, engine):
    """gs_run(poll = 7) through the shared run loop: status, the number of poll
    rows, the totals and tick_99 are the restatement's under gs_run's rule."""
    deg, ids = table
    e, rows = restatement(oracle, engine, deg, ids), None
    if engine == "rumor_set":
        status, rows = set_reference_run(e, 7, 10_000)
        tick_99 = e.set_tick_99
    elif engine == "median":
        status, tick_99 = median_reference_run(oracle, e, 7, 10_000)
    elif engine == "rumor_pull":
        e, status, tick_99 = modes_gpu.reference_run(oracle, dict(RUMOR, n=N), deg, ids, SENDER, K_RUMOR, PULL, 7, 10_000)
    else:
        e, status, tick_99 = rumor_gpu.reference_run(oracle, dict(RUMOR, n=N), deg, ids, SENDER, K_RUMOR, 7, 10_000)
    assert status in (0, 1) and 0 < e.t < 10_000 and e.t % 7 == 0
    steps = restatement(oracle, engine, deg, ids).run(e.t)
    with begun(gs, engine, deg, ids) as sim:
        got, st = sim.run(poll=7, max_ticks=10_000)
        assert st == status and len(got) == e.t // 7
        if rows is not None:
            assert got.tolist() == rows
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (e.t, e.received, e.pending)
        assert [tot[f] for f in ("fired", "sent", "messages")] == [int(steps[:, c].sum()) for c in (1, 2, 3)]
        tr = trial_row(gs, sim)
        assert (tr["tick_99"], tr["status"], tr["tick"]) == (tick_99, status, e.t)
        assert tr["received"] == e.received and tr["messages"] == tot["messages"]
        check_sets(sim, e, engine)
