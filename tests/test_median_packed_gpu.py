"""Packed median batches on the GPU (GS_FLAG_MEDIAN_PACKED, Config.median_packed;
k_mdt16_rounds in gs_median_trials.hip): the batched
median rounds with a 16-bit tally per node, two nodes to a 32-bit LDS word.
Every case is bit-exact per round and per trial against one PyMedian
restatement per trial, through the helpers of tests/test_median_trials_gpu.py
(`parity` there with median_packed=True: `packed_parity` below), unless it says
otherwise: word edges (an odd n leaves a low half with no mate), both halves of
one word hit by every wave with opposite signs, the packed plan's 64 KiB
opt-in boundary, the limit from the query, the default n = 50,000 against the
GPU's one-trial engine, a field driven to 1 and to 0xFFFF, the in-degree guard
and the lifecycle calls.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import random_table
from test_median import MEDIAN, words_of
from test_median_trials_gpu import (Truth, begin, cfg_of, check_state, hub_table, restatements, stacked, step_all,
                                    tables)

pytestmark = pytest.mark.gpu

LIMIT_64K = (65536 - 320) // 208 * 64   # gs_mdt16_plan.h restated: 208 B per 64 nodes and 320 B of scratch
UNPACKED_MAX = 31104                    # gs_median_trials_max_n on an MI355X
BOUND = 32766                           # kMdt16MaxNamed


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def packed_batch(gs, kw, k, T):
    return gs.Simulator.median_batch(cfg_of(gs, kw, k, trials=T, median_packed=True))


def packed_parity(gs, oracle, kw, tabs, sender, k=2, rounds=30, failed=None, load=None):
    """test_median_trials_gpu.parity on a packed batch."""
    T = len(tabs)
    es = restatements(oracle, kw, tabs, sender, k, failed)
    tr = Truth(oracle, es, kw["trial"])
    with packed_batch(gs, kw, k, T) as sim:
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


# ---- 1. word edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 4133])
def test_word_edges(gs, oracle, n):
    """64-node words and 2-node tally words: at an odd n the last node is a low half with no mate.  Rows
    with duplicates, self entries and (n > 2) empty rows."""
    T, kw = 3, dict(MEDIAN, n=n, trial=2)
    tabs = [random_table(n, 6, 0 if n > 2 else 1, 6, seed=10 * n + i) for i in range(T)]
    for deg, _ in tabs:
        deg[n // 2] = max(deg[n // 2], 1)
    es = packed_parity(gs, oracle, kw, tabs, n // 2, rounds=30)
    if n == 4133:
        assert any(e.received > n // 2 and e.removed.sum() > n // 2 for e in es)


# ---- 2. contended halves ---------------------------------------------------------------------
def pair_table(n, seed):
    """Every row names node 0 and node 1: the two halves of tally word 0 take adds from every wave."""
    rng = np.random.default_rng(seed)
    deg = np.full(n, 4, np.uint8)
    ids = rng.integers(0, n, size=(n, 4)).astype(np.uint32)
    ids[:, 0] = 0
    ids[:, 1] = 1
    return deg, ids


@pytest.mark.parametrize("n", [777, 4133])
def test_both_halves_of_one_word_from_every_wave(gs, oracle, n):
    T, k = 3, 3
    kw = dict(MEDIAN, n=n, fanout=4, fanin=4, drop_rate=0.1, trial=0)
    tabs = tables(n, T, seed0=n, table=pair_table)
    es = restatements(oracle, kw, tabs, 7, k)
    tr = Truth(oracle, es, 0)
    most, opposite = 0, False
    with packed_batch(gs, kw, k, T) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, 7)
        for _ in range(30):
            before = [e.state.copy() for e in es]
            step_all(sim, tr, 1)
            for e, S in zip(es, before):
                if 1 <= S[0] <= k and 1 <= S[1] <= k:   # both halves are counting this round
                    c0, c1 = e.last[0][e.last[1] == 0], e.last[0][e.last[1] == 1]
                    most = max(most, min(c0.size, c1.size))
                    opposite |= bool((S[c0] >= S[0]).any() and (S[c1] < S[1]).any())
    assert most > n // 8 and opposite and all(e.removed[0] and e.removed[1] for e in es)


@pytest.mark.parametrize("n", [777, 4133])
def test_hub_with_a_failure_mask(gs, oracle, n):
    """The masked instantiation: every row names node 0, 5 % of each trial failed."""
    T = 3
    kw = dict(MEDIAN, n=n, fanout=4, fanin=4, drop_rate=0.1, trial=1)
    tabs = tables(n, T, seed0=5 + n, table=hub_table)
    dead = [np.random.default_rng(40 + i).random(n) < 0.05 for i in range(T)]
    for d in dead:
        d[0] = d[7] = False
    es = packed_parity(gs, oracle, kw, tabs, 7, k=3, rounds=30, failed=dead)
    assert not any((e.inf & d).any() for e, d in zip(es, dead)) and all(e.received > n // 2 for e in es)


# ---- 3. the plan's boundaries ------------------------------------------------------------------
@pytest.mark.parametrize("n", [LIMIT_64K, LIMIT_64K + 64])
def test_the_64_kib_opt_in_boundary(gs, oracle, n):
    W = (n + 63) // 64
    assert (W * 208 + 320 <= 65536) == (n == LIMIT_64K) and LIMIT_64K == 20032
    es = packed_parity(gs, oracle, dict(MEDIAN, n=n, trial=1), tables(n, 2, seed0=n), -1, k=3, rounds=22)
    assert all(e.received > n // 2 for e in es)


def test_limit(gs, oracle):
    m = gs.median_trials_max_n(packed=True)   # from the query, never a constant
    assert m >= 50_000 and m % 64 == 0
    kw = dict(MEDIAN, n=m, trial=0)
    es = packed_parity(gs, oracle, kw, tables(m, 2, seed0=41), -1, k=3, rounds=20)
    assert all(e.received > 1000 for e in es)
    with pytest.raises(gs.GossipError) as ei:
        packed_batch(gs, dict(kw, n=m + 64), 3, 2)
    assert ei.value.code == -1 and str(m) in str(ei.value) and "gs_median_trials_max_n_packed" in str(ei.value)
    # without the flag: today's limit and today's message
    u = gs.median_trials_max_n()
    assert u == UNPACKED_MAX < m
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator.median_batch(cfg_of(gs, dict(kw, n=u + 64), 3, trials=2))
    why = str(ei.value)
    assert ei.value.code == -1 and f"n must be <= {u} on this device (gs_median_trials_max_n), not {u + 64}" in why
    assert "packed" not in why.lower()


# ---- 4. the default n against the GPU's one-trial engine ---------------------------------------
def test_default_n_equals_one_trial_contexts(gs):
    """n = 50,000, the batch's own overlays, gs_run(1, 150): trial i is the one-trial gs_create context of
    trial + i with trial i's table.  (The truth is the one-trial engine, itself pinned to the restatement
    in tests/test_median_gpu.py, which keeps this to seconds.)"""
    n, T, k = 50_000, 3, 5
    kw = dict(MEDIAN, n=n, drop_rate=0.1, trial=4)
    with packed_batch(gs, kw, k, T) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        sim.broadcast_begin(-1)
        _, status = sim.run(poll=1, max_ticks=150)
        got = (sim.trial_results(), sim.median_state(), sim.received(), sim.removed())
    ones = []
    for i in range(T):
        with gs.Simulator(cfg_of(gs, dict(kw, trial=4 + i), k)) as one:
            one.load_peers(deg[i * n:(i + 1) * n], ids[i * n:(i + 1) * n])
            one.broadcast_begin(-1)
            _, st = one.run(poll=1, max_ticks=150)
            ones.append((one.trial_results()[0], one.median_state(), one.received(), one.removed(), st))
    assert np.array_equal(got[0], np.array([o[0] for o in ones])), f"\n{got[0]}\n{[o[0] for o in ones]}"
    for i, o in enumerate(ones):
        assert np.array_equal(got[1][i], o[1]), f"trial {i}: state bytes"
        assert np.array_equal(got[2][i], o[2].reshape(-1)) and np.array_equal(got[3][i], o[3].reshape(-1)), i
    assert status == max(o[4] for o in ones)
    assert all(int(r[6]) > 0.99 * n for r in got[0])


# ---- 5. both extremes of a field, and the guard ------------------------------------------------
EXT_N = 32_768


def star_table(last):
    """Rows 1 .. n-2 are [0], node 0's row is [1], the last node's row is [`last`]."""
    deg = np.ones(EXT_N, np.uint8)
    ids = np.zeros((EXT_N, 1), np.uint32)
    ids[0, 0] = 1
    ids[EXT_N - 1, 0] = last
    return deg, ids


EXT_KW = dict(MEDIAN, n=EXT_N, fanout=1, fanin=1, drop_rate=0.0, trial=0)


def test_a_field_reaches_both_extremes(gs, oracle):
    """Node 0 has 32,767 partners a round (32,766 callers and its own call): all behind it in round 1
    (ge - lt = -32,767, field 1), all level with it in round 2 (+32,767, field 0xFFFF).  Node 1 is the
    other half of its word."""
    tabs = [star_table(1), star_table(1)]
    assert (tabs[0][1][:, 0] == 0).sum() == BOUND
    es = restatements(oracle, EXT_KW, tabs, 0, 2)
    tr = Truth(oracle, es, 0)
    with packed_batch(gs, EXT_KW, 2, 2) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, 0)
        step_all(sim, tr, 1)
        assert all(e.st[0] == 1 and (e.st[1:BOUND + 1] == 1).all() for e in es)   # 0 stayed B-1; its callers joined
        step_all(sim, tr, 1)
        assert all(e.st[0] == 2 for e in es)                                       # the majority was level: B-2
        step_all(sim, tr, 4)
        st = sim.median_state()
        assert all(np.array_equal(st[i][:2], e.st[:2]) for i, e in enumerate(es))


def test_the_guard_refuses_one_slot_too_many_and_the_context_lives_on(gs, oracle):
    """32,767 used slots name node 0: refused at begin, naming the node, the count and the bound.  A
    refusal, nothing faults; the table is kept, and the accepted table loaded on the same context runs."""
    bad, good = [star_table(1), star_table(0)], [star_table(1), star_table(1)]
    es = restatements(oracle, EXT_KW, good, 0, 2)
    with packed_batch(gs, EXT_KW, 2, 2) as sim:
        sim.load_peers(*stacked(bad))
        for _ in range(2):   # the answer stays until another table enters
            with pytest.raises(gs.GossipError) as ei:
                sim.broadcast_begin(0)
            why = str(ei.value)
            assert ei.value.code == -1 and "node 0 " in why and "32767" in why and "32766" in why, why
            assert "trial 1" in why
        deg, ids = sim.read_peers()   # the table is kept (rows of one slot come back in their padded stride)
        assert np.array_equal(ids[:, 0], stacked(bad)[1][:, 0]) and np.array_equal(deg, stacked(bad)[0])
        sim.load_peers(*stacked(good))
        begin(sim, es, 0)
        step_all(sim, Truth(oracle, es, 0), 3)
    # without the flag there is no such bound (and n = 32,768 needs the flag on this device anyway)
    small = dict(EXT_KW, n=BOUND)   # n <= 32,766: every table passes, no count is taken
    deg = np.ones(BOUND, np.uint8)
    ids = np.zeros((BOUND, 1), np.uint32)
    packed_parity(gs, oracle, small, [(deg, ids)] * 2, 0, rounds=3)


# ---- 6. lifecycle --------------------------------------------------------------------------------
def test_lifecycle(gs, oracle):
    n, T, R, k = 4133, 3, 44, 5   # k: the CLI's default at this n, with which a trial ends by itself
    kw, kw3 = dict(MEDIAN, n=n, trial=0), dict(MEDIAN, n=n, trial=T)
    tabs, tabs2 = tables(n, T, seed0=21), tables(n, T, seed0=61)
    es = restatements(oracle, kw, tabs, 9, k)
    tr = Truth(oracle, es, 0)
    with packed_batch(gs, kw, k, T) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, 9)
        singles, end = [], [0] * T
        for _ in range(R):   # gs_step(1) x R, every round checked, past a trial's own end
            want = tr.step()
            got = [int(x) for x in sim.step(1)[0]]
            assert got == want, f"round {es[0].t}"
            singles.append(got)
            for i, e in enumerate(es):
                if e.pending == 0 and not end[i]:
                    end[i] = e.t
        check_state(sim, es, "after the single steps")
        assert min(e.t for e in es) == R
        assert any(0 < t < R - 8 for t in end), end   # rounds stepped after a trial had ended by itself
        sets = (sim.median_state(), sim.received(), sim.removed(), sim.trial_results())
        sim.reset()
        assert not sim.received().any() and not sim.removed().any() and not sim.median_state().any()
        sim.broadcast_begin(9)
        assert sim.step(R).astype(np.int64).tolist() == singles   # gs_step(R): launches of 16, 16 and 12 rounds
        for a, b in zip(sets, (sim.median_state(), sim.received(), sim.removed(), sim.trial_results())):
            assert np.array_equal(a, b)
        sim.reset()          # set_trial plus a new table: parity with the new numbers
        sim.set_trial(T)
        sim.load_peers(*stacked(tabs2))
        es3 = restatements(oracle, kw3, tabs2, -1, k)
        begin(sim, es3, -1)
        step_all(sim, Truth(oracle, es3, T), 20, "after set_trial")


@pytest.mark.parametrize("n", [65, 4133])
def test_load_peers_device(gs, oracle, n):
    """Tables back to back in device memory."""
    T = 3
    kw = dict(MEDIAN, n=n, trial=2)
    tabs = tables(n, T, seed0=41 + n)
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
        es = packed_parity(gs, oracle, kw, tabs, n // 3, rounds=25,
                           load=lambda sim: sim.load_peers_device(bufs[0].value, bufs[1].value, ids.shape[1]))
        assert all(e.received > n // 2 for e in es)
    finally:
        for d in bufs:
            hip.hipFree(d)
