"""The three trial-resident kernels -- k_ppt_rounds (gs_pushpull_trials.hip),
k_rmt_rounds (gs_rumor_trials.hip) and k_mdt_rounds (gs_median_trials.hip): a
workgroup per trial, the trial's state in LDS -- over the instantiations, block
sizes, row shapes, counter lengths and LDS layouts that the kernels' own test
files leave out.  Nothing new is restated here: the truth is PyRumorModes per
trial (tests/test_rumor_modes.py), PyMedian per trial (tests/test_median.py)
and oracle.Engine with model = 1 per trial, through the helpers of
tests/test_rumor_trials_gpu.py, tests/test_median_trials_gpu.py and
tests/test_trial_masks.py.  Unless a part says otherwise a GPU case compares
the summed stats row and every trial's informed and removed sets (median: the
state bytes too) after every gs_step(1).

  A  all 16 instantiations of k_rmt_rounds<MODE, kMasked> on a block of 256
     threads (n = 2049: 33 words over 4 waves, a last word of one node), each
     mode masked, with all-zero masks (the masked kernel against the unmasked
     restatement) and masked again in one context; the same modes and trial 0's
     mask on the one-trial engine (gs_rumor.hip: a coin with a failure mask)
  B  the block rule's edges, n = 16 * block and 16 * block + 1 for blocks of
     64..512, in all three engines: both layouts of k_ppt_rounds (masked: a
     third bitset), both instantiations of k_mdt_rounds, a push and a pull
     instantiation of k_rmt_rounds; one gs_step(25), every row, the sets at
     the end
  C  rows of 1, 8, 32 and 255 slots in the rumor batch (the device pads a
     one-slot row to two)
  D  miss bytes counted to the end: k = 255 until nobody is hot, so a byte
     passes 127 and a node is removed at exactly 255; k = 1; and the median
     counter with k = 127 until nodes are done (state 254 -> 255)
  E  the LDS layouts of rmt_plan that test_limit leaves out, at the limit the
     device answers: 3 sets without miss bytes, 5 sets without, 3 sets with,
     and mode 0 masked; the sender is the last node, so the last word of every
     set is used from round 1
  F  a push trial skipped from its first launch: a sender with an empty row

The unmarked tests prove from the restatements alone that every case reaches
the path it is named for (spied: the restatement's own draws and events,
recorded, not restated).  They also show what a kernel that dropped the
`& tmask` of a callee id would do: every callee of a trial i > 0 would lie
outside the trial, so the trial would never inform a second node; every batch
here has a trial i > 0 that informs more.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import test_median_trials_gpu as mdt
import test_trial_masks as tm
from test_gpu_parity import masked, random_table
from test_median import MEDIAN
from test_median_gpu import parity as median_parity
from test_rumor import RUMOR, words_of
from test_rumor_gpu import check_round
from test_rumor_modes import BLIND, COIN, PULL, PyRumorModes
from test_rumor_modes_gpu import cfg_of, mode_id, parity, ring_table
from test_rumor_trials_gpu import begin, check_sets, restatements, stacked, step_all, summed, tables

RUNNING = -1


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def spied(e):
    """Records what the restatement e does from here on: per round its calls
    (callers, callees, kept), and its events (how many, how many removed)."""
    e.log = dict(calls=[], events=0, gone=0, hot_miss=0)
    calls, events = e.calls, e.events

    def calls_(v):
        u, kept = calls(v)
        e.log["calls"].append((v, u, kept))
        return u, kept

    def events_(v):
        before = int(e.hot[v].sum())
        events(v)
        e.log["events"] += int(v.size)
        e.log["gone"] += before - int(e.hot[v].sum())
        e.log["hot_miss"] = max(e.log["hot_miss"], int(e.miss[e.hot].max(initial=0)))

    e.calls, e.events = calls_, events_
    return e


def block_of(n):
    """The plans' block rule: the smallest power of two in 64..1024 with block * 16 >= n."""
    b = 64
    while b < 1024 and b * 16 < n:
        b *= 2
    return b


def one_call(sim, want):
    """One gs_step call for all of `want`, compared row by row."""
    got = sim.step(len(want)).astype(np.int64).tolist()
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"round {bad[0] + 1}:\n{got[bad[0]]}\n{want[bad[0]]}"


def sender_of(oracle, kw, i):
    return int(oracle.pick_sender(oracle.make_params(**dict(kw, trial=kw["trial"] + i))))


def keyed_masks(oracle, kw, T, frac, seed):
    """A mask of `frac` per trial that leaves the trial's keyed sender alive."""
    dead = [np.random.default_rng(seed + i).random(kw["n"]) < frac for i in range(T)]
    for i, d in enumerate(dead):
        d[sender_of(oracle, kw, i)] = False
    return dead


# ---- A. every instantiation of k_rmt_rounds, masked, on a 256-thread block ------------------------
A_N, A_T, A_K, A_BASE, A_SENDER, A_ROUNDS, A_SEED = 2049, 3, 3, 2, 1000, 30, 7


@functools.lru_cache(maxsize=None)
def case_a():
    """Tables with degrees 0..6 and the masks: 5 %; 30 % with the sender; 5 % with the one node of the last word."""
    tabs = tables(A_N, A_T, seed0=A_SEED, dlo=0)
    for deg, _ in tabs:
        deg[A_SENDER] = max(deg[A_SENDER], 1)
    dead = [np.random.default_rng(A_SEED + 50 + i).random(A_N) < f for i, f in enumerate((0.05, 0.30, 0.05))]
    dead[0][A_SENDER] = dead[2][A_SENDER] = False
    dead[1][A_SENDER] = True
    dead[0][A_N - 1], dead[2][A_N - 1] = False, True
    return tabs, dead


A_KW = dict(RUMOR, n=A_N, trial=A_BASE)


def test_a_cases_reach_the_masked_paths(oracle):
    assert block_of(A_N) == 256 and (A_N + 63) // 64 == 33 and A_N % 64 == 1
    tabs, dead = case_a()
    assert not np.array_equal(dead[0], dead[2]) and dead[2][A_N - 1] and dead[1][A_SENDER]
    for mode in range(8):
        es = [spied(e) for e in restatements(oracle, A_KW, tabs, A_SENDER, A_K, mode, dead)]
        rows = np.array([[e.step() for e in es] for _ in range(A_ROUNDS)], dtype=np.int64)  # [round, trial, field]
        lost = (rows[:, :, 2] - rows[:, :, 3]).sum(0)
        assert lost[0] > 0 and lost[2] > 0, (mode, lost)   # kept calls to a failed callee: the mask is read
        assert es[1].received == 0 and es[1].pending == 0 and (mode & PULL or not rows[:, 1, 1:].any())
        assert es[2].received > 1, mode                     # a trial i > 0 informs a second node
        assert es[0].received > 1, mode                     # (trial 0 is also the one-trial engine's case)
        if not mode & BLIND:
            assert min(es[0].received, es[2].received) > A_N // 4, (mode, [e.received for e in es])
        if mode & COIN:
            gone = sum(e.log["gone"] for e in es)
            kept = sum(e.log["events"] for e in es) - gone
            assert gone >= 20 and kept >= 20, (mode, gone, kept)
            assert not any(e.miss.any() for e in es)
        assert not any((e.inf & d).any() for e, d in zip(es, dead))
        plain = restatements(oracle, A_KW, tabs, A_SENDER, A_K, mode)
        other = np.array([[e.step() for e in plain] for _ in range(A_ROUNDS)], dtype=np.int64)
        assert all(not np.array_equal(rows[:, i], other[:, i]) for i in range(A_T)), mode   # every mask matters


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(8), ids=mode_id)
def test_a_masked_instantiations_on_a_256_thread_block(gs, oracle, mode):
    tabs, dead = case_a()
    masks = np.stack([words_of(d) for d in dead])
    with gs.Simulator.batch(cfg_of(gs, A_KW, A_K, mode, trials=A_T)) as sim:
        sim.load_peers(*stacked(tabs))
        for what, m, failed in (("masked", masks, dead), ("all-zero masks", np.zeros_like(masks), None),
                                ("masked again", masks, dead)):
            sim.set_failed(m)
            es = restatements(oracle, A_KW, tabs, A_SENDER, A_K, mode, failed)
            begin(sim, es, A_SENDER)
            step_all(sim, es, A_ROUNDS, what)
            assert np.array_equal(sim.crashed(), m), what
            if failed is not None:
                assert es[1].received == 0 and not sim.received()[1].any() and not sim.removed()[1].any()
            sim.reset()
            assert not sim.received().any() and not sim.removed().any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(8), ids=mode_id)
def test_a_one_trial_engine_with_the_same_mask(gs, oracle, mode):
    """Trial 0 of the batch on a one-trial context: in particular every coin mode with a failure mask."""
    (deg, ids), dead = case_a()[0][0], case_a()[1][0]
    e, row = parity(gs, oracle, A_KW, deg, ids, A_SENDER, mode, k=A_K, rounds=A_ROUNDS, failed=dead)
    assert not (e.inf & dead).any() and row[4] > 1


# ---- B. the block rule's edges, all three engines ---------------------------------------------------
B_SIZES = [1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193]
B_T, B_ROUNDS, B_K = 2, 25, 3
B_KINDS = ["rumor-mode0", "rumor-pull+coin", "median", "median-masked", "pushpull", "pushpull-masked"]
B_CASES = [(kind, n) for kind in B_KINDS for n in B_SIZES]


@functools.lru_cache(maxsize=None)
def b_inputs(kind, n):
    """(tables, per-trial failed bits or None) of a case."""
    oracle = tm.O()
    if kind.startswith("rumor"):
        pull = kind.endswith("coin")
        return tables(n, B_T, seed0=n + pull, dlo=1, table=ring_table if pull else None), None
    if kind.startswith("median"):
        tabs = mdt.tables(n, B_T, seed0=n + 1)
        return tabs, keyed_masks(oracle, dict(MEDIAN, n=n, trial=1), B_T, 0.05, n) if kind.endswith("masked") else None
    tabs = [tm.table(n, 6, 1, 6, seed=3 * n + t) for t in range(B_T)]
    if not kind.endswith("masked"):
        return tabs, None
    return tabs, [tm.random_mask(n, 0.05, n + t, keep=[oracle.pick_sender(tm.params(n, t, 1))]) for t in range(B_T)]


class BTruth:
    """The restatements of a case, just begun: .es, and .run() -> (the 25 summed rows, informed per trial)."""

    def __init__(self, oracle, kind, n):
        self.kind, self.n = kind, n
        tabs, failed = b_inputs(kind, n)
        if kind.startswith("rumor"):
            self.mode = PULL | COIN if kind.endswith("coin") else 0
            self.kw = dict(RUMOR, n=n, trial=1)
            self.es = restatements(oracle, self.kw, tabs, -1, B_K, self.mode)
        elif kind.startswith("median"):
            self.kw = dict(MEDIAN, n=n, trial=1)
            self.es = mdt.restatements(oracle, self.kw, tabs, -1, B_K, failed)
        else:
            self.es = [tm.engine(tm.params(n, t, 1), tabs[t], failed[t] if failed else None) for t in range(B_T)]

    def run(self):
        if self.kind.startswith("pushpull"):
            rows = [e.step(B_ROUNDS) for e in self.es]
            return tm.batch_rows(rows).tolist(), [int(r[-1, 4]) for r in rows]
        rows = [summed([e.step() for e in self.es]) for _ in range(B_ROUNDS)]
        return rows, [e.received for e in self.es]


def test_b_sizes_sit_on_the_block_rule_and_every_case_spreads(oracle):
    assert [block_of(n) for n in B_SIZES] == [64, 128, 128, 256, 256, 512, 512, 1024]
    assert all(block_of(n - 1) == block_of(n) < block_of(n + 1) for n in B_SIZES[::2])   # n = 16 * block
    for kind, n in B_CASES:
        tr = BTruth(oracle, kind, n)
        rows, informed = tr.run()
        assert len(rows) == B_ROUNDS and all(x > n // 2 for x in informed), (kind, n, informed)
        if kind.endswith("masked"):   # the same tables without the masks give other rows
            assert all(np.asarray(f).any() for f in b_inputs(kind, n)[1])
            assert rows != BTruth(oracle, kind[:-len("-masked")], n).run()[0], (kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", B_CASES)
def test_b_block_rule_edges(gs, oracle, kind, n):
    tr = BTruth(oracle, kind, n)
    tabs, failed = b_inputs(kind, n)
    if kind.startswith("rumor"):
        with gs.Simulator.batch(cfg_of(gs, tr.kw, B_K, tr.mode, trials=B_T)) as sim:
            sim.load_peers(*stacked(tabs))
            begin(sim, tr.es, -1)
            want, _ = tr.run()
            one_call(sim, want)
            check_sets(sim, tr.es, f"round {B_ROUNDS}")
    elif kind.startswith("median"):
        with gs.Simulator.median_batch(mdt.cfg_of(gs, tr.kw, B_K, trials=B_T)) as sim:
            sim.load_peers(*stacked(tabs))
            if failed is not None:
                sim.set_failed(np.stack([words_of(f) for f in failed]))
            mdt.begin(sim, tr.es, -1)
            want, _ = tr.run()
            one_call(sim, want)
            mdt.check_state(sim, tr.es, f"round {B_ROUNDS}")
    else:
        with gs.Simulator(tm.config(gs, n, B_T)) as sim:
            sim.load_peers(*stacked(tabs))
            if failed is not None:
                sim.set_failed(np.array(failed))
            sim.broadcast_begin(-1)
            assert sim.totals()["received"] == B_T
            want, _ = tr.run()
            one_call(sim, want)
            rec = sim.received()
            for t, e in enumerate(tr.es):
                assert np.array_equal(rec[t], e.received()), f"trial {t}: informed set differs"
            cr = sim.crashed()
            assert np.array_equal(cr, np.array(failed)) if failed is not None else not cr.any()


# ---- C. row shapes in the rumor batch -----------------------------------------------------------------
C_N, C_T, C_K, C_SENDER = 3001, 2, 6, 17
C_STRIDES = [1, 8, 32, 255]
C_MODES = [0, PULL | COIN]
C_SEED = {1: 3, 8: 8, 32: 32, 255: 255}


def c_rounds(stride):
    return 40 if stride > 1 else 60


def c_kw(stride):
    return dict(RUMOR, n=C_N, fanout=stride, fanin=stride, trial=0)


@functools.lru_cache(maxsize=None)
def c_tables(stride):
    tabs = [random_table(C_N, stride, 0, stride, seed=C_SEED[stride] + i) for i in range(C_T)]
    for deg, _ in tabs:
        deg[C_SENDER] = stride   # the sender's row is full
    return tabs


def test_c_rows_reach_the_high_slots_and_the_empty_rows(oracle):
    for stride in C_STRIDES:
        tabs = c_tables(stride)
        assert all(deg.min() == 0 and deg.max() == stride == ids.shape[1] for deg, ids in tabs)
        for mode in C_MODES:
            es = [spied(e) for e in restatements(oracle, c_kw(stride), tabs, C_SENDER, C_K, mode)]
            for _ in range(c_rounds(stride)):
                for e in es:
                    e.step()
            empty = [bool((e.inf & (e.deg == 0)).any()) for e in es]
            if mode & PULL:    # a node with an empty row never calls, so it never learns the rumor
                assert not any(empty) and (stride == 1 or es[1].received > C_N // 2)
            else:              # informed with an empty row: removed at once
                assert all(empty), (stride, empty)
                assert es[1].received > 1
            if stride == 255:  # a kept call whose callee is in none of the row's first 128 slots
                for e in es:
                    assert any((e.ids[v[k], :128] != u[k][:, None]).all(1).any() for v, u, k in e.log["calls"]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("stride", C_STRIDES)
@pytest.mark.parametrize("mode", C_MODES, ids=mode_id)
def test_c_row_shapes(gs, oracle, mode, stride):
    tabs = c_tables(stride)
    es = restatements(oracle, c_kw(stride), tabs, C_SENDER, C_K, mode)
    with gs.Simulator.batch(cfg_of(gs, c_kw(stride), C_K, mode, trials=C_T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, C_SENDER)
        step_all(sim, es, c_rounds(stride))
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (c_rounds(stride), sum(e.received for e in es),
                                                                  sum(e.pending for e in es))


# ---- D. miss counts to the end ----------------------------------------------------------------------------
D_N, D_K, D_T, D_BASE, D_SENDER = 65, 255, 2, 4, 5
D_MODES = [0, BLIND, PULL]
D_SEED = {0: 1, BLIND: 1, PULL: 9}
D_CAP = {0: 350, BLIND: 320, PULL: 1500}   # rounds; the restatements fall quiet below (test_d_...)
D_KW = dict(RUMOR, n=D_N, trial=D_BASE)


def d_table(n, seed):
    """Degrees 1..6, a ring in the first slot: every node has a caller, so a feedback pull falls quiet."""
    deg, ids = random_table(n, 6, 1, 6, seed=seed)
    ids[:, 0] = (np.arange(n) + 1) % n
    return deg, ids


@functools.lru_cache(maxsize=None)
def d_tables(mode):
    return tables(D_N, D_T, seed0=D_SEED[mode], table=d_table)


def test_d_miss_bytes_pass_127_and_end_at_255(oracle):
    for mode in D_MODES:
        es = [spied(e) for e in restatements(oracle, D_KW, d_tables(mode), D_SENDER, D_K, mode)]
        for e in es:
            while e.pending:
                e.step()
                assert e.t < D_CAP[mode], (mode, e.t, e.pending)
            assert e.log["hot_miss"] >= 128                         # a hot node whose byte has its top bit set
            assert e.log["hot_miss"] == D_K - 1 and e.miss.max() == D_K
            assert (e.removed & (e.miss == 255)).any() and e.received == D_N
            assert e.t > 255


def d_quiet(sim_step, es, cap):
    """Steps until every restatement is quiet; sim_step() steps the GPU once and compares."""
    while any(e.pending for e in es):
        assert es[0].t < cap
        sim_step()
    assert max(int(e.miss.max()) for e in es) == D_K


@pytest.mark.gpu
@pytest.mark.parametrize("mode", D_MODES, ids=mode_id)
def test_d_k255_to_quiescence_one_trial(gs, oracle, mode):
    deg, ids = d_tables(mode)[0]
    e = PyRumorModes(oracle, oracle.make_params(**D_KW), deg, masked(deg, ids), D_SENDER, D_K, None, mode)
    with gs.Simulator(cfg_of(gs, D_KW, D_K, mode)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(D_SENDER)
        d_quiet(lambda: check_round(sim, e, sim.step(1)[0], e.step(), e.t), [e], D_CAP[mode])
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (e.t, D_N, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", D_MODES, ids=mode_id)
def test_d_k255_to_quiescence_batch(gs, oracle, mode):
    tabs = d_tables(mode)
    es = restatements(oracle, D_KW, tabs, D_SENDER, D_K, mode)
    with gs.Simulator.batch(cfg_of(gs, D_KW, D_K, mode, trials=D_T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, D_SENDER)
        d_quiet(lambda: step_all(sim, es, 1), es, D_CAP[mode])
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (es[0].t, D_T * D_N, 0)
        assert np.array_equal(sim.removed(), sim.received())


D1_N, D1_T, D1_ROUNDS = 777, 3, 40
D1_MODES = [0, COIN, PULL]
D1_KW = dict(RUMOR, n=D1_N, trial=1)


@functools.lru_cache(maxsize=None)
def d1_tables(mode):
    return tables(D1_N, D1_T, seed0=7 + mode, dlo=1, table=ring_table if mode & PULL else None)


def test_d_k1_every_coin_removes(oracle):
    for mode in D1_MODES:
        es = [spied(e) for e in restatements(oracle, D1_KW, d1_tables(mode), 5, 1, mode)]
        for _ in range(D1_ROUNDS):
            for e in es:
                e.step()
        assert all(e.log["events"] > 0 and e.log["events"] == e.log["gone"] for e in es), mode
        assert all(e.received > 1 for e in es), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", D1_MODES, ids=mode_id)
def test_d_k1_batch(gs, oracle, mode):
    tabs = d1_tables(mode)
    es = restatements(oracle, D1_KW, tabs, 5, 1, mode)
    with gs.Simulator.batch(cfg_of(gs, D1_KW, 1, mode, trials=D1_T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, 5)
        step_all(sim, es, D1_ROUNDS)


# tests/test_median_gpu.py::test_counter_lengths and its batched twin stop k = 127 at 40 and 36 rounds, with
# every counter still running (they assert that nobody is done).  Here the same shape runs until every trial
# has done nodes: the state byte goes 127 (B-k), 128 (C-1) .. 254 (C-k), 255 (D).
DM_N, DM_K, DM_T, DM_ROUNDS = 65, 127, 2, 300
DM_KW = dict(MEDIAN, n=DM_N, trial=3)


@functools.lru_cache(maxsize=None)
def dm_tables():
    return mdt.tables(DM_N, DM_T, seed0=DM_K + DM_N)


def test_d_median_counter_reaches_done_from_254(oracle):
    for e in mdt.restatements(oracle, DM_KW, dm_tables(), 5, DM_K):
        seen = False
        for _ in range(DM_ROUNDS):
            before = e.state.copy()
            e.step()
            seen |= bool(((before == 2 * DM_K) & (e.state == 255)).any())
            assert not ((before != 2 * DM_K) & (before != 255) & (e.state == 255)).any()
        assert seen and e.removed.sum() > DM_N // 2


@pytest.mark.gpu
def test_d_median_k127_until_done_one_trial(gs, oracle):
    deg, ids = dm_tables()[0]
    e, row = median_parity(gs, oracle, DM_KW, deg, ids, 5, k=DM_K, rounds=DM_ROUNDS)
    assert e.removed.sum() > DM_N // 2


@pytest.mark.gpu
def test_d_median_k127_until_done_batch(gs, oracle):
    es = mdt.parity(gs, oracle, DM_KW, dm_tables(), 5, k=DM_K, rounds=DM_ROUNDS)
    assert all(e.removed.sum() > DM_N // 2 for e in es)


# ---- E. the LDS layouts at their limits ---------------------------------------------------------------------
E_T, E_K, E_ROUNDS = 2, 3, 12
E_CASES = [(COIN, False), (PULL | COIN, False), (PULL | BLIND, False), (0, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,with_mask", E_CASES, ids=["coin", "pull+coin", "pull+blind", "mode0-masked"])
def test_e_layouts_at_their_limits(gs, oracle, mode, with_mask):
    m = gs.rumor_trials_max_n(mode)   # from the query, never a constant
    assert m >= 64 and m % 64 == 0
    assert gs.rumor_trials_max_n(PULL) < gs.rumor_trials_max_n(PULL | BLIND) == gs.rumor_trials_max_n(0)
    assert gs.rumor_trials_max_n(0) < gs.rumor_trials_max_n(PULL | COIN) < gs.rumor_trials_max_n(COIN)
    kw = dict(RUMOR, n=m, trial=0)
    sender = m - 1                    # the last node: the last word of every set is live from round 1
    tabs = tables(m, E_T, seed0=44 + mode, table=ring_table)
    dead = None
    if with_mask:
        dead = [np.random.default_rng(60 + i).random(m) < 0.05 for i in range(E_T)]
        for d in dead:
            d[sender] = False
    es = restatements(oracle, kw, tabs, sender, E_K, mode, dead)
    with gs.Simulator.batch(cfg_of(gs, kw, E_K, mode, trials=E_T)) as sim:
        sim.load_peers(*stacked(tabs))
        if dead is not None:
            sim.set_failed(np.stack([words_of(d) for d in dead]))
        begin(sim, es, sender)
        want = [summed([e.step() for e in es]) for _ in range(E_ROUNDS)]
        one_call(sim, want)
        check_sets(sim, es, f"round {E_ROUNDS}")
    assert all(e.received > 100 for e in es), [e.received for e in es]
    if with_mask:
        assert sum(r[2] - r[3] for r in want) > 0
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator.batch(cfg_of(gs, dict(kw, n=m + 64), E_K, mode, trials=E_T))
    assert ei.value.code == -1 and str(m) in str(ei.value) and "gs_rumor_trials_max_n" in str(ei.value)


# ---- F. the push skip -----------------------------------------------------------------------------------------
F_N, F_T, F_K, F_BASE, F_SENDER = 777, 3, 2, 1, 9
F_KW = dict(RUMOR, n=F_N, trial=F_BASE)


@functools.lru_cache(maxsize=None)
def f_tables():
    tabs = tables(F_N, F_T, seed0=90, dlo=0)
    for i, (deg, _) in enumerate(tabs):
        deg[F_SENDER] = 0 if i == 1 else max(deg[F_SENDER], 1)   # trial 1's sender has nobody to call
    return tabs


def test_f_trial_1_is_quiet_before_round_1(oracle):
    es = restatements(oracle, F_KW, f_tables(), F_SENDER, F_K, 0)
    assert (es[1].received, es[1].pending) == (1, 0) and es[1].removed[F_SENDER]
    assert all((e.received, e.pending) == (1, 1) for e in (es[0], es[2]))
    for t in range(1, 21):
        rows = [e.step() for e in es]
        assert rows[1] == [t, 0, 0, 0, 1, 0, 0]
    assert es[0].received > 100 and es[2].received > 100


@pytest.mark.gpu
def test_f_push_skip_of_a_sender_with_an_empty_row(gs, oracle):
    tabs = f_tables()
    es = restatements(oracle, F_KW, tabs, F_SENDER, F_K, 0)
    alone = words_of(np.arange(F_N) == F_SENDER)
    cum = np.zeros((F_T, 3), dtype=np.int64)
    with gs.Simulator.batch(cfg_of(gs, F_KW, F_K, 0, trials=F_T)) as sim:
        sim.load_peers(*stacked(tabs))
        begin(sim, es, F_SENDER)
        assert sim.totals()["pending"] == 2
        for call in (17, 1, 1, 1):   # a launch boundary falls inside the first call
            want = []
            for _ in range(call):
                rows = [e.step() for e in es]
                assert rows[1][1:] == [0, 0, 0, 1, 0, 0]
                cum += np.array(rows, dtype=np.int64)[:, 1:4]
                want.append(summed(rows))
            got = sim.step(call).astype(np.int64).tolist()
            assert got == want, f"step({call}) ending at round {es[0].t}:\n{got}\n{want}"
            check_sets(sim, es, f"after round {es[0].t}")
            rec, rem = sim.received(), sim.removed()
            assert np.array_equal(rec[1], alone) and np.array_equal(rem[1], alone)
            res = sim.trial_results()
            assert res[1].tolist() == [F_BASE + 1, 0, es[0].t, 0, 0, 0, 1, 0, RUNNING]
            for i in (0, 2):
                assert res[i, 2:7].tolist() == [es[0].t, *cum[i].tolist(), es[i].received], i
        tot = sim.totals()
        fired, sent, messages = (int(x) for x in cum.sum(0))
        assert tot == dict(tick=20, fired=fired, sent=sent, messages=messages, received=sum(e.received for e in es),
                           crashed=0, pending=sum(e.pending for e in es))
    assert es[0].received > 100 and es[2].received > 100
