"""The HIP rumor-set engine (gs_rumorset.hip) against the Python restatement of
tests/test_rumorset.py: bit-exact per round -- the stats row, the rumor words,
the 64 per-rumor counts and the holds-every-rumor set after every gs_step(1) --
over the shapes at which the kernels can go wrong; then every column against
the existing one-rumor push-pull engine, gs_run's stop rule and the lifecycle
calls.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumorset import RS, PyRumorSet, bit_counts, reference_run, words_of

pytestmark = pytest.mark.gpu

RUN_NAMES = {0: "COVERED", 1: "QUIESCENT", 2: "MAX_TICKS"}


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def cfg_of(gs, kw, **more):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], model="pushpull", **more)


def check_state(sim, e, t):
    assert np.array_equal(sim.rumor_words(), e.have), f"rumor words differ at round {t}"
    assert np.array_equal(sim.received(), words_of(e.holds_all)), f"holds-every-rumor set differs at round {t}"
    res = sim.rumor_results()
    assert [r["received"] for r in res] == e.counts.tolist(), f"per-rumor counts differ at round {t}"
    assert [r["sender"] for r in res] == e.senders and [r["started"] for r in res] == e.started
    assert [r["tick_99"] for r in res] == e.tick_99, f"per-rumor tick_99 differs at round {t}"


def parity(gs, oracle, kw, deg, ids, senders, rounds, failed=None, sim=None):
    """gs_step(1) x rounds against the restatement (every tick is a poll);
    returns it and its last row."""
    e = PyRumorSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, failed)
    own = sim is None
    if own:
        sim = gs.Simulator.rumor_set(cfg_of(gs, kw), len(senders))
        sim.load_peers(deg, ids)
        if failed is not None:
            sim.set_failed(words_of(failed))
    try:
        sim.begin_rumors(senders)
        tot = sim.totals()
        assert (tot["received"], tot["pending"]) == (e.received, e.pending)
        check_state(sim, e, 0)
        row = None
        for t in range(1, rounds + 1):
            row = e.step()
            e.poll()
            got = [int(x) for x in sim.step(1)[0]]
            assert got == row, f"round {t}:\n{got}\n{row}"
            check_state(sim, e, t)
        tot = sim.totals()
        assert tot["tick"] == rounds and tot["received"] == e.received and tot["pending"] == e.pending
    finally:
        if own:
            sim.close()
    return e, row


def spread(n, R, seed=0):
    """R senders over the id range, node n - 1 among them."""
    s = [(j * n) // R for j in range(R)]
    s[-1] = n - 1
    return s


def ring_table(n, seed, stride=6, lo=5):
    deg, ids = random_table(n, stride, lo, stride, seed=seed)
    ids[:, 0] = (np.arange(n) + 1) % n
    return deg, ids


@pytest.mark.parametrize("R", [1, 2, 63, 64])
@pytest.mark.parametrize("n", [1, 64, 65, 100, 4133])
def test_sizes_and_rumor_counts(gs, oracle, n, R):
    """One node, an exact word, one bit into the second word, ragged tails; R =
    64 uses bit 63 and the all-ones live mask, R = 63 leaves a bit that stays 0.
    Rows with duplicates, self entries and (n > 2) empty rows."""
    deg, ids = random_table(n, 6, 0 if n > 2 else 1, 6, seed=n)
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, spread(n, R), rounds=14)
    assert int(e.have.max()) >> R == 0
    if n == 4133:
        assert row[4] > R * n // 2
        assert (R < 64) or (e.have == np.uint64(2**64 - 1)).any()


@pytest.mark.parametrize("drop", [0.0, 0.1, 1.0])
def test_drop_rates(gs, oracle, drop):
    n = 4133
    deg, ids = ring_table(n, seed=11)
    e, row = parity(gs, oracle, dict(RS, n=n, drop_rate=drop), deg, ids, spread(n, 5), rounds=16)
    if drop == 1.0:    # nothing ever moves
        assert row == [16, n, 0, 0, 5, 0, 5]
    else:
        assert row[4] > 4 * n and (row[2] == row[1]) == (drop == 0.0)


def test_every_call_lost_ends_at_max_ticks(gs, oracle):
    n = 777
    deg, ids = ring_table(n, seed=1)
    with gs.Simulator.rumor_set(cfg_of(gs, dict(RS, n=n, drop_rate=1.0)), 3) as sim:
        sim.load_peers(deg, ids)
        sim.begin_rumors([0, 5, 776])
        rows, st = sim.run(poll=10, max_ticks=30)
        assert RUN_NAMES[st] == "MAX_TICKS" and len(rows) == 3
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"], tot["sent"], tot["fired"]) == (30, 3, 3, 0, 30 * n)


@pytest.mark.parametrize("mask", ["none", "five_percent", "failed_sender", "all"])
def test_failure_masks(gs, oracle, mask):
    n = 4133
    deg, ids = ring_table(n, seed=9)
    dead = {"none": np.zeros(n, bool), "five_percent": np.random.default_rng(3).random(n) < 0.05,
            "failed_sender": np.random.default_rng(4).random(n) < 0.05, "all": np.ones(n, bool)}[mask]
    senders = [100, 100, 2000, n - 1, 64]     # duplicate senders, sender n - 1
    if mask != "all":
        dead[senders] = False
    if mask == "failed_sender":
        dead[2000] = True                      # a failed sender among live ones
    e, row = parity(gs, oracle, dict(RS, n=n, drop_rate=0.0), deg, ids, senders, rounds=14, failed=dead)
    assert not e.have[dead].any()
    if mask == "all":
        assert e.live == 0 and row == [14, 0, 0, 0, 0, 0, 0]
        with gs.Simulator.rumor_set(cfg_of(gs, dict(RS, n=n)), 5) as sim:   # quiescent at the first poll
            sim.load_peers(deg, ids)
            sim.set_failed(words_of(dead))
            sim.begin_rumors(senders)
            rows, st = sim.run(poll=10, max_ticks=1000)
            assert RUN_NAMES[st] == "QUIESCENT" and len(rows) == 1 and [int(x) for x in rows[0]] == [10] + [0] * 6
            assert not any(r["started"] for r in sim.rumor_results())
    else:
        assert e.started == [True, True, mask != "failed_sender", True, True]
        assert (not e.column(2).any()) == (mask == "failed_sender")
        assert np.array_equal(e.column(0), e.column(1)) and row[4] > 3 * n


@pytest.mark.parametrize("rows", ["empty", "self_only", "one_friend_repeated", "stride_2", "stride_32"])
def test_row_shapes(gs, oracle, rows):
    n = 3001
    rng = np.random.default_rng(5)
    stride = {"stride_2": 2, "stride_32": 32}.get(rows, 6)
    deg, ids = ring_table(n, seed=3, stride=stride, lo=1)
    if rows == "empty":
        deg[::3] = 0
    elif rows == "self_only":
        pick = np.arange(0, n, 4)
        ids[pick] = pick[:, None]
    elif rows == "one_friend_repeated":
        ids[:] = rng.integers(0, n, size=(n, 1))
        ids[::2, :] = ((np.arange(0, n, 2) + 1) % n)[:, None]
    kw = dict(RS, n=n, fanout=stride, fanin=stride)
    e, row = parity(gs, oracle, kw, deg, ids, spread(n, 7), rounds=14)
    assert row[4] > 7


def test_hub(gs, oracle):
    """n = 70,000, every node's only friend is node 0: 69,999 callers meet in
    node 0's words, and with 64 senders over the id range node 0's word and the
    per-rumor counts must be exact (every word gains up to 64 bits in one
    commit once node 0 holds them all)."""
    n, R = 70_000, 64
    deg = np.ones(n, np.uint8)
    ids = np.zeros((n, 2), np.uint32)
    kw = dict(RS, n=n, fanout=2, fanin=2)
    e, row = parity(gs, oracle, kw, deg, ids, spread(n, R), rounds=6)
    assert (e.last[1] == 0).sum() > 60_000
    assert int(e.have[0]) == 2**64 - 1 and e.counts.min() > 0.9 * n and row[6] < R


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_grid_of_few_blocks(gs, oracle, blocks, monkeypatch):
    """65 words through 4 and 12 waves (GS_RUMORSET_GRID, read per broadcast):
    17 and 6 passes of the round's and the commit's loops, the same bits."""
    monkeypatch.setenv("GS_RUMORSET_GRID", blocks)
    n = 4133
    deg, ids = ring_table(n, seed=20)
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, spread(n, 64), rounds=14)
    assert row[4] > 32 * n


def test_default_grid_takes_a_second_pass(gs, oracle):
    """n = 600,000: 9,375 words against the default grid's 8,192 waves."""
    n = 600_000
    deg, ids = ring_table(n, seed=6)
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, spread(n, 64), rounds=5)
    tail = bit_counts(e.have[8192 * 64:], 64)   # what the waves' second pass wrote
    assert tail.sum() > 640 and row[4] > 64 * 50


@pytest.mark.parametrize("mask", [False, True])
def test_columns_equal_the_pushpull_engine(gs, oracle, mask):
    """n = 4133, R = 64, 12 rounds: columns 0, 1, 31, 62 and 63 are the informed
    sets of the existing one-rumor push-pull engine from those senders, per
    round; rumor_column(j) is bit j of rumor_words()."""
    n, R, cols = 4133, 64, (0, 1, 31, 62, 63)
    deg, ids = random_table(n, 6, 0, 6, seed=8)
    senders = [int(x) for x in np.random.default_rng(12).integers(0, n, size=R)]
    failed = np.random.default_rng(13).random(n) < 0.05 if mask else None
    if mask:
        failed[senders] = False
        failed[senders[31]] = True    # a dead rumor: the one-rumor engine informs nobody either
    kw = dict(RS, n=n)
    sims = []
    try:
        for j in cols:
            s = gs.Simulator(cfg_of(gs, kw))
            sims.append(s)
            s.load_peers(deg, ids)
            if mask:
                s.set_failed(words_of(failed))
            s.broadcast_begin(senders[j])
        with gs.Simulator.rumor_set(cfg_of(gs, kw), R) as rs:
            rs.load_peers(deg, ids)
            if mask:
                rs.set_failed(words_of(failed))
            rs.begin_rumors(senders)
            for t in range(13):
                words = rs.rumor_words()
                for j, s in zip(cols, sims):
                    col = rs.rumor_column(j)
                    assert np.array_equal(col, s.received()), f"column {j} differs at round {t}"
                    assert np.array_equal(col, words_of((words >> np.uint64(j)) & np.uint64(1) != 0)), (j, t)
                rs.step(1)
                for s in sims:
                    s.step(1)
            assert rs.rumor_column(0).any() and rs.rumor_column(31).any() == (not mask)
            with pytest.raises(gs.GossipError):
                rs.rumor_column(R)
    finally:
        for s in sims:
            s.close()


@pytest.mark.parametrize("poll", [1, 10])
def test_run_agrees_with_the_restatement(gs, oracle, poll):
    """Stop tick, status, the polls' rows, per-rumor tick_99 and the set's row."""
    n, senders = 4133, [7, 7, 4000, 4132, 63, 64]
    deg, ids = ring_table(n, seed=70)
    kw = dict(RS, n=n)
    e = PyRumorSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders)
    status, want = reference_run(e, poll, 10_000)
    assert RUN_NAMES[status] == "COVERED" and all(e.tick_99) and e.set_tick_99 == e.t == max(e.tick_99)
    with gs.Simulator.rumor_set(cfg_of(gs, kw), len(senders)) as sim:
        sim.load_peers(deg, ids)
        sim.begin_rumors(senders)
        rows, st = sim.run(poll=poll, max_ticks=10_000)
        assert st == status and [[int(x) for x in r] for r in rows] == want
        check_state(sim, e, e.t)
        tr = dict(zip(gs.engine.TRIAL_FIELDS, sim.trial_results()[0]))
        tot = sim.totals()
        assert tr["tick_99"] == e.set_tick_99 and tr["status"] == status and tr["tick"] == e.t
        assert tr["received"] == e.received == tot["received"] and tr["messages"] == tot["messages"]
        # gs_step(1) repeated equals one gs_step(k), and a reset context equals a fresh one
        sim.reset()
        assert not sim.rumor_words().any() and not sim.received().any()
        sim.begin_rumors(senders)
        many = sim.step(e.t).tolist()
        sim.reset()
        sim.begin_rumors(senders)
        assert [sim.step(1)[0].tolist() for _ in range(e.t)] == many
        assert np.array_equal(sim.rumor_words(), e.have)
        fresh = PyRumorSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders)
        assert many == fresh.run(e.t).tolist()


def test_broadcast_begin_forms(gs, oracle):
    """gs_broadcast_begin on a set: s < 0 draws every sender, s >= 0 starts rumor
    j at (s + j) mod n; and a masked run that cannot reach 99 % ends at max_ticks."""
    n = 1000
    deg, ids = ring_table(n, seed=2)
    kw = dict(RS, n=n)
    p = oracle.make_params(**kw)
    dead = np.zeros(n, bool)
    dead[500:520] = True
    with gs.Simulator.rumor_set(cfg_of(gs, kw), 4) as sim:
        sim.load_peers(deg, ids)
        for s, senders in ((-1, [-1] * 4), (998, [998, 999, 0, 1])):
            e = PyRumorSet(oracle, p, deg, masked(deg, ids), senders)
            sim.broadcast_begin(s)
            assert [r["sender"] for r in sim.rumor_results()] == e.senders
            assert sim.step(10).tolist() == e.run(10).tolist() and np.array_equal(sim.rumor_words(), e.have)
            sim.reset()
        assert e.senders == [998, 999, 0, 1]
        sim.set_failed(words_of(dead))
        e = PyRumorSet(oracle, p, deg, masked(deg, ids), [1, 2, 3, 4], dead)
        status, want = reference_run(e, 10, 60)
        assert RUN_NAMES[status] == "MAX_TICKS" and e.t == 60
        sim.begin_rumors([1, 2, 3, 4])
        rows, st = sim.run(poll=10, max_ticks=60)
        assert st == status and rows.tolist() == want
        with pytest.raises(gs.GossipError):
            sim.begin_rumors([1, 2, 3, 4])       # already begun
        sim.reset()
        for bad in ([1, 2, 3], [1, 2, 3, n]):   # count != rumors, an entry >= n
            with pytest.raises(gs.GossipError) as ei:
                sim.begin_rumors(bad)
            assert ei.value.code == -1
        for call in (sim.removed, sim.median_state):
            with pytest.raises(gs.GossipError) as ei:
                call()
            assert ei.value.code == -1


def test_caller_stream_and_crashed_mask(gs, oracle):
    """gs_set_stream and gs_read_crashed as on a one-trial push-pull context: the
    rounds run on a stream the caller owns, and crashed() is the failure mask."""
    import ctypes as C
    n = 4133
    deg, ids = ring_table(n, seed=33)
    dead = np.random.default_rng(6).random(n) < 0.05
    senders = spread(n, 64)
    dead[senders] = False
    dead[n - 5:] = True     # failed nodes in the ragged last word
    dead[senders[-1]] = True
    with open("/proc/self/maps") as f:   # the HIP runtime the library itself loaded
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipStreamCreate.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p)], [C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        with gs.Simulator.rumor_set(cfg_of(gs, dict(RS, n=n)), 64) as sim:
            sim.load_peers(deg, ids)
            sim.set_failed(words_of(dead))
            sim.set_stream(stream.value)
            e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, senders, rounds=12, failed=dead, sim=sim)
            assert np.array_equal(sim.crashed(), words_of(dead)) and not e.started[-1] and row[4] > 32 * n
            sim.set_stream(None)         # back on the context's own stream: the same broadcast again
            sim.reset()
            assert np.array_equal(sim.crashed(), words_of(dead))   # the mask outlives a reset
            parity(gs, oracle, dict(RS, n=n), deg, ids, senders, rounds=3, failed=dead, sim=sim)
    finally:
        hip.hipStreamDestroy(stream)


def test_cli_prints_every_rumor(gs, oracle):
    """gossip_sim -model pushpull -rumors 5: each poll's line shows the
    least-covered started rumor, then a line per rumor and the round at which all
    were covered; without -rumors the push-pull output has none of it."""
    import subprocess
    from gossip_simulator_amd import _lib
    n, R = 3000, 5
    kw = dict(RS, n=n, seed=77)
    with gs.Simulator.rumor_set(cfg_of(gs, kw), R) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
    e = PyRumorSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), [-1] * R)
    want, msgs = [], 0
    while True:
        msgs += int(e.run(10)[:, 3].sum())
        e.poll()
        pct = np.float32(int(e.counts.min())) / np.float32(n) * np.float32(100.0)
        want.append(f"{_lib.format_float32(float(pct))}% covered, took {_lib.format_duration(e.t * 1_000_000)}")
        if e.pending == 0:
            break
        assert e.t < 200
    want += [f"rumor {j}: sender {e.senders[j]}, {int(e.counts[j])} nodes, 99% after "
             f"{_lib.format_duration(e.tick_99[j] * 1_000_000)}" for j in range(R)]
    want.append(f"--- Took {_lib.format_duration(e.t * 1_000_000)} to get 99% of all {R} rumors ---")
    args = [_lib.CLI_PATH, "-n", str(n), "-model", "pushpull", "-seed", "77"]
    r = subprocess.run(args + ["-rumors", str(R)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    tail = r.stdout.split(f"=== Broadcast {R} rumors ===\n")[1].splitlines()
    assert tail[:len(want)] == want
    assert tail[len(want):] == ["", f"Total message {msgs} Total Crashed 0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "=== Broadcast one message ===" in plain.stdout and "rumor" not in plain.stdout
    assert plain.stdout.split("=== Broadcast")[0] == r.stdout.split("=== Broadcast")[0]   # the same overlay lines


def test_trial_second_table_overlay_and_timing(gs, oracle):
    n = 4133
    deg, ids = ring_table(n, seed=21)
    deg2, ids2 = ring_table(n, seed=22)
    kw, kw7 = dict(RS, n=n), dict(RS, n=n, trial=7)
    senders = spread(n, 9)

    def ref_of(kw, deg, ids):
        return PyRumorSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders).run(12).tolist()
    ref, ref7, ref2 = ref_of(kw, deg, ids), ref_of(kw7, deg, ids), ref_of(kw, deg2, ids2)
    assert ref != ref7   # another trial draws other calls
    with gs.Simulator.rumor_set(cfg_of(gs, kw), 9) as sim:
        sim.load_peers(deg, ids)
        sim.begin_rumors(senders)
        assert sim.step(12).tolist() == ref
        sim.reset()
        sim.load_peers(deg2, ids2)       # a second table on the same context
        sim.begin_rumors(senders)
        assert sim.step(12).tolist() == ref2
        sim.reset()
        sim.set_trial(7)
        sim.load_peers(deg, ids)
        sim.begin_rumors(senders)
        assert sim.step(12).tolist() == ref7
        assert not sim.crashed().any()
    kwo = dict(RS, n=5000)
    with gs.Simulator.rumor_set(cfg_of(gs, kwo, timing=True), 64) as sim:   # an overlay-built table, keyed senders
        sim.build_overlay()
        deg, ids = sim.read_peers()
        e = PyRumorSet(oracle, oracle.make_params(**kwo), deg, masked(deg, ids), [-1] * 64)
        sim.broadcast_begin(-1)
        assert sim.step(12).tolist() == e.run(12).tolist() and np.array_equal(sim.rumor_words(), e.have)
        tm = sim.timing()
        assert tm["deliver_launches"] == 12 and tm["resolve_launches"] == 12
        assert tm["deliver_ms"] > 0 and tm["resolve_ms"] > 0
