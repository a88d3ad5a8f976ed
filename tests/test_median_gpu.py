"""The HIP median-counter engine (gs_median.hip) against the Python restatement
of tests/test_median.py: bit-exact per round -- the stats row, the informed
set, the done set and the state bytes after every gs_step(1) -- over the shapes
at which the kernels can go wrong, then gs_run's stop rule, the lifecycle calls
and the combinations the model refuses.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_median import MEDIAN, PyMedian, reference_run, words_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_NAMES = {0: "COVERED", 1: "QUIESCENT", 2: "MAX_TICKS"}


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def cfg_of(gs, kw, k=2, **more):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], model="median", rumor_k=k, **more)


def check_state(sim, e, t):
    assert np.array_equal(sim.median_state(), e.st), f"state bytes differ at round {t}"
    assert np.array_equal(sim.received(), words_of(e.inf)), f"informed set differs at round {t}"
    assert np.array_equal(sim.removed(), words_of(e.removed)), f"done set differs at round {t}"


def check_round(sim, e, got, row, t):
    assert [int(x) for x in got] == row, f"round {t}:\n{got}\n{row}"
    check_state(sim, e, t)


def parity(gs, oracle, kw, deg, ids, sender, k=2, rounds=40, failed=None):
    """gs_step(1) x rounds against the restatement; returns it and its last row."""
    e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, k, failed)
    with gs.Simulator(cfg_of(gs, kw, k)) as sim:
        sim.load_peers(deg, ids)
        if failed is not None:
            sim.set_failed(words_of(failed))
        sim.broadcast_begin(sender)
        tot = sim.totals()
        assert (tot["received"], tot["pending"]) == (e.received, e.pending)
        check_state(sim, e, 0)
        row = None
        for t in range(1, rounds + 1):
            row = e.step()
            check_round(sim, e, sim.step(1)[0], row, t)
        tot = sim.totals()
        assert tot["tick"] == rounds and tot["received"] == e.received and tot["pending"] == e.pending
    return e, row


def ring_table(n, seed, stride=6, lo=5):
    """A random table whose first slot is a ring, so every node has a caller and
    the run ends by itself."""
    deg, ids = random_table(n, stride, max(lo, 1), stride, seed=seed)
    ids[:, 0] = (np.arange(n) + 1) % n
    return deg, ids


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4133, 20_000, 65_613])
def test_sizes(gs, oracle, n):
    """Word edges, a partial last word and more than one block; rows with
    duplicates, self entries and (n > 2) empty rows."""
    deg, ids = random_table(n, 6, 0 if n > 2 else 1, 6, seed=n)
    deg[n // 2] = max(deg[n // 2], 1)
    e, row = parity(gs, oracle, dict(MEDIAN, n=n), deg, ids, sender=n // 2, rounds=30)
    if n >= 4133:
        assert row[4] > n // 2 and e.removed.sum() > n // 2


@pytest.mark.parametrize("k,n", [(1, 4133), (3, 4133), (127, 4133), (1, 65), (127, 65), (3, 20_000)])
def test_counter_lengths(gs, oracle, k, n):
    deg, ids = ring_table(n, seed=k + n)
    e, row = parity(gs, oracle, dict(MEDIAN, n=n), deg, ids, sender=5, k=k, rounds=40)
    assert row[4] > 0.99 * n
    if k == 127:  # the counters are still running
        assert 20 < e.st.max() <= 127 and not e.removed.any() and row[6] == n
    if n == 20_000:
        assert e.removed.all() and row[6] == 0
    # (at the small sizes a few B nodes whose every partner is done already stay B: DESIGN.md 4.8)


@pytest.mark.parametrize("drop", [0.0, 0.1, 0.57])
def test_drop_rates(gs, oracle, drop):
    n = 4133
    deg, ids = ring_table(n, seed=11)
    e, row = parity(gs, oracle, dict(MEDIAN, n=n, drop_rate=drop), deg, ids, sender=9, k=2, rounds=45)
    assert row[4] > 0.9 * n and (row[2] == row[1]) == (drop == 0.0)


def test_every_call_lost_reaches_max_ticks(gs, oracle):
    n = 777
    deg, ids = ring_table(n, seed=1)
    kw = dict(MEDIAN, n=n, drop_rate=1.0)
    e, row = parity(gs, oracle, kw, deg, ids, sender=0, rounds=5)
    assert row == [5, n, 0, 0, 1, 0, 1]
    with gs.Simulator(cfg_of(gs, kw)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(0)
        rows, st = sim.run(poll=10, max_ticks=30)
        assert RUN_NAMES[st] == "MAX_TICKS" and len(rows) == 3
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"], tot["sent"]) == (30, 1, 1, 0)


@pytest.mark.parametrize("mask", ["one_percent", "all_but_sender", "all", "sender"])
def test_failure_masks(gs, oracle, mask):
    n = 4133
    deg, ids = ring_table(n, seed=9)
    dead = {"one_percent": np.random.default_rng(3).random(n) < 0.01, "all_but_sender": np.ones(n, bool),
            "all": np.ones(n, bool), "sender": np.zeros(n, bool)}[mask]
    dead[100] = mask in ("all", "sender")
    e, row = parity(gs, oracle, dict(MEDIAN, n=n, drop_rate=0.0), deg, ids, 100, k=2, rounds=40, failed=dead)
    assert not (e.inf & dead).any()
    if mask == "one_percent":
        assert row[4] > 0.9 * n
    elif mask == "all_but_sender":   # it calls a failed friend every round: sent, never a connection
        assert row == [40, 1, 1, 0, 1, 0, 1]
    else:
        assert row[4] == 0 and row[6] == 0


@pytest.mark.parametrize("fanout,fanin", [(5, 6), (3, 4)])
def test_overlay_built_tables(gs, oracle, fanout, fanin):
    kw = dict(MEDIAN, n=5000, fanout=fanout, fanin=fanin)
    with gs.Simulator(cfg_of(gs, kw, 2, timing=True)) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
        e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), -1, 2)
        sim.broadcast_begin(-1)
        for t in range(1, 36):
            check_round(sim, e, sim.step(1)[0], e.step(), t)
        assert e.received > 0.9 * kw["n"]
        tm = sim.timing()
        assert tm["deliver_launches"] == 35 and tm["resolve_launches"] == 35
        assert tm["deliver_ms"] > 0 and tm["resolve_ms"] > 0


@pytest.mark.parametrize("stride", [1, 255])
def test_row_lengths_1_and_255(gs, oracle, stride):
    n = 3001
    deg = np.full(n, stride, np.uint8)
    ids = np.random.default_rng(stride).integers(0, n, size=(n, stride)).astype(np.uint32)
    ids[:, 0] = (np.arange(n) + 1) % n
    kw = dict(MEDIAN, n=n, fanout=stride, fanin=stride)
    if stride == 1:   # gs_load_peers_device wants rows of two slots or more; the host call takes one
        deg[::7] = 0  # and empty rows sprinkled in
    e, row = parity(gs, oracle, kw, deg, ids, sender=17, k=2, rounds=40)
    assert row[4] > 1


def hub_table(n, seed):
    """Every row names node 0 (twice in every third row), so all tally adds and
    flag ORs of a round meet in node 0's words."""
    rng = np.random.default_rng(seed)
    deg = np.full(n, 4, np.uint8)
    ids = rng.integers(1, n, size=(n, 4)).astype(np.uint32)
    ids[:, 1] = 0
    ids[::3, 3] = 0
    return deg, ids


def test_hub_takes_every_add_of_a_round(gs, oracle):
    """n = 20,000: about a third of the callers pick node 0, several thousand a
    round.  While node 0 is in B its tally takes that many adds in both fields
    (ge from callers at least as far along, lt from the others), and its gotb
    and gotc bits that many requests: a field that spilled into its neighbour or
    a lost update would change node 0's next state or stall its counter."""
    n = 20_000
    deg, ids = hub_table(n, 5)
    kw = dict(MEDIAN, n=n, fanout=4, fanin=4, drop_rate=0.0)
    e = PyMedian(oracle, oracle.make_params(**kw), deg, ids, 7, 3)
    most = 0
    with gs.Simulator(cfg_of(gs, kw, 3)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(7)
        for t in range(1, 31):
            before = int(e.state[0])
            check_round(sim, e, sim.step(1)[0], e.step(), t)
            if 1 <= before <= 3:
                most = max(most, int((e.last[1] == 0).sum()))
    assert most > 5000 and e.removed[0]


def test_ring(gs, oracle):
    n = 777
    deg = np.ones(n, np.uint8)
    ids = np.zeros((n, 2), np.uint32)
    ids[:, 0] = (np.arange(n) + 1) % n
    kw = dict(MEDIAN, n=n, fanout=2, fanin=2, drop_rate=0.0)
    e, row = parity(gs, oracle, kw, deg, ids, sender=3, k=2, rounds=40)
    assert 2 < row[4] < n


GRID_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import gossip_simulator_amd as gs
from test_gpu_parity import random_table
n, rounds = 20_000, int(sys.argv[2])
deg, ids = random_table(n, 6, 5, 6, seed=20)
ids[:, 0] = (np.arange(n) + 1) % n
cfg = gs.Config(n=n, droprate=0.1, crashrate=0.0, seed=0x5EED, model="median", rumor_k=2)
with gs.Simulator(cfg) as sim:
    sim.load_peers(deg, ids)
    sim.broadcast_begin(12345)
    rows = [[int(x) for x in sim.step(1)[0]] for _ in range(rounds)]
    print(json.dumps(dict(rows=rows, st=sim.median_state().tolist(), recv=sim.received().tolist(),
                          done=sim.removed().tolist())))
"""


@pytest.fixture(scope="module")
def grid_case(oracle):
    """n = 20,000, k = 2, 30 rounds: the restatement's rows and final sets (computed once)."""
    n = 20_000
    deg, ids = ring_table(n, seed=20)
    e = PyMedian(oracle, oracle.make_params(**dict(MEDIAN, n=n)), deg, masked(deg, ids), 12345, 2)
    rows = e.run(30).tolist()
    return rows, e.st.tolist(), words_of(e.inf).tolist(), words_of(e.removed).tolist()


@pytest.mark.parametrize("blocks", ["1", "2", "7"])
def test_grid_of_few_blocks(gs, grid_case, blocks, tmp_path):
    """313 words through 4, 8 and 28 waves (GS_MEDIAN_GRID): many passes per
    wave, the same bits.  In a child process, which keeps this one's
    environment clean."""
    rows, st, recv, done = grid_case
    script = tmp_path / "grid_child.py"
    script.write_text(GRID_CHILD)
    env = dict(os.environ, GS_MEDIAN_GRID=blocks)
    r = subprocess.run([sys.executable, str(script), ROOT, "30"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["rows"] == rows
    assert got["st"] == st and got["recv"] == recv and got["done"] == done


@pytest.fixture(scope="module")
def run_case(oracle):
    n = 4133
    deg, ids = ring_table(n, seed=70)   # (a table on which k = 3 leaves no B node behind: DESIGN.md 4.8)
    kw = dict(MEDIAN, n=n)
    e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 3, 3)
    rows = []
    while e.pending:
        rows.append(e.step())
        assert e.t < 500
    rows += [e.step() for _ in range(64)]   # the rounds a poll runs past the end
    return kw, deg, ids, rows


@pytest.mark.parametrize("poll", [1, 3, 10, 64])
def test_run_agrees_with_stepping(gs, oracle, run_case, poll):
    kw, deg, ids, step_rows = run_case
    e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 3, 3)
    status, tick_99 = reference_run(oracle, e, poll, 10_000)
    assert RUN_NAMES[status] == "COVERED" and tick_99 and tick_99 % poll == 0
    with gs.Simulator(cfg_of(gs, kw, 3)) as sim:
        sim.load_peers(deg, ids)
        sim.broadcast_begin(3)
        rows, st = sim.run(poll=poll, max_ticks=10_000)
        assert st == status and len(rows) * poll == e.t
        for i, r in enumerate(rows):   # a poll's row: the sums of its ticks' rows, the last one's cumulative fields
            chunk = np.array(step_rows[i * poll:(i + 1) * poll], dtype=np.uint64)
            want = [int(chunk[-1, 0])] + [int(chunk[:, c].sum()) for c in (1, 2, 3)] + [int(x) for x in chunk[-1, 4:]]
            assert [int(x) for x in r] == want, f"poll {i}"
        tot = sim.totals()
        assert (tot["tick"], tot["received"], tot["pending"]) == (e.t, e.received, 0)
        check_state(sim, e, e.t)
        tr = dict(zip(gs.engine.TRIAL_FIELDS, sim.trial_results()[0]))
        assert tr["tick_99"] == tick_99 and tr["status"] == status and tr["tick"] == e.t
        assert tr["received"] == e.received and tr["messages"] == tot["messages"]
        assert tot["messages"] == sum(r[3] for r in step_rows[:e.t])
        sim.reset()                      # stepping the same broadcast gives the rows the polls summed
        sim.broadcast_begin(3)
        got = sim.step(e.t)
        assert got.tolist() == step_rows[:e.t]


def test_run_statuses(gs, oracle):
    """Quiescent below 99 % (the sender's component is 3,000 of the 4,133 nodes),
    the failed sender's first poll, and max_ticks for a sender whose every
    friend is failed."""
    n = 4133
    d1, i1 = ring_table(3000, seed=30)
    d2, i2 = ring_table(n - 3000, seed=31)
    deg, ids = np.concatenate([d1, d2]), np.concatenate([i1, i2 + 3000]).astype(np.uint32)
    none = np.zeros(n, bool)
    kw = dict(MEDIAN, n=n)
    for sender, failed, max_ticks, want in ((3, none, 200, "QUIESCENT"), (1, np.arange(n) == 1, 200, "QUIESCENT"),
                                            (3, np.arange(n) != 3, 40, "MAX_TICKS")):
        e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, 3, failed)
        status, tick_99 = reference_run(oracle, e, 10, max_ticks)
        assert RUN_NAMES[status] == want and tick_99 == 0
        with gs.Simulator(cfg_of(gs, kw, 3)) as sim:
            sim.load_peers(deg, ids)
            sim.set_failed(words_of(failed))
            sim.broadcast_begin(sender)
            rows, st = sim.run(poll=10, max_ticks=max_ticks)
            assert st == status and len(rows) * 10 == e.t
            check_state(sim, e, e.t)
            tot = sim.totals()
            assert (tot["received"], tot["pending"]) == (e.received, e.pending)


def steps(sim, rounds):
    return [[int(x) for x in sim.step(1)[0]] for _ in range(rounds)]


def test_reset_trial_and_two_contexts(gs, oracle):
    n = 4133
    deg, ids = ring_table(n, seed=21)
    deg2, ids2 = ring_table(n, seed=22)
    kw, kw7 = dict(MEDIAN, n=n), dict(MEDIAN, n=n, trial=7)

    def ref_of(kw, deg, ids, sender):
        return PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), sender, 2).run(30).tolist()
    ref, ref7, ref2 = ref_of(kw, deg, ids, 9), ref_of(kw7, deg, ids, 9), ref_of(kw, deg2, ids2, 11)
    assert ref != ref7   # another trial draws other calls
    with gs.Simulator(cfg_of(gs, kw)) as a, gs.Simulator(cfg_of(gs, kw)) as b:
        a.load_peers(deg, ids)
        b.load_peers(deg2, ids2)
        a.broadcast_begin(9)
        b.broadcast_begin(11)
        ra, rb = [], []
        for _ in range(30):   # side by side, a round each in turn
            ra += steps(a, 1)
            rb += steps(b, 1)
        assert ra == ref and rb == ref2
        a.reset()             # a second broadcast equals the first
        assert not a.received().any() and not a.removed().any() and not a.median_state().any()
        a.broadcast_begin(9)
        assert steps(a, 30) == ref
        a.reset()
        a.set_trial(7)
        a.load_peers(deg, ids)
        a.broadcast_begin(9)
        assert steps(a, 30) == ref7


def test_load_peers_device(gs, oracle):
    import ctypes as C
    n = 4133
    deg, ids = ring_table(n, seed=41)
    kw = dict(MEDIAN, n=n)
    e = PyMedian(oracle, oracle.make_params(**kw), deg, masked(deg, ids), 8, 2)
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
        with gs.Simulator(cfg_of(gs, kw)) as sim:
            sim.load_peers_device(bufs[0].value, bufs[1].value, ids.shape[1])
            sim.broadcast_begin(8)
            for t in range(1, 31):
                check_round(sim, e, sim.step(1)[0], e.step(), t)
    finally:
        for d in bufs:
            hip.hipFree(d)


def test_refusals(gs):
    kw = dict(MEDIAN, n=20000)

    def two_trials():
        return gs.Simulator(cfg_of(gs, kw, trials=2))
    for make in (two_trials, lambda: gs.Simulator(cfg_of(gs, kw), devices=[0, 0]),
                 lambda: gs.Simulator.rank(cfg_of(gs, kw), 2, 0, None),
                 lambda: gs.Simulator.batch(cfg_of(gs, kw)), lambda: gs.Simulator.batch(cfg_of(gs, kw, trials=2))):
        with pytest.raises(gs.GossipError) as ei:
            make()
        assert ei.value.code == -1 and "GS_MODEL_MEDIAN" in str(ei.value)
    with gs.Simulator(gs.Config(n=1000, model="pushpull")) as sim:
        with pytest.raises(gs.GossipError) as ei:
            sim.median_state()
        assert ei.value.code == -1 and "GS_MODEL_MEDIAN" in str(ei.value)
        with pytest.raises(gs.GossipError) as ei:
            sim.removed()    # keeps its answer for the other models
        assert ei.value.code == -1 and "GS_MODEL_RUMOR" in str(ei.value)
