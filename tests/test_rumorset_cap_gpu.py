"""The capped round kernel, the start-aware seed and the injection
(gs_rumorset_cap.hip) against PyCappedSet of tests/test_rumorset_cap.py:
bit-exact per gs_step(1) in the rumor words, the stats row, the per-rumor
counts, the holds-every-rumor set and the three traffic counters, over the
shapes at which the kernels can go wrong.  Every case with B < R asserts from
the restatement that the cap binds within its rounds.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumorset import RS, bit_counts, reference_run, words_of
from test_rumorset_cap import POLICIES, PyCappedSet
from test_rumorset_gpu import RUN_NAMES, cfg_of, check_state, ring_table, spread

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def parity(gs, oracle, kw, deg, ids, senders, rounds, B, pick="low", starts=None, failed=None, binds=None):
    """set_payload(B, pick), begin_rumors(senders, starts), then gs_step(1) x
    rounds against the restatement (every tick is a poll).  binds (default: B <
    R): the cap must bind within the rounds."""
    R = len(senders)
    e = PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, starts, B, POLICIES[pick], failed)
    row = None
    with gs.Simulator.rumor_set(cfg_of(gs, kw), R) as sim:
        sim.load_peers(deg, ids)
        if failed is not None:
            sim.set_failed(words_of(failed))
        sim.set_payload(B, pick)
        sim.begin_rumors(senders, starts)
        tot = sim.totals()
        assert (tot["received"], tot["pending"]) == (e.received, e.pending)
        check_state(sim, e, 0)
        if B:
            assert sim.rumor_traffic() == e.traffic
        for t in range(1, rounds + 1):
            row = e.step()
            e.poll()
            got = [int(x) for x in sim.step(1)[0]]
            assert got == row, f"round {t}:\n{got}\n{row}"
            check_state(sim, e, t)
            if B:
                assert sim.rumor_traffic() == e.traffic, f"traffic differs at round {t}"
        tot = sim.totals()
        assert tot["tick"] == rounds and tot["received"] == e.received and tot["pending"] == e.pending
    if B < R if binds is None else binds:
        assert e.bound > 0 and e.carried < e.wanted, "the cap never bound: the case shows nothing"
    elif B:
        assert e.bound == 0 and e.carried == e.wanted
    return e, row


def clustered(n, R):
    """Senders a few nodes apart, so that rumors meet (and the cap binds) early."""
    return [(j * 3) % n for j in range(R)]


SIZES = [(1, 2, 1, "low"), (1, 64, 63, "rotate"),
         (64, 2, 1, "high"), (64, 63, 2, "rotate"), (64, 64, 64, "low"), (64, 63, 62, "low"),
         (65, 2, 2, "rotate"), (65, 64, 63, "high"), (65, 63, 63, "high"), (65, 64, 1, "low"),
         (4133, 2, 1, "rotate"), (4133, 63, 62, "rotate"), (4133, 64, 2, "low"), (4133, 64, 2, "high"),
         (4133, 64, 2, "rotate"), (4133, 64, 63, "low"), (4133, 63, 1, "high"), (4133, 64, 64, "rotate")]


@pytest.mark.parametrize("n,R,B,pick", SIZES)
def test_sizes_rumor_counts_caps_and_policies(gs, oracle, n, R, B, pick):
    """One node, an exact word, one bit into the second word, ragged tails; R =
    64 uses bit 63, R = 63 leaves a bit that stays 0, R = 2 is the shortest ring
    with a choice.  Rows with duplicates, self entries and (n > 2) empty rows.
    On one node nothing ever connects to another, so nothing can bind there."""
    deg, ids = random_table(n, 6, 0 if n > 2 else 1, 6, seed=n)
    senders = clustered(n, R)
    if n > 1 and B == R - 1:
        senders = [5 % n] * R    # only a node that holds all R against one that holds none wants more than R - 1
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, senders, 14, B, pick, binds=B < R and n > 1)
    assert int(e.have.max()) >> R == 0
    if n == 4133:
        assert row[4] > min(R, 4 * B) * n // 4    # well under way, also where B = 1 moves one rumor per message


@pytest.mark.parametrize("R", [2, 63, 64])
@pytest.mark.parametrize("pick", list(POLICIES))
def test_two_nodes_bind_in_round_one(gs, oracle, R, pick):
    """n = 2, rows 0 <-> 1, no loss, every sender at node 0, B = R - 1: node 1
    wants all R rumors in round 1, one more than a message carries."""
    deg = np.ones(2, np.uint8)
    ids = np.array([[1, 0], [0, 0]], np.uint32)   # (rows of two slots, one used)
    kw = dict(RS, n=2, fanout=2, fanin=2, drop_rate=0.0)
    e, row = parity(gs, oracle, kw, deg, ids, [0] * R, 4, R - 1, pick)
    assert e.bound >= 1 and e.have.tolist() == [2**R - 1] * 2


@pytest.mark.parametrize("drop", [0.0, 0.1, 1.0])
def test_drop_rates(gs, oracle, drop):
    n = 4133
    deg, ids = ring_table(n, seed=11)
    e, row = parity(gs, oracle, dict(RS, n=n, drop_rate=drop), deg, ids, clustered(n, 9), 16, 2, "rotate",
                    binds=drop < 1.0)
    if drop == 1.0:    # nothing ever moves, nothing is ever wanted
        assert row == [16, n, 0, 0, 9, 0, 9] and e.traffic == dict(wanted=0, carried=0, bound=0)
    else:
        assert row[4] > 4 * n and (row[2] == row[1]) == (drop == 0.0)


def test_mask(gs, oracle):
    n = 4133
    deg, ids = ring_table(n, seed=9)
    dead = np.random.default_rng(3).random(n) < 0.05
    senders = clustered(n, 12)
    dead[senders] = False
    dead[senders[4]] = True     # a dead rumor among live ones
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, senders, 14, 3, "high", failed=dead)
    assert not e.have[dead].any() and not e.started[4] and not e.column(4).any() and row[4] > 5 * n


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
    senders = [j // 3 for j in range(7)]   # nodes 0 and 1 hold three rumors each, one more than B
    e, row = parity(gs, oracle, kw, deg, ids, senders, 14, 2, "low")
    assert row[4] > 7


def test_hub(gs, oracle):
    """n = 70,000, every node's only friend is node 0: 69,999 callers meet in
    node 0's word, each with a message of at most B = 3 rumors of its own choice
    (ROTATE: its own offsets), and node 0's word is their union."""
    n, R = 70_000, 64
    deg = np.ones(n, np.uint8)
    ids = np.zeros((n, 2), np.uint32)
    kw = dict(RS, n=n, fanout=2, fanin=2)
    e, row = parity(gs, oracle, kw, deg, ids, spread(n, R), 5, 3, "rotate")
    assert (e.last[1] == 0).sum() > 60_000 and int(e.have[0]) == 2**64 - 1 and e.bound > n


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_grid_of_few_blocks(gs, oracle, blocks, monkeypatch):
    """65 words through 4 and 12 waves (GS_RUMORSET_GRID): the same bits and the same six sums."""
    monkeypatch.setenv("GS_RUMORSET_GRID", blocks)
    n = 4133
    deg, ids = ring_table(n, seed=20)
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, clustered(n, 64), 14, 4, "rotate", starts=[j // 8 for j in range(64)])
    assert row[4] > 16 * n


def test_default_grid_takes_a_second_pass(gs, oracle):
    """n = 600,000: 9,375 words against the default grid's 8,192 waves; the
    senders sit in the second pass's nodes."""
    n = 600_000
    deg, ids = ring_table(n, seed=6)
    senders = [8192 * 64 + 100 + (j % 8) for j in range(64)]
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, senders, 5, 2, "high")
    assert bit_counts(e.have[8192 * 64:], 64).sum() > 2 * 64   # what the waves' second pass wrote, beyond the senders' bits


# ---- starts -----------------------------------------------------------------------------

@pytest.mark.parametrize("B", [0, 2])
def test_mixed_starts(gs, oracle, B):
    """Starts 0, 0, 3, 3, 7 (two in one round, two of them at one node), with and
    without a cap: an uncapped set with late starts runs k_rs_round and the injection."""
    n = 4133
    deg, ids = ring_table(n, seed=31)
    senders, starts = [10, 11, 12, 12, 14], [0, 0, 3, 3, 7]
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, senders, 16, B, "low", starts=starts, binds=B > 0)
    assert e.counts.min() > 0 and row[4] > n


def test_dead_late_rumor_and_the_holds_all_bit(gs, oracle):
    n = 300
    deg, ids = ring_table(n, seed=32)
    dead = np.zeros(n, bool)
    dead[40] = True
    e, row = parity(gs, oracle, dict(RS, n=n), deg, ids, [7, 40, 9], 12, 1, "low", starts=[0, 4, 6], failed=dead)
    assert e.started == [True, False, True] and not e.column(1).any() and e.holds_all.any()
    # R = 1, s = 5: nothing to hold for five rounds, then the injection completes the sender's word
    e = PyCappedSet(oracle, oracle.make_params(**dict(RS, n=n)), deg, masked(deg, ids), [33], [5], 1)
    with gs.Simulator.rumor_set(cfg_of(gs, dict(RS, n=n)), 1) as sim:
        sim.load_peers(deg, ids)
        sim.set_payload(1)
        sim.begin_rumors([33], [5])
        for t in range(1, 9):
            assert [int(x) for x in sim.step(1)[0]] == e.step()
            assert np.array_equal(sim.received(), words_of(e.holds_all)) and e.holds_all.any() == (t >= 5)
            assert np.array_equal(sim.rumor_words(), e.have)


def test_run_goes_on_past_a_late_start(gs, oracle):
    """Rumor 1 starts at round 40, long after rumor 0 is everywhere: gs_run(poll =
    10) must not stop GS_RUN_COVERED before it is in and covered."""
    n, senders, starts = 4133, [5, 4000], [0, 40]
    deg, ids = ring_table(n, seed=70)
    kw = dict(RS, n=n)
    e = PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, starts, 1)
    status, want = reference_run(e, 10, 10_000)
    assert RUN_NAMES[status] == "COVERED" and 0 < e.tick_99[0] < 40 < e.tick_99[1] == e.set_tick_99 == e.t
    with gs.Simulator.rumor_set(cfg_of(gs, kw), 2) as sim:
        sim.load_peers(deg, ids)
        sim.set_payload(1)
        sim.begin_rumors(senders, starts)
        rows, st = sim.run(poll=10, max_ticks=10_000)
        assert st == status and [[int(x) for x in r] for r in rows] == want
        check_state(sim, e, e.t)
        assert sim.rumor_traffic() == e.traffic


def test_a_start_past_one_ring_of_stat_slots(gs, oracle):
    """One gs_step call of 4,200 rounds spans the 4,096 stat slots and the start
    at round 4,100: n = 64 keeps the restatement's 4,200 rounds short."""
    n, senders, starts = 64, [3, 60], [0, 4100]
    deg, ids = ring_table(n, seed=41)
    kw = dict(RS, n=n)
    e = PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, starts, 1)
    want = e.run(4200)
    with gs.Simulator.rumor_set(cfg_of(gs, kw), 2) as sim:
        sim.load_peers(deg, ids)
        sim.set_payload(1)
        sim.begin_rumors(senders, starts)
        got = sim.step(4200)
        assert np.array_equal(got, want)
        assert got[4098, 4] == n and got[4099, 4] == n + 1 and got[-1, 4] == 2 * n
        assert np.array_equal(sim.rumor_words(), e.have) and sim.rumor_traffic() == e.traffic


# ---- the uncapped engine, gs_run, the lifecycle, the CLI -----------------------------------------

@pytest.mark.parametrize("pick", list(POLICIES))
def test_payload_of_R_equals_the_uncapped_engine(gs, oracle, pick):
    """n = 4133, R = 64, every start 0: k_rsc_round under set_payload(64) against
    k_rs_round on a second context, words and rows per round."""
    n, R = 4133, 64
    deg, ids = random_table(n, 6, 0, 6, seed=8)
    senders = [int(x) for x in np.random.default_rng(12).integers(0, n, size=R)]
    kw = dict(RS, n=n)
    with gs.Simulator.rumor_set(cfg_of(gs, kw), R) as a, gs.Simulator.rumor_set(cfg_of(gs, kw), R) as b:
        for sim in (a, b):
            sim.load_peers(deg, ids)
        b.set_payload(R, pick)
        a.begin_rumors(senders)
        b.begin_rumors(senders)
        for t in range(1, 15):
            assert np.array_equal(a.step(1), b.step(1)), t
            assert np.array_equal(a.rumor_words(), b.rumor_words()), t
            assert np.array_equal(a.received(), b.received()), t
        tr = b.rumor_traffic()
        assert tr["wanted"] == tr["carried"] > n and tr["bound"] == 0
        with pytest.raises(gs.GossipError) as ei:   # an uncapped set does not count its traffic
            a.rumor_traffic()
        assert ei.value.code == -1


def test_run_agrees_with_the_restatement(gs, oracle):
    n, R = 4133, 16
    deg, ids = ring_table(n, seed=70)
    kw = dict(RS, n=n)
    senders, starts = clustered(n, R), list(range(R))
    e = PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, starts, 2, POLICIES["high"])
    status, want = reference_run(e, 10, 10_000)
    assert RUN_NAMES[status] == "COVERED" and all(e.tick_99) and e.set_tick_99 == e.t and e.bound > 0
    with gs.Simulator.rumor_set(cfg_of(gs, kw), R) as sim:
        sim.load_peers(deg, ids)
        sim.set_payload(2, "high")
        sim.begin_rumors(senders, starts)
        rows, st = sim.run(poll=10, max_ticks=10_000)
        assert st == status and [[int(x) for x in r] for r in rows] == want
        check_state(sim, e, e.t)
        assert sim.rumor_traffic() == e.traffic


def test_set_payload_lifecycle(gs, oracle):
    """Refused on other contexts, out of range and mid-broadcast; kept by reset and set_trial."""
    n = 1000
    deg, ids = ring_table(n, seed=2)
    kw, kw7 = dict(RS, n=n), dict(RS, n=n, trial=7)
    senders = clustered(n, 6)

    def ref_of(kw, B, pick):
        return PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), senders, None, B, pick).run(10).tolist()
    capped, capped7, plain = ref_of(kw, 1, 1), ref_of(kw7, 1, 1), ref_of(kw, 0, 0)
    assert capped != plain
    with gs.Simulator(cfg_of(gs, kw)) as one:
        with pytest.raises(gs.GossipError) as ei:
            one.set_payload(2)
        assert ei.value.code == -1
    with gs.Simulator.rumor_set(cfg_of(gs, kw), 6) as sim:
        sim.load_peers(deg, ids)
        for bad in ((65, 0), (1, 3)):
            with pytest.raises(gs.GossipError) as ei:
                sim.set_payload(*bad)
            assert ei.value.code == -1
        sim.set_payload(1, "high")
        assert sim.rumor_traffic() == dict(wanted=0, carried=0, bound=0)   # nothing begun yet
        sim.begin_rumors(senders)
        with pytest.raises(gs.GossipError):
            sim.set_payload(2)                  # mid-broadcast
        assert sim.step(10).tolist() == capped
        sim.reset()                             # the cap outlives a reset
        sim.begin_rumors(senders)
        assert sim.step(10).tolist() == capped
        sim.reset()
        sim.set_trial(7)                        # and a new trial
        sim.load_peers(deg, ids)
        sim.begin_rumors(senders)
        assert sim.step(10).tolist() == capped7
        sim.reset()
        sim.set_trial(0)
        sim.load_peers(deg, ids)
        sim.set_payload(0)                      # back to no cap: the engine of section 4.9
        sim.begin_rumors(senders)
        assert sim.step(10).tolist() == plain
        for bad in ([0] * 5, [0] * 5 + [-1], [0] * 5 + [2**31]):
            sim.reset()
            with pytest.raises((gs.GossipError, ValueError)):
                sim.begin_rumors(senders, bad)


def test_cli_prints_starts_and_traffic(gs, oracle):
    """gossip_sim -rumors 5 -payload 1 -pick high -every 3: the polls' lines, a
    line per rumor with its start and its rounds from there to 99 % (every
    round is a poll), and the traffic line; -every alone runs a payload of 64."""
    import subprocess
    from gossip_simulator_amd import _lib
    n, R, E = 3000, 5, 3
    kw = dict(RS, n=n, seed=77)
    with gs.Simulator.rumor_set(cfg_of(gs, kw), R) as sim:
        sim.build_overlay()
        deg, ids = sim.read_peers()
    dur = lambda t: _lib.format_duration(t * 1_000_000)
    for flags, B, pick in ((["-payload", "1", "-pick", "high", "-every", str(E)], 1, 1), (["-every", str(E)], 64, 0)):
        e = PyCappedSet(oracle, oracle.make_params(**kw), deg, masked(deg, ids), [-1] * R, [j * E for j in range(R)], B, pick)
        want, msgs = [], 0
        while True:
            for _ in range(10):
                msgs += e.step()[3]
                e.poll()
            pct = np.float32(int(e.counts.min())) / np.float32(n) * np.float32(100.0)
            want.append(f"{_lib.format_float32(float(pct))}% covered, took {dur(e.t)}")
            if e.pending == 0:
                break
            assert e.t < 300
        want += [f"rumor {j}: sender {e.senders[j]}, {int(e.counts[j])} nodes, start {dur(j * E)}, 99% after "
                 f"{dur(e.tick_99[j])}, {e.tick_99[j] - j * E} rounds from start" for j in range(R)]
        want += [f"--- Took {dur(e.t)} to get 99% of all {R} rumors ---", "", f"Total message {msgs} Total Crashed 0",
                 f"Rumor copies wanted {e.wanted} carried {e.carried}, messages bound by the payload {e.bound}"]
        assert (e.bound > 0) == (B == 1)
        args = [_lib.CLI_PATH, "-n", str(n), "-model", "pushpull", "-seed", "77", "-rumors", str(R)] + flags
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split(f"=== Broadcast {R} rumors ===\n")[1].splitlines() == want
