"""Concurrent rumors for push-pull (gs_create_rumorset):
up to 64 push-pull broadcasts over one table, one seed and one trial in one
pass, a bit per rumor in a uint64 per node.  The model is pinned here by a
pure-Python restatement written from the specification, itself pinned three
ways: by hand-derived answers, by the oracle's push-pull (every column of the
words is one push-pull broadcast's informed set, per round), and by a
restatement with the pull direction removed, which the oracle tells apart.
The HIP rounds (gs_rumorset.hip) must match the restatement bit-exactly per
round (tests/test_rumorset_gpu.py).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumor import ROOT, cli, philox_np, words_of

K_SENDER, K_PUSHPULL = 1, 9
U32 = np.uint64(32)
RS = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.0,
          seed=0x5EED, trial=0, model=1)


def bit_counts(have, R):
    """Nodes that hold rumor j, j < R."""
    bits = np.unpackbits(np.ascontiguousarray(have, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1,
                         bitorder="little")
    return bits.sum(axis=0, dtype=np.int64)[:R]


class PyRumorSet:
    """The specification, round by round.  State per node: the word have (bit j:
    the node holds rumor j) and the failed bit.  Every decision of a round
    reads H, the words at its start.

    `wrong` restates a mistake, for the non-vacuity test only: "no_pull" drops
    the caller's own end of a connection (push only)."""

    def __init__(self, oracle, p, deg, ids, senders, failed=None, wrong=None):
        self.oracle, self.n, self.t, self.wrong = oracle, int(p.n), 0, wrong
        self.key = [int(p.seed) & 0xFFFFFFFF, int(p.seed) >> 32]
        self.c3 = (K_PUSHPULL << 24) | (int(p.trial) & 0xFFFFFF)
        self.kd = oracle.threshold(p.drop_rate)
        self.deg, self.ids = np.asarray(deg).astype(np.int64), np.asarray(ids)
        self.dead = np.zeros(self.n, bool) if failed is None else np.asarray(failed, bool)
        self.R = len(senders)
        assert 1 <= self.R <= 64
        self.senders = []
        for j, s in enumerate(senders):
            if s < 0:   # rumor j's keyed sender: uniform(Philox{j, 0, 0, SENDER}.x, n)
                r = oracle.philox([j, 0, 0, (K_SENDER << 24) | (int(p.trial) & 0xFFFFFF)], self.key)
                s = (r[0] * self.n) >> 32
            self.senders.append(int(s))
        self.have = np.zeros(self.n, np.uint64)
        self._counted = None
        self.started = [not self.dead[s] for s in self.senders]
        for j, s in enumerate(self.senders):
            if self.started[j]:
                self.have[s] |= np.uint64(1 << j)
        self.live = sum(1 << j for j in range(self.R) if self.started[j])
        self.tick_99 = [0] * self.R   # per rumor: the first poll at which its rule held
        self.set_tick_99 = 0          # the first poll with no started rumor uncovered
        self.last = (np.zeros(0, np.int64),) * 2

    @property
    def counts(self):
        if self._counted is not self.have:   # (step replaces have; nothing writes into it)
            self._counts, self._counted = bit_counts(self.have, self.R), self.have
        return self._counts

    received = property(lambda self: int(self.counts.sum()))
    holds_all = property(lambda self: (self.have == np.uint64(self.live)) if self.live else np.zeros(self.n, bool))

    @property
    def covered(self):
        """Per rumor: does float32(count) / float32(n) >= 0.99 hold?"""
        return [bool(self.oracle.covered(int(c), self.n)) for c in self.counts]

    @property
    def pending(self):
        return sum(1 for s, c in zip(self.started, self.covered) if s and not c)

    def column(self, j):
        return (self.have >> np.uint64(j)) & np.uint64(1) != 0

    def calls(self, v):
        r0, r1 = philox_np(v, self.t, 0, self.c3, self.key)
        u = self.ids[v, ((r0 * self.deg[v].astype(np.uint64)) >> U32).astype(np.int64)].astype(np.int64)
        kept = ((r1 * np.uint64(100)) >> U32).astype(np.int64) >= self.kd
        return u, kept

    def step(self):
        self.t += 1
        H = self.have.copy()
        v = np.nonzero(~self.dead & (self.deg > 0))[0]
        u, kept = self.calls(v)
        conn = kept & ~self.dead[u]
        cv, cu = v[conn], u[conn]
        self.last = (cv, cu)
        messages = int((H[cv] != 0).sum()) + int((H[cu] != 0).sum())
        nxt = H.copy()
        np.bitwise_or.at(nxt, cu, H[cv])
        if self.wrong != "no_pull":
            np.bitwise_or.at(nxt, cv, H[cu])
        assert not nxt[self.dead].any()   # no connection reaches a failed node
        self.have = nxt
        return [self.t, v.size, int(kept.sum()), messages, self.received, 0, self.pending]

    def poll(self):
        cov = self.covered
        for j in range(self.R):
            if self.started[j] and not self.tick_99[j] and cov[j]:
                self.tick_99[j] = self.t
        if self.live and not self.set_tick_99 and all(c for s, c in zip(self.started, cov) if s):
            self.set_tick_99 = self.t

    def run(self, rounds):
        return np.array([self.step() for _ in range(rounds)], dtype=np.uint64).reshape(rounds, 7)


def reference_run(e, poll, max_ticks):
    """gs_run's rule on the restatement e (just begun): polls every `poll`
    rounds; stops at the first poll with no started rumor uncovered (quiescent
    if none started), or at max_ticks.  Returns the status (GS_RUN_*) and the
    polls' rows (the sums of their ticks' counters, the last tick's cumulative fields)."""
    rows = []
    while True:
        chunk = e.run(poll)
        e.poll()
        rows.append([int(chunk[-1, 0])] + [int(chunk[:, c].sum()) for c in (1, 2, 3)] + [int(x) for x in chunk[-1, 4:]])
        if not e.live:
            return 1, rows
        if e.pending == 0:
            return 0, rows
        if e.t >= max_ticks:
            return 2, rows


# ---- (a) hand-derived answers ---------------------------------------------------

def six(oracle, drop=0.0, wrong=None):
    """Six nodes with one friend each, so every callee is fixed: 0 -> 1, 1 -> 2,
    2 -> 2 (itself), 3 -> 4, 4 -> 5, 5 -> 0; node 5 is failed.  Rumor 0 starts at
    node 0, rumor 1 at node 1, rumor 2 at node 5: it is dead."""
    deg = np.ones(6, np.uint8)
    ids = np.array([[1], [2], [2], [4], [5], [0]], np.uint32)
    p = oracle.make_params(**dict(RS, n=6, fanout=1, fanin=1, drop_rate=drop))
    return PyRumorSet(oracle, p, deg, ids, [0, 1, 5], np.arange(6) == 5, wrong)


def test_six_nodes_by_hand(oracle):
    """Begin: have = [1, 2, 0, 0, 0, 0]; rumor 2's sender is failed, so it never
    starts: two pairs received, two started rumors pending (99 % of 6 nodes is
    all 6, and node 5 can hold nothing, so neither is ever covered).

    Round 1, no loss.  Callers 0..4 (5 is failed): fired = sent = 5.  The
    connections: 0-1 (both ends hold a rumor: 2 messages; two rumors meet on
    one connection: node 0 gets rumor 1 and node 1 gets rumor 0), 1-2 (1
    message; node 2 gets rumor 1 -- what node 1 held at the START of the round,
    not the rumor 0 it is receiving), 2-2 (a self-call: a connection that changes
    nothing, 0 messages while node 2 holds nothing), 3-4 (0 messages), 4-5 (a
    failed callee: sent, no connection).  messages = 3, have = [3, 3, 2, 0, 0, 0],
    received = 5.

    Round 2: 0-1 (2 messages, nothing new), 1-2 (2; node 2 gets rumor 0), 2-2
    (both ends hold: 2), 3-4 (0): messages = 6, have = [3, 3, 3, 0, 0, 0],
    received = 6.  Round 3 changes nothing: nobody who holds a rumor is connected
    to node 3 or 4."""
    e = six(oracle)
    assert e.senders == [0, 1, 5] and e.started == [True, True, False] and e.live == 3
    assert (e.have.tolist(), e.received, e.pending) == ([1, 2, 0, 0, 0, 0], 2, 2)
    assert e.step() == [1, 5, 5, 3, 5, 0, 2] and e.have.tolist() == [3, 3, 2, 0, 0, 0]
    assert e.step() == [2, 5, 5, 6, 6, 0, 2] and e.have.tolist() == [3, 3, 3, 0, 0, 0]
    assert e.step() == [3, 5, 5, 6, 6, 0, 2] and e.have.tolist() == [3, 3, 3, 0, 0, 0]
    assert e.counts.tolist() == [3, 3, 0] and not e.column(2).any()
    assert e.holds_all.tolist() == [True, True, True, False, False, False]
    e.poll()
    assert e.tick_99 == [0, 0, 0] and e.set_tick_99 == 0


def test_every_call_lost(oracle):
    # droprate 1: int(1.0 * 100) = 100 > every U_100: fired, never sent; nothing ever moves
    e = six(oracle, drop=1.0)
    assert [e.step() for _ in range(3)] == [[t, 5, 0, 0, 2, 0, 2] for t in (1, 2, 3)]
    assert e.have.tolist() == [1, 2, 0, 0, 0, 0]


def test_one_lost_call_among_kept_ones(oracle):
    """droprate 0.5 on the six nodes: the restatement's lost calls are the ones
    whose own draw says so (U_100(Philox{v, t, 0, PUSHPULL}.y) < 50), and a lost
    call moves nothing in either direction."""
    e = six(oracle, drop=0.5)
    for _ in range(6):
        H = e.have.copy()
        row = e.step()
        lost = [v for v in range(5)
                if (oracle.philox([v, e.t, 0, (K_PUSHPULL << 24)], e.key)[1] * 100) >> 32 < 50]
        assert row[1] == 5 and row[2] == 5 - len(lost)
        want = H.copy()
        for v, u in ((0, 1), (1, 2), (3, 4)):   # (2-2 changes nothing, 4-5 never connects)
            if v not in lost:
                want[u] |= H[v]
                want[v] |= H[u]
        assert e.have.tolist() == want.tolist()


def test_duplicate_senders_and_all_dead(oracle):
    deg = np.ones(3, np.uint8)
    ids = np.array([[1], [2], [0]], np.uint32)
    p = oracle.make_params(**dict(RS, n=3, fanout=1, fanin=1, drop_rate=0.0))
    e = PyRumorSet(oracle, p, deg, ids, [1, 1])   # two rumors may share a sender
    assert e.have.tolist() == [0, 3, 0] and e.holds_all.tolist() == [False, True, False]
    # round 1: 0-1 (node 0 pulls both), 1-2 (node 2 is pushed both), 2-0 (nothing yet): all covered
    assert e.step() == [1, 3, 3, 2, 6, 0, 0] and e.have.tolist() == [3, 3, 3]
    st, rows = reference_run(PyRumorSet(oracle, p, deg, ids, [1, 1]), 10, 100)
    assert st == 0 and len(rows) == 1 and rows[0][0] == 10
    # every sender failed: nothing starts, and the first poll is quiescent
    e = PyRumorSet(oracle, p, deg, ids, [0, 2], np.array([True, False, True]))
    assert e.live == 0 and not e.holds_all.any()
    st, rows = reference_run(e, 10, 100)
    assert st == 1 and len(rows) == 1 and rows[0] == [10, 10, 10, 0, 0, 0, 0] and e.set_tick_99 == 0


def test_keyed_senders(oracle):
    p = oracle.make_params(**dict(RS, n=1000))
    deg, ids = random_table(1000, 6, 1, 6, seed=1)
    e = PyRumorSet(oracle, p, deg, ids, [-1] * 5)
    assert e.senders[0] == oracle.pick_sender(p)   # rumor 0's keyed sender is keyed_sender()'s
    assert len(set(e.senders)) > 1 and all(0 <= s < 1000 for s in e.senders)


# ---- (b) the oracle, (c) non-vacuity ------------------------------------------------

def oracle_columns(oracle, p, deg, ids, senders, rounds, failed):
    """Per sender the oracle's push-pull informed sets after rounds 0..rounds."""
    out = []
    for s in senders:
        e = oracle.Engine(p, deg, ids)
        if failed is not None:
            e.set_failed(words_of(failed))
        e.begin(int(s))
        sets = [e.received().copy()]
        for _ in range(rounds):
            e.step(1)
            sets.append(e.received().copy())
        out.append(sets)
    return out


@pytest.mark.parametrize("n", [100, 1000])
@pytest.mark.parametrize("mask", [False, True])
def test_columns_are_the_oracles_pushpull(oracle, n, mask):
    """R = 1 and every column of an R = 5 run equal the oracle's push-pull from
    that sender after every round; the restatement without the pull direction
    does not."""
    rounds = 25
    deg, ids = random_table(n, 6, 0, 6, seed=n + 1)
    p = oracle.make_params(**dict(RS, n=n))
    failed = (np.random.default_rng(n).random(n) < 0.05) if mask else None
    senders = [int(x) for x in np.random.default_rng(7).integers(0, n, size=5)]
    if mask:
        senders[3] = int(np.nonzero(failed)[0][0])   # a dead rumor among live ones
    ref = oracle_columns(oracle, p, deg, ids, senders, rounds, failed)
    runs = [PyRumorSet(oracle, p, deg, masked(deg, ids), senders, failed),
            PyRumorSet(oracle, p, deg, masked(deg, ids), senders[:1], failed)]
    bad = PyRumorSet(oracle, p, deg, masked(deg, ids), senders, failed, wrong="no_pull")
    differs = False
    for t in range(rounds + 1):
        for e in runs:
            for j in range(e.R):
                assert np.array_equal(words_of(e.column(j)), ref[j][t]), (e.R, j, t)
        differs |= any(not np.array_equal(words_of(bad.column(j)), ref[j][t]) for j in range(5))
        for e in runs + [bad]:
            e.step()
    assert differs
    assert runs[0].counts.max() > n // 2


# ---- the ABI, with no device ----------------------------------------------------------

BASE = dict(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1)


def test_create_refusals_come_before_the_device():
    """GS_EINVAL with the field in the reason, with or without a GPU."""
    from gossip_simulator_amd import _lib
    L = _lib.load()
    assert L.gs_version() == 6 and C.sizeof(_lib.RumorStats) == 32 and C.sizeof(_lib.Params) == 112
    h = C.c_void_p()
    cases = [(dict(model=0), 4, "model"), (dict(model=2, rumor_k=2), 4, "model"), (dict(model=3, rumor_k=2), 4, "model"),
             (dict(model=4), 4, "model"),   # model 4 is still no model
             (dict(model=1), 0, "rumors"), (dict(model=1), 65, "rumors"), (dict(model=1, trials=2), 4, "trials"),
             (dict(model=1, flags=2), 4, "flags"), (dict(model=1, flags=1 | 8), 4, "flags"),
             (dict(model=1, flags=128), 4, "flags")]
    for kw, rumors, word in cases:
        p = _lib.Params(**dict(BASE, **kw))
        assert L.gs_create_rumorset(C.byref(p), rumors, C.byref(h)) == _lib.GS_EINVAL and not h.value, kw
        assert word in L.gs_last_error(None).decode(), (kw, L.gs_last_error(None).decode())
    # the checks every create makes still run
    p = _lib.Params(**dict(BASE, model=1, n=0))
    assert L.gs_create_rumorset(C.byref(p), 4, C.byref(h)) == _lib.GS_EINVAL
    # valid sets get past the parameter checks
    for rumors, flags in ((1, 0), (64, 1)):
        p = _lib.Params(**dict(BASE, model=1, flags=flags, rumor_k=9, rumor_mode=8))   # rumor_* are unused
        rc = L.gs_create_rumorset(C.byref(p), rumors, C.byref(h))
        assert rc in (_lib.GS_OK, _lib.GS_EDEVICE)
        if rc == _lib.GS_OK:
            L.gs_destroy(h)
    # the other creates keep their answers: push-pull with flags is theirs to take
    p = _lib.Params(**dict(BASE, model=1, flags=8))
    rc = L.gs_create(C.byref(p), C.byref(h))
    assert rc in (_lib.GS_OK, _lib.GS_EDEVICE)
    if rc == _lib.GS_OK:
        L.gs_destroy(h)


def test_cli_rumors_usage_errors():
    """-rumors is legal only with -model pushpull, 1..64, one trial on one device:
    anything else is a usage error before the parameter echo and any device call."""
    for args, word in ((("-rumors", "4"), "needs -model pushpull"),
                       (("-model", "flood", "-rumors", "4"), "needs -model pushpull"),
                       (("-model", "rumor", "-rumors", "4"), "needs -model pushpull"),
                       (("-model", "median", "-rumors", "4"), "needs -model pushpull"),
                       (("-model", "pushpull", "-rumors", "0"), "1..64"),
                       (("-model", "pushpull", "-rumors", "65"), "1..64"),
                       (("-model", "pushpull", "-rumors", "-2"), "1..64"),
                       (("-model", "pushpull", "-rumors", "4", "-trials", "2"), "one trial on one device"),
                       (("-model", "pushpull", "-rumors", "4", "-gpus", "2"), "one trial on one device")):
        r = cli("-n", "1000", *args)
        assert r.returncode == 2 and word in r.stderr and "-rumors" in r.stderr, (args, r.stderr)
        assert r.stdout == ""   # not even the parameter echo
    r = cli("-model", "pushpull", "-rumors", "x")
    assert r.returncode == 2 and 'invalid value "x" for flag -rumors' in r.stderr
    r = cli("-h")
    assert r.returncode == 0 and re.search(r"^  -rumors int$", r.stderr, re.M) and "gs_create_rumorset" in r.stderr
    # a valid command line gets to the create (no device here: exit 1 after the parameter echo)
    r = cli("-n", "1000", "-model", "pushpull", "-rumors", "64")
    assert r.returncode == 1 and "=== Parameters ===" in r.stdout and "gs_create failed" in r.stderr
    # without the flag nothing changes: the same echo, and the create of old
    a, b = cli("-n", "1000", "-model", "pushpull"), cli("-n", "1000", "-model", "pushpull", "-rumors", "3")
    assert a.stdout == b.stdout and "rumors" not in a.stdout


def test_lists_of_names():
    def read(*p):
        with open(os.path.join(ROOT, *p)) as f:
            return f.read()
    from gossip_simulator_amd import _lib
    import gossip_simulator_amd as gs
    hdr, integ = read("include", "gossip.h"), read("INTEGRATION.md")
    L = _lib.load()
    for name in ("gs_create_rumorset", "gs_rumorset_begin", "gs_rumorset_results", "gs_read_rumorset",
                 "gs_read_rumor_column"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert name in integ, name
    assert re.search(r"#define GS_RUMORSET_MAX 64u\b", hdr) and _lib.GS_RUMORSET_MAX == 64
    assert "typedef struct gs_rumor_stats" in hdr and "#define GS_ABI_VERSION 6" in hdr
    for name in ("rumor_set", "begin_rumors", "rumor_results", "rumor_words", "rumor_column"):
        assert hasattr(gs.Simulator, name), name
    assert "gs_rumorset.hip" in gs.__doc__
