"""Shard parity sweep: shard counts, range edges, window paths and switches of
the node-range shard layer (gs_shards.cpp, gs_win_shard.hip, the grouped
launches of gs_win_*.hip, pp_shard_step and the sharded push-pull round).

All shards are in-process on device 0 (Simulator(cfg, devices=[0] * G)).
Every GPU case is bit-exact against oracle.Engine: every stats row of every
step call, the received bitset's SHA-256 after every call, the crashed bitset
at the end, and all of it again in a second broadcast after reset() (which
runs on the buffers the first one grew).  sim.shard_info() equals
shard_ranges() in every case.  The case lists are module data shared with CPU
tests that run each case through the oracle and numpy alone and assert that
it is worth running.  The case families:

0. the split restated (shard_ranges) and pinned by hand-derived rows; refused
   n answer GS_EINVAL naming n and G, and n + 1 runs (a case of A);
A. G = 1..9, 12, 16, 17, 32 with last shards of 1, 63, 64, 65, 16383 and
   16384 nodes; a 1-node shard beside 32768-node shards; 256 shards refused;
B. ranges of more than one 2^22-node chunk (G = 1 and G = 2);
C. window lengths, rings, step calls of 1 / 7 / 10 ticks and gs_run polls of
   1 / 3 / 10 at G = 3; what shards refuse (ring 257, 33 slots, tick engine);
D. the five window paths (device-driven grouped, GS_SYNC_WINDOWS,
   GS_SHARD_SERIAL, the timing flag, GS_DD_GROUP=0 in a child process);
E. traffic patterns at G = 4: a shard nobody sends to, one only shard 0
   sends to, one that never fires, one failed as a whole, a hub on the last
   node, senders on range edges, a failed sender;
F. push-pull shards: G x tail x stride x mask x GS_PP_NO_REPLICA x
   GS_PP_SHARD_BOTTOM (a pairwise selection), per round and through gs_run;
   the three round kinds; a shard that only pulls;
G. shards that build their own overlay.
"""
from __future__ import annotations

import itertools
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from test_flood_shapes import cfg_of, frozen, oracle_overlay, popcount
from test_gpu_parity import random_table, sha
from test_pushpull import PP, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shard_shapes_worker.py")
FINE = 16384      # kFineNodes: shards are whole fine buckets
CHUNK = 1 << 22   # a coarse bin's nodes (kCoarseShift)
GS_EINVAL = -1


# ---- 0. the split -------------------------------------------------------------------
def shard_ranges(n, G):
    """[(lo, hi)] of the G shards of n nodes, or None where the split is refused."""
    seg = (-(-n // G) + FINE - 1) // FINE * FINE
    if (G - 1) * seg >= n:
        return None
    return [(r * seg, min((r + 1) * seg, n)) for r in range(G)]


REFUSED = [(65536, 3), (FINE, 2), (7 * FINE, 8)]  # (n, G): refused; n + 1 is a case of A


def owners(n, G):
    """The shard of every node."""
    own = np.zeros(n, np.int64)
    for r, (lo, hi) in enumerate(shard_ranges(n, G)):
        own[lo:hi] = r
    return own


def bits_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- the cases ------------------------------------------------------------------------
FLOOD = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.03, seed=11, trial=0)
Case = namedtuple("Case", "kw G deg ids failed sender second chunk")
# (failed: mask words or None; second: the sender after reset(); chunk: ticks per step call)

# A. shard counts and last-shard edges
A_GS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 32]  # (the issue allows 24 for 32: 32 fits the budget)
A_TAILS = [65, 16383, 16384, 1, 63, 64]
A_CASES = [((G - 1) * FINE + A_TAILS[i % len(A_TAILS)], G) for i, G in enumerate(A_GS)] + \
          [(81921, 3), (65537, 3), (FINE + 1, 2), (7 * FINE + 1, 8)]
# table seeds chosen on the CPU (default 1): the flood spreads; a 1-node shard's row names the other shards
A_SEEDS = {(3 * FINE, 3): 2, (3 * FINE + 1, 4): 6, (7 * FINE + 1, 8): 224}
A_TOO_MANY = (255 * FINE + 1, 256)


def a_table(n, G):
    deg, ids = random_table(n, 6, 1, 6, seed=A_SEEDS.get((n, G), 1) * 1000 + G)
    deg[::97] = 0
    return deg, ids


def build_a(n, G):
    deg, ids = a_table(n, G)
    return Case(dict(FLOOD, n=n), G, deg, ids, None, -1, -1, 10)


# B. ranges of more than one chunk
B_KW = dict(fanout=1, fanin=2, delay_low=3, delay_high=8, drop_rate=0.0, crash_rate=0.01, seed=11, trial=0)
B_CASES = [(CHUNK + FINE + 77, 1), (2 * CHUNK + 77, 2)]
B_CHUNK = 8


def build_b(n, G):
    deg, ids = random_table(n, 2, 1, 2, seed=n % 1000)
    return Case(dict(B_KW, n=n), G, deg, ids, None, -1, -1, B_CHUNK)


# C. window lengths, rings and polls
C_G, C_N = 3, 2 * FINE + 65
C_DELAYS = [(1, 2), (2, 7), (3, 8), (5, 6), (9, 40), (10, 20), (16, 256)]
C_CHUNKS = [1, 7, 10]
C_CASES = [(dl, dh, chunk) for dl, dh in C_DELAYS for chunk in C_CHUNKS]
C_POLLS = [(dl, dh, poll) for dl, dh in ((10, 20), (4, 9)) for poll in (1, 3, 10)]
C_REFUSED = {"ring-257": dict(delay_low=200, delay_high=257), "33-slots": dict(fanout=32, fanin=33),
             "tick-engine": {}}


def c_kw(dl, dh):
    return dict(FLOOD, n=C_N, delay_low=dl, delay_high=dh)


def build_c(dl, dh, chunk):
    deg, ids = a_table(C_N, C_G)
    return Case(c_kw(dl, dh), C_G, deg, ids, None, -1, -1, chunk)


# D. the five window paths
D_CASES = [(2 * FINE + 65, 3), (4 * FINE + 1, 5)]
D_PATHS = ["default", "sync", "serial", "timing"]  # and GS_DD_GROUP=0, in the worker
D_ENV = {"sync": "GS_SYNC_WINDOWS", "serial": "GS_SHARD_SERIAL"}


def build_d(n, G):
    deg, ids = random_table(n, 6, 1, 6, seed=1050 + G)
    deg[::97] = 0
    return Case(dict(FLOOD, n=n), G, deg, ids, None, -1, -1, 10)


# E. traffic patterns
E_G, E_N = 4, 3 * FINE + 64
E_HUB_IN = 4000  # the hub's in-degree: below the 65535 receipts a node takes in one tick
E_PATTERNS = ["norecv", "only0", "nofire", "failed", "hub"]
E_SENDERS = {"first": (0, FINE), "last-of-0": (FINE - 1, E_N - 1), "first-of-1": (FINE, 0),
             "last": (E_N - 1, FINE - 1), "failed-sender": (2 * FINE + 7, 9)}
E_CASES = E_PATTERNS + list(E_SENDERS)


E_SEEDS = {"nofire": 4005, "failed": 4005}  # table seeds chosen on the CPU (default 4004)


def e_base(name):
    deg, ids = random_table(E_N, 6, 1, 6, seed=E_SEEDS.get(name, 4004))
    deg[5::97] = 0
    return deg, ids


def build_e(name):
    deg, ids = e_base(name)
    failed, sender, second = None, 6, E_N - 2
    in1 = (ids >= FINE) & (ids < 2 * FINE)
    if name == "norecv":  # no row points into shard 1
        ids[in1] += FINE
    elif name == "only0":  # only shard 0's rows point into shard 1
        in1[:FINE] = False
        ids[in1] += FINE
    elif name == "nofire":  # shard 2 only receives
        deg[2 * FINE:3 * FINE] = 0
    elif name == "failed":  # shard 2 failed as a whole
        b = np.zeros(E_N, bool)
        b[2 * FINE:3 * FINE] = True
        failed = words_of(b)
    elif name == "hub":
        rows = np.random.default_rng(7).choice(np.flatnonzero(deg[:E_N - 1] > 0), E_HUB_IN, replace=False)
        ids[ids == E_N - 1] = 3
        ids[rows, 0] = E_N - 1
    else:
        sender, second = E_SENDERS[name]
        if name == "failed-sender":
            b = np.random.default_rng(8).random(E_N) < 0.03
            b[sender], b[second] = True, False
            failed = words_of(b)
    return Case(dict(FLOOD, n=E_N), E_G, deg, ids, failed, sender, second, 10)


# F. push-pull shards: (G, tail, stride, mask, no replica, bottom-up only)
F_GS = [1, 2, 3, 5, 6, 7, 8, 9, 16]
F_TAILS = [1, 63, 64, 65]
F_STRIDES = [1, 6, 16]
F_MASK = 0.02
F_CAP = 60  # rounds, as test_pushpull_shapes


def f_valid(s, m):
    return not (s == 16 and m)  # push-pull shards take a failure mask with rows <= 8 slots (asserted below)


def f_pairwise():
    """One case per (G, tail); stride, mask and the two switches chosen greedily
    so that every value of every axis meets every value of every other axis."""
    rest = [c for c in itertools.product(F_STRIDES, (False, True), (False, True), (False, True)) if f_valid(c[0], c[1])]
    seen, out = set(), []

    def pairs(case):
        return {(i, j, case[i], case[j]) for i in range(6) for j in range(i + 1, 6)}

    for k, (g, t) in enumerate(itertools.product(F_GS, F_TAILS)):
        k = 7 * k % len(rest)  # ties go round the combinations
        best = max(rest[k:] + rest[:k], key=lambda r: len(pairs((g, t) + r) - seen))
        out.append((g, t) + best)
        seen |= pairs(out[-1])
    return out


F_CASES = f_pairwise()
F_UNREACHABLE = (3, 65, 6, False, False, False)  # its own table: no row points into shard 1
F_REFUSED_STRIDE = 17


def f_id(c):
    return "G%d-t%d-s%d" % c[:3] + "-m" * c[3] + "-norep" * c[4] + "-bottom" * c[5]


def f_named(kind):
    """The cases in which round kind `kind` must occur: more than one shard,
    rows that spread fast, and the switch that takes the kind away unset."""
    return [c for c in F_CASES if c[0] >= 2 and c[2] >= 6 and not (kind == "early" and c[4]) and
            not (kind == "answer" and c[5])]


FCase = namedtuple("FCase", "kw G deg ids failed bits sender")


def build_f(c, unreachable=False):
    G, tail, s, m = c[:4]
    n = (G - 1) * FINE + tail
    deg, ids = random_table(n, s, 1, s, seed=7000 + 10 * G + tail + s)
    bits = None
    if m:
        bits = np.random.default_rng(7100 + G + tail).random(n) < F_MASK
        bits[n - 1] = False  # the last shard's last node stays live (a 1-node shard stays worth running)
    if unreachable:
        in1 = (ids >= FINE) & (ids < 2 * FINE)
        ids[in1] -= FINE
    # rows of one slot spread along one path: the run starts on the last node, so the last shard is informed
    sender = n - 1 if s == 1 else int(np.flatnonzero((deg > 0) & (True if bits is None else ~bits))[n // 3])
    kw = dict(PP, n=n, fanout=max(1, s - 1), fanin=s)
    return FCase(kw, G, deg, ids, words_of(bits) if m else None, bits, sender)


# G. shards that build their own overlay
G_CASES = [(5, 18, 19, 4 * FINE + 65), (2, 3, 4, FINE + 1)]


def g_kw(fo, fi, n):
    return dict(n=n, fanout=fo, fanin=fi, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.01, seed=5, trial=1)


# ---- the oracle's side, once per case ---------------------------------------------------
_CASES, _REFS = {}, {}
Ref = namedtuple("Ref", "rows hashes crashed received")
BUILDERS = {"A": build_a, "B": build_b, "C": build_c, "D": build_d, "E": build_e}


def case_of(family, *args):
    key = (family,) + args
    if key not in _CASES:
        c = BUILDERS[family](*args)
        frozen(*[a for a in (c.deg, c.ids, c.failed) if a is not None])
        _CASES[key] = c
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def tables_freed():
    """Nothing of this module's tables stays behind for the rest of the suite."""
    yield
    _CASES.clear()
    _REFS.clear()


def reference(oracle, key, c, sender, cap=8000):
    """The oracle's broadcast of case c from `sender`, stepped as the GPU test
    steps: per call the rows and the received bitset's hash; the crashed hash
    and the received bitset at the end."""
    key = key + (sender,)
    if key not in _REFS:
        e = oracle.Engine(oracle.make_params(**c.kw), c.deg, c.ids)
        if c.failed is not None:
            e.set_failed(c.failed)
        e.begin(sender)
        rows, hashes = [], []
        for _ in range(0, cap, c.chunk):
            rows.append(e.step(c.chunk))
            hashes.append(sha(e.received()))
            if int(rows[-1][-1][6]) == 0:
                break
        else:
            raise AssertionError(f"{key}: still pending after {cap} ticks")
        _REFS[key] = Ref(rows, hashes, sha(e.crashed()), frozen(e.received())[0])
        _REFS[key + ("crashed",)] = popcount(e.crashed())
    return _REFS[key]


def reachable(c, sender):
    """The nodes a flood from `sender` could inform with no drop and no crash:
    the sender's descendants over live nodes (the sender itself by an echo only)."""
    n = c.kw["n"]
    live = np.ones(n, bool) if c.failed is None else ~bits_of(c.failed, n)
    seen = np.zeros(n, bool)
    if not live[sender]:
        return seen
    front = np.array([sender])
    slots = np.arange(c.ids.shape[1])[None, :]
    while front.size:
        t = c.ids[front][slots < c.deg[front][:, None]]
        t = np.unique(t[live[t] & ~seen[t]])
        seen[t] = True
        front = t
    return seen


def edge_matrix(c):
    """[G, G]: table edges from shard a's nodes into shard b's range."""
    n, G = c.kw["n"], c.G
    own = owners(n, G)
    valid = np.arange(c.ids.shape[1])[None, :] < c.deg[:, None]
    src = np.broadcast_to(own[:, None], c.ids.shape)[valid]
    return np.bincount(src * G + own[c.ids[valid]], minlength=G * G).reshape(G, G)


def flood_is_worth_running(oracle, key, c, skip_shards=(), skip_pairs=(), second=False):
    """The conditions every flood case meets: the broadcast (the one after
    reset() with second=True) informs 90 % of the nodes its sender can reach
    and crashes a node; every shard but skip_shards ends with an informed node;
    every ordered pair of those shards but skip_pairs carries a table edge (past
    9 shards: every shard has an edge from and an edge to another shard)."""
    n, G = c.kw["n"], c.G
    asked = c.second if second else c.sender
    sender = asked if asked >= 0 else oracle.pick_sender(oracle.make_params(**c.kw))
    ref = reference(oracle, key, c, asked)
    got = bits_of(ref.received, n)
    reach = reachable(c, sender)
    assert int(reach.sum()) > 1, key
    assert int((got & reach).sum()) >= 0.9 * int(reach.sum()), (key, int(got.sum()), int(reach.sum()))
    if c.kw["crash_rate"] > 0:
        assert _REFS[key + (asked, "crashed")] > (popcount(c.failed) if c.failed is not None else 0), key
    ranges = shard_ranges(n, G)
    assert ranges is not None and ranges[-1][1] == n and len(ranges) == G, key
    for r, (lo, hi) in enumerate(ranges):
        assert (r in skip_shards) != bool(got[lo:hi].any()), (key, r)
    m = edge_matrix(c)
    if G <= 9:
        slots = c.ids.shape[1]
        for a, b in itertools.permutations([r for r in range(G) if r not in skip_shards], 2):
            one = [r for r in (a, b) if ranges[r][1] - ranges[r][0] == 1]
            if one and G - 1 > slots:
                # a 1-node shard with fewer slots than there are other shards: its row is full and
                # names as many other shards as it has slots; its in-degree is Poisson(3.5), so an edge
                # from each of 7 shards is beyond a seed search: an edge from another shard, as past G = 9
                r = one[0]
                assert int((np.delete(m[r], r) > 0).sum()) == slots == int(c.deg[ranges[r][0]]), (key, r)
                assert int(np.delete(m[:, r], r).sum()) > 0, (key, r)
                continue
            assert (m[a, b] > 0) != ((a, b) in skip_pairs), (key, a, b)
    else:
        off = m - np.diag(np.diag(m))
        assert (off.sum(axis=0) > 0).all() and (off.sum(axis=1) > 0).all(), key
    return ref, m


# ---- CPU: the split, and the cases are worth running ------------------------------------
def test_shard_ranges_hand_derived():
    """0. The split by hand: seg = roundup(ceil(n / G), 16384)."""
    sizes = lambda n, G: [hi - lo for lo, hi in shard_ranges(n, G)]  # noqa: E731
    assert sizes(81921, 3) == [32768, 32768, 16385]   # ceil(81921 / 3) = 27307 -> 32768
    assert shard_ranges(65536, 3) is None             # ceil = 21846 -> 32768; 2 * 32768 >= 65536
    assert sizes(65537, 3) == [32768, 32768, 1]
    assert shard_ranges(65537, 3) == [(0, 32768), (32768, 65536), (65536, 65537)]
    for G in (2, 8):
        assert shard_ranges(FINE * (G - 1), G) is None
        assert sizes(FINE * (G - 1) + 1, G) == [FINE] * (G - 1) + [1]
    assert sizes(1, 1) == [1] and sizes(FINE, 1) == [FINE]
    for n, G in REFUSED:
        assert shard_ranges(n, G) is None and (n + 1, G) in A_CASES
    assert shard_ranges(*A_TOO_MANY) is not None  # refused for its 256 shards, not for its n


def test_a_cases_are_worth_running(oracle):
    """A: every G of the issue, every tail at two or more G, ragged last shards
    of 1 node beside 16384- and 32768-node shards; the conditions of
    flood_is_worth_running."""
    assert [G for _, G in A_CASES[:len(A_GS)]] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 32]
    tails = {}
    for n, G in A_CASES[:len(A_GS)]:
        tails.setdefault(n - (G - 1) * FINE, set()).add(G)
    assert sorted(tails) == [1, 63, 64, 65, 16383, 16384] and min(len(g) for g in tails.values()) >= 2
    for n, G in A_CASES:
        c = case_of("A", n, G)
        assert int(c.deg.max()) == 6 and (c.deg[::97] == 0).all()
        flood_is_worth_running(oracle, ("A", n, G), c)
    last = [shard_ranges(n, G)[-1] for n, G in A_CASES]
    assert sum(hi - lo == 1 for lo, hi in last) >= 5
    assert [hi - lo for lo, hi in shard_ranges(65537, 3)] == [32768, 32768, 1]


def chunk1_arrivals(oracle, c, calls):
    """Per step call of the oracle's run: the nodes first informed in chunk 1 of
    shard 0 (each took at least one message there)."""
    lo = CHUNK
    hi = min(shard_ranges(c.kw["n"], c.G)[0][1], 2 * CHUNK)
    e = oracle.Engine(oracle.make_params(**c.kw), c.deg, c.ids)
    e.begin(c.sender)
    out, prev = [], 0
    for _ in range(calls):
        e.step(c.chunk)
        now = int(bits_of(e.received(), c.kw["n"])[lo:hi].sum())
        out.append(now - prev)
        prev = now
    return out


def test_b_cases_are_worth_running(oracle):
    """B: shard 0 has two chunks in both cases (the second nearly empty at
    G = 1), and messages land in chunk 1 of shard 0."""
    for n, G in B_CASES:
        c = case_of("B", n, G)
        r = shard_ranges(n, G)
        assert r[0][1] - r[0][0] > CHUNK and (G == 1 or r[1][1] - r[1][0] <= CHUNK)
        ref, _ = flood_is_worth_running(oracle, ("B", n, G), c)
        got = chunk1_arrivals(oracle, c, len(ref.rows))
        assert max(got) > 0, (n, G)
    assert shard_ranges(*B_CASES[0])[0][1] - CHUNK == FINE + 77


def test_c_cases_are_worth_running(oracle):
    """C: every delay range at every step length; the rings wrap."""
    assert len(shard_ranges(C_N, C_G)) == 3 and shard_ranges(C_N, C_G)[-1] == (2 * FINE, 2 * FINE + 65)
    for dl, dh, chunk in C_CASES:
        c = case_of("C", dl, dh, chunk)
        ref, _ = flood_is_worth_running(oracle, ("C", dl, dh, chunk), c)
        assert len(ref.rows) * chunk > dh
    assert {min(dl, 10) for dl, _ in C_DELAYS} >= {1, 2, 3, 5, 9, 10} and max(dh for _, dh in C_DELAYS) == 256
    for dl, dh, _ in C_POLLS:
        rows, _ = oracle.run_to_coverage(oracle.make_params(**c_kw(dl, dh)), *a_table(C_N, C_G), poll=1)
        assert len(rows) > dh


def test_d_cases_are_worth_running(oracle):
    """D: ragged tails of 65 and 1."""
    assert [shard_ranges(n, G)[-1][1] - shard_ranges(n, G)[-1][0] for n, G in D_CASES] == [65, 1]
    for n, G in D_CASES:
        flood_is_worth_running(oracle, ("D", n, G), case_of("D", n, G))


def test_e_cases_are_worth_running(oracle):
    """E: each pattern's defining property, on the table."""
    assert shard_ranges(E_N, E_G) == [(0, FINE), (FINE, 2 * FINE), (2 * FINE, 3 * FINE), (3 * FINE, 3 * FINE + 64)]
    skip = {"norecv": ((1,), ()), "only0": ((), ((2, 1), (3, 1))), "nofire": ((), ((2, 0), (2, 1), (2, 3))),
            "failed": ((2,), ())}
    for name in E_CASES:
        c = case_of("E", name)
        shards, pairs = skip.get(name, ((), ()))
        # (a failed sender starts nothing: that case's conditions are its second broadcast's)
        ref = reference(oracle, ("E", name), c, c.sender)
        second, m = flood_is_worth_running(oracle, ("E", name), c, shards, pairs, second=True)
        if name != "failed-sender":
            flood_is_worth_running(oracle, ("E", name), c, shards, pairs)
        own = owners(E_N, E_G)
        assert own[c.second] != own[c.sender] and c.deg[c.second] > 0 and c.deg[c.sender] > 0
        if name == "norecv":
            assert m[:, 1].sum() == 0 and m[1].sum() > 0  # nothing in; its rows still point out
        elif name == "only0":
            assert m[0, 1] > 0 and m[1:, 1].sum() == 0
        elif name == "nofire":
            assert m[2].sum() == 0 and m[:, 2].sum() > 0
        elif name == "failed":
            b = bits_of(c.failed, E_N)
            assert b[2 * FINE:3 * FINE].all() and int(b.sum()) == FINE
        elif name == "hub":
            valid = np.arange(6)[None, :] < c.deg[:, None]
            assert int(((c.ids == E_N - 1) & valid).sum()) == E_HUB_IN < 65535
            assert bits_of(ref.received, E_N)[E_N - 1]
        elif name == "failed-sender":
            b = bits_of(c.failed, E_N)
            assert b[c.sender] and not b[c.second]
            assert popcount(ref.received) == 0 and len(ref.rows) == 1  # nothing starts
            assert popcount(second.received) >= 0.8 * E_N
    assert {s for s, _ in E_SENDERS.values()} >= {0, FINE - 1, FINE, E_N - 1}


def f_reference(oracle, c, unreachable=False):
    """The oracle's push-pull run of a case, a round per call: until 99 % are
    informed or a round informs nobody new and no later one can, at most F_CAP
    rounds.  (rows, hashes, informed per round start, the final informed set)"""
    key = ("F", c, unreachable)
    if key not in _REFS:
        d = build_f(c, unreachable)
        p = oracle.make_params(**d.kw)
        e = oracle.Engine(p, d.deg, d.ids)
        if d.failed is not None:
            e.set_failed(d.failed)
        e.begin(d.sender)
        rows, hashes, starts, prev = [], [], [], popcount(e.received())
        for _ in range(F_CAP):
            starts.append(prev)
            a = e.step(1)
            rows.append(a[0])
            hashes.append(sha(e.received()))
            recv = int(a[0, 4])
            if oracle.covered(recv, d.kw["n"]) or recv == 0:
                break
            if recv == prev and oracle.pp_stalled(p, d.deg, d.ids, e.received(), e.crashed()):
                break
            prev = recv
        _REFS[key] = (np.array(rows, dtype=np.uint64), hashes, starts, frozen(e.received())[0], d)
    return _REFS[key]


def test_f_cases_are_worth_running(oracle):
    """F: the selection is pairwise complete (but 16 slots with a mask, which
    shards refuse); every shard ends with an informed node; the named cases
    cross both mode thresholds."""
    axes = [F_GS, F_TAILS, F_STRIDES, (False, True), (False, True), (False, True)]
    for i, j in itertools.combinations(range(6), 2):
        want = {(a, b) for a in axes[i] for b in axes[j] if not ((i, j) == (2, 3) and not f_valid(a, b))}
        assert {(c[i], c[j]) for c in F_CASES} >= want, (i, j)
    assert all(f_valid(c[2], c[3]) for c in F_CASES) and len(F_CASES) == len(F_GS) * len(F_TAILS)
    for c in F_CASES + [F_UNREACHABLE]:
        unreachable = c is F_UNREACHABLE
        rows, _, starts, recv, d = f_reference(oracle, c, unreachable)
        n, G = d.kw["n"], d.G
        got = bits_of(recv, n)
        for r, (lo, hi) in enumerate(shard_ranges(n, G)):
            assert got[lo:hi].any(), (c, r)
        assert d.bits is None or (int(d.bits.sum()) >= n // 100 or n < 100)
        named = c in f_named("bottom")
        if named or unreachable:
            assert starts[0] <= n >> 8, c
            assert any(n >> 8 < s < (96 * n) >> 8 for s in starts), (c, starts)
            assert any(s >= (96 * n) >> 8 for s in starts), (c, starts)
    for kind in ("early", "answer", "bottom"):
        assert len(f_named(kind)) >= 1
    d = build_f(F_UNREACHABLE, True)
    m = edge_matrix(Case(d.kw, d.G, d.deg, d.ids, None, d.sender, None, 1))
    assert m[:, 1].sum() == 0 and m[1, 0] > 0 and m[1, 2] > 0  # nothing points in; its rows point out
    assert not (FINE <= d.sender < 2 * FINE)


# ---- the GPU's side -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def broadcast(sim, ref, chunk, sender):
    """One broadcast on sim against the oracle's: every row of every step call,
    the received bitset after every call, the crashed bitset at the end."""
    sim.broadcast_begin(sender)
    for i, (want, h) in enumerate(zip(ref.rows, ref.hashes)):
        got = sim.step(chunk)
        assert np.array_equal(got, want), f"stats differ in step call {i} ({chunk} ticks):\n{want}\n{got}"
        assert sha(sim.received()) == h, f"received differs after step call {i} ({chunk} ticks)"
    assert sha(sim.crashed()) == ref.crashed, "crashed differs"


def shards_of(gs, c, **extra):
    """A sharded context of case c with its table and mask; shard_info() is the restated split."""
    sim = gs.Simulator(cfg_of(gs, c.kw, **extra), devices=[0] * c.G)
    try:
        assert sim.shard_info() == shard_ranges(c.kw["n"], c.G)
        sim.load_peers(c.deg, c.ids)
        if c.failed is not None:
            sim.set_failed(c.failed)
    except BaseException:
        sim.close()
        raise
    return sim


def twice(gs, oracle, key, c, **extra):
    """Case c: a broadcast, reset(), a second broadcast (from c.second) on the grown buffers."""
    with shards_of(gs, c, **extra) as sim:
        broadcast(sim, reference(oracle, key, c, c.sender), c.chunk, c.sender)
        fb = sim.timing()["dd_fallbacks"]
        sim.reset()
        broadcast(sim, reference(oracle, key, c, c.second), c.chunk, c.second)
        return fb, sim.timing()


def refused(gs, cfg, G, *words):
    with pytest.raises(gs.GossipError) as e:
        gs.Simulator(cfg, devices=[0] * G).close()
    assert e.value.code == GS_EINVAL, e.value
    for w in words:
        assert w in str(e.value), e.value


@pytest.mark.gpu
@pytest.mark.parametrize("n,G", REFUSED + [A_TOO_MANY], ids=lambda v: str(v))
def test_refused_splits(gs, n, G):
    """0 / A. (G - 1) * seg >= n is refused with n and G in the message (n + 1
    runs: test_shard_counts_and_tails); 256 shards are refused at an n that 255
    would take."""
    if (n, G) == A_TOO_MANY:
        refused(gs, cfg_of(gs, dict(FLOOD, n=n)), G, "G <= 255")
    else:
        refused(gs, cfg_of(gs, dict(FLOOD, n=n)), G, f"n = {n} ", f"{G} shards")


@pytest.mark.gpu
@pytest.mark.parametrize("n,G", A_CASES, ids=[f"G{g}-n{n}" for n, g in A_CASES])
def test_shard_counts_and_tails(gs, oracle, n, G):
    """A. Every shard count with a ragged last shard: unused bins where G does
    not divide 256, more senders than sub-regions past G = 8, grouped grids
    sized by the largest shard over a last shard of one bucket."""
    twice(gs, oracle, ("A", n, G), case_of("A", n, G))


@pytest.mark.gpu
@pytest.mark.parametrize("n,G", B_CASES, ids=[f"G{g}-n{n}" for n, g in B_CASES])
def test_ranges_of_two_chunks(gs, oracle, n, G):
    """B. bin = owner * obins + k with k = 1: plan_coarse_owner's chunk loop
    and the receive layout's c < obins loop."""
    twice(gs, oracle, ("B", n, G), case_of("B", n, G))


@pytest.mark.gpu
@pytest.mark.parametrize("dl,dh,chunk", C_CASES, ids=[f"d{a}-{b}-step{c}" for a, b, c in C_CASES])
def test_window_lengths_and_rings_on_shards(gs, oracle, dl, dh, chunk):
    """C. Window lengths 1..10 cut again at the end of every step call, rings
    up to 256 slots."""
    twice(gs, oracle, ("C", dl, dh, chunk), case_of("C", dl, dh, chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("dl,dh,poll", C_POLLS, ids=[f"d{a}-{b}-poll{p}" for a, b, p in C_POLLS])
def test_run_polls_on_shards(gs, oracle, dl, dh, poll):
    """C. gs_run on shards (the poll rule on the device, k_close_dd): the
    unsharded context's polls and status, the oracle's bitsets; twice."""
    deg, ids = a_table(C_N, C_G)
    kw = c_kw(dl, dh)
    _, e = oracle.run_to_coverage(oracle.make_params(**kw), deg, ids, poll=poll)
    with gs.Simulator(cfg_of(gs, kw)) as one:
        one.load_peers(deg, ids)
        one.broadcast_begin(-1)
        want, status = one.run(poll=poll)
    with gs.Simulator(cfg_of(gs, kw), devices=[0] * C_G) as sim:
        assert sim.shard_info() == shard_ranges(C_N, C_G)
        sim.load_peers(deg, ids)
        for _ in range(2):
            sim.reset()
            sim.broadcast_begin(-1)
            got, st = sim.run(poll=poll)
            assert st == status and np.array_equal(got, want), f"\n{got}\n{want}"
            assert np.array_equal(sim.received(), e.received()) and np.array_equal(sim.crashed(), e.crashed())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C_REFUSED))
def test_what_shards_refuse(gs, name):
    """C. Shards run on the window engine only: a 257-slot ring, 33-slot rows
    and GS_FLAG_TICK_ENGINE answer GS_EINVAL."""
    kw = dict(FLOOD, n=C_N, **C_REFUSED[name])
    cfg = cfg_of(gs, kw, "tick" if name == "tick-engine" else "window")
    refused(gs, cfg, C_G, "node-range shards run on the window engine")


@pytest.mark.gpu
@pytest.mark.parametrize("path", D_PATHS)
@pytest.mark.parametrize("n,G", D_CASES, ids=[f"G{g}-n{n}" for n, g in D_CASES])
def test_window_paths(gs, oracle, monkeypatch, n, G, path):
    """D. The default (device-driven, grouped), GS_SYNC_WINDOWS, GS_SHARD_SERIAL
    and the timing flag.  dd_fallbacks counts device-driven windows that were
    stopped by an overflow and redone host-driven: the first broadcast meets
    empty message buffers, so it has some; the second, on the grown buffers,
    none; the three host-driven paths never start a device-driven window.  Only
    the timing flag counts `windows`."""
    for var in D_ENV.values():
        monkeypatch.delenv(var, raising=False)
    if path in D_ENV:
        monkeypatch.setenv(D_ENV[path], "1")
    fb, tm = twice(gs, oracle, ("D", n, G), case_of("D", n, G), timing=path == "timing")
    if path == "default":
        assert fb > 0 and tm["dd_fallbacks"] == fb, (fb, tm["dd_fallbacks"])
    else:
        assert fb == 0 and tm["dd_fallbacks"] == 0, (fb, tm["dd_fallbacks"])
    assert (tm["windows"] > 0) == (path == "timing"), tm["windows"]


@pytest.mark.gpu
@pytest.mark.parametrize("n,G", D_CASES, ids=[f"G{g}-n{n}" for n, g in D_CASES])
def test_one_launch_per_shard_in_a_fresh_process(oracle, n, G):
    """D. GS_DD_GROUP=0 (read once per process): device-driven windows with one
    launch per shard instead of the grouped launches, in a child process."""
    c = case_of("D", n, G)
    r = subprocess.run([sys.executable, WORKER, json.dumps(dict(n=n, G=G))], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["dd_group"] == "0"
    assert [tuple(x) for x in got["shard_info"]] == shard_ranges(n, G)
    ref = reference(oracle, ("D", n, G), c, c.sender)
    assert len(got["runs"]) == 2
    for run in got["runs"]:
        assert len(run["rows"]) == len(ref.rows)
        for i, (rows, h) in enumerate(zip(run["rows"], run["received_sha256"])):
            assert ref.rows[i].tolist() == rows, f"step call {i}:\n{ref.rows[i]}\n{rows}"
            assert ref.hashes[i] == h, f"step call {i}: received"
        assert run["crashed_sha256"] == ref.crashed
    fb = [run["dd_fallbacks"] for run in got["runs"]]
    assert fb[0] > 0 and fb[1] == fb[0], fb


@pytest.mark.gpu
@pytest.mark.parametrize("name", E_CASES)
def test_traffic_patterns(gs, oracle, name):
    """E. Shards that receive nothing, receive from one shard only, never fire
    or are failed as a whole; a hub on the last node of the ragged shard;
    senders on the first and last node of a range; a failed sender."""
    twice(gs, oracle, ("E", name), case_of("E", name))


def pp_cfg(gs, kw, **extra):
    return gs.Config(n=kw["n"], fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                     seed=kw["seed"], trial=kw["trial"], model="pushpull", **extra)


def pushpull_case(gs, oracle, monkeypatch, c, unreachable=False):
    G, _, s, m, norep, bottom = c
    for var, on in (("GS_PP_NO_REPLICA", norep), ("GS_PP_SHARD_BOTTOM", bottom)):
        monkeypatch.delenv(var, raising=False)
        if on:
            monkeypatch.setenv(var, "1")
    rows, hashes, _, _, d = f_reference(oracle, c, unreachable)
    n = d.kw["n"]
    crashed = sha(d.failed if d.failed is not None else np.zeros((n + 63) // 64, np.uint64))
    runs = {}
    with gs.Simulator(pp_cfg(gs, d.kw)) as one:  # the unsharded context's gs_run
        one.load_peers(d.deg, d.ids)
        if d.failed is not None:
            one.set_failed(d.failed)
        for poll in (1, 10):
            one.reset()
            one.broadcast_begin(d.sender)
            runs[poll] = one.run(poll=poll, max_ticks=F_CAP) + (sha(one.received()),)
    with gs.Simulator(pp_cfg(gs, d.kw), devices=[0] * G) as sim:
        assert sim.shard_info() == shard_ranges(n, G)
        sim.load_peers(d.deg, d.ids)
        if d.failed is not None:
            sim.set_failed(d.failed)
        for rep in range(2):  # the second broadcast after reset()
            sim.reset()
            sim.broadcast_begin(d.sender)
            for r, want in enumerate(rows):
                got = sim.step(1)
                assert np.array_equal(got[0], want), f"broadcast {rep} round {r + 1}:\n{want}\n{got[0]}"
                assert sha(sim.received()) == hashes[r], f"broadcast {rep}: informed set differs at round {r + 1}"
            assert sha(sim.crashed()) == crashed
            tm = sim.timing()
            kinds = {k: int(tm[f"pp_{k}_rounds"]) for k in ("early", "answer", "bottom")}
            assert sum(kinds.values()) == len(rows), kinds
            if norep:
                assert kinds["early"] == 0, kinds
            if bottom:
                assert kinds["answer"] == 0, kinds
            # (in the first broadcast too: pull-answer rounds were once chosen before a masked
            # shard's failed-slot mask existed, and only later broadcasts ran them)
            for kind in kinds:
                if c in f_named(kind) or unreachable:
                    assert kinds[kind] > 0, (kind, kinds)
        for poll in (1, 10):
            sim.reset()
            sim.broadcast_begin(d.sender)
            polls, status = sim.run(poll=poll, max_ticks=F_CAP)
            want, wstatus, wsha = runs[poll]
            assert status == wstatus and np.array_equal(polls, want), f"poll {poll}:\n{polls}\n{want}"
            assert sha(sim.received()) == wsha


@pytest.mark.gpu
@pytest.mark.parametrize("c", F_CASES, ids=[f_id(c) for c in F_CASES])
def test_pushpull_shards(gs, oracle, monkeypatch, c):
    """F. Push-pull shards per round against the oracle (twice), then gs_run
    with polls of 1 and 10 against the unsharded context; the round kinds sum
    to the rounds run, and each kind occurs in the cases named for it."""
    pushpull_case(gs, oracle, monkeypatch, c)


@pytest.mark.gpu
def test_pushpull_shard_that_only_pulls(gs, oracle, monkeypatch):
    """F. No row points into shard 1 and its own rows point out: its words of
    the replicated informed set start at zero and fill by its own pulls."""
    pushpull_case(gs, oracle, monkeypatch, F_UNREACHABLE, unreachable=True)


@pytest.mark.gpu
def test_pushpull_shards_refuse_wide_rows_and_wide_masks(gs):
    """F. 17-slot rows on shards, and a failure mask with rows past 8 slots."""
    n, G = 2 * FINE + 65, 3
    refused(gs, pp_cfg(gs, dict(PP, n=n, fanout=16, fanin=F_REFUSED_STRIDE)), G, "at most 16 slots")
    deg, ids = random_table(n, 16, 1, 16, seed=1)
    with gs.Simulator(pp_cfg(gs, dict(PP, n=n, fanout=15, fanin=16)), devices=[0] * G) as sim:
        sim.load_peers(deg, ids)
        with pytest.raises(gs.GossipError) as e:
            sim.set_failed(words_of(np.arange(n) % 50 == 0))
        assert e.value.code == GS_EINVAL and "rows <= 8 slots" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("G,fo,fi,n", G_CASES, ids=[f"G{g}-{a}-{b}" for g, a, b, _ in G_CASES])
def test_shards_build_their_overlay(gs, oracle, G, fo, fi, n):
    """G. The replicated build, each shard keeping its partition: windows and
    the final tick, then the flood over the oracle's overlay, twice."""
    kw = g_kw(fo, fi, n)
    deg, ids, wins, final = oracle_overlay(oracle, kw)
    c = Case(kw, G, deg, ids, None, -1, -1, 10)
    with gs.Simulator(cfg_of(gs, kw), devices=[0] * G) as sim:
        assert sim.shard_info() == shard_ranges(n, G)
        gw, gf = sim.build_overlay()
        assert gf == final and [tuple(w) for w in gw] == wins
        for _ in range(2):
            sim.reset()
            broadcast(sim, reference(oracle, ("G", G, fo, fi, n), c, -1), 10, -1)
