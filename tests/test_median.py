"""Median-counter push-pull (GS_MODEL_MEDIAN): no
reference semantics exist (simulator.go only floods), so the model is pinned
here by a pure-Python restatement written from the specification, itself
pinned by hand-derived answers; the HIP rounds (gs_median.hip) must match it
bit-exactly per round (tests/test_median_gpu.py).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from test_rumor import ROOT, cli, philox_np, words_of  # noqa: F401 (words_of: for the GPU tests)

K_MEDIAN = 12
D = 255
U32 = np.uint64(32)
MEDIAN = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.0,
              seed=0x5EED, trial=0, model=3)
COLS = [0, 1, 2, 3, 4, 6]  # tick, fired, sent, messages, received, pending


class PyMedian:
    """The specification, round by round.  State per node: the byte st (0 = A,
    m = B-m, k + c = C-c, 255 = D) and the failed bit.  Every decision of a
    round reads S, the states at its start.

    `wrong` restates a kernel mistake, for the non-vacuity tests only:
    "no_own" drops a caller's own end of its connection (only the callee's end
    is tallied), "c_as_b" counts a partner in C as one in B-k."""

    def __init__(self, oracle, p, deg, ids, sender, k, failed=None, wrong=None):
        self.n, self.k, self.t, self.wrong = int(p.n), int(k), 0, wrong
        self.key = [int(p.seed) & 0xFFFFFFFF, int(p.seed) >> 32]
        self.c3 = (K_MEDIAN << 24) | (int(p.trial) & 0xFFFFFF)
        self.kd = oracle.threshold(p.drop_rate)
        self.deg, self.ids = np.asarray(deg).astype(np.int64), np.asarray(ids)
        self.dead = np.zeros(self.n, bool) if failed is None else np.asarray(failed, bool)
        self.state = np.zeros(self.n, np.int64)
        self.last = (np.zeros(0, np.int64),) * 2  # the last round's connections: callers, callees
        if sender < 0:
            sender = int(oracle.pick_sender(p))
        if not self.dead[sender]:
            self.state[sender] = 1

    st = property(lambda self: self.state.astype(np.uint8))
    inf = property(lambda self: self.state != 0)
    removed = property(lambda self: self.state == D)
    act = property(lambda self: (self.state != 0) & (self.state != D))
    received = property(lambda self: int(self.inf.sum()))
    pending = property(lambda self: int(self.act.sum()))

    def calls(self, v):
        r0, r1 = philox_np(v, self.t, 0, self.c3, self.key)
        u = self.ids[v, ((r0 * self.deg[v].astype(np.uint64)) >> U32).astype(np.int64)].astype(np.int64)
        kept = ((r1 * np.uint64(100)) >> U32).astype(np.int64) >= self.kd
        return u, kept

    def step(self):
        self.t += 1
        n, k, S = self.n, self.k, self.state.copy()
        v = np.nonzero(~self.dead & (self.deg > 0) & (S != D))[0]
        u, kept = self.calls(v)
        conn = kept & ~self.dead[u]
        cv, cu = v[conn], u[conn]
        self.last = (cv, cu)
        active = (S != 0) & (S != D)
        messages = int(active[cv].sum()) + int(active[cu].sum())
        # each connection makes each end a partner of the other, once: x's partner is y
        x, y = (cu, cv) if self.wrong == "no_own" else (np.concatenate([cv, cu]), np.concatenate([cu, cv]))
        Sx, Sy = S[x], S[y]
        if self.wrong == "c_as_b":
            Sy = np.where((Sy > k) & (Sy != D), k, Sy)
        yB, yC, xB = (Sy >= 1) & (Sy <= k), (Sy > k) & (Sy != D), (Sx >= 1) & (Sx <= k)

        def count(sel):
            return np.bincount(x[sel], minlength=n)
        c, b = count(yC), count(yB)
        ge, lt = count(xB & yB & (Sy >= Sx)), count(xB & ((Sy == 0) | (yB & (Sy < Sx))))
        new = S.copy()
        A, B, Cs = S == 0, (S >= 1) & (S <= k), (S > k) & (S != D)
        new[A & (c == 0) & (b > 0)] = 1
        adv = B & (c == 0) & (ge > lt)
        new[adv] = np.where(S[adv] < k, S[adv] + 1, k + 1)
        new[(A | B) & (c > 0)] = k + 1
        new[Cs] = np.where(S[Cs] < 2 * k, S[Cs] + 1, D)
        assert not (new != S)[self.dead].any()  # no connection reaches a failed node
        self.state = new
        return [self.t, v.size, int(kept.sum()), messages, self.received, 0, self.pending]

    def run(self, rounds):
        return np.array([self.step() for _ in range(rounds)], dtype=np.uint64).reshape(rounds, 7)


def reference_run(oracle, e, poll, max_ticks):
    """gs_run's rule on the restatement e (just begun): polls every `poll` rounds;
    stops at the first poll with nobody active, or at max_ticks.  Returns the
    status (GS_RUN_*) and tick_99."""
    tick_99 = 0
    while True:
        for _ in range(poll):
            e.step()
        cov = oracle.covered(e.received, e.n)
        if cov and not tick_99:
            tick_99 = e.t
        if e.pending == 0:
            return (0 if cov else 1), tick_99
        if e.t >= max_ticks:
            return 2, tick_99


def trace(e, rounds):
    """[(row[COLS], st)] of `rounds` rounds."""
    out = []
    for _ in range(rounds):
        row = e.step()
        out.append(([row[i] for i in COLS], e.st.tolist()))
    return out


def pair(oracle, k, drop=0.0, failed=None, wrong=None):
    p = oracle.make_params(**dict(MEDIAN, n=2, drop_rate=drop))
    return PyMedian(oracle, p, np.array([1, 1], np.uint8), np.array([[1], [0]], np.uint32), 0, k, failed, wrong)


def test_two_nodes_k1(oracle):
    # round 1: S = [B-1, A]; both call, two connections, one active end each: messages = 2.  Node 0's two
    # partners are A: lt = 2, it stays; node 1 has two B partners: B-1.  round 2: each has two B-1
    # partners, ge = 2 > 0 and m == k: C-1 (st 2); four active ends.  round 3: C-1 is C-k: D.
    # round 4: D nodes do not call.
    e = pair(oracle, 1)
    assert (e.received, e.pending, e.st.tolist()) == (1, 1, [1, 0])
    assert trace(e, 4) == [([1, 2, 2, 2, 2, 2], [1, 1]), ([2, 2, 2, 4, 2, 2], [2, 2]),
                           ([3, 2, 2, 4, 2, 0], [D, D]), ([4, 0, 0, 0, 2, 0], [D, D])]
    assert e.removed.all()


def test_two_nodes_k2(oracle):
    # B-1, B-2, then C-1 (st 3), C-2 (st 4), D: a counter step and a final round more than k = 1
    e = pair(oracle, 2)
    assert trace(e, 6) == [([1, 2, 2, 2, 2, 2], [1, 1]), ([2, 2, 2, 4, 2, 2], [2, 2]), ([3, 2, 2, 4, 2, 2], [3, 3]),
                           ([4, 2, 2, 4, 2, 2], [4, 4]), ([5, 2, 2, 4, 2, 0], [D, D]), ([6, 0, 0, 0, 2, 0], [D, D])]


def test_sender_alone_calls_itself(oracle):
    # n = 1, its friend is itself: one connection, counted once for each end: two transmissions and two
    # B-1 partners (ge = 2): C-1, then D.
    p = oracle.make_params(**dict(MEDIAN, n=1, drop_rate=0.0))
    e = PyMedian(oracle, p, np.ones(1, np.uint8), np.zeros((1, 1), np.uint32), 0, 1)
    assert trace(e, 3) == [([1, 1, 1, 2, 1, 1], [2]), ([2, 1, 1, 2, 1, 0], [D]), ([3, 0, 0, 0, 1, 0], [D])]


def test_sender_with_an_empty_row_that_nobody_calls(oracle):
    # 1 and 2 call each other; nobody connects to the sender: B-1 for ever, GS_RUN_MAX_TICKS
    p = oracle.make_params(**dict(MEDIAN, n=3, drop_rate=0.0))
    deg, ids = np.array([0, 1, 1], np.uint8), np.array([[0], [2], [1]], np.uint32)
    e = PyMedian(oracle, p, deg, ids, 0, 2)
    assert trace(e, 30) == [([t, 2, 2, 0, 1, 1], [1, 0, 0]) for t in range(1, 31)]
    e = PyMedian(oracle, p, deg, ids, 0, 2)
    assert reference_run(oracle, e, 10, 50) == (2, 0) and e.t == 50


def test_failed_sender(oracle):
    e = pair(oracle, 2, failed=np.array([True, False]))
    assert (e.received, e.pending) == (0, 0)
    # node 1 calls the failed node 0: sent, no connection
    assert trace(e, 2) == [([1, 1, 1, 0, 0, 0], [0, 0]), ([2, 1, 1, 0, 0, 0], [0, 0])]
    e = pair(oracle, 2, failed=np.array([True, False]))
    assert reference_run(oracle, e, 10, 1000) == (1, 0) and e.t == 10   # the first poll is quiescent


def star(oracle, k, wrong=None, leaves=4):
    n = leaves + 1
    deg = np.ones(n, np.uint8)
    ids = np.zeros((n, leaves), np.uint32)
    deg[0] = leaves
    ids[0] = 1 + np.arange(leaves)
    p = oracle.make_params(**dict(MEDIAN, n=n, fanout=leaves, fanin=leaves, drop_rate=0.0))
    return PyMedian(oracle, p, deg, ids, 0, k, None, wrong)


def test_star_whose_hub_is_the_sender(oracle):
    # round 1: every leaf calls the hub and is informed by pull, whichever leaf the hub calls; the hub
    # has five A partners (four callers and its callee): lt = 5, it stays B-1.  messages = 1 + 4.
    # round 2: everybody is B-1: the hub has ge = 5, every leaf ge >= 1: B-2.  round 3: C-1 (st 3),
    # round 4: C-2, round 5: D.
    e = star(oracle, 2)
    assert trace(e, 6) == [([1, 5, 5, 5, 5, 5], [1] * 5), ([2, 5, 5, 10, 5, 5], [2] * 5),
                           ([3, 5, 5, 10, 5, 5], [3] * 5), ([4, 5, 5, 10, 5, 5], [4] * 5),
                           ([5, 5, 5, 10, 5, 0], [D] * 5), ([6, 0, 0, 0, 5, 0], [D] * 5)]


def set_state(e, st):
    e.state = np.asarray(st, np.int64)
    return e


def test_c_partner_turns_a_and_b_straight_to_c1(oracle):
    # k = 2, S = [C-1, A]: node 1's two partners are in C: C-1 (st 3), received += 1; node 0: C-2.
    e = set_state(pair(oracle, 2), [3, 0])
    assert trace(e, 1) == [([1, 2, 2, 2, 2, 2], [4, 3])]
    # S = [C-1, B-1]: c(1) > 0 wins over the counter: C-1, not B-2
    e = set_state(pair(oracle, 2), [3, 1])
    assert trace(e, 1) == [([1, 2, 2, 4, 2, 2], [4, 3])]


def test_d_partners_count_nowhere(oracle):
    # S = [D, B-1]: node 0 is silent and does not call; node 1 calls it: a connection with one active
    # end.  Its partner counts in none of c, b, ge, lt: ge = lt = 0, it stays B-1 for ever.
    e = set_state(pair(oracle, 2), [D, 1])
    assert trace(e, 3) == [([t, 1, 1, 1, 2, 1], [D, 1]) for t in (1, 2, 3)]
    # an A node that calls a D node learns nothing
    e = set_state(pair(oracle, 2), [D, 0])
    assert trace(e, 2) == [([t, 1, 1, 0, 1, 0], [D, 0]) for t in (1, 2)]


def test_droprate_1_never_ends(oracle):
    e = pair(oracle, 1, drop=1.0)
    assert trace(e, 30) == [([t, 2, 0, 0, 1, 1], [1, 0]) for t in range(1, 31)]


def test_the_sweep_can_catch_a_wrongly_merged_tally(oracle):
    """The two likeliest kernel mistakes give other states than the specified
    ones in the hub case and the C-partner case, so the GPU sweep
    (tests/test_median_gpu.py) tells them apart."""
    good, bad = star(oracle, 2), star(oracle, 2, wrong="no_own")
    good.run(2)
    bad.run(2)
    assert good.st[0] == 2 and bad.st[0] == 1   # the hub's own end made ge > lt: without it, it stays B-1
    assert good.st.tolist() != bad.st.tolist()
    good, bad = set_state(pair(oracle, 2), [3, 0]), set_state(pair(oracle, 2, wrong="c_as_b"), [3, 0])
    good.step()
    bad.step()
    assert good.st.tolist() == [4, 3] and bad.st.tolist() == [4, 1]


def random_rows(n, stride, seed):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, stride + 1, size=n).astype(np.uint8)
    ids = rng.integers(0, n, size=(n, stride)).astype(np.uint32)
    return deg, ids


def scalar_round(S, k, cv, cu):
    """One round of the table above from its connections, node by node."""
    n = S.size
    part = [[] for _ in range(n)]
    for a, b in zip(cv.tolist(), cu.tolist()):
        part[a].append(int(S[b]))
        part[b].append(int(S[a]))
    new = S.copy()
    for x in range(n):
        s = int(S[x])
        c = sum(1 for q in part[x] if k < q < D)
        b = sum(1 for q in part[x] if 1 <= q <= k)
        if s == 0:
            new[x] = k + 1 if c else 1 if b else 0
        elif s <= k:
            ge = sum(1 for q in part[x] if s <= q <= k)
            lt = sum(1 for q in part[x] if q < s)
            new[x] = k + 1 if c else (s + 1 if s < k else k + 1) if ge > lt else s
        elif s != D:
            new[x] = s + 1 if s < 2 * k else D
    return new


@pytest.mark.parametrize("k,drop", [(1, 0.1), (3, 0.0), (3, 0.57)])
def test_random_tables(oracle, k, drop):
    """messages = the active ends summed over the connections, received is
    monotone, and the vectorised round equals the table applied node by node."""
    n = 500
    deg, ids = random_rows(n, 6, 7 + k)
    deg[5] = 6
    dead = np.random.default_rng(2).random(n) < 0.05
    dead[5] = False
    e = PyMedian(oracle, oracle.make_params(**dict(MEDIAN, n=n, drop_rate=drop)), deg, ids, 5, k, dead)
    seen, last = set(), 1
    for t in range(60):
        S = e.state.copy()
        row = e.step()
        cv, cu = e.last
        assert not dead[cv].any() and not dead[cu].any() and (deg[cv] > 0).all() and (S[cv] != D).all()
        ends = sum(int(S[a] not in (0, D)) + int(S[b] not in (0, D)) for a, b in zip(cv.tolist(), cu.tolist()))
        assert row[3] == ends and row[2] >= cv.size and row[1] >= row[2]
        assert np.array_equal(e.state, scalar_round(S, k, cv, cu)), t
        assert row[4] >= last and not (e.inf & dead).any()
        last = row[4]
        seen |= set(np.unique(e.state).tolist())
    # (informed nodes that nobody connects to stay B: pending need not reach 0 on a random table)
    assert last > n // 2 and D in seen and k + 1 in seen and 2 * k in seen


def test_config_validation():
    import gossip_simulator_amd as gs
    from gossip_simulator_amd import _lib
    p = gs.Config(n=100, model="median").to_params()
    assert (p.model, p.rumor_k, p.rumor_mode, p.trials) == (_lib.GS_MODEL_MEDIAN, 2, 0, 1) == (3, 2, 0, 1)
    assert gs.Config(n=100, model="median", rumor_k=127).to_params().rumor_k == 127
    for k in (0, 128, 255, -1):
        with pytest.raises(ValueError, match="rumor_k"):
            gs.Config(n=100, model="median", rumor_k=k).to_params()
    assert gs.Config(n=100, model="rumor", rumor_k=255).to_params().rumor_k == 255   # the rumor model's range stays
    with pytest.raises(ValueError, match="rumor"):
        gs.Config(n=100, model="gossip").to_params()
    # the rumor model's variants are not the median model's
    assert gs.Config(n=100, model="median", rumor_pull=True).to_params().rumor_mode == 0
    assert hasattr(gs.Simulator, "median_state")


BASE = dict(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1)


def test_create_checks_k_and_trials_before_the_device():
    """GS_EINVAL with a reason, with or without a GPU."""
    from gossip_simulator_amd import _lib
    L = _lib.load()
    assert L.gs_version() == 6 and C.sizeof(_lib.Params) == 112 and _lib.Params.reserved_.offset == 80
    for k in (0, 128, 255):
        p = _lib.Params(model=3, rumor_k=k, **BASE)
        h = C.c_void_p()
        assert L.gs_create(C.byref(p), C.byref(h)) == _lib.GS_EINVAL and not h.value
        assert "rumor_k" in L.gs_last_error(None).decode()
    # model 4 is still no model; a valid median context gets past the parameter check
    p = _lib.Params(model=4, rumor_k=2, **BASE)
    h = C.c_void_p()
    assert L.gs_create(C.byref(p), C.byref(h)) == _lib.GS_EINVAL and "model" in L.gs_last_error(None).decode()
    p = _lib.Params(model=3, rumor_k=127, rumor_mode=8, **BASE)   # rumor_mode is unused
    rc = L.gs_create(C.byref(p), C.byref(h))
    assert rc in (_lib.GS_OK, _lib.GS_EDEVICE)
    if rc == _lib.GS_OK:
        L.gs_destroy(h)


def test_creates_that_refuse_the_model_name_it():
    from gossip_simulator_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    p2 = _lib.Params(model=3, rumor_k=2, trials=2, **BASE)
    p1 = _lib.Params(model=3, rumor_k=2, **BASE)
    for call in (lambda: L.gs_create(C.byref(p2), C.byref(h)),
                 lambda: L.gs_create_trials(C.byref(p2), C.byref(h)),
                 lambda: L.gs_create_trials(C.byref(p1), C.byref(h)),
                 lambda: L.gs_create_multi(C.byref(p1), devs, 2, C.byref(h)),
                 lambda: L.gs_create_multi(C.byref(p2), devs, 2, C.byref(h)),
                 lambda: L.gs_create_rank(C.byref(p1), 0, 2, 0, None, C.byref(h)),
                 lambda: L.gs_create_rank(C.byref(p2), 0, 2, 0, None, C.byref(h))):
        assert call() == _lib.GS_EINVAL and not h.value
        assert "GS_MODEL_MEDIAN" in L.gs_last_error(None).decode()
    # the rumor model's refusals keep their texts
    pr = _lib.Params(model=2, rumor_k=2, **BASE)
    assert L.gs_create_multi(C.byref(pr), devs, 2, C.byref(h)) == _lib.GS_EINVAL
    why = L.gs_last_error(None).decode()
    assert "GS_MODEL_RUMOR" in why and "GS_MODEL_MEDIAN" not in why


def test_lists_of_names():
    def read(*p):
        with open(os.path.join(ROOT, *p)) as f:
            return f.read()
    from gossip_simulator_amd import _lib
    hdr, integ = read("include", "gossip.h"), read("INTEGRATION.md")
    assert re.search(r"#define GS_MODEL_MEDIAN 3u\b", hdr) and _lib.GS_MODEL_MEDIAN == 3
    assert re.search(r"\bint gs_read_median_state\(gs_ctx\*", hdr)
    assert "gs_read_median_state" in _lib.EXPORTS and hasattr(_lib.load(), "gs_read_median_state")
    assert "uint64_t reserved_[4];" in hdr and "#define GS_ABI_VERSION 6" in hdr
    for name in ("GS_MODEL_MEDIAN", "gs_read_median_state", "-model median", "median_state"):
        assert name in integ, name
    rng = read("gossip_simulator_amd", "csrc", "gs_rng.h")
    assert "K_MEDIAN = 12" in rng and "K_RUMOR = 11" in rng


@pytest.mark.parametrize("k", ["0", "128", "-3"])
def test_cli_rejects_a_bad_k_before_any_device_call(k):
    r = cli("-n", "1000", "-model", "median", "-k", k)
    assert r.returncode == 2
    assert f'invalid value "{k}" for flag -k' in r.stderr and "1..127" in r.stderr
    assert r.stdout == ""  # not even the parameter echo


def test_cli_refuses_trials_and_the_rumor_flags():
    r = cli("-n", "1000", "-model", "median", "-trials", "2")
    assert r.returncode == 2 and "-trials" in r.stderr and "GS_MODEL_MEDIAN" in r.stderr and r.stdout == ""
    for flag in ("-pull", "-blind", "-coin"):
        r = cli("-n", "1000", "-model", "median", flag)
        assert r.returncode != 0 and f"{flag} needs -model rumor" in r.stderr and r.stdout == ""


def test_cli_names_the_fourth_model():
    r = cli("-model", "gossip")
    assert r.returncode == 2 and "flood, pushpull or rumor" in r.stderr and "median" in r.stderr
    r = cli("-h")
    assert r.returncode == 0 and "median" in r.stderr and re.search(r"^  -model string$", r.stderr, re.M)
    # a valid median command line gets to the create (no device here: exit 1 after the parameter echo)
    r = cli("-n", "1000", "-model", "median", "-k", "127")
    assert r.returncode == 1 and "=== Parameters ===" in r.stdout and "gs_create failed" in r.stderr
