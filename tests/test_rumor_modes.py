"""The variants of rumor mongering (gs_params.rumor_mode: GS_RUMOR_BLIND,
GS_RUMOR_COIN, GS_RUMOR_PULL): a pure-Python restatement
of all eight modes, written from the specification, pinned by hand-derived
answers and by tests/test_rumor.py's PyRumor in mode 0.  The HIP rounds must
match it bit-exactly per round (tests/test_rumor_modes_gpu.py).
"""
from __future__ import annotations

import ctypes as C
import itertools
import os

import numpy as np
import pytest

from test_rumor import ROOT, RUMOR, PyRumor, cli, philox_np, words_of  # noqa: F401 (words_of: for the GPU tests)

BLIND, COIN, PULL = 1, 2, 4
K_RUMOR = 11
U32 = np.uint64(32)


class PyRumorModes:
    """The specification, round by round.  State per node: informed, failed,
    miss, hot.  Every decision of a round reads I and H as they were at its
    start."""

    def __init__(self, oracle, p, deg, ids, sender, k, failed=None, mode=0):
        self.n, self.k, self.t, self.mode = int(p.n), int(k), 0, int(mode)
        self.key = [int(p.seed) & 0xFFFFFFFF, int(p.seed) >> 32]
        self.c3 = (K_RUMOR << 24) | (int(p.trial) & 0xFFFFFF)
        self.kd = oracle.threshold(p.drop_rate)
        self.deg, self.ids = np.asarray(deg).astype(np.int64), np.asarray(ids)
        self.dead = np.zeros(self.n, bool) if failed is None else np.asarray(failed, bool)
        self.inf = np.zeros(self.n, bool)
        self.hot = np.zeros(self.n, bool)
        self.miss = np.zeros(self.n, np.int64)
        self.last_served = np.zeros(0, np.int64)
        self.last_vain = np.zeros(0, np.int64)
        if sender < 0:
            sender = int(oracle.pick_sender(p))
        if not self.dead[sender]:
            self.inf[sender] = True
            # push: hot needs a friend to call; pull: a hot node answers, it need not call
            self.hot[sender] = True if self.mode & PULL else self.deg[sender] > 0

    received = property(lambda self: int(self.inf.sum()))
    pending = property(lambda self: int(self.hot.sum()))
    removed = property(lambda self: self.inf & ~self.hot)

    def calls(self, v):
        r0, r1 = philox_np(v, self.t, 0, self.c3, self.key)
        u = self.ids[v, ((r0 * self.deg[v].astype(np.uint64)) >> U32).astype(np.int64)].astype(np.int64)
        kept = ((r1 * np.uint64(100)) >> U32).astype(np.int64) >= self.kd
        return u, kept

    def events(self, v):
        """One event for each node of v (all hot): counter or coin."""
        if self.mode & COIN:
            r0, _ = philox_np(v, self.t, 1, self.c3, self.key)
            gone = v[((r0 * np.uint64(self.k)) >> U32) == 0]
        else:
            self.miss[v] += 1
            gone = v[self.miss[v] == self.k]
        self.hot[gone] = False

    def step(self):
        self.t += 1
        I, H = self.inf.copy(), self.hot.copy()
        if self.mode & PULL:
            v = np.nonzero(~self.dead & (self.deg > 0))[0]   # informed or not, hot or removed
            u, kept = self.calls(v)
            live = kept & ~self.dead[u]
            answered = live & H[u]
            served, vain = answered & ~I[v], answered & I[v]
            fresh = v[served]
            self.last_served, self.last_vain = u[served], u[vain]
            if self.mode & BLIND:
                ev = H
            else:
                ev = np.zeros(self.n, bool)
                ev[u[vain]] = True
                ev[u[served]] = False
            self.events(np.nonzero(ev)[0])
            self.inf[fresh] = True
            self.hot[fresh] = True
        else:
            v = np.nonzero(H)[0]
            u, kept = self.calls(v)
            live = kept & ~self.dead[u]
            fresh = u[live & ~I[u]]
            self.events(v if self.mode & BLIND else v[live & I[u]])
            self.inf[fresh] = True
            self.hot[fresh[self.deg[fresh] > 0]] = True
        return [self.t, v.size, int(kept.sum()), int(live.sum()), self.received, 0, self.pending]

    def run(self, rounds):
        return np.array([self.step() for _ in range(rounds)], dtype=np.uint64).reshape(rounds, 7)


def random_rows(n, stride, seed):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, stride + 1, size=n).astype(np.uint8)
    ids = rng.integers(0, n, size=(n, stride)).astype(np.uint32)
    return deg, ids


def test_mode_0_is_the_first_model(oracle):
    n = 777
    deg, ids = random_rows(n, 6, 1)
    deg[5] = 6
    dead = np.random.default_rng(2).random(n) < 0.05
    dead[5] = False
    p = oracle.make_params(**dict(RUMOR, n=n))
    a, b = PyRumor(oracle, p, deg, ids, 5, 2, dead), PyRumorModes(oracle, p, deg, ids, 5, 2, dead, 0)
    for t in range(40):
        assert a.step() == b.step(), t
        assert np.array_equal(a.inf, b.inf) and np.array_equal(a.hot, b.hot) and np.array_equal(a.miss, b.miss)
    assert a.received > 100


def pair(oracle, k, mode, drop=0.0):
    p = oracle.make_params(**dict(RUMOR, n=2, drop_rate=drop))
    return PyRumorModes(oracle, p, np.array([1, 1], np.uint8), np.array([[1], [0]], np.uint32), 0, k, None, mode)


COLS = [0, 1, 2, 3, 4, 6]  # tick, fired, sent, messages, received, pending


def test_pair_blind_push(oracle):
    # k = 1.  round 1: 0 calls 1 (informed, hot); 0's call is its event: removed.  round 2: 1 calls
    # 0 (informed already, which a blind caller never learns); its event: removed.
    e = pair(oracle, 1, BLIND)
    assert (e.received, e.pending) == (1, 1)
    assert e.run(3)[:, COLS].tolist() == [[1, 1, 1, 1, 2, 1], [2, 1, 1, 1, 2, 0], [3, 0, 0, 0, 2, 0]]
    assert e.removed.all()
    # k = 2.  round 1: miss[0] = 1, 1 informed.  round 2: both call; miss[0] = 2: removed;
    # miss[1] = 1.  round 3: 1 calls, miss[1] = 2: removed.
    e = pair(oracle, 2, BLIND)
    assert e.run(4)[:, COLS].tolist() == [[1, 1, 1, 1, 2, 2], [2, 2, 2, 2, 2, 1], [3, 1, 1, 1, 2, 0],
                                          [4, 0, 0, 0, 2, 0]]
    assert e.miss.tolist() == [2, 2]


def test_pair_feedback_pull(oracle):
    # Both nodes call every round, for ever: fired = sent = messages = 2 in every row.
    # k = 1.  round 1: H = {0}.  0 asks 1 (not hot: nothing); 1 asks 0: 1 is informed, 0 was served:
    # no event.  round 2: H = {0, 1}, each asked in vain by the other, neither served: both removed.
    e = pair(oracle, 1, PULL)
    assert (e.received, e.pending) == (1, 1)
    assert e.run(3)[:, COLS].tolist() == [[1, 2, 2, 2, 2, 2], [2, 2, 2, 2, 2, 0], [3, 2, 2, 2, 2, 0]]
    assert e.removed.all()
    # k = 2: round 2 makes miss = 1 each, round 3 removes both.
    e = pair(oracle, 2, PULL)
    assert e.run(4)[:, COLS].tolist() == [[1, 2, 2, 2, 2, 2], [2, 2, 2, 2, 2, 2], [3, 2, 2, 2, 2, 0],
                                          [4, 2, 2, 2, 2, 0]]
    assert e.miss.tolist() == [2, 2]


def test_pair_blind_pull(oracle):
    # k = 1.  round 1: H = {0}; 1 asks 0 and is informed; 0 was hot this round: removed.
    # round 2: H = {1}: removed.
    e = pair(oracle, 1, PULL | BLIND)
    assert e.run(3)[:, COLS].tolist() == [[1, 2, 2, 2, 2, 1], [2, 2, 2, 2, 2, 0], [3, 2, 2, 2, 2, 0]]
    # k = 2.  round 1: miss[0] = 1, 1 informed.  round 2: miss[0] = 2: removed; miss[1] = 1.
    # round 3: miss[1] = 2: removed.
    e = pair(oracle, 2, PULL | BLIND)
    assert e.run(4)[:, COLS].tolist() == [[1, 2, 2, 2, 2, 2], [2, 2, 2, 2, 2, 1], [3, 2, 2, 2, 2, 0],
                                          [4, 2, 2, 2, 2, 0]]
    assert e.removed.all()


def test_pull_sender_alone_with_an_empty_row(oracle):
    p = oracle.make_params(**dict(RUMOR, n=1))
    deg, ids = np.zeros(1, np.uint8), np.zeros((1, 1), np.uint32)
    e = PyRumorModes(oracle, p, deg, ids, 0, 2, None, PULL)
    assert (e.received, e.pending) == (1, 1)      # hot without a friend: it answers
    assert e.run(30)[:, 1:].tolist() == [[0, 0, 0, 1, 0, 1]] * 30   # nobody ever calls it: hot for ever
    e = PyRumorModes(oracle, p, deg, ids, 0, 3, None, PULL | BLIND)
    assert e.run(4)[:, [0, 4, 6]].tolist() == [[1, 1, 1], [2, 1, 1], [3, 1, 0], [4, 1, 0]]
    # push: the same sender is removed at once
    assert PyRumorModes(oracle, p, deg, ids, 0, 3, None, BLIND).pending == 0


@pytest.mark.parametrize("mode", [0, BLIND, PULL, PULL | BLIND])
def test_coin_with_k1_is_the_counter(oracle, mode):
    n = 777
    deg, ids = random_rows(n, 6, 3)
    deg[5] = 6
    p = oracle.make_params(**dict(RUMOR, n=n))
    a, b = PyRumorModes(oracle, p, deg, ids, 5, 1, None, mode), PyRumorModes(oracle, p, deg, ids, 5, 1, None,
                                                                             mode | COIN)
    for t in range(40):
        assert a.step() == b.step(), t
        assert np.array_equal(a.hot, b.hot) and np.array_equal(a.inf, b.inf)
    assert not b.miss.any() and a.miss.any()
    assert a.received > 1


def test_coin_draws_its_own_stream(oracle):
    """k = 2: the coin is U_2 of the event node's {v, t, 1} draw, whoever made the call."""
    e = pair(oracle, 2, PULL | COIN)
    e.step()  # 1 informed, 0 served
    r0, _ = philox_np(np.array([0, 1]), 2, 1, e.c3, e.key)
    want = [bool((int(x) * 2) >> 32) for x in r0]  # stays hot iff U_2 != 0
    e.step()  # both asked in vain: one coin each
    assert e.hot.tolist() == want and not e.miss.any()


def test_blind_push_ends_when_every_call_is_lost(oracle):
    e = pair(oracle, 4, BLIND, drop=1.0)
    rows = e.run(6)[:, COLS].tolist()
    assert rows == [[1, 1, 0, 0, 1, 1], [2, 1, 0, 0, 1, 1], [3, 1, 0, 0, 1, 1], [4, 1, 0, 0, 1, 0],
                    [5, 0, 0, 0, 1, 0], [6, 0, 0, 0, 1, 0]]
    # with feedback the same run never ends
    assert pair(oracle, 4, 0, drop=1.0).run(30)[-1, 6] == 1


def test_failed_callee_and_lost_call_are_blind_events_only(oracle):
    p = oracle.make_params(**dict(RUMOR, n=2, drop_rate=0.0))
    deg, ids, dead = np.array([1, 1], np.uint8), np.array([[1], [0]], np.uint32), np.array([False, True])
    assert PyRumorModes(oracle, p, deg, ids, 0, 2, dead, BLIND).run(3)[:, COLS].tolist() == \
        [[1, 1, 1, 0, 1, 1], [2, 1, 1, 0, 1, 0], [3, 0, 0, 0, 1, 0]]
    assert PyRumorModes(oracle, p, deg, ids, 0, 2, dead, 0).run(3)[:, 6].tolist() == [1, 1, 1]
    # pull: the failed node never calls, so the hot sender is never asked
    assert PyRumorModes(oracle, p, deg, ids, 0, 2, dead, PULL).run(3)[:, COLS].tolist() == \
        [[1, 1, 1, 0, 1, 1], [2, 1, 1, 0, 1, 1], [3, 1, 1, 0, 1, 1]]


def test_config_arguments():
    import gossip_simulator_amd as gs
    from gossip_simulator_amd import _lib
    assert (_lib.GS_RUMOR_BLIND, _lib.GS_RUMOR_COIN, _lib.GS_RUMOR_PULL) == (BLIND, COIN, PULL)
    assert gs.Config(n=100, model="rumor").to_params().rumor_mode == 0
    for b, c, q in itertools.product((False, True), repeat=3):
        p = gs.Config(n=100, model="rumor", rumor_blind=b, rumor_coin=c, rumor_pull=q).to_params()
        assert p.rumor_mode == b * BLIND | c * COIN | q * PULL
    # the other models ignore the arguments
    assert gs.Config(n=100, model="pushpull", rumor_pull=True).to_params().rumor_mode == 0
    with open(os.path.join(ROOT, "include", "gossip.h")) as f:
        hdr = f.read()
    for name, val in (("GS_RUMOR_BLIND", 1), ("GS_RUMOR_COIN", 2), ("GS_RUMOR_PULL", 4)):
        assert f"#define {name} {val}u" in hdr
    assert "uint32_t rumor_mode;" in hdr and "uint64_t reserved_[4];" in hdr


def test_create_checks_the_mode_before_the_device():
    from gossip_simulator_amd import _lib
    L = _lib.load()
    assert C.sizeof(_lib.Params) == 112
    assert _lib.Params.rumor_mode.offset == 72 and _lib.Params.reserved_.offset == 80
    base = dict(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, rumor_k=2)
    for mode in (8, 15, 1 << 31):
        p = _lib.Params(model=2, rumor_mode=mode, **base)
        h = C.c_void_p()
        assert L.gs_create(C.byref(p), C.byref(h)) == _lib.GS_EINVAL and not h.value
        assert "rumor_mode" in L.gs_last_error(None).decode()
    # the other models ignore the field: the create gets past the parameter check
    # (with no device visible that is GS_EDEVICE, never GS_EINVAL)
    p = _lib.Params(model=0, rumor_mode=8, **base)
    h = C.c_void_p()
    rc = L.gs_create(C.byref(p), C.byref(h))
    assert rc != _lib.GS_EINVAL
    if rc == _lib.GS_OK:
        L.gs_destroy(h)
    else:
        assert rc == _lib.GS_EDEVICE


@pytest.mark.parametrize("flag", ["-pull", "-blind", "-coin"])
def test_cli_mode_flags_need_the_rumor_model(flag):
    r = cli("-n", "1000", flag)
    assert r.returncode != 0 and f"-{flag[1:]} needs -model rumor" in r.stderr
    assert r.stdout == ""  # not even the parameter echo
    r = cli("-n", "1000", "-model", "pushpull", flag)
    assert r.returncode != 0 and "needs -model rumor" in r.stderr


def test_cli_help_lists_the_mode_flags():
    r = cli("-h")
    assert r.returncode == 0
    for flag in ("-blind", "-coin", "-pull"):
        assert f"\n  {flag}\n" in r.stderr, flag
