"""Rumor mongering (GS_MODEL_RUMOR): no reference
semantics exist (simulator.go only floods, :140-149), so the model is pinned
here by a pure-Python restatement written from the specification, itself
pinned by hand-derived answers; the HIP rounds (gs_rumor.hip) must match it
bit-exactly per round (tests/test_rumor_gpu.py).
"""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_RUMOR = 11
RUMOR = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.0,
             seed=0x5EED, trial=0, model=2)
M32 = np.uint64(0xFFFFFFFF)


def philox_np(c0, c1, c2, c3, key):
    """Philox4x32-10 over arrays (uint64 lanes holding 32-bit words); the first two outputs."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1


def words_of(bits):
    n = bits.size
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    idx = np.nonzero(bits)[0]
    np.bitwise_or.at(w, idx // 64, np.left_shift(np.uint64(1), (idx % 64).astype(np.uint64)))
    return w


class PyRumor:
    """The specification, round by round: state per node = informed, failed,
    miss count; hot = informed, miss < k, live, a friend to call."""

    def __init__(self, oracle, p, deg, ids, sender, k, failed=None):
        self.n, self.k, self.t = int(p.n), int(k), 0
        self.key = [int(p.seed) & 0xFFFFFFFF, int(p.seed) >> 32]
        self.c3 = (K_RUMOR << 24) | (int(p.trial) & 0xFFFFFF)
        self.kd = oracle.threshold(p.drop_rate)
        self.deg, self.ids = np.asarray(deg).astype(np.int64), np.asarray(ids)
        self.dead = np.zeros(self.n, bool) if failed is None else np.asarray(failed, bool)
        self.inf = np.zeros(self.n, bool)
        self.hot = np.zeros(self.n, bool)
        self.miss = np.zeros(self.n, np.int64)
        if sender < 0:
            sender = int(oracle.pick_sender(p))
        if not self.dead[sender]:
            self.inf[sender] = True
            self.hot[sender] = self.deg[sender] > 0  # an empty row: removed at once
        self.tick_99 = 0

    received = property(lambda self: int(self.inf.sum()))
    pending = property(lambda self: int(self.hot.sum()))
    removed = property(lambda self: self.inf & ~self.hot)

    def step(self):
        self.t += 1
        v = np.nonzero(self.hot)[0]
        r0, r1 = philox_np(v, self.t, 0, self.c3, self.key)
        u = self.ids[v, ((r0 * self.deg[v].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)].astype(np.int64)
        kept = ((r1 * np.uint64(100)) >> np.uint64(32)).astype(np.int64) >= self.kd
        live = kept & ~self.dead[u]        # a failed callee: no delivery, no feedback, no miss
        hit = live & self.inf[u]           # I as it was at the start of the round
        fresh = u[live & ~self.inf[u]]     # several callers may reach one fresh node: all useful
        self.last_fresh = fresh
        self.miss[v[hit]] += 1
        self.hot[v[hit & (self.miss[v] >= self.k)]] = False
        self.inf[fresh] = True
        self.hot[fresh[self.deg[fresh] > 0]] = True
        return [self.t, v.size, int(kept.sum()), int(live.sum()), self.received, 0, self.pending]

    def run(self, rounds):
        return np.array([self.step() for _ in range(rounds)], dtype=np.uint64).reshape(rounds, 7)


def test_numpy_philox_matches_the_oracle(oracle):
    key = [0x5EED, 0x1234ABCD]
    v = np.array([0, 1, 63, 64, 4132, 299_999, 2**31 - 1])
    for t in (1, 2, 40, 70000):
        r0, r1 = philox_np(v, t, 0, (K_RUMOR << 24) | 5, key)
        for i, node in enumerate(v):
            want = oracle.philox([int(node), t, 0, (K_RUMOR << 24) | 5], key)
            assert [int(r0[i]), int(r1[i])] == want[:2]


def pair(oracle, k, **kw):
    p = oracle.make_params(**dict(RUMOR, n=2, drop_rate=0.0, **kw))
    return PyRumor(oracle, p, np.array([1, 1], np.uint8), np.array([[1], [0]], np.uint32), 0, k)


def test_two_nodes_k1(oracle):
    e = pair(oracle, 1)
    assert (e.received, e.pending) == (1, 1)
    rows = e.run(3)[:, [0, 1, 2, 3, 4, 6]].tolist()
    assert rows == [[1, 1, 1, 1, 2, 2], [2, 2, 2, 2, 2, 0], [3, 0, 0, 0, 2, 0]]
    assert set(np.nonzero(e.removed)[0]) == {0, 1}


def test_two_nodes_k2_takes_one_round_more(oracle):
    e = pair(oracle, 2)
    rows = e.run(4)[:, [0, 1, 2, 3, 4, 6]].tolist()
    assert rows == [[1, 1, 1, 1, 2, 2], [2, 2, 2, 2, 2, 2], [3, 2, 2, 2, 2, 0], [4, 0, 0, 0, 2, 0]]
    assert set(np.nonzero(e.removed)[0]) == {0, 1}


def test_directed_ring_k1(oracle):
    n = 9
    p = oracle.make_params(**dict(RUMOR, n=n, drop_rate=0.0))
    e = PyRumor(oracle, p, np.ones(n, np.uint8), ((np.arange(n) + 1) % n).astype(np.uint32)[:, None], 0, 1)
    for t in range(1, n):  # round t informs node t; node t - 1 stays hot (its call was useful)
        row = e.step()
        assert e.inf[t] and row[4] == t + 1
        # node t - 2 was removed by this round's call (node t - 1 was informed already)
        assert set(np.nonzero(e.hot)[0]) == {t - 1, t}
        assert row[1:4] == ([1, 1, 1] if t == 1 else [2, 2, 2])
    # round n: node n - 2 misses (removed), node n - 1 calls the sender back and misses (removed)
    row = e.step()
    assert row == [n, 2, 2, 2, n, 0, 0]
    assert e.removed.all() and not e.hot.any()
    assert e.step() == [n + 1, 0, 0, 0, n, 0, 0]


def test_sender_with_no_friend_and_failed_sender(oracle):
    n = 5
    deg, ids = np.array([0, 1, 1, 1, 1], np.uint8), np.zeros((n, 1), np.uint32)
    p = oracle.make_params(**dict(RUMOR, n=n))
    e = PyRumor(oracle, p, deg, ids, 0, 2)
    assert (e.received, e.pending) == (1, 0) and e.removed[0]
    assert e.step() == [1, 0, 0, 0, 1, 0, 0]
    dead = np.zeros(n, bool)
    dead[1] = True
    e = PyRumor(oracle, p, deg, ids, 1, 2, dead)
    assert (e.received, e.pending) == (0, 0) and not e.removed.any()
    assert e.step() == [1, 0, 0, 0, 0, 0, 0]


def test_failed_callee_is_sent_not_delivered_and_no_miss(oracle):
    # 0 -> 1 (failed): every round fired = sent = 1, messages = 0, and node 0 never cools off
    p = oracle.make_params(**dict(RUMOR, n=2, drop_rate=0.0))
    e = PyRumor(oracle, p, np.array([1, 1], np.uint8), np.array([[1], [0]], np.uint32), 0, 1,
                np.array([False, True]))
    assert e.run(5)[:, 1:].tolist() == [[1, 1, 0, 1, 0, 1]] * 5


def test_every_call_lost_gives_no_feedback(oracle):
    p = oracle.make_params(**dict(RUMOR, n=2, drop_rate=1.0))
    e = PyRumor(oracle, p, np.array([1, 1], np.uint8), np.array([[1], [0]], np.uint32), 0, 1)
    assert e.run(30)[:, 1:].tolist() == [[1, 0, 0, 1, 0, 1]] * 30


def test_config_validation():
    import gossip_simulator_amd as gs
    from gossip_simulator_amd import _lib
    p = gs.Config(n=100, model="rumor").to_params()
    assert (p.model, p.rumor_k) == (_lib.GS_MODEL_RUMOR, 2) == (2, 2)
    assert gs.Config(n=100, model="rumor", rumor_k=255).to_params().rumor_k == 255
    for k in (0, 256, -1):
        with pytest.raises(ValueError, match="rumor_k"):
            gs.Config(n=100, model="rumor", rumor_k=k).to_params()
    with pytest.raises(ValueError, match="rumor"):
        gs.Config(n=100, model="gossip").to_params()
    # the other models ignore the field
    assert gs.Config(n=100, model="pushpull", rumor_k=0).to_params().model == _lib.GS_MODEL_PUSHPULL
    assert gs.Config(n=100, rumor_k=999).to_params().model == _lib.GS_MODEL_FLOOD
    assert gs.engine.STAT_FIELDS == ("tick", "fired", "sent", "messages", "received", "crashed", "pending")


def test_create_checks_k_and_trials_before_the_device():
    """GS_EINVAL with a reason for a bad rumor_k or trials > 1, with or without a GPU."""
    import ctypes as C
    from gossip_simulator_amd import _lib
    L = _lib.load()
    for k, trials, word in ((0, 1, "rumor_k"), (256, 1, "rumor_k"), (2, 2, "trials")):
        p = _lib.Params(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, model=2,
                        rumor_k=k, trials=trials)
        h = C.c_void_p()
        assert L.gs_create(C.byref(p), C.byref(h)) == _lib.GS_EINVAL and not h.value
        assert word in L.gs_last_error(None).decode()
    p = _lib.Params(n=100, fanout=5, fanin=6, delay_low=10, delay_high=20, model=2, rumor_k=2)
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert L.gs_create_multi(C.byref(p), devs, 2, C.byref(h)) == _lib.GS_EINVAL
    assert "GS_MODEL_RUMOR" in L.gs_last_error(None).decode()
    assert L.gs_create_rank(C.byref(p), 0, 2, 0, None, C.byref(h)) == _lib.GS_EINVAL
    assert "GS_MODEL_RUMOR" in L.gs_last_error(None).decode()
    assert C.sizeof(_lib.Params) == 8 + 4 * 4 + 8 + 8 + 8 + 4 + 4 + 4 + 4 + 8 + 8 + 4 * 8


def cli(*args):
    from gossip_simulator_amd import _lib
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")  # never touches a device
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("k", ["0", "256", "-3"])
def test_cli_rejects_a_bad_k_before_any_device_call(k):
    r = cli("-n", "1000", "-model", "rumor", "-k", k)
    assert r.returncode == 2
    assert f'invalid value "{k}" for flag -k' in r.stderr and "1..255" in r.stderr
    assert r.stdout == ""  # not even the parameter echo


def test_cli_names_the_third_model():
    r = cli("-model", "gossip")
    assert r.returncode == 2 and "flood, pushpull or rumor" in r.stderr
    r = cli("-h")
    assert r.returncode == 0 and "rumor" in r.stderr and re.search(r"^  -k int$", r.stderr, re.M)


def test_lists_of_names():
    def read(*p):
        with open(os.path.join(ROOT, *p)) as f:
            return f.read()
    from gossip_simulator_amd import _lib
    hdr, integ = read("include", "gossip.h"), read("INTEGRATION.md")
    assert re.search(r"\bint gs_read_removed\(gs_ctx\*", hdr)
    assert "gs_read_removed" in _lib.EXPORTS and hasattr(_lib.load(), "gs_read_removed")
    assert re.search(r"#define GS_MODEL_RUMOR 2u\b", hdr) and _lib.GS_MODEL_RUMOR == 2
    assert re.search(r"\buint32_t rumor_k;", hdr) and "reserved0_" not in hdr
    assert ("rumor_k", __import__("ctypes").c_uint32) in _lib.Params._fields_
    for name in ("gs_read_removed", "GS_MODEL_RUMOR", "rumor_k", "-model rumor", "-k"):
        assert name in integ, name
    assert "K_RUMOR = 11" in read("gossip_simulator_amd", "csrc", "gs_rng.h")
