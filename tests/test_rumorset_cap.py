"""Bounded rumor sets: a payload cap per message
(gs_rumorset_set_payload) and rumors that start later than round 0
(gs_rumorset_begin_at).  The model is pinned here by PyCappedSet, a pure-Python
restatement written from the specification, itself pinned by hand-derived
answers, by the uncapped restatement (a cap that cannot bind changes nothing),
by the oracle's push-pull for one rumor, by invariants checked every round and
by a restatement that caps the receiver's union, which the hand answers tell
apart.  The selection header (csrc/gs_pick.h) is compiled alone with the host
compiler and compared with the specification's pick.  The HIP rounds
(gs_rumorset_cap.hip) must match the restatement bit-exactly per round
(tests/test_rumorset_cap_gpu.py).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_parity import masked, random_table
from test_rumor import M32, ROOT, cli, words_of
from test_rumorset import RS, PyRumorSet, oracle_columns

LOW, HIGH, ROTATE = 0, 1, 2
POLICIES = {"low": LOW, "high": HIGH, "rotate": ROTATE}
U1, U32 = np.uint64(1), np.uint64(32)


def philox4_np(c0, c1, c2, c3, key):
    """Philox4x32-10 over arrays (uint64 lanes holding 32-bit words): all four outputs."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U32) ^ c1 ^ k0, p1 & M32, (p0 >> U32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def py_pick(x, B, pick, o, R):
    """The specification's pick on one Python int, bit by bit."""
    bits = [i for i in range(R) if (x >> i) & 1]
    if len(bits) <= B:
        return x
    if pick == LOW:
        sel = bits[:B]
    elif pick == HIGH:
        sel = bits[-B:]
    else:
        sel = [i for i in ((o + k) % R for k in range(R)) if (x >> i) & 1][:B]
    return sum(1 << i for i in sel)


def popcounts(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1).sum(
        axis=1, dtype=np.int64)


def pick_np(x, B, pick, o, R):
    """pick over arrays: only the words with more than B bits are touched.  A
    word's bits are laid out in the order the policy meets them (upwards, for
    ROTATE from o with the wrap, for HIGH downwards), the first B kept."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    out = x.copy()
    over = np.nonzero(popcounts(x) > B)[0]
    if over.size == 0:
        return out
    bits = np.unpackbits(x[over].astype("<u8").view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :R]
    if pick == LOW:
        order = np.broadcast_to(np.arange(R), bits.shape)
    elif pick == HIGH:
        order = np.broadcast_to(np.arange(R)[::-1], bits.shape)
    else:
        order = (np.asarray(o, np.int64)[over, None] + np.arange(R)[None, :]) % R
    met = np.take_along_axis(bits, order, axis=1).astype(np.int64)
    keep = (met == 1) & (np.cumsum(met, axis=1) <= B)
    w = np.zeros(over.size, np.uint64)
    for k in range(R):   # (R <= 64 column passes)
        w |= np.where(keep[:, k], U1 << order[:, k].astype(np.uint64), np.uint64(0))
    out[over] = w
    return out


class PyCappedSet(PyRumorSet):
    """Section 4.9.1, round by round, on top of section 4.9's restatement (who
    calls whom, lost calls, failed nodes, fired, sent, messages, the float32
    rule).  B = 0: no cap.  starts[j]: rumor j enters at its sender after round
    starts[j]'s commit (0: at begin); a rumor whose sender is failed is dead,
    every other one counts as started from begin on.

    `wrong` restates a mistake, for the non-vacuity test only: "union_cap" caps
    what a node receives from all its connections together instead of every
    message by itself."""

    def __init__(self, oracle, p, deg, ids, senders, starts=None, B=0, pick=LOW, failed=None, wrong=None):
        super().__init__(oracle, p, deg, ids, senders, failed, wrong)
        self.B, self.pick = int(B), int(pick)
        self.starts = [0] * self.R if starts is None else [int(s) for s in starts]
        assert len(self.starts) == self.R and all(0 <= s < 2**31 for s in self.starts)
        self.have = np.zeros(self.n, np.uint64)   # (the base class put every live rumor in at begin)
        self.inject(0)
        self.wanted = self.carried = self.bound = 0
        self.gains = None

    traffic = property(lambda self: dict(wanted=self.wanted, carried=self.carried, bound=self.bound))

    def inject(self, t):
        into = np.zeros(self.n, np.int64)
        for j in range(self.R):
            if self.started[j] and self.starts[j] == t:
                self.have[self.senders[j]] |= np.uint64(1 << j)
                into[self.senders[j]] += 1
        return into

    def calls4(self, v):
        r0, r1, r2, r3 = philox4_np(v, self.t, 0, self.c3, self.key)
        u = self.ids[v, ((r0 * self.deg[v].astype(np.uint64)) >> U32).astype(np.int64)].astype(np.int64)
        kept = ((r1 * np.uint64(100)) >> U32).astype(np.int64) >= self.kd
        R = np.uint64(self.R)
        return u, kept, ((r2 * R) >> U32).astype(np.int64), ((r3 * R) >> U32).astype(np.int64)

    def step(self):
        self.t += 1
        H = self.have.copy()
        v = np.nonzero(~self.dead & (self.deg > 0))[0]
        u, kept, o_push, o_pull = self.calls4(v)
        conn = kept & ~self.dead[u]
        cv, cu = v[conn], u[conn]
        self.last = (cv, cu)
        messages = int((H[cv] != 0).sum()) + int((H[cu] != 0).sum())
        want_u, want_v = H[cv] & ~H[cu], H[cu] & ~H[cv]
        nxt = H.copy()
        if self.wrong == "union_cap":
            union = np.zeros(self.n, np.uint64)
            np.bitwise_or.at(union, cu, want_u)
            np.bitwise_or.at(union, cv, want_v)
            nxt |= pick_np(union, self.B, LOW, None, self.R)
        else:
            give, take = want_u, want_v
            if self.B:
                give = pick_np(want_u, self.B, self.pick, o_push[conn], self.R)
                take = pick_np(want_v, self.B, self.pick, o_pull[conn], self.R)
                pu, pv = popcounts(want_u), popcounts(want_v)
                self.wanted += int(pu.sum() + pv.sum())
                self.carried += int(popcounts(give).sum() + popcounts(take).sum())
                self.bound += int((pu > self.B).sum() + (pv > self.B).sum())
            np.bitwise_or.at(nxt, cu, give)
            np.bitwise_or.at(nxt, cv, take)
        assert not nxt[self.dead].any()
        self.have = nxt
        callers = np.bincount(cu[cu != cv], minlength=self.n)   # connected callers per node (a self-call moves nothing)
        into = self.inject(self.t)                               # after the round's commit, inside its row
        self.gains = (popcounts(self.have & ~H), callers, into)
        return [self.t, v.size, int(kept.sum()), messages, self.received, 0, self.pending]


# ---- hand-derived answers ---------------------------------------------------------------

def one_caller(oracle, senders, starts=None, B=0, pick=LOW, wrong=None, trial=0, table=((0, 1),), failed=None):
    """Six nodes; only the callers of `table` have a friend (one, so the callee is fixed); no loss."""
    deg = np.zeros(6, np.uint8)
    ids = np.zeros((6, 1), np.uint32)
    for v, u in table:
        deg[v], ids[v, 0] = 1, u
    p = oracle.make_params(**dict(RS, n=6, fanout=1, fanin=1, drop_rate=0.0, trial=trial))
    return PyCappedSet(oracle, p, deg, ids, senders, starts, B, pick, failed, wrong)


def test_three_rumors_meet_one_under_each_policy(oracle):
    """Node 0 holds rumors {0, 1, 2} and calls node 1, which holds {3}; B = 2.
    The callee wants three rumors, one more than a message carries: bound = 1;
    the caller wants one, which fits.  LOW sends {0, 1}: have[1] = {0, 1, 3} =
    11; HIGH sends {1, 2}: have[1] = {1, 2, 3} = 14; either way the reply brings
    rumor 3: have[0] = 15.  wanted = 3 + 1, carried = 2 + 1.  One caller: fired =
    sent = 1; both ends hold something: messages = 2; received = 4 + 3.  Round 2
    (LOW): node 1 still wants {2}, which fits: wanted 5, carried 4, bound still 1."""
    for pick, word in ((LOW, 11), (HIGH, 14)):
        e = one_caller(oracle, [0, 0, 0, 1], B=2, pick=pick)
        assert e.have.tolist() == [7, 8, 0, 0, 0, 0] and e.received == 4
        assert e.step() == [1, 1, 1, 2, 7, 0, 4] and e.have.tolist() == [15, word, 0, 0, 0, 0]
        assert e.traffic == dict(wanted=4, carried=3, bound=1)
        assert e.step() == [2, 1, 1, 2, 8, 0, 4] and e.have.tolist() == [15, 15, 0, 0, 0, 0]
        assert e.traffic == dict(wanted=5, carried=4, bound=1)


def test_rotate_starts_at_the_draws_offset_and_wraps(oracle):
    """ROTATE on the same meeting: going up from o_push = uniform(r.z, 4) of
    node 0's own draw the first two of {0, 1, 2} are {0, 1} from 0, {1, 2} from
    1, {2, 0} from 2 (past 3, which is not wanted, and round to 0) and {0, 1}
    from 3.  Sixteen trials draw every offset."""
    sent_from = {0: 0b0011, 1: 0b0110, 2: 0b0101, 3: 0b0011}
    seen = set()
    for trial in range(16):
        e = one_caller(oracle, [0, 0, 0, 1], B=2, pick=ROTATE, trial=trial)
        z = oracle.philox([0, 1, 0, (9 << 24) | trial], e.key)[2]
        o = (z * 4) >> 32
        seen.add(o)
        e.step()
        assert e.have.tolist() == [15, 8 | sent_from[o], 0, 0, 0, 0], (trial, o)
        assert e.traffic == dict(wanted=4, carried=3, bound=1)
    assert seen == {0, 1, 2, 3}
    assert py_pick(0b0111, 2, ROTATE, 2, 4) == 0b0101 and py_pick(0b1001, 1, ROTATE, 1, 4) == 0b1000


def test_two_callers_are_capped_one_by_one(oracle):
    """Nodes 0 and 1 both call node 2; node 0 holds {0, 1}, node 1 holds {2, 3},
    B = 1 (LOW).  Each message is capped by itself: node 2 gets rumor 0 from one
    caller and rumor 2 from the other, two rumors in a round with B = 1; have[2]
    = 5.  wanted = 4, carried = 2, both messages bound; node 2 held nothing, so
    messages = 2.  A cap on what node 2 receives in all would leave it {0} only."""
    kw = dict(senders=[0, 0, 1, 1], B=1, table=((0, 2), (1, 2)))
    e = one_caller(oracle, **kw)
    assert e.step() == [1, 2, 2, 2, 6, 0, 4] and e.have.tolist() == [3, 12, 5, 0, 0, 0]
    assert e.traffic == dict(wanted=4, carried=2, bound=2)
    bad = one_caller(oracle, wrong="union_cap", **kw)
    bad.step()
    assert bad.have.tolist() == [3, 12, 1, 0, 0, 0]   # the mistake is visible to the hand answer


def test_starts_by_hand(oracle):
    """Node 0 calls node 1; node 5 is failed.  Rumor 0 starts at node 0 at begin,
    rumors 1 and 2 both at node 1 after round 2, rumor 3 at node 5 after round 1:
    its sender is failed, so it is dead and never enters.  B = 1, LOW.

    Begin: have = [1, 0, ...]; three rumors are live from here on (pending 3: 99 %
    of 6 is all 6).  Round 1: node 1 gets rumor 0: received 2.  Round 2: nothing
    is wanted (2 messages); then rumors 1 and 2 enter at node 1, inside round
    2's row: have[1] = 7, received 4, counts [2, 1, 1, 0].  Round 3: node 0 wants
    {1, 2}, one more than B: bound, and LOW sends rumor 1: have[0] = 3.  Round 4:
    rumor 2 follows; both nodes hold all three live rumors."""
    e = one_caller(oracle, [0, 1, 1, 5], starts=[0, 2, 2, 1], B=1, failed=np.arange(6) == 5)
    assert e.started == [True, True, True, False] and e.live == 7
    assert (e.have.tolist(), e.received, e.pending) == ([1, 0, 0, 0, 0, 0], 1, 3) and not e.holds_all.any()
    assert e.step() == [1, 1, 1, 1, 2, 0, 3] and e.have.tolist() == [1, 1, 0, 0, 0, 0]
    assert not e.column(1).any() and not e.column(2).any()
    assert e.step() == [2, 1, 1, 2, 4, 0, 3] and e.have.tolist() == [1, 7, 0, 0, 0, 0]
    assert e.counts.tolist() == [2, 1, 1, 0] and e.traffic == dict(wanted=1, carried=1, bound=0)
    assert e.holds_all.tolist() == [False, True, False, False, False, False]
    assert e.step() == [3, 1, 1, 2, 5, 0, 3] and e.have.tolist() == [3, 7, 0, 0, 0, 0]
    assert e.traffic == dict(wanted=3, carried=2, bound=1)
    assert e.step() == [4, 1, 1, 2, 6, 0, 3] and e.have.tolist() == [7, 7, 0, 0, 0, 0]
    assert e.traffic == dict(wanted=4, carried=3, bound=1) and not e.column(3).any()
    assert e.holds_all.tolist() == [True, True, False, False, False, False]
    # R = 1, s = 5: the injection itself completes the sender's word
    e = one_caller(oracle, [1], starts=[5])
    for t in range(1, 7):
        row = e.step()
        assert row[4] == {5: 1, 6: 2}.get(t, 0)   # node 0 pulls it in round 6
        assert e.holds_all.tolist() == [t >= 6, t >= 5, False, False, False, False]


# ---- against the uncapped restatement and the oracle --------------------------------------

@pytest.mark.parametrize("n", [100, 1000])
@pytest.mark.parametrize("mask", [False, True])
def test_a_cap_that_cannot_bind_changes_nothing(oracle, n, mask):
    """B >= R and every start 0: word for word and row for row section 4.9's
    restatement, under every policy; carried == wanted and bound == 0."""
    rounds, R = 25, 5
    deg, ids = random_table(n, 6, 0, 6, seed=n + 1)
    p = oracle.make_params(**dict(RS, n=n))
    failed = (np.random.default_rng(n).random(n) < 0.05) if mask else None
    senders = [int(x) for x in np.random.default_rng(7).integers(0, n, size=R)]
    ref = PyRumorSet(oracle, p, deg, masked(deg, ids), senders, failed)
    runs = [PyCappedSet(oracle, p, deg, masked(deg, ids), senders, None, B, pick, failed)
            for pick in POLICIES.values() for B in (R, 64)]
    for t in range(rounds):
        row = ref.step()
        for e in runs:
            assert e.step() == row and np.array_equal(e.have, ref.have), (e.B, e.pick, t)
    for e in runs:
        assert e.wanted == e.carried > n and e.bound == 0
    assert ref.counts.max() > n // 2


def test_one_rumor_is_the_oracles_pushpull(oracle):
    n, rounds = 1000, 25
    deg, ids = random_table(n, 6, 0, 6, seed=3)
    p = oracle.make_params(**dict(RS, n=n))
    ref = oracle_columns(oracle, p, deg, ids, [17], rounds, None)[0]
    e = PyCappedSet(oracle, p, deg, masked(deg, ids), [17], None, 1, ROTATE)
    for t in range(rounds + 1):
        assert np.array_equal(words_of(e.column(0)), ref[t]), t
        e.step()
    assert e.bound == 0 and e.carried == e.wanted >= int(e.counts[0]) - 1   # (two callers may bring a node the same copy)


@pytest.mark.parametrize("pick", list(POLICIES))
def test_invariants_every_round(oracle, pick):
    """have only grows; column j is empty before s_j; carried <= wanted; a node
    gains at most B x (1 + its connected callers) rumors besides those that
    enter at it; and the cap binds."""
    n, R, B = 1000, 12, 2
    deg, ids = random_table(n, 6, 0, 6, seed=5)
    ids[:, 0] = np.arange(n) // 8    # shared friends: several callers per callee
    p = oracle.make_params(**dict(RS, n=n))
    starts = [2 * j for j in range(R)]
    e = PyCappedSet(oracle, p, deg, masked(deg, ids), [(83 * j) % n for j in range(R)], starts, B, POLICIES[pick])
    for t in range(1, 41):
        before = e.have.copy()
        e.step()
        assert not (before & ~e.have).any()
        for j in range(R):
            assert e.column(j).any() == (t >= starts[j])
        gained, callers, into = e.gains
        assert (gained <= B * (1 + callers) + into).all() and e.carried <= e.wanted
    assert e.bound > 0 and e.carried < e.wanted and e.counts.min() > n // 2


# ---- the selection header, compiled alone ----------------------------------------------------

PICK_MAIN = r"""
#include "gs_pick.h"
extern "C" void pick_many(const uint64_t* x, uint64_t n, uint32_t B, uint32_t pick, uint32_t o, uint32_t R,
                          uint64_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = gs::rs_pick(x[i], B, pick, o, R);
}
"""


def test_selection_header_against_the_specification(tmp_path):
    """csrc/gs_pick.h through the host compiler: every B in 1..64, random, sparse
    and all-ones words, R in {1, 2, 63, 64}, and for ROTATE every offset 0..R-1
    (uniform(a, R) yields nothing larger)."""
    src, lib = tmp_path / "pick_main.cpp", tmp_path / "libpick.so"
    src.write_text(PICK_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "gossip_simulator_amd", "csrc"), "-o", str(lib), str(src)], check=True)
    fn = C.CDLL(str(lib)).pick_many
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    rng = np.random.default_rng(64)
    for R in (1, 2, 63, 64):
        full = (1 << R) - 1
        words = [full, 0, 1 << (R - 1), full & 0x5555555555555555, full & ~1] + \
            [int(x) & full for x in rng.integers(0, 2**64, size=4, dtype=np.uint64)] + \
            [int(x & y) & full for x, y in rng.integers(0, 2**64, size=(2, 2), dtype=np.uint64)]
        x = np.array(words, np.uint64)
        out = np.zeros_like(x)
        for B in range(1, 65):
            for pick in (LOW, HIGH, ROTATE):
                for o in (range(R) if pick == ROTATE else (0,)):
                    fn(x.ctypes.data, x.size, B, pick, o, R, out.ctypes.data)
                    want = [py_pick(w, B, pick, o, R) for w in words]
                    assert out.tolist() == want, (R, B, pick, o)
                    # the arrays' pick of the restatement is the same function
                    if B in (1, 2, R - 1, R, 64):
                        assert pick_np(x, B, pick, np.full(x.size, o), R).tolist() == want, (R, B, pick, o)


# ---- the ABI, with no device ---------------------------------------------------------------------

def test_symbols_sizes_and_refusals():
    def read(*p):
        with open(os.path.join(ROOT, *p)) as f:
            return f.read()
    from gossip_simulator_amd import _lib
    import gossip_simulator_amd as gs
    hdr, integ, design = read("include", "gossip.h"), read("INTEGRATION.md"), read("DESIGN.md")
    L = _lib.load()
    assert L.gs_version() == 6 and "#define GS_ABI_VERSION 6" in hdr
    for name in ("gs_rumorset_set_payload", "gs_rumorset_begin_at", "gs_rumorset_traffic_get"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert name in integ, name
    for name, val in (("GS_PICK_LOW", 0), ("GS_PICK_HIGH", 1), ("GS_PICK_ROTATE", 2)):
        assert re.search(rf"#define {name} {val}u\b", hdr) and getattr(_lib, name) == val
    assert "typedef struct gs_rumorset_traffic" in hdr and C.sizeof(_lib.RumorTraffic) == 32
    assert C.sizeof(_lib.RumorStats) == 32 and C.sizeof(_lib.Params) == 112   # no struct changed size
    for name in ("set_payload", "begin_rumors", "rumor_traffic"):
        assert hasattr(gs.Simulator, name), name
    assert "### 4.9.1" in design and "gs_rumorset_cap.hip" in design and "gs_rumorset_cap.hip" in read("README.md")
    # a NULL context is refused
    t = _lib.RumorTraffic()
    one = (C.c_int64 * 1)(0)
    assert L.gs_rumorset_set_payload(None, 1, 0) == _lib.GS_EINVAL
    assert L.gs_rumorset_begin_at(None, one, one, 1) == _lib.GS_EINVAL
    assert L.gs_rumorset_traffic_get(None, C.byref(t)) == _lib.GS_EINVAL


def test_cli_bounded_set_usage_errors():
    """-payload, -pick and -every are legal only with -rumors and in range:
    anything else is a usage error before the parameter echo and any device call."""
    pp = ("-n", "1000", "-model", "pushpull")
    for args, word in ((("-payload", "2"), "-payload needs -rumors"),
                       (("-pick", "high"), "-pick needs -rumors"),
                       (("-every", "3"), "-every needs -rumors"),
                       (pp + ("-payload", "2"), "-payload needs -rumors"),
                       (pp + ("-every", "1"), "-every needs -rumors"),
                       (("-model", "median", "-batch", "2", "-pick", "low"), "-pick needs -rumors"),
                       (pp + ("-rumors", "4", "-payload", "65"), "flag -payload: want 0..64"),
                       (pp + ("-rumors", "4", "-payload", "-1"), "flag -payload: want 0..64"),
                       (pp + ("-rumors", "4", "-pick", "oldest"), "flag -pick: want low, high or rotate"),
                       (pp + ("-rumors", "4", "-every", "-1"), "flag -every"),
                       (pp + ("-rumors", "4", "-every", "1000000000"), "flag -every")):
        r = cli(*args)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)
        assert r.stdout == ""   # not even the parameter echo
    r = cli(*pp, "-rumors", "4", "-payload", "x")
    assert r.returncode == 2 and 'invalid value "x" for flag -payload' in r.stderr
    r = cli("-h")
    for flag in ("payload int", "pick string", "every int"):
        assert re.search(rf"^  -{flag}$", r.stderr, re.M), flag
    # valid command lines get to the create (no device here: exit 1 after the same parameter echo)
    plain = cli(*pp, "-rumors", "4")
    for more in (("-payload", "2"), ("-payload", "64", "-pick", "rotate", "-every", "3"), ("-every", "0")):
        r = cli(*pp, "-rumors", "4", *more)
        assert r.returncode == 1 and r.stdout == plain.stdout and "gs_create failed" in r.stderr
