"""Push-pull parity sweep of the one-trial engine (gs_pp_*.hip): round
paths, slot widths, region boundaries, caps, hubs and row content.

The engine picks its code from the row stride (packed slot bytes up to 16
slots, the failed-slot mask up to 8), from the round mode (early, dense
top-down, pull-answer, bottom-up), from n (words per wave, ranges, buckets,
workgroups, summary words, coarse bins), from what a round informs (the
deferred lists and regions and their caps) and from seven process-wide
switches, two of which are also the fallbacks after a failed allocation.
Every GPU case here is bit-exact per round against oracle.Engine (model 1):
every stats row and the informed bitset's hash after every round, until the
oracle's run is covered or can inform nobody new (at most CAP rounds), and the
crashed bitset at the end.  The oracle's side is computed once per (table,
mask) and shared by the modes.  The switches run in child processes
(tests/pushpull_shapes_worker.py).  CPU tests, one per group, run every case up
to n = 100,000 (and the 400,000-node cap case) through the oracle alone and
assert that it can do what it is there for.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from test_gpu_parity import masked, random_table, sha
from test_pushpull import PP, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "pushpull_shapes_worker.py")
CAP = 60  # rounds, as test_gpu_pushpull_bit_exact

Data = namedtuple("Data", "kw deg ids failed bits sender stride")
Ref = namedtuple("Ref", "rows hashes crashed covered")


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def mask_bits(n, frac, seed, also=()):
    bits = np.random.default_rng(seed).random(n) < frac
    bits[list(also)] = True
    return bits


def live_sender(deg, bits, start):
    """The first live node with a non-empty row at or after `start`."""
    n = deg.size
    for k in range(n):
        v = (start + k) % n
        if deg[v] > 0 and not (bits is not None and bits[v]):
            return v
    raise AssertionError("no live caller")


# ---- the cases: key -> (parameters, table, mask, sender) --------------------------
# A. slot widths x modes x masks at n = 4,133 (two ranges, a ragged last word)
A_N = 4133
A_STRIDES = [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 32, 64, 255]
A_CONTROL = 8  # the stride <= 16 that also runs dense and top-down
A_FAIL = 0.03


def a_modes(s):
    return (("bottom", "answer", "auto") if s <= 16 else ()) + (("dense", "topdown") if s > 16 or s == A_CONTROL else ())


A_CASES = [(f"A-s{s}-{shape}{'-m' if m else ''}", mode)
           for s in A_STRIDES for shape in ("full", "ragged") for m in (False, True) for mode in a_modes(s)]


def build_a(s, shape, m):
    deg, ids = random_table(A_N, s, s if shape == "full" else 0, s, seed=(1000 if shape == "full" else 2000) + s)
    bits = mask_bits(A_N, A_FAIL, 3000 + s) if m else None
    # the sender: the live caller most rows name (rows of 0..1 friends form small trees)
    live = np.ones(A_N, bool) if bits is None else ~bits
    valid = np.arange(s)[None, :] < deg[:, None]
    indeg = np.bincount(ids[valid & live[:, None]], minlength=A_N)
    return dict(PP, n=A_N), deg, ids, bits, int(np.argmax(np.where(live & (deg > 0), indeg, -1)))


# B. sizes at, one below and one above each boundary that changes launch shape
# or indexing: one word, kPPU words per wave, kPPRange / one S1 summary word /
# one early-list segment, the fine bucket (kPPDTile), a second k_ppa_round
# workgroup and deferred list; then a second S2 summary word and a second
# coarse digit / coarse bin
B_BOUNDS = [64, 512, 4096, 16384, 65536]
B_SIZES = [b + d for b in B_BOUNDS for d in (-1, 0, 1)]
B_MODES = ("auto", "bottom", "answer", "early", "dense")
B_FAIL = 0.03
B_CASES = [(f"B-n{n}{'-m' if m else ''}", mode) for n in B_SIZES for m in (False, True) for mode in B_MODES]
B_S2, B_COARSE = 262144 + 1, (1 << 22) + 4133
# the oracle dominates these: one run per (table, mask).  The masks fail 0.5 %
# of the nodes, so that 99 % coverage ends the masked runs too.
B_LARGE_FAIL = 0.005
B_LARGE = [(f"B-n{B_S2}", "auto"), (f"B-n{B_S2}", "answer"), (f"B-n{B_S2}-m", "auto"),
           (f"B-n{B_COARSE}", "auto"), (f"B-n{B_COARSE}", "answer"), (f"B-n{B_COARSE}-m", "answer")]
B_L2 = [f"B-n{4097}", f"B-n{4097}-m", f"B-n{B_S2}"]


def build_b(n, m):
    deg, ids = random_table(n, 6, 5, 6, seed=n)
    # the last node (the last bit of a ragged last word) is failed in every mask
    bits = mask_bits(n, B_FAIL if n <= 65537 else B_LARGE_FAIL, 5000 + n % 1000, also=(n - 1,)) if m else None
    return dict(PP, n=n), deg, ids, bits, live_sender(deg, bits, n // 3) if m else -1


# C. the tables every switch configuration runs, in bottom-up and pull-answer rounds
C_TABLES = {"C-20000": (20000, 6, 5, 6, 0.0), "C-20000-m": (20000, 6, 5, 6, 0.03),
            "C-9000": (9000, 16, 1, 16, 0.0), "C-70001-m": (70001, 8, 5, 8, 0.02)}
C_CASES = [(k, mode) for k in C_TABLES for mode in ("bottom", "answer")]
C_CONFIGS = {
    "words0": {"GS_PPB_WORDS": "0"},
    "words1": {"GS_PPB_WORDS": "1"},
    "mixed-ranges": {"GS_PPA_WORD_MAXI": "8", "GS_PPB_WORD_MAXU": "8"},
    "pullfirst0": {"GS_PPB_PULLFIRST": "0"},
    "nodeg0": {"GS_PP_NODEG": "0"},
    "norfail": {"GS_PP_NORFAIL": "1"},
    "nodefer": {"GS_PP_NODEFER": "1"},
    "words0-nodefer": {"GS_PPB_WORDS": "0", "GS_PP_NODEFER": "1"},
    "control": {},
}


def build_c(key):
    n, s, dlo, dhi, frac = C_TABLES[key]
    deg, ids = random_table(n, s, dlo, dhi, seed=n + s)
    bits = mask_bits(n, frac, 6000 + s) if frac else None
    return dict(PP, n=n), deg, ids, bits, live_sender(deg, bits, n // 3)


# D. caps, hubs and row content
D_FAIL = 0.02
D_OVER_N, D_FCAP = 100_000, 16384          # PPSparse::fcap: targets a fine region holds
D_HUB_N, D_HUBS, D_HUB_FAIL = 20_000, {5: 64, 6: 65}, 0.03  # kRfailScan = 64: at the bound and one past it
D_HUB_FAILED_CALLERS = 20
D_ROW_N = 4133
D_DUP_FAIL = 0.15
D_BLOCK, D_BLOCK_NODE = range(1000, 1200), 77
# "answer-all": pull-answer rounds at every |I| (the bottom-up threshold is
# switched off for that broadcast): the default threshold, 96 n / 256, ends the
# pull-answer rounds before 2 * fcap / 0.9 nodes are informed
D_OVER_CASES = [(k, mode) for k in ("D-overflow", "D-overflow-m") for mode in ("answer", "answer-all", "bottom")]
D_FINE_N = 400_000  # 7 k_ppa_round workgroups: their lists hold 7 * dcap = 28,672 targets, past fcap
D_CASES = D_OVER_CASES + [("D-fine", "answer-all"), ("D-fine-m", "answer-all"), ("D-hub-m", "answer-all")] + \
          [(k, mode) for k in ("D-hub", "D-hub-m", "D-self", "D-self-m", "D-dup", "D-dup-m",
                                              "D-block", "D-block-m") for mode in ("answer", "bottom")]


def build_d(name, m):
    if name in ("overflow", "fine"):  # every friend in bucket 0: its fine region takes every push of a round
        n = D_OVER_N if name == "overflow" else D_FINE_N
        deg = np.full(n, 6, np.uint8)
        ids = np.random.default_rng(41).integers(0, 16384, size=(n, 6)).astype(np.uint32)
        bits = mask_bits(n, D_FAIL, 42) if m else None
        return dict(PP, n=n), deg, ids, bits, live_sender(deg, bits, 100)
    if name == "hub":
        n = D_HUB_N
        deg, ids = random_table(n, 6, 5, 6, seed=43)
        bits = mask_bits(n, D_HUB_FAIL, 44)  # the table's callers are chosen by it, masked or not
        for h in D_HUBS:  # no in-edge but the chosen ones
            ids[ids == h] = 1000 + h
        rng = np.random.default_rng(45)
        rows = np.arange(100, n)
        dead, alive = rows[bits[rows]], rows[~bits[rows]]
        rng.shuffle(dead)
        rng.shuffle(alive)
        for i, (h, k) in enumerate(D_HUBS.items()):
            callers = np.concatenate([dead[i * D_HUB_FAILED_CALLERS:(i + 1) * D_HUB_FAILED_CALLERS],
                                      alive[i * 100:i * 100 + k - D_HUB_FAILED_CALLERS]])
            ids[callers, rng.integers(0, 5, size=k)] = h  # slots 0..4: within every degree
        return dict(PP, n=n), deg, ids, bits if m else None, live_sender(deg, bits, n // 3)
    n = D_ROW_N
    deg, ids = random_table(n, 6, 5, 6, seed=46)
    if name == "self":  # every row's slot 0 is the node itself
        ids[:, 0] = np.arange(n)
        bits = mask_bits(n, D_FAIL, 47) if m else None
    elif name == "dup":  # slots 0 and 1 name one friend: two in-edges (v, 0), (v, 1) -> u
        ids[:, 1] = ids[:, 0]
        bits = mask_bits(n, D_DUP_FAIL, 48) if m else None
    else:  # a block of rows whose every slot names one node, failed in the masked variant
        ids[D_BLOCK.start:D_BLOCK.stop, :] = D_BLOCK_NODE
        bits = mask_bits(n, D_FAIL, 49, also=(D_BLOCK_NODE,)) if m else None
    return dict(PP, n=n), deg, ids, bits, live_sender(deg, bits, n // 3)


_DATA, _REFS, _TABLES = {}, {}, {}
LARGE = 100_000  # tables past this many rows are kept for one (table, masks) at a time


def base_of(key):
    return key[:-2] if key.endswith("-m") else key


def release(keep=None):
    """Drops the cached tables and oracle runs of the large cases (all cases
    with keep = "all"), but those of table `keep`."""
    for key in [k for k, d in _DATA.items() if (keep == "all" or d.kw["n"] > LARGE) and base_of(k) != keep]:
        del _DATA[key]
        _REFS.pop(key, None)
        _TABLES.pop(base_of(key), None)


def case_data(key):
    """The case's parameters, table, mask (words and bits) and sender, built
    once per process from the key alone (the child processes build them
    again).  A table's masked and unmasked variants share its arrays."""
    if key not in _DATA:
        g, _, rest = key.partition("-")
        m = rest.endswith("-m")
        rest = rest[:-2] if m else rest
        if g == "A":
            s, shape = rest.split("-")
            kw, deg, ids, bits, sender = build_a(int(s[1:]), shape, m)
        elif g == "B":
            kw, deg, ids, bits, sender = build_b(int(rest[1:]), m)
        elif g == "C":
            kw, deg, ids, bits, sender = build_c(key)
        else:
            kw, deg, ids, bits, sender = build_d(rest, m)
        if kw["n"] > LARGE:
            release(keep=base_of(key))
        if g != "C":  # (C's keys are tables of their own)
            tdeg, tids = _TABLES.setdefault(base_of(key), (deg, ids))
            assert np.array_equal(tdeg, deg) and np.array_equal(tids, ids), key
            deg, ids = tdeg, tids
        failed = words_of(bits) if bits is not None else None
        frozen(deg, ids, failed, bits)
        _DATA[key] = Data(kw, deg, ids, failed, bits, sender, ids.shape[1])
    return _DATA[key]


@pytest.fixture(scope="module", autouse=True)
def tables_freed():
    """Nothing of this module's tables stays behind for the rest of the suite."""
    yield
    release(keep="all")
    _DATA.clear()
    _REFS.clear()
    _TABLES.clear()


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def reference(oracle, key):
    """The oracle's run of a case, once: per round the stats row and the
    informed bitset's hash, until 99 % are informed, the sender is failed, or a
    round informs nobody new and no later round can (the exact stop test)."""
    if key not in _REFS:
        d = case_data(key)
        p = oracle.make_params(**d.kw)
        e = oracle.Engine(p, d.deg, d.ids)
        if d.failed is not None:
            e.set_failed(d.failed)
        e.begin(d.sender)
        rows, hashes, prev, cov = [], [], popcount(e.received()), False
        for _ in range(CAP):
            a = e.step(1)
            rows.append(a[0])
            hashes.append(sha(e.received()))
            recv = int(a[0, 4])
            cov = oracle.covered(recv, d.kw["n"])
            if cov or recv == 0:
                break
            if recv == prev and oracle.pp_stalled(p, d.deg, d.ids, e.received(), e.crashed()):
                break
            prev = recv
        _REFS[key] = Ref(frozen(np.array(rows, dtype=np.uint64))[0], hashes, frozen(e.crashed())[0], cov)
    return _REFS[key]


# ---- the GPU's side (also run by the worker) ----------------------------------------
def gpu_rounds(gs, key, mode, nrounds=None, l2_only=False):
    """One broadcast of a case in a fresh context, a round per step call.  Runs
    nrounds rounds, or (None) until 99 % are informed, at most CAP.  Returns
    JSON-able results: rows, informed hashes, the crashed hash, the counters."""
    d = case_data(key)
    kw, n = d.kw, d.kw["n"]
    cfg = gs.Config(n=n, fanout=kw["fanout"], fanin=kw["fanin"], delaylow=kw["delay_low"],
                    delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"],
                    seed=kw["seed"], trial=kw["trial"], model="pushpull", pp_l2_only=l2_only, timing=l2_only,
                    pp_rounds="answer" if mode == "answer-all" else mode)
    old = os.environ.get("GS_PP_BOTTOM256")
    if mode == "answer-all":
        os.environ["GS_PP_BOTTOM256"] = "256"  # read at broadcast_begin
    try:
        with gs.Simulator(cfg) as sim:
            sim.load_peers(d.deg, d.ids)
            if d.failed is not None:
                sim.set_failed(d.failed)
            sim.broadcast_begin(d.sender)
            prep = sim.timing()["prep_ms"] > 0
            rows, hashes = [], []
            for _ in range(CAP if nrounds is None else nrounds):
                b = sim.step(1)
                rows.append([int(x) for x in b[0]])
                hashes.append(sha(sim.received()))
                if nrounds is None and (gs.covered(rows[-1][4], n) or rows[-1][4] == 0):
                    break
            tm = sim.timing()
            return dict(key=key, mode=mode, rows=rows, hashes=hashes, crashed=sha(sim.crashed()), prep=prep,
                        early=int(tm["pp_early_rounds"]), bottom=int(tm["pp_bottom_rounds"]),
                        answer=int(tm["pp_answer_rounds"]), rev_part=int(tm["pp_rev_part"]))
    finally:
        if mode == "answer-all":
            if old is None:
                del os.environ["GS_PP_BOTTOM256"]
            else:
                os.environ["GS_PP_BOTTOM256"] = old


def check(ref, got):
    """got (gpu_rounds' result) against the oracle's run, and the mode counters
    as test_gpu_pushpull_bit_exact asserts them."""
    key, mode = got["key"], got["mode"]
    d = case_data(key)
    assert len(got["rows"]) >= len(ref.rows), f"{key} {mode}: {len(got['rows'])} rounds, the oracle ran {len(ref.rows)}"
    for r, want in enumerate(ref.rows):
        assert [int(x) for x in want] == got["rows"][r], f"{key} {mode} round {r + 1}:\n{want}\n{got['rows'][r]}"
        assert ref.hashes[r] == got["hashes"][r], f"{key} {mode}: informed set differs at round {r + 1}"
    assert got["crashed"] == sha(ref.crashed), f"{key} {mode}: crashed differs"
    assert got["crashed"] == sha(d.failed if d.failed is not None else np.zeros((d.kw["n"] + 63) // 64, np.uint64))
    # bottom-up and pull-answer need packed slot bytes (stride <= 16) and, with
    # failed nodes, the failed-slot mask (stride <= 8)
    can_bottom = d.stride <= 16 and (d.failed is None or d.stride <= 8)
    dense = len(got["rows"]) - got["early"]
    assert got["prep"] == (mode != "dense")  # the reverse table is built at begin unless dense-only
    if mode in ("dense", "topdown") or not can_bottom:
        assert got["bottom"] == 0 and got["answer"] == 0, got
    elif mode == "bottom":
        assert got["bottom"] == dense and got["answer"] == 0, got
    elif mode == "answer":
        assert got["answer"] + got["bottom"] == dense, got
    elif mode == "answer-all":
        assert got["answer"] == dense and got["bottom"] == 0, got
    if mode == "early":
        assert got["early"] >= 1, got
    if mode != "dense" and d.kw["n"] > 100 and not key.startswith("D-"):
        assert got["rev_part"] >= 1, got  # the reverse table came from the edge partition (D: skew may refuse it)


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def ids_of(cases):
    return [f"{k}-{m}" for k, m in cases]


@pytest.mark.gpu
@pytest.mark.parametrize("key,mode", A_CASES, ids=ids_of(A_CASES))
def test_slot_widths(gs, oracle, key, mode):
    """A. Every packed slot width (j | (d-1) << 4 decoded in ppa_resolve,
    ppb_resolve, k_pp_rfail), the 8 -> 9 step where the failed-slot mask stops
    existing, the 16 -> 17 step to dense-only rounds; full rows (lane-per-word
    ranges) and rows of 0..stride friends (nlive0 > 0: the lane-per-node loop,
    with the mask too)."""
    ref = reference(oracle, key)
    check(ref, gpu_rounds(gs, key, mode, len(ref.rows)))


@pytest.mark.gpu
@pytest.mark.parametrize("key,mode", B_CASES, ids=ids_of(B_CASES))
def test_region_boundaries(gs, oracle, key, mode):
    """B. n at, below and above 64, 512, 4,096, 16,384 and 65,536."""
    ref = reference(oracle, key)
    check(ref, gpu_rounds(gs, key, mode, len(ref.rows)))


@pytest.mark.gpu
@pytest.mark.parametrize("key,mode", B_LARGE, ids=ids_of(B_LARGE))
def test_region_boundaries_large(gs, oracle, key, mode):
    """B. A second S2 summary word (n = 262,145) and a second coarse digit of
    the deferred sets' partition / coarse bin of the reverse table's
    (n = 2^22 + 4,133: several lists into several coarse regions)."""
    ref = reference(oracle, key)
    assert ref.covered
    check(ref, gpu_rounds(gs, key, mode, len(ref.rows)))


@pytest.mark.gpu
@pytest.mark.parametrize("key", B_L2, ids=B_L2)
def test_region_boundaries_l2_only(gs, oracle, key):
    """B. The dense rounds without the LDS summary level past one S1 word and
    past one S2 word."""
    ref = reference(oracle, key)
    for mode in ("dense", "auto"):
        check(ref, gpu_rounds(gs, key, mode, len(ref.rows), l2_only=True))


@pytest.mark.gpu
@pytest.mark.parametrize("key,mode", D_CASES, ids=ids_of(D_CASES))
def test_caps_hubs_and_rows(gs, oracle, key, mode):
    """D. A fine region of the deferred sets past its cap; in-lists of 64 and 65
    entries with failed callers (k_pp_rfail's scan bound); a self-friend in a
    drawn slot, one friend in two slots, rows naming one failed node only."""
    ref = reference(oracle, key)
    check(ref, gpu_rounds(gs, key, mode, len(ref.rows)))


def child_cases(name):
    return C_CASES + (D_OVER_CASES if name == "words0" else [])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C_CONFIGS))
def test_switches_in_a_fresh_process(gs, oracle, name):
    """C. The process-wide switches (read once): a child process sets them,
    runs the cases per round and prints one JSON line, compared here with the
    oracle.  GS_PP_NORFAIL and GS_PP_NODEFER are also what runs after a failed
    allocation of pp_rfail / pp_dset.  The control child (no switch) must also
    equal this process's own run of the same cases."""
    cases = child_cases(name)
    arg = json.dumps({"env": C_CONFIGS[name], "cases": cases})
    r = subprocess.run([sys.executable, WORKER, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["env"] == C_CONFIGS[name]
    assert [(g["key"], g["mode"]) for g in out["results"]] == [tuple(c) for c in cases]
    for got in out["results"]:
        check(reference(oracle, got["key"]), got)
        if name == "control":
            assert got == gpu_rounds(gs, got["key"], got["mode"]), (got["key"], got["mode"])


# ---- E. non-vacuity, on the CPU -----------------------------------------------------
# Every case of A to D up to n = 100,000 through the oracle alone (and D-fine,
# n = 400,000, whose oracle run takes 0.1 s), one test per group.
def spreads(oracle, key):
    """What every case must do: a live sender, the mask as the crashed set, a
    broadcast that informs more than one node and, unmasked on a connected
    table, 99 % of them within the cap."""
    d, ref = case_data(key), reference(oracle, key)
    n = d.kw["n"]
    live = np.ones(n, bool) if d.bits is None else ~d.bits
    assert d.ids.shape[1] == d.stride and int(d.deg.max()) <= d.stride, key
    assert live[d.sender if d.sender >= 0 else oracle.pick_sender(oracle.make_params(**d.kw))], key
    assert np.array_equal(ref.crashed, d.failed if d.failed is not None else np.zeros((n + 63) // 64, np.uint64)), key
    assert int(ref.rows[-1][4]) > 1, (key, ref.rows[-1])
    assert (ref.rows[:, 6] == ref.rows[:, 4]).all() and (ref.rows[:, 5] == 0).all(), key
    if d.bits is not None:
        assert d.bits.any() and int(ref.rows[-1][4]) <= int(live.sum()), key
    # a random k-out graph is connected for k >= 2: unmasked, such a table is covered within the cap
    if d.bits is None and int(d.deg.min()) >= 2:
        assert ref.covered, (key, len(ref.rows), ref.rows[-1])


def informed_at_round_starts(oracle, key):
    """The informed set (a bool per node) at the start of every round of the
    case's oracle run."""
    d = case_data(key)
    e = oracle.Engine(oracle.make_params(**d.kw), d.deg, d.ids)
    if d.failed is not None:
        e.set_failed(d.failed)
    e.begin(d.sender)
    for _ in range(len(reference(oracle, key).rows)):
        yield np.unpackbits(e.received().view(np.uint8), bitorder="little")[:d.kw["n"]].astype(bool)
        e.step(1)


def keep_rate(oracle):
    return 1.0 - oracle.threshold(PP["drop_rate"]) / 100.0


def test_a_cases_can_do_what_they_are_for(oracle):
    """A: rows of 0..stride friends leave live nodes that never call
    (nlive0 > 0); full rows leave none; the widest row uses its last slot."""
    for key in sorted({k for k, _ in A_CASES}):
        spreads(oracle, key)
        d = case_data(key)
        live = np.ones(A_N, bool) if d.bits is None else ~d.bits
        assert int(d.deg.max()) == d.stride, key
        if "-ragged" in key:
            assert (d.deg[live] == 0).any(), key
        else:
            assert (d.deg[live] > 0).all(), key
        if d.bits is not None:
            assert int(d.bits.sum()) >= A_N // 50, key
    assert A_N > 4096 and A_N % 64  # two ranges, a ragged last word
    assert {s for s in A_STRIDES if s <= 16} >= {1, 8, 9, 16} and min(s for s in A_STRIDES if s > 16) == 17


def test_b_cases_can_do_what_they_are_for(oracle):
    """B: the sizes sit on the boundaries; every mask fails the last node."""
    for key in sorted({k for k, _ in B_CASES}):
        spreads(oracle, key)
    assert sorted(B_SIZES) == sorted(b + d for b in (64, 8 * 64, 64 * 64, 16384, 16 * 64 * 64) for d in (-1, 0, 1))
    assert B_S2 == 64 * 64 * 64 + 1 and B_COARSE > 1 << 22
    for n in B_SIZES:
        assert case_data(f"B-n{n}-m").bits[n - 1]
    for n in (B_S2, B_COARSE):  # at each large size: auto and answer, one of them masked
        modes = {(k.endswith("-m"), mode) for k, mode in B_LARGE if base_of(k) == f"B-n{n}"}
        assert {mode for _, mode in modes} == {"auto", "answer"} and {m for m, _ in modes} == {False, True}


def test_c_cases_can_do_what_they_are_for(oracle):
    """C: a second k_ppa_round workgroup (16 waves of one 64-word range each)
    at 70,001; the widest packed rows at 9,000, in more than two ranges."""
    for key in C_TABLES:
        spreads(oracle, key)
    assert (70001 + 4095) // 4096 > 16 and 9000 > 2 * 4096
    assert int(case_data("C-9000").deg.max()) == 16 and int(case_data("C-9000").deg.min()) == 1
    assert len(C_CONFIGS) == 9 and C_CONFIGS["control"] == {}


def test_d_cap_cases_can_do_what_they_are_for(oracle):
    """D, overflow: some round starts with 2 * fcap / (1 - drop) informed live
    nodes; every friend lies in bucket 0, so the expected kept pushes into that
    fine region are then twice its cap.  But at n = 100,000 k_ppa_round has two
    workgroups, whose lists pass on 2 * dcap = 8,192 targets a round (the rest
    are atomicOr at once): the lists and the coarse regions overflow there, the
    fine region cannot.  D-fine: 7 workgroups, 28,672 listed targets <= the
    8 x ccap = 32,768 of coarse bin 0, all of bucket 0, in a round that starts
    with 1.25 times as many kept pushes (the informed nodes spread over the
    workgroups evenly: every list fills) and with at least 1,000 uninformed
    live nodes left in bucket 0."""
    keep = keep_rate(oracle)
    for key in ("D-overflow", "D-overflow-m"):
        spreads(oracle, key)
        d, ref = case_data(key), reference(oracle, key)
        assert int(d.ids.max()) < 16384 and (d.deg == 6).all()
        starts = [int(x) for x in ref.rows[:-1, 4]]  # informed (all live) at the start of rounds 2..
        assert max(starts) * keep >= 2 * D_FCAP, (key, starts)

    def wgs(n):  # ranges of 4,096 nodes, 16 waves per workgroup
        return -(-(-(-n // 4096)) // 16)

    dcap = ccap = 4096  # max(4096, 0.6 n / 512) and max(4096, 0.6 n / 2048) at these n
    assert wgs(D_OVER_N) * dcap < D_FCAP < wgs(D_FINE_N) * dcap <= 8 * ccap and 0.6 * D_FINE_N / 512 <= 4096
    for key in ("D-fine", "D-fine-m"):
        spreads(oracle, key)
        d = case_data(key)
        assert int(d.ids.max()) < 16384 and (d.deg == 6).all()
        live0 = np.ones(16384, bool) if d.bits is None else ~d.bits[:16384]
        assert any(int(rec.sum()) * keep >= 1.25 * wgs(D_FINE_N) * dcap and int((live0 & ~rec[:16384]).sum()) >= 1000
                   for rec in informed_at_round_starts(oracle, key)), key


def test_d_hub_cases_can_do_what_they_are_for(oracle):
    """D, hub: in-degrees 64 and 65 exactly, each hub with 20 failed callers;
    and with pull-answer rounds to the end ("answer-all"), each hub, once
    informed, is picked by a failed caller whose call is kept at least 3 times:
    only then does the answer test read that in-edge's failed-caller bit."""
    bits = case_data("D-hub-m").bits
    for key in ("D-hub", "D-hub-m"):
        spreads(oracle, key)
        d = case_data(key)
        valid = masked(d.deg, d.ids + 1) - 1  # empty slots: 0xFFFFFFFF
        for h, k in D_HUBS.items():
            callers = np.nonzero((valid == h).any(axis=1))[0]
            assert int((valid == h).sum()) == k == callers.size, (key, h)
            assert int(bits[callers].sum()) == D_HUB_FAILED_CALLERS and not bits[h], (key, h)
    assert sorted(D_HUBS.values()) == [64, 65]
    d = case_data("D-hub-m")
    p = oracle.make_params(**d.kw)
    pkey = [int(p.seed) & 0xFFFFFFFF, int(p.seed) >> 32]
    kd = oracle.threshold(p.drop_rate)
    # the hubs' in-edges (v, j) whose caller v is failed
    edges = {h: [(int(v), int(j)) for v, j in zip(*np.nonzero(d.ids == h)) if bits[v] and j < d.deg[v]] for h in D_HUBS}
    events = dict.fromkeys(D_HUBS, 0)
    for t, rec in enumerate(informed_at_round_starts(oracle, "D-hub-m"), start=1):
        if int(rec.sum()) <= D_HUB_N >> 8:
            continue  # a sparse early round: it gathers the caller's failed word
        for h in D_HUBS:
            for v, j in edges[h] if rec[h] else ():
                r = oracle.philox([v, t, 0, (9 << 24) | int(p.trial)], pkey)  # v's draw of round t
                picked, kept = ((r[0] * int(d.deg[v])) >> 32) == j, ((r[1] * 100) >> 32) >= kd
                events[h] += picked and kept
    assert min(events.values()) >= 3, events


def test_d_row_cases_can_do_what_they_are_for(oracle):
    """D, rows: the self slot and the duplicated slot are drawn (within every
    degree); at least 100 failed callers have a duplicated friend, and at least
    100 live callers a failed one; the block's node is failed and its callers
    are (mostly) live."""
    for key in ("D-self", "D-self-m", "D-dup", "D-dup-m", "D-block", "D-block-m"):
        spreads(oracle, key)
    d = case_data("D-self-m")
    assert (d.ids[:, 0] == np.arange(D_ROW_N)).all() and int(d.deg.min()) >= 2
    d = case_data("D-dup-m")
    assert (d.ids[:, 0] == d.ids[:, 1]).all() and int(d.deg.min()) >= 2
    assert int(d.bits.sum()) >= 100 and int((~d.bits & d.bits[d.ids[:, 0]]).sum()) >= 100
    d = case_data("D-block-m")
    blk = np.arange(D_BLOCK.start, D_BLOCK.stop)
    assert (d.ids[blk] == D_BLOCK_NODE).all() and d.bits[D_BLOCK_NODE] and int((~d.bits[blk]).sum()) >= 150
    assert case_data("D-block").bits is None


def test_every_case_has_its_cpu_conditions():
    keys = {k for k, _ in A_CASES + B_CASES + C_CASES + D_CASES}
    assert {k for k in keys if k.startswith("D-")} == {
        f"D-{t}{m}" for t in ("overflow", "fine", "hub", "self", "dup", "block") for m in ("", "-m")}
    assert {k for k in keys if k.startswith("C-")} == set(C_TABLES)
