"""Table-entry sweep: every way a peer table gets into a context, what the
loads refuse, and the state a refusal leaves.

The engines' parity sweeps all enter their table through gs_load_peers from
host arrays on the context's own stream.  Here the same engines -- the flood
window engine, the flood tick engine, push-pull, rumor mode 0, rumor pull,
median and a rumor set of 64 -- take their table from device memory
(gs_load_peers_device), from an overlay another context built (gs_read_peers
-> device load) and on a stream the caller owns (gs_set_stream), and every
round (stats row, received set, and the engine's extra sets) is bit-exact
against the reference the suite already has for that engine: oracle.Engine
(flood, push-pull), PyRumor, PyRumorModes, PyMedian and PyRumorSet, which
always get masked(deg, ids).

Families (GPU tests are marked gpu; the unmarked *_worth_running tests run the
references alone and assert that the cases can show what they are there for):

A  entry matrix: engine x {host load, device load, overlay -> read_peers ->
   device load into a fresh context}; row shapes through the device call on
   the window engine and push-pull; stride 33 on the tick engine; a rank of
   one (the c->shard branch of the device load).
B  slots past a row's length hold 0xFFFFFFFF, or n and 2^31.  Safe to run
   because no engine follows such a slot -- read in the kernels:
   * window engine: k_expand reads whole rows without the length byte and
     relies on the seal -- seal_rows runs k_seal_rows (gs_win_expand.hip) on
     the context's copy after either load and sets slots j >= deg to
     0xFFFFFFFF, which expand skips; shards copy the sealed rows (own_rows).
   * tick engine (gs_broadcast.hip): `if (j >= st.deg[v]) continue` before the
     row read.
   * push-pull rounds (gs_pp_round.hip, gs_pp_early.hip, gs_pp_dense.hip), the
     rumor engines (gs_rumor.hip), median (gs_median.hip) and the rumor set
     (gs_rumorset.hip): the one slot read is j = uniform(r, deg) < deg, and a
     row with deg 0 makes no call.
   * push-pull's reverse table and failed-slot mask (gs_pp_rev.hip,
     gs_pp_fmask.hip): `for (j = 0; j < deg; ++j)`.
   * batched trials: upload_table copies slots j < deg only.
   gs_read_peers returns the loaded ids in used slots; in unused slots the
   window engine returns 0xFFFFFFFF (sealed), the others what was loaded.
C  refusals: a length above the stride, a used slot >= n, both; through both
   calls on a one-device context, a batched-trials context, [0, 0] shard groups
   (flood, push-pull) and a [0, 0] trials group; the stride limits and the
   other argument refusals.  A shard group needs n > 16384 (each shard holds
   whole 16384-node buckets), so the groups' cases run at n = 16385 and 20517
   in place of 1, 257 and 4133.
D  after a refused load or a GS_ELIVELOCK overlay build the context has no
   table: broadcast_begin and read_peers refuse until the next good load, and
   that load's broadcast is bit-exact.  (Before the fix the stale `peers` flag
   let broadcast_begin through with the refused table in device memory; the
   test stops at that assertion and never steps such a context.)
E  caller-owned stream: set_stream(s), load, masked rounds, set_stream(None)
   between two steps, the rest, reset, the same broadcast on the own stream.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import pytest

import devbuf
from test_gpu_parity import masked
from test_median import MEDIAN, PyMedian
from test_pushpull import PP
from test_rumor import RUMOR, PyRumor, words_of
from test_rumor_modes import PULL, PyRumorModes
from test_rumorset import RS, PyRumorSet

N = 4133          # a ragged last word, several blocks
ROUNDS = 30       # rounds compared (flood: ticks, see FLOOD)
FLOOD_TICKS = 40
R = 64            # rumors of the rumor set
FFFF = 0xFFFFFFFF
GROUP_N = 16384 + N   # the smallest shapes a [0, 0] shard group takes: two ranges, the second ragged

# delays of 2..3 ticks: a window of two ticks, and 40 ticks are a dozen hops
FLOOD = dict(fanout=5, fanin=6, delay_low=2, delay_high=4, drop_rate=0.1, crash_rate=0.0, seed=0x5EED, trial=0,
             model=0)
ENGINES = ["window", "tick", "pushpull", "rumor0", "rumorpull", "median", "rumorset"]
KW = {"window": FLOOD, "tick": FLOOD, "pushpull": PP, "rumor0": RUMOR, "rumorpull": RUMOR, "median": MEDIAN,
      "rumorset": RS}
RUMOR_K = {"rumor0": 3, "rumorpull": 2, "median": 2}
MSG_LEN = "a friends-list length exceeds the row stride"
MSG_ID = "a friend id is >= n"
MSG_BEGIN = "load peers or build the overlay first"
MSG_READ = "no peer table"

Round = namedtuple("Round", "row recv extra")


def rounds_of(eng):
    return FLOOD_TICKS if eng in ("window", "tick") else ROUNDS


# ---- tables ------------------------------------------------------------------------
def make_table(n, stride, seed, dmin=None, dmax=None):
    """Mostly rows of dmax (default: the stride) friends, so the message spreads;
    one row in seven has a length drawn from dmin (default 0) .. dmax, and rows
    with deg 0 and deg dmax are there whatever the draw."""
    rng = np.random.default_rng(seed)
    dmax = stride if dmax is None else dmax
    dmin = 0 if dmin is None else dmin
    deg = np.full(n, dmax, np.uint8)
    odd = rng.random(n) < 1 / 7
    deg[odd] = rng.integers(dmin, dmax + 1, size=int(odd.sum()))
    ids = rng.integers(0, n, size=(n, stride)).astype(np.uint32)
    if n >= 4:
        deg[n // 3] = 0
        deg[n - 1] = 0            # an empty last row
        deg[n // 2] = dmax
        deg[0] = dmax
    return deg, ids


def sender_of(deg, failed=None):
    """A live node with a full row near the middle."""
    n = deg.size
    for v in list(range(n // 2, n)) + list(range(n // 2)):
        if deg[v] == deg.max() and not (failed is not None and failed[v]):
            return v
    raise AssertionError("no sender")


def senders_of(n):
    s = [(j * n) // R for j in range(R)]
    s[-1] = n - 1
    return s


def mask_of(n, seed, keep=()):
    dead = np.random.default_rng(seed).random(n) < 0.05
    dead[n - 3:] = True          # failed nodes in the ragged last word
    dead[list(keep)] = False
    return dead


SHAPES = {  # key -> (stride, dmin, dmax)
    "s2": (2, 0, 2), "s6": (6, 0, 6), "s8-rows6": (8, 0, 6), "s8-rows7-8": (8, 7, 8), "s19": (19, 0, 19),
    "s32": (32, 0, 32), "s33": (33, 0, 33),
}
_TABLES = {}


def shape_table(key, n=N):
    if (key, n) not in _TABLES:
        stride, dmin, dmax = SHAPES[key]
        # (rows of two slots: a seed whose sender's friends do not both end the flood at once)
        seed = 0 if key == "s2" else 1000 + stride * 10 + dmax + n
        deg, ids = make_table(n, stride, seed=seed, dmin=dmin, dmax=dmax)
        if key == "s8-rows7-8":       # rows of 7 and 8 only, but for the empty ones make_table plants
            assert set(np.unique(deg)) == {0, 7, 8}
        deg.flags.writeable = ids.flags.writeable = False
        _TABLES[(key, n)] = (deg, ids)
    return _TABLES[(key, n)]


def overlay_table(oracle, eng, fanout=5, fanin=6, n=N):
    """The overlay of the engine's parameters: what every context of that key
    and those delays builds (test_gpu_parity pins the GPU overlay to the oracle's)."""
    kw = dict(KW[eng], n=n, fanout=fanout, fanin=fanin, model=0)
    k = ("overlay", kw["delay_low"], kw["delay_high"], fanout, fanin, n)
    if k not in _TABLES:
        deg, ids, _, _ = oracle.overlay(oracle.make_params(**kw))
        deg.flags.writeable = ids.flags.writeable = False
        _TABLES[k] = (deg, ids)
    return _TABLES[k]


def poisoned(deg, ids, values, seed=7):
    """ids with every slot at index >= deg holding one of `values`."""
    rng = np.random.default_rng(seed)
    unused = np.arange(ids.shape[1])[None, :] >= deg[:, None]
    fill = np.asarray(values, dtype=np.uint32)[rng.integers(0, len(values), size=ids.shape)]
    return np.where(unused, fill, ids).astype(np.uint32)


POISON = {"ffff": (FFFF,), "n-2^31": None}   # None: (n, 2^31), n known at the call


def poison_values(name, n):
    return POISON[name] or (n, 1 << 31)


# ---- the references ----------------------------------------------------------------
_REFS = {}


# the flood over rows of two slots: without loss and with delays of 1..2 ticks,
# or its 40 ticks end before half the nodes are reached
OVER = {("window", "s2"): dict(drop_rate=0.0, delay_low=1, delay_high=3)}


def reference(oracle, eng, tkey, deg, ids, sender, failed=None, rounds=None, trial=0, fanout=None, fanin=None):
    """The engine's reference over masked(deg, ids), once per key: a Round per
    round.  sender: a node, or (rumor set) the list of senders."""
    key = (eng, tkey, None if failed is None else failed.tobytes(), rounds, trial,
           tuple(sender) if isinstance(sender, list) else sender)
    if key in _REFS:
        return _REFS[key]
    n, mids, rounds = deg.size, masked(deg, ids), rounds or rounds_of(eng)
    kw = dict(KW[eng], n=n, trial=trial, **OVER.get((eng, tkey), {}))
    if fanout:
        kw.update(fanout=fanout, fanin=fanin)
    p = oracle.make_params(**kw)
    out = []
    if eng in ("window", "tick", "pushpull"):
        e = oracle.Engine(p, deg, mids)
        if failed is not None:
            e.set_failed(words_of(failed))
        e.begin(sender)
        for _ in range(rounds):
            a = e.step(1)
            out.append(Round([int(x) for x in a[0]], e.received(), {}))
    elif eng == "rumorset":
        e = PyRumorSet(oracle, p, deg, mids, sender, failed)
        for _ in range(rounds):
            row = e.step()
            e.poll()
            out.append(Round(row, words_of(e.holds_all), {"words": e.have.copy()}))
    else:
        k = RUMOR_K[eng]
        e = {"rumor0": lambda: PyRumor(oracle, p, deg, mids, sender, k, failed),
             "rumorpull": lambda: PyRumorModes(oracle, p, deg, mids, sender, k, failed, PULL),
             "median": lambda: PyMedian(oracle, p, deg, mids, sender, k, failed)}[eng]()
        for _ in range(rounds):
            row = e.step()
            extra = {"removed": words_of(e.removed)}
            if eng == "median":
                extra["state"] = e.st.copy()
            out.append(Round(row, words_of(e.inf), extra))
    _REFS[key] = out
    return out


def informed(rnd, n):
    return np.unpackbits(rnd.recv.view(np.uint8), bitorder="little")[:n].astype(bool)


def spreads(ref, eng, n, failed=None):
    """More than n/2 nodes within the rounds compared (a rumor set: of every
    rumor's n), and no failed node among them."""
    got = ref[-1].row[4]
    assert got > (R if eng == "rumorset" else 1) * n // 2, (eng, got)
    if failed is not None:
        assert not (informed(ref[-1], n) & failed).any()
        if eng == "rumorset":
            assert not ref[-1].extra["words"][failed].any()


# ---- the GPU's side ------------------------------------------------------------------
@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def config(gs, eng, n, fanout=None, fanin=None, trials=1, tkey=None):
    kw = dict(KW[eng], **OVER.get((eng, tkey), {}))
    more = dict(trials=trials)
    if eng in ("window", "tick"):
        more.update(model="flood", engine=eng)
    elif eng in ("pushpull", "rumorset"):
        more.update(model="pushpull")
    elif eng == "median":
        more.update(model="median", rumor_k=RUMOR_K[eng])
    else:
        more.update(model="rumor", rumor_k=RUMOR_K[eng], rumor_pull=eng == "rumorpull")
    return gs.Config(n=n, fanout=fanout or kw["fanout"], fanin=fanin or kw["fanin"], delaylow=kw["delay_low"],
                     delayhigh=kw["delay_high"], droprate=kw["drop_rate"], crashrate=kw["crash_rate"], seed=kw["seed"],
                     trial=kw["trial"], **more)


def make_sim(gs, eng, n, **kw):
    cfg = config(gs, eng, n, **kw)
    return gs.Simulator.rumor_set(cfg, R) if eng == "rumorset" else gs.Simulator(cfg)


def begin(sim, eng, sender):
    if eng == "rumorset":
        sim.begin_rumors(sender)
    else:
        sim.broadcast_begin(sender)


def check_state(sim, eng, rnd, t):
    assert np.array_equal(sim.received(), rnd.recv), f"{eng}: received set differs at round {t}"
    if "removed" in rnd.extra:
        assert np.array_equal(sim.removed(), rnd.extra["removed"]), f"{eng}: removed set differs at round {t}"
    if "state" in rnd.extra:
        assert np.array_equal(sim.median_state(), rnd.extra["state"]), f"{eng}: state bytes differ at round {t}"
    if "words" in rnd.extra:
        assert np.array_equal(sim.rumor_words(), rnd.extra["words"]), f"{eng}: rumor words differ at round {t}"


def step_check(sim, eng, ref, t0, k=1):
    """k rounds in one gs_step call from round t0 (0-based): every row, and the
    sets after the last."""
    rows = sim.step(k)
    for i in range(k):
        assert [int(x) for x in rows[i]] == ref[t0 + i].row, \
            f"{eng} round {t0 + i + 1}:\n{[int(x) for x in rows[i]]}\n{ref[t0 + i].row}"
    check_state(sim, eng, ref[t0 + k - 1], t0 + k)
    return t0 + k


def run_check(sim, eng, ref, sender, also=None):
    """begin, then gs_step(1) per round against ref (and, round for round, the
    context `also` that runs the same broadcast)."""
    begin(sim, eng, sender)
    if also is not None:
        begin(also, eng, sender)
    for t in range(len(ref)):
        if also is not None:
            got = [int(x) for x in also.step(1)[0]]
            assert got == ref[t].row, f"{eng}: the overlay's own context, round {t + 1}"
            check_state(also, eng, ref[t], t + 1)
        step_check(sim, eng, ref, t)


def load(sim, how, deg, ids):
    if how == "host":
        sim.load_peers(deg, ids)
    else:
        with devbuf.device_copy(deg, ids) as (d_deg, d_ids):
            sim.load_peers_device(d_deg, d_ids, ids.shape[1])   # copied: the buffers may go


def refused(gs, call, msg, code=-1):
    with pytest.raises(gs.GossipError) as ei:
        call()
    assert ei.value.code == code and msg in str(ei.value), str(ei.value)


# ==== A. entry matrix =================================================================
def a_case(oracle, eng, tkey="s6"):
    deg, ids = shape_table(tkey)
    sender = senders_of(N) if eng == "rumorset" else sender_of(deg)
    return deg, ids, sender, reference(oracle, eng, tkey, deg, ids, sender)


A_SHAPES = [(e, k) for e in ("window", "pushpull") for k in ("s2", "s6", "s8-rows6", "s8-rows7-8", "s19", "s32")] + \
    [("tick", "s33")]
OVERLAYS = [(e, 5, 6) for e in ENGINES] + [("window", 18, 19)]   # (rows of 6 padded to 8; of 19 to 20)


def overlay_case(oracle, eng, fo, fi):
    deg, ids = overlay_table(oracle, eng, fo, fi)
    sender = senders_of(N) if eng == "rumorset" else sender_of(deg)
    tkey = ("overlay", KW[eng]["delay_low"], fo, fi)
    return deg, ids, sender, reference(oracle, eng, tkey, deg, ids, sender, fanout=fo, fanin=fi)


def test_a_cases_are_worth_running(oracle):
    for eng in ENGINES:
        deg, ids, sender, ref = a_case(oracle, eng)
        assert deg.min() == 0 and deg.max() == ids.shape[1]
        spreads(ref, eng, N)
    for eng, tkey in A_SHAPES:
        deg, ids, sender, ref = a_case(oracle, eng, tkey)
        assert deg.min() == 0 and deg.max() == SHAPES[tkey][2] and ids.shape[1] == SHAPES[tkey][0]
        spreads(ref, eng, N)
    for eng, fo, fi in OVERLAYS:
        deg, ids, sender, ref = overlay_case(oracle, eng, fo, fi)
        assert ids.shape[1] == fi and fo <= deg.min() and deg.max() == fi   # read_peers' unpadded stride
        spreads(ref, eng, N)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("eng", ENGINES)
def test_entry_by_load(gs, oracle, eng, how):
    deg, ids, sender, ref = a_case(oracle, eng)
    with make_sim(gs, eng, N) as sim:
        load(sim, how, deg, ids)
        run_check(sim, eng, ref, sender)


@pytest.mark.gpu
@pytest.mark.parametrize("eng,fo,fi", OVERLAYS, ids=[f"{e}-{fi}" for e, fo, fi in OVERLAYS])
def test_entry_by_overlay_then_device_load(gs, oracle, eng, fo, fi):
    """build_overlay -> read_peers -> device load into a fresh context of the
    same key: read_peers hands back the unpadded rows (the window engine's table
    has 8, or 20, slots a row), and the loaded copy runs as the built one."""
    deg, ids, sender, ref = overlay_case(oracle, eng, fo, fi)
    with make_sim(gs, eng, N, fanout=fo, fanin=fi) as built, make_sim(gs, eng, N, fanout=fo, fanin=fi) as fresh:
        built.build_overlay()
        gdeg, gids = built.read_peers()
        assert gids.shape == (N, fi) and np.array_equal(gdeg, deg)
        assert np.array_equal(masked(gdeg, gids), masked(deg, ids))
        load(fresh, "device", gdeg, gids)
        fdeg, fids = fresh.read_peers()
        assert np.array_equal(fdeg, gdeg) and np.array_equal(masked(fdeg, fids), masked(gdeg, gids))
        run_check(fresh, eng, ref, sender, also=built)


@pytest.mark.gpu
@pytest.mark.parametrize("eng,tkey", A_SHAPES, ids=[f"{e}-{k}" for e, k in A_SHAPES])
def test_row_shapes_by_device_load(gs, oracle, eng, tkey):
    """The device call's minimum stride, the strides at which the window
    engine's row gather changes (uint2 loads, uint4 + uint2 / uint4 at 8, uint4
    at multiples of 4, scalar at 19), push-pull's packed slot bytes (<= 16) and
    failed-slot mask (<= 8), and 33 slots on the tick engine.  (A loaded
    stride-8 table is read in place whatever its rows' lengths: the packed view
    is built for overlay tables of 5..6 slots, which the overlay entry runs.)"""
    deg, ids, sender, ref = a_case(oracle, eng, tkey)
    with make_sim(gs, eng, N, tkey=tkey) as sim:
        load(sim, "device", deg, ids)
        rdeg, rids = sim.read_peers()
        assert np.array_equal(rdeg, deg) and np.array_equal(masked(rdeg, rids), masked(deg, ids))
        run_check(sim, eng, ref, sender)


@pytest.mark.gpu
def test_rank_of_one_takes_a_device_table(gs, oracle):
    """is_rank(c) with c->shard: gs_load_peers_device validates and seals the
    full table, then partition_from(c, {c}) keeps the rank's rows ([0, n) here)."""
    from gossip_simulator_amd import engine
    deg, ids, sender, ref = a_case(oracle, "window")
    sim = gs.Simulator.rank(config(gs, "window", N), 1, 0, engine.comm_unique_id())
    try:
        load(sim, "device", deg, ids)
        refused(gs, sim.read_peers, "a sharded context keeps only its partition of the table")
        run_check(sim, "window", ref, sender)
    finally:
        sim.close()


# ==== B. slots past a row's length ====================================================
def test_b_cases_are_worth_running(oracle):
    deg, ids = shape_table("s6")
    for name in POISON:
        vals = poison_values(name, N)
        assert all(v >= N for v in vals)
        bad = poisoned(deg, ids, vals)
        assert np.array_equal(masked(deg, bad), masked(deg, ids))
        rows = ((bad != masked(deg, ids)) & (np.arange(6)[None, :] >= deg[:, None])).any(axis=1)
        assert rows.sum() >= N // 10
        unused = np.arange(6)[None, :] >= deg[:, None]
        assert (bad[unused] >= N).all() and set(np.unique(bad[unused])) == set(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POISON))
@pytest.mark.parametrize("eng", ENGINES)
def test_unused_slots_are_never_followed(gs, oracle, eng, name):
    deg, ids, sender, ref = a_case(oracle, eng)     # the run on masked(deg, ids)
    bad = poisoned(deg, ids, poison_values(name, N))
    used = np.arange(6)[None, :] < deg[:, None]
    for how in ("host", "device"):
        with make_sim(gs, eng, N) as sim:
            load(sim, how, deg, bad)
            rdeg, rids = sim.read_peers()
            assert np.array_equal(rdeg, deg) and np.array_equal(rids[used], ids[used])
            if eng == "window":      # sealed
                assert (rids[~used] == FFFF).all()
            else:                    # kept as loaded
                assert np.array_equal(rids, bad)
            run_check(sim, eng, ref, sender)


# ==== C. refusals =====================================================================
def valid(deg, ids, n):
    """The validation rule, restated: no length above the stride, no used slot >= n.
    Returns (rows with a long list, (row, slot) pairs with a bad id)."""
    stride = ids.shape[1]
    long_rows = np.nonzero(deg.astype(np.int64) > stride)[0]
    used = np.arange(stride)[None, :] < np.minimum(deg, stride)[:, None]
    used[long_rows] = False           # (the kernel does not look at the slots of such a row)
    return long_rows.tolist(), [tuple(x) for x in np.argwhere(used & (ids.astype(np.int64) >= n)).tolist()]


def c_rows(n):
    return sorted({0, n // 2, n - 1})


def c_tables(n, stride=6, reps=1):
    """(name, deg, ids, message, faults) for every refused table of a context
    of n nodes (reps: tables back to back; the fault is in the last one)."""
    base_deg, base_ids = make_table(n, stride, seed=50 + n)
    base_deg, base_ids = np.tile(base_deg, reps), np.tile(base_ids, (reps, 1))
    off = (reps - 1) * n
    out = []

    def add(name, msg, nlong, nbad, edit):
        deg, ids = base_deg.copy(), base_ids.copy()
        edit(deg, ids)
        out.append((name, deg, ids, msg, (nlong, nbad)))

    for r in c_rows(n):
        add(f"len-row{r}", MSG_LEN, 1, 0, lambda d, i, r=r: d.__setitem__(off + r, stride + 1))
        for what, val in (("n", n), ("ffff", FFFF)):
            def edit(d, i, r=r, val=val):
                d[off + r] = max(d[off + r], 1)
                i[off + r, d[off + r] // 2] = val
            add(f"id-{what}-row{r}", MSG_ID, 0, 1, edit)

    def last(d, i):
        d[off + n - 1] = stride
        i[off + n - 1, stride - 1] = n
    add("id-n-last-slot", MSG_ID, 0, 1, last)
    return out


def c_double(n, stride=6, reps=1):
    """Both faults in one table, the bad id in an earlier row than the long list
    (n = 1: the one row has the long list; its slots are not looked at)."""
    deg, ids = make_table(n, stride, seed=50 + n)
    deg, ids = np.tile(deg, reps), np.tile(ids, (reps, 1))
    off = (reps - 1) * n
    deg[off + n - 1] = stride + 1
    if n > 1:
        deg[off] = stride
        ids[off, 0] = n
    return deg, ids


C_SIZES = [1, 257, N]
C_BIG = 4096 * 256 + 1   # one node past k_validate_peers' grid: its grid-stride loop takes a second pass


def test_c_cases_are_worth_running():
    for n in C_SIZES + [16385, GROUP_N]:
        for reps in (1, 4):
            for name, deg, ids, msg, faults in c_tables(n, reps=reps):
                for t in range(reps):   # per table of the batch: only the last one is refused
                    long_rows, bad = valid(deg[t * n:(t + 1) * n], ids[t * n:(t + 1) * n], n)
                    want = faults if t == reps - 1 else (0, 0)
                    assert (len(long_rows), len(bad)) == want, (n, name, t)
                assert (msg == MSG_LEN) == (faults[0] == 1)
            deg, ids = c_double(n, reps=reps)
            long_rows, bad = valid(deg[(reps - 1) * n:], ids[(reps - 1) * n:], n)
            assert long_rows == [n - 1] and bad == ([(0, 0)] if n > 1 else [])
        good = make_table(n, 6, seed=50 + n)
        assert valid(*good, n) == ([], [])
    deg, ids = big_table()
    assert valid(deg, ids, C_BIG) == ([], [(C_BIG - 1, 1)]) and C_BIG - 1 == 4096 * 256


def big_table():
    deg = np.full(C_BIG, 2, np.uint8)
    ids = (np.arange(2 * C_BIG, dtype=np.uint64) % np.uint64(C_BIG)).astype(np.uint32).reshape(C_BIG, 2)
    ids[C_BIG - 1, 1] = C_BIG
    return deg, ids


def sweep_refusals(gs, sim, n, hows, reps=1, double_msg=MSG_LEN):
    for how in hows:
        for name, deg, ids, msg, _ in c_tables(n, reps=reps):
            refused(gs, lambda: load(sim, how, deg, ids), msg)
        deg, ids = c_double(n, reps=reps)
        refused(gs, lambda: load(sim, how, deg, ids), double_msg if n > 1 else MSG_LEN)
        refused(gs, sim.read_peers, MSG_READ)   # (nothing is begun on a context in this state)


@pytest.mark.gpu
@pytest.mark.parametrize("n", C_SIZES)
@pytest.mark.parametrize("eng", ["window", "pushpull", "median"])
def test_refused_tables_one_device(gs, eng, n):
    """validate_table / k_validate_peers through both calls; with both faults in
    a table the length's message wins (the error word's bit 0 is looked at first)."""
    with make_sim(gs, eng, n) as sim:
        sweep_refusals(gs, sim, n, ("host", "device"))


@pytest.mark.gpu
@pytest.mark.parametrize("n", C_SIZES)
def test_refused_tables_batched_trials(gs, n):
    """upload_table validates a batch on the host, row by row: the same two
    messages; with both faults in a table the first in row order is reported."""
    with make_sim(gs, "window", n, trials=4) as sim:
        sweep_refusals(gs, sim, n, ("host",), reps=4, double_msg=MSG_ID)


@pytest.mark.gpu
@pytest.mark.parametrize("n", C_SIZES)
def test_refused_tables_trials_group(gs, n):
    with gs.Simulator(config(gs, "window", n, trials=4), devices=[0, 0]) as sim:
        sweep_refusals(gs, sim, n, ("host",), reps=4, double_msg=MSG_ID)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16385, GROUP_N])
@pytest.mark.parametrize("eng", ["window", "pushpull"])
def test_refused_tables_shard_group(gs, eng, n):
    with gs.Simulator(config(gs, eng, n), devices=[0, 0]) as sim:
        sweep_refusals(gs, sim, n, ("host",))


@pytest.mark.gpu
def test_refused_table_past_one_grid(gs):
    """n = 4096 x 256 + 1, stride 2, the fault in the last row: only the second
    pass of k_validate_peers' grid-stride loop sees it.  Loads only."""
    deg, ids = big_table()
    with make_sim(gs, "pushpull", C_BIG) as sim:
        for how in ("host", "device"):
            refused(gs, lambda: load(sim, how, deg, ids), MSG_ID)
            refused(gs, lambda: sim.broadcast_begin(0), MSG_BEGIN)
        good = ids.copy()
        good[C_BIG - 1, 1] = C_BIG - 1   # the largest id there is: accepted
        load(sim, "device", deg, good)


@pytest.mark.gpu
def test_argument_refusals_keep_the_table(gs, oracle):
    """The stride limits of the two calls (1..255 and 2..255), a device table
    offered to a group or a batched non-median context, a load after
    broadcast_begin: refused on their arguments, and the table loaded before
    stays (the broadcast that follows is the reference's).  Rows of 33 slots on
    a window-engine context are refused inside the load: that one drops the table."""
    deg, ids, sender, ref = a_case(oracle, "window")
    one = np.ones(N, np.uint8)

    def host(sim, stride):
        return lambda: sim.load_peers(one, np.zeros((N, stride), np.uint32))

    def dev(sim, stride, deg=one):
        def call():
            with devbuf.device_copy(deg, np.zeros((deg.size, max(stride, 1)), np.uint32)) as (d, i):
                sim.load_peers_device(d, i, stride)
        return call
    with make_sim(gs, "window", N) as sim:
        load(sim, "host", deg, ids)
        for stride in (0, 256):
            refused(gs, host(sim, stride), "bad peer table")
        for stride in (0, 1, 256):
            refused(gs, dev(sim, stride), "bad device peer table (stride must be in [2,255])")
        rdeg, rids = sim.read_peers()
        assert np.array_equal(rdeg, deg) and np.array_equal(masked(rdeg, rids), masked(deg, ids))
        sim.broadcast_begin(sender)
        for call in (host(sim, 6), dev(sim, 6)):
            refused(gs, call, "peers must be loaded before gs_broadcast_begin")
        refused(gs, sim.build_overlay, "overlay must be built before gs_broadcast_begin")
        for t in range(len(ref)):          # the table of before the refusals
            step_check(sim, "window", ref, t)
        sim.reset()
        for call in (host(sim, 33), dev(sim, 33)):
            refused(gs, call, "rows longer than 32 need GS_FLAG_TICK_ENGINE (or fanin > 32 at create)")
            refused(gs, lambda: sim.broadcast_begin(sender), MSG_BEGIN)
            refused(gs, sim.read_peers, MSG_READ)
        load(sim, "device", deg, ids)
        run_check(sim, "window", ref, sender)
    with make_sim(gs, "tick", N) as sim:   # the same rows on the tick engine, and one slot through the host call
        sim.load_peers(one, np.zeros((N, 33), np.uint32))
        sim.load_peers(one, np.zeros((N, 1), np.uint32))
        sim.load_peers(np.full(N, 255, np.uint8), np.zeros((N, 255), np.uint32))
    msg = "device tables load into one-device, one-trial contexts"
    with gs.Simulator(config(gs, "window", GROUP_N), devices=[0, 0]) as sim:
        refused(gs, dev(sim, 6, np.ones(GROUP_N, np.uint8)), msg)
    with make_sim(gs, "window", N, trials=4) as sim:
        refused(gs, dev(sim, 6, np.ones(4 * N, np.uint8)), msg)
    with gs.Simulator(config(gs, "window", N, trials=4), devices=[0, 0]) as sim:
        refused(gs, dev(sim, 6, np.ones(4 * N, np.uint8)), msg)


# ==== D. state after a refusal ========================================================
D_KINDS = ["one-window", "one-pushpull", "batched", "shards-window", "shards-pushpull", "trials-group"]
D_T = 4


def d_case(oracle, kind):
    """(engine, n, trials, first table, second table, sender, the second
    table's rows and received sets).  Batched kinds: D_T tables back to back,
    the reference is the trials' sum (rows) and stack (sets)."""
    eng = "pushpull" if kind.endswith("pushpull") else "window"
    n = GROUP_N if kind.startswith("shards") else N
    T = D_T if kind in ("batched", "trials-group") else 1
    seeds = (300, 400)
    tabs = [[make_table(n, 6, seed=s + 10 * t + n) for t in range(T)] for s in seeds]
    sender = sender_of(np.minimum.reduce([d for tab in tabs for d, _ in tab]))
    runs = []
    for s, tab in zip(seeds, tabs):
        per = [reference(oracle, eng, ("D", n, s, t), d, i, sender, trial=t) for t, (d, i) in enumerate(tab)]
        rows = []
        for r in range(len(per[0])):
            row = [sum(p[r].row[c] for p in per) for c in range(7)]
            row[0] = per[0][r].row[0]
            rows.append(Round(row, np.stack([p[r].recv for p in per]) if T > 1 else per[0][r].recv, {}))
        runs.append(rows)
    first, second = [(np.concatenate([d for d, _ in tab]), np.concatenate([i for _, i in tab])) for tab in tabs]
    return eng, n, T, first, second, sender, runs


def d_sim(gs, kind, eng, n, T):
    if kind in ("batched",) or kind.startswith("one"):
        return make_sim(gs, eng, n, trials=T)
    return gs.Simulator(config(gs, eng, n, trials=T), devices=[0, 0])


def test_d_cases_are_worth_running(oracle):
    for kind in D_KINDS:
        eng, n, T, first, second, sender, (ref1, ref2) = d_case(oracle, kind)
        assert [r.row for r in ref1] != [r.row for r in ref2]   # a context that kept the first table would fail
        assert ref1[5].row != ref2[5].row
        assert ref2[-1].row[4] > T * n // 2
        for t in range(T):
            assert valid(second[0][t * n:(t + 1) * n], second[1][t * n:(t + 1) * n], n) == ([], [])
        bad = d_refused(second, n, T)
        assert valid(bad[0][(T - 1) * n:], bad[1][(T - 1) * n:], n) == ([], [(n // 2, 0)])


def d_refused(table, n, T):
    deg, ids = table[0].copy(), table[1].copy()
    r = (T - 1) * n + n // 2
    deg[r] = max(deg[r], 1)
    ids[r, 0] = n
    return deg, ids


def no_table(gs, sim, sender):
    refused(gs, lambda: sim.broadcast_begin(sender), MSG_BEGIN)
    refused(gs, sim.read_peers, MSG_READ)
    refused(gs, lambda: sim.run(poll=10, max_ticks=10), MSG_BEGIN)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", D_KINDS)
def test_refused_load_leaves_no_table(gs, oracle, kind):
    eng, n, T, first, second, sender, (ref1, ref2) = d_case(oracle, kind)
    hows = ("host", "device") if kind.startswith("one") else ("host",)
    with d_sim(gs, kind, eng, n, T) as sim:
        for how in hows:
            load(sim, how, *first)
            refused(gs, lambda: load(sim, how, *d_refused(second, n, T)), MSG_ID)
            no_table(gs, sim, sender)
        load(sim, hows[-1], *second)
        run_check(sim, eng, ref2, sender)


@pytest.mark.gpu
@pytest.mark.parametrize("eng", ["window", "pushpull"])
def test_livelocked_overlay_leaves_no_table(gs, oracle, eng):
    _, n, T, first, second, sender, (ref1, ref2) = d_case(oracle, "one-" + eng)
    with make_sim(gs, eng, n) as sim:
        load(sim, "host", *first)
        refused(gs, lambda: sim.build_overlay(max_ticks=1), "", code=-2)   # GS_ELIVELOCK
        no_table(gs, sim, sender)
        load(sim, "device", *second)
        run_check(sim, eng, ref2, sender)


# ==== E. caller-owned stream ==========================================================
E_ENGINES = ["window", "tick", "pushpull", "rumor0", "rumorpull", "median"]
E_HOW = {"window": "device", "tick": "host", "pushpull": "device", "rumor0": "host", "rumorpull": "device",
         "median": "host"}


def e_case(oracle, eng):
    deg, ids = shape_table("s6")
    failed = mask_of(N, seed=77)
    sender = sender_of(deg, failed)
    return deg, ids, failed, sender, reference(oracle, eng, "s6", deg, ids, sender, failed)


def test_e_cases_are_worth_running(oracle):
    for eng in E_ENGINES:
        deg, ids, failed, sender, ref = e_case(oracle, eng)
        assert failed.sum() > N // 40 and failed[N - 1] and not failed[sender]
        spreads(ref, eng, N, failed)
        plain = a_case(oracle, eng)[3]
        assert [r.row for r in plain] != [r.row for r in ref]   # the mask changes the run


@pytest.mark.gpu
@pytest.mark.parametrize("eng", E_ENGINES)
def test_caller_owned_stream(gs, oracle, eng):
    """The load, the mask, begin and the first rounds on the caller's stream,
    set_stream(None) between two steps, the rest and -- after reset -- the same
    broadcast again on the context's own stream.  The window engine steps in
    calls of 1 and of 7 ticks: the per-tick path and the windowed path."""
    deg, ids, failed, sender, ref = e_case(oracle, eng)
    mask = words_of(failed)
    sizes = [1, 7, 1, 1, 7] if eng == "window" else [1] * 12
    with devbuf.stream() as s, make_sim(gs, eng, N) as sim:
        sim.set_stream(s)
        load(sim, E_HOW[eng], deg, ids)
        sim.set_failed(mask)
        begin(sim, eng, sender)
        assert np.array_equal(sim.crashed(), mask)
        t = 0
        for k in sizes:
            t = step_check(sim, eng, ref, t, k)
        assert np.array_equal(sim.crashed(), mask)
        sim.set_stream(None)
        while t < len(ref):
            k = min(sizes[t % len(sizes)], len(ref) - t)
            t = step_check(sim, eng, ref, t, k)
        assert np.array_equal(sim.crashed(), mask)
        sim.reset()
        assert np.array_equal(sim.crashed(), mask) and not sim.received().any()
        run_check(sim, eng, ref, sender)
        assert np.array_equal(sim.crashed(), mask)


@pytest.mark.gpu
def test_set_stream_refused_on_groups_and_ranks(gs):
    from gossip_simulator_amd import engine
    msg = "multi-device contexts keep their own streams"
    with devbuf.stream() as s:
        with gs.Simulator(config(gs, "window", GROUP_N), devices=[0, 0]) as sim:
            refused(gs, lambda: sim.set_stream(s), msg)
        with gs.Simulator(config(gs, "window", N, trials=4), devices=[0, 0]) as sim:
            refused(gs, lambda: sim.set_stream(s), msg)
        sim = gs.Simulator.rank(config(gs, "window", N), 1, 0, engine.comm_unique_id())
        try:
            refused(gs, lambda: sim.set_stream(s), msg)
        finally:
            sim.close()
