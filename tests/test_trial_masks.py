"""Per-trial failure masks on batched trials, both models (gs_set_failed with
trials > 1).  Trial i of a masked batch must behave
exactly like a one-trial context of trial base + i given trial i's mask, so
the reference of every GPU case is oracle.Engine with set_failed, run once per
trial with that trial's number, table and mask.  The references are computed
once per case (lru_cache) and shared by the GPU tests and the CPU tests that
show every mask matters.

The tick engine (GS_FLAG_TICK_ENGINE) does not run batches at all (gs_create
refuses the combination), so it takes part where it can: as the second
one-trial GPU reference of the flood gs_run case.
"""
from __future__ import annotations

import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip_simulator_amd", "csrc")
COVERED, QUIESCENT, MAX_TICKS = 0, 1, 2
SEED = 0x5EED


@pytest.fixture(scope="module")
def gs():
    import gossip_simulator_amd as mod
    mod.load()
    return mod


def O():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def table(n, stride, dlo, dhi, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(dlo, dhi + 1, size=n).astype(np.uint8),
            rng.integers(0, n, size=(n, stride)).astype(np.uint32))


def stacked(tabs):
    return np.concatenate([d for d, _ in tabs]), np.concatenate([i for _, i in tabs])


def words_of(n, nodes):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    idx = np.asarray(sorted(set(int(x) for x in nodes)), dtype=np.int64)
    np.bitwise_or.at(w, idx // 64, np.left_shift(np.uint64(1), (idx % 64).astype(np.uint64)))
    return w


def random_mask(n, frac, seed, keep=()):
    """round(frac * n) failed nodes, at least one, none of `keep`."""
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(n), np.asarray(list(keep), dtype=np.int64))
    k = min(len(pool), max(1, int(round(frac * n))))
    return words_of(n, rng.choice(pool, size=k, replace=False))


def popcount(words):
    return int(sum(bin(int(x)).count("1") for x in np.asarray(words).ravel()))


def params(n, trial, model, drop=0.1, crash=0.0, dlo=10, dhi=20):
    return O().make_params(n=n, fanout=5, fanin=6, delay_low=dlo, delay_high=dhi, drop_rate=drop, crash_rate=crash,
                           seed=SEED, trial=trial, model=model)


def config(gs, n, T, model="pushpull", drop=0.1, crash=0.0, dlo=10, dhi=20, trial=0, engine="window"):
    return gs.Config(n=n, fanout=5, fanin=6, delaylow=dlo, delayhigh=dhi, droprate=drop, crashrate=crash, seed=SEED,
                     trial=trial, model=model, trials=T, engine=engine)


def engine(p, tab, mask, sender=-1):
    e = O().Engine(p, *tab)
    if mask is not None:
        e.set_failed(mask)
    e.begin(sender)
    return e


def batch_rows(per_trial):
    """gs_step's rows of a batch from the trials' rows: the sums, with the tick."""
    rows = np.array(per_trial).astype(np.int64)  # [T, ticks, 7]
    want = rows.sum(0)
    want[:, 0] = rows[0][:, 0]
    return want


def trial_row(p, tab, mask, sender=-1, poll=10, max_ticks=100000):
    """One trial's gs_trial_results row from the oracle (gs_run's rule per
    trial), and the engine left at the stopping poll."""
    o = O()
    n, flood = int(p.n), p.model == 0
    rows, e = o.run_to_coverage(p, *tab, sender=sender, poll=poll, max_ticks=max_ticks, failed=mask)
    tick99 = next((int(r[0]) for r in rows if o.covered(int(r[4]), n)), 0)
    last = rows[-1]
    s = o.pick_sender(p) if sender < 0 else sender
    begun = 0 if mask is not None and (int(mask[s >> 6]) >> (s & 63)) & 1 else 1
    before = int(rows[-poll - 1][4]) if len(rows) > poll else (0 if flood else begun)
    if o.covered(int(last[4]), n):
        st = COVERED
    elif flood and int(last[6]) == 0:
        st = QUIESCENT
    elif not flood and int(last[4]) == before and o.pp_stalled(p, *tab, e.received(), e.crashed()):
        st = QUIESCENT
    else:
        assert int(last[0]) >= max_ticks
        st = MAX_TICKS
    return [int(p.trial), tick99, int(last[0]), *[int(x) for x in rows[:, 1:4].sum(0)], int(last[4]),
            int(last[5]), st], e


def assert_masks_matter(model, n, tabs, masks, want, base=0, sender=-1, poll=10):
    """Oracle only: every non-empty mask changes its trial's row against the
    unmasked run of the same trial, and (push-pull) some round of the case has
    sent > messages, a kept push to a failed node."""
    assert any(np.asarray(m).any() for m in masks)
    for t, m in enumerate(masks):
        if np.asarray(m).any():
            plain = trial_row(params(n, base + t, model), tabs[t], None, sender=sender, poll=poll)[0]
            assert list(want[t]) != plain, f"trial {base + t}'s mask changes nothing"
    if model == 1:
        assert sum(int(w[4]) - int(w[5]) for w in want) > 0, "no push ever reached a failed node"


# ---- Case A: push-pull, per round ------------------------------------------------
A_N = [63, 64, 65, 1025, 5000, 20000]
A_DROP = [0.0, 0.1]
A_T, A_STEP, A_CALLS = 5, 37, 2


def pp_masks(n, tabs, base=0, seed=0):
    """Empty; 1 %; 30 %; every node of the last word; all but the sender and one friend."""
    s4 = O().pick_sender(params(n, base + 4, 1))
    keep = {s4, int(tabs[4][1][s4, 0])}
    return [np.zeros((n + 63) // 64, dtype=np.uint64), random_mask(n, 0.01, seed + 1),
            random_mask(n, 0.30, seed + 2), words_of(n, range((n - 1) // 64 * 64, n)),
            words_of(n, set(range(n)) - keep)]


@functools.lru_cache(maxsize=None)
def case_a(n, drop):
    tabs = [table(n, 6, 1, 6, seed=7 * n + t) for t in range(A_T)]
    masks = pp_masks(n, tabs, seed=n)
    out = dict(tabs=tabs, masks=masks)
    for key, ms in (("masked", masks), ("plain", [None] * A_T)):
        es = [engine(params(n, t, 1, drop), tabs[t], ms[t]) for t in range(A_T)]
        begun = [popcount(e.received()) for e in es]
        calls = []
        for _ in range(A_CALLS):
            rows = [e.step(A_STEP) for e in es]
            calls.append((rows, [e.received() for e in es]))
        out[key] = (begun, calls)
    return out


@pytest.mark.parametrize("drop", A_DROP)
@pytest.mark.parametrize("n", A_N)
def test_oracle_pp_masks_matter(n, drop):
    c = case_a(n, drop)
    (_, masked), (_, plain) = c["masked"], c["plain"]
    assert not c["masks"][0].any() and all(m.any() for m in c["masks"][1:])
    rows = lambda calls, t: np.concatenate([r[t] for r, _ in calls])  # noqa: E731
    assert np.array_equal(rows(masked, 0), rows(plain, 0))  # the empty mask changes nothing
    for t in range(1, A_T):
        assert not np.array_equal(rows(masked, t), rows(plain, t)), f"trial {t}'s mask changes no row"
    dead = sum(int((rows(masked, t)[:, 2] - rows(masked, t)[:, 3]).sum()) for t in range(A_T))
    assert dead > 0, "no push ever reached a failed node"
    assert all(int((rows(plain, t)[:, 2] - rows(plain, t)[:, 3]).sum()) == 0 for t in range(A_T))


@pytest.mark.gpu
@pytest.mark.parametrize("drop", A_DROP)
@pytest.mark.parametrize("n", A_N)
def test_pp_per_round_bit_exact(gs, n, drop):
    c = case_a(n, drop)
    deg, ids = stacked(c["tabs"])
    got0 = []
    for key in ("masked", "plain"):
        begun, calls = c[key]
        with gs.Simulator(config(gs, n, A_T, drop=drop)) as sim:
            sim.load_peers(deg, ids)
            if key == "masked":
                sim.set_failed(np.array(c["masks"]))
            sim.broadcast_begin(-1)
            assert sim.totals()["received"] == sum(begun) and sim.totals()["pending"] == sum(begun)
            cum = np.zeros((A_T, 3), dtype=np.int64)
            for k, (rows, recv) in enumerate(calls):
                got = sim.step(A_STEP).astype(np.int64)
                want = batch_rows(rows)
                bad = np.nonzero((got != want).any(1))[0]
                assert bad.size == 0, f"{key}, call {k}, round {bad[0] + 1}:\n{got[bad[0]]}\n{want[bad[0]]}"
                rec = sim.received()
                assert rec.shape == (A_T, (n + 63) // 64)
                res = sim.trial_results()
                for t in range(A_T):
                    assert np.array_equal(rec[t], recv[t]), f"{key}, call {k}, trial {t}: informed set"
                    cum[t] += rows[t][:, 1:4].astype(np.int64).sum(0)
                    assert list(res[t, 3:7]) == [*cum[t], int(rows[t][-1, 4])], f"{key}, call {k}, trial {t}"
                got0.append((got if key == "plain" else None, rec[0].copy(), res[0].copy()))
            cr = sim.crashed()
            assert np.array_equal(cr, np.array(c["masks"])) if key == "masked" else not cr.any()
    # the empty-mask trial of the masked batch = the same trial of the unmasked batch
    for a, b in zip(got0[:A_CALLS], got0[A_CALLS:]):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- Case B: failed senders ---------------------------------------------------------
B_N, B_T, B_EXPLICIT = 1025, 5, 7


@functools.lru_cache(maxsize=None)
def case_b(explicit):
    n = B_N
    tabs = [table(n, 6, 1, 6, seed=900 + t) for t in range(B_T)]
    senders = [B_EXPLICIT if explicit else O().pick_sender(params(n, t, 1)) for t in range(B_T)]
    dead = (1, 3) if explicit else (2,)
    masks = [random_mask(n, 0.01, 50 + t, keep=[senders[t]]) for t in range(B_T)]
    for t in dead:
        masks[t] = masks[t] | words_of(n, [senders[t]])
    want = [trial_row(params(n, t, 1), tabs[t], masks[t], sender=B_EXPLICIT if explicit else -1)
            for t in range(B_T)]
    return tabs, masks, dead, [w for w, _ in want], [e.received() for _, e in want]


@pytest.mark.parametrize("explicit", [False, True])
def test_oracle_failed_senders(explicit):
    tabs, masks, dead, want, _ = case_b(explicit)
    assert_masks_matter(1, B_N, tabs, masks, want, sender=B_EXPLICIT if explicit else -1)
    for t, w in enumerate(want):
        if t in dead:
            assert w[6] == 0 and w[2] == 10 and w[8] == QUIESCENT and w[3] > 0  # never starts; live nodes still call
        else:
            assert w[6] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True])
def test_pp_failed_senders(gs, explicit):
    tabs, masks, dead, want, recv = case_b(explicit)
    with gs.Simulator(config(gs, B_N, B_T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(np.array(masks).ravel())  # the flat form
        sim.broadcast_begin(B_EXPLICIT if explicit else -1)
        assert sim.totals()["received"] == B_T - len(dead)
        sim.run(poll=10)
        got = sim.trial_results()
        assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"
        assert np.array_equal(sim.received(), np.array(recv))


# ---- Case C: the stop rule ---------------------------------------------------------
C_N, C_T = 5000, 4
C_FRAC = [0.005, 0.05, 0.005, 0.05]


def cut_table(seed):
    """n = 200: halves A = [0, 100) and B = [100, 200), joined only through the
    bridge nodes 98 and 99 (their friends are in B; B's 100 and 101 know them)."""
    n, h = 200, 100
    deg, ids = table(n, 6, 3, 6, seed)
    ids[:h] %= h - 2            # A knows A, never the bridge ...
    ids[h:] = h + ids[h:] % h   # ... B knows B
    ids[:40, 0] = 98 + (np.arange(40) & 1)  # ... but 40 of A call the bridge too
    ids[98:100] = h + ids[98:100] % h
    ids[100, :] = 98
    ids[101, :] = 99
    return deg, ids.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case_c(poll):
    tabs = [table(C_N, 6, 5, 6, seed=300 + t) for t in range(C_T)]
    masks = [random_mask(C_N, C_FRAC[t], 310 + t, keep=[O().pick_sender(params(C_N, t, 1))]) for t in range(C_T)]
    want = [trial_row(params(C_N, t, 1), tabs[t], masks[t], poll=poll)[0] for t in range(C_T)]
    # n = 200, sender 0 in A: trial 0 unmasked, trial 1 with the bridge failed, trial 2 with 5 % failed
    ctabs = [cut_table(330)] * 3
    cmasks = [np.zeros(4, dtype=np.uint64), words_of(200, [98, 99]), random_mask(200, 0.05, 333, keep=[0, 98, 99])]
    cwant = [trial_row(params(200, t, 1), ctabs[t], cmasks[t], sender=0, poll=poll) for t in range(3)]
    return tabs, masks, want, ctabs, cmasks, [w for w, _ in cwant], [e.received() for _, e in cwant]


@pytest.mark.parametrize("poll", [10, 1])
def test_oracle_stop_rule(poll):
    tabs, masks, want, ctabs, cmasks, cwant, crecv = case_c(poll)
    assert_masks_matter(1, C_N, tabs, masks, want, poll=poll)
    assert_masks_matter(1, 200, ctabs, cmasks, cwant, sender=0, poll=poll)
    assert [w[8] for w in want] == [COVERED, QUIESCENT, COVERED, QUIESCENT]
    assert cwant[1][8] == QUIESCENT and cwant[0][8] == COVERED
    b = np.arange(100, 200)
    in_b = lambda w: int(((w[b >> 6] >> (b & 63).astype(np.uint64)) & np.uint64(1)).sum())  # noqa: E731
    assert in_b(crecv[1]) == 0 and cwant[1][6] == 98  # all of A but the bridge, none of B
    assert in_b(crecv[0]) > 90


@pytest.mark.gpu
@pytest.mark.parametrize("poll", [10, 1])
def test_pp_stop_rule(gs, poll):
    tabs, masks, want, ctabs, cmasks, cwant, crecv = case_c(poll)
    with gs.Simulator(config(gs, C_N, C_T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(np.array(masks))
        sim.broadcast_begin(-1)
        _, status = sim.run(poll=poll)
        got = sim.trial_results()
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"
    assert status == gs.GS_RUN_QUIESCENT
    with gs.Simulator(config(gs, 200, 3)) as sim:
        sim.load_peers(*stacked(ctabs))
        sim.set_failed(np.array(cmasks))
        sim.broadcast_begin(0)
        sim.run(poll=poll)
        got = sim.trial_results()
        assert np.array_equal(got, np.array(cwant)), f"\n{got}\n{np.array(cwant)}"
        assert np.array_equal(sim.received(), np.array(crecv))


# ---- Case D: lifecycle ----------------------------------------------------------------
D_N, D_T = 5000, 4


@functools.lru_cache(maxsize=None)
def case_d(base):
    tabs = [table(D_N, 6, 5, 6, seed=400 + base + t) for t in range(D_T)]
    masks = [random_mask(D_N, 0.01, 410 + base + t) for t in range(D_T)]
    want = [trial_row(params(D_N, base + t, 1), tabs[t], masks[t])[0] for t in range(D_T)]
    return tabs, np.array(masks), np.array(want)


def test_oracle_lifecycle_cases_differ():
    assert not np.array_equal(case_d(0)[2][:, 1:], case_d(D_T)[2][:, 1:])
    for base in (0, D_T):
        tabs, masks, want = case_d(base)
        assert_masks_matter(1, D_N, tabs, masks, want, base=base)


@pytest.mark.gpu
def test_pp_lifecycle(gs):
    tabs, masks, want = case_d(0)
    words = masks.shape[1]

    def go(sim):
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        return sim.trial_results()

    with gs.Simulator(config(gs, D_N, D_T)) as sim:
        sim.load_peers(*stacked(tabs))
        with pytest.raises(gs.GossipError) as ei:  # too few words
            sim.set_failed(masks.ravel()[:-1])
        assert ei.value.code == -1
        with pytest.raises(gs.GossipError):
            sim.set_failed(masks[0])
        sim.set_failed(masks)  # the refused calls left the context usable
        assert np.array_equal(go(sim), want)
        with pytest.raises(gs.GossipError) as ei:  # after broadcast_begin
            sim.set_failed(masks)
        assert ei.value.code == -1
        assert np.array_equal(sim.trial_results(), want)
        sim.reset()  # keeps the masks
        assert np.array_equal(sim.crashed(), masks) and not sim.received().any()
        assert np.array_equal(go(sim), want)
        sim.reset()
        sim.set_trial(D_T)  # new tables and new masks for trials T .. 2T-1
        tabs2, masks2, want2 = case_d(D_T)
        sim.load_peers(*stacked(tabs2))
        sim.set_failed(masks2)
        got = go(sim)
        assert np.array_equal(got, want2), f"\n{got}\n{want2}"
        assert sim.crashed().shape == (D_T, words) and np.array_equal(sim.crashed(), masks2)


# ---- Case E: split over members -----------------------------------------------------------
E_T = 5


@functools.lru_cache(maxsize=None)
def case_e(model):
    n = 5000
    tabs = [table(n, 6, 5, 6, seed=500 + t) for t in range(E_T)]
    masks = [random_mask(n, 0.01, 510 + t) for t in range(E_T)]
    s3 = O().pick_sender(params(n, 3, model))
    masks[3] = masks[3] | words_of(n, [s3])  # one trial never starts
    masks[1][:] = 0
    want = [trial_row(params(n, t, model), tabs[t], masks[t])[0] for t in range(E_T)]
    return n, tabs, np.array(masks), np.array(want)


def test_oracle_split_case():
    for model in (0, 1):
        n, tabs, masks, want = case_e(model)
        assert_masks_matter(model, n, tabs, masks, want)
        assert want[3, 6] == 0 and (want[[0, 1, 2, 4], 6] > 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0], [0, 0, 0]])
def test_pp_split_over_members(gs, devices):
    n, tabs, masks, want = case_e(1)
    with gs.Simulator(config(gs, n, E_T), devices=devices) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(masks)
        sim.broadcast_begin(-1)
        assert sim.totals()["received"] == E_T - 1 and sim.totals()["pending"] == E_T - 1
        sim.run(poll=10)
        got = sim.trial_results()
        assert sim.received().shape == (E_T, (n + 63) // 64)
        assert np.array_equal(sim.crashed(), masks)
    assert np.array_equal(got, want), f"\n{got}\n{want}"


# ---- Case F: the masked limit -------------------------------------------------------------
F_T = 2
F_M355 = (163840 - 256) // 24 * 64  # the plan's arithmetic at the 160 KiB an MI355X grants a workgroup


@functools.lru_cache(maxsize=None)
def case_f(m):
    tabs = [table(m, 6, 5, 6, seed=600 + t) for t in range(F_T)]
    masks = [random_mask(m, 0.01, 610 + t) for t in range(F_T)]
    want = [trial_row(params(m, t, 1), tabs[t], masks[t])[0] for t in range(F_T)]
    return tabs, masks, want


def test_oracle_limit_case():
    tabs, masks, want = case_f(F_M355)
    assert F_M355 == 436224
    assert_masks_matter(1, F_M355, tabs, masks, want)


@pytest.mark.gpu
def test_pp_masked_limit(gs):
    m = gs.pp_trials_max_n_masked()
    assert m % 64 == 0 and 0 < m < gs.pp_trials_max_n()
    tabs, masks, want = case_f(m)
    with gs.Simulator(config(gs, m, F_T)) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(np.array(masks))
        sim.broadcast_begin(-1)
        sim.run(poll=10)
        got = sim.trial_results()
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_pp_past_the_masked_limit(gs, devices):
    """The refusal names the limit and leaves the context (or every member of a
    split one) unmasked and usable."""
    m = gs.pp_trials_max_n_masked()
    n, T = m + 64, 2 if devices is None else 4  # two trials per member: each a trial-resident batch
    tabs = [table(n, 6, 5, 6, seed=620 + t) for t in range(T)]
    want = [trial_row(params(n, t, 1), tabs[t], None)[0] for t in range(T)]
    with gs.Simulator(config(gs, n, T), devices=devices) as sim:
        sim.load_peers(*stacked(tabs))
        with pytest.raises(gs.GossipError) as ei:
            sim.set_failed(np.array([random_mask(n, 0.01, 630 + t) for t in range(T)]))
        assert ei.value.code == -1 and str(m) in str(ei.value)
        sim.broadcast_begin(-1)  # the context still runs, unmasked
        sim.run(poll=10)
        got = sim.trial_results()
        assert not sim.crashed().any()
    assert np.array_equal(got, np.array(want)), f"\n{got}\n{np.array(want)}"


# ---- Case G: flood batches ------------------------------------------------------------------
G_N = [3, 257, 4099, 20000]
G_FRAC = [0.0, 0.01, 0.30]
G_CHUNK, G_MAXT = 40, 600


def flood_masks(n, T, seed, base=0, crash=0.0, delays=(10, 20)):
    """Trial t: empty, 1 % or 30 % failed, in turn; never the trial's own sender."""
    out = []
    for t in range(T):
        s = O().pick_sender(params(n, base + t, 0, crash=crash, dlo=delays[0], dhi=delays[1]))
        f = G_FRAC[t % 3]
        out.append(np.zeros((n + 63) // 64, dtype=np.uint64) if f == 0 or n < 4 and t % 3 == 2
                   else random_mask(n, f, seed + t, keep=[s]))
    return out


@functools.lru_cache(maxsize=None)
def case_g(n, T, delays, crash):
    tabs = [table(n, 6, 1 if n < 10 else 4, 6 if n > 10 else 2, seed=11 * n + t) for t in range(T)]
    masks = flood_masks(n, T, seed=n + T, crash=crash, delays=delays)
    out = dict(tabs=tabs, masks=masks)
    for key, ms in (("masked", masks), ("plain", [None] * T)):
        es = [engine(params(n, t, 0, crash=crash, dlo=delays[0], dhi=delays[1]), tabs[t], ms[t]) for t in range(T)]
        chunks = []
        while True:
            rows = [e.step(G_CHUNK) for e in es]
            chunks.append(rows)
            if all(int(r[-1, 6]) == 0 for r in rows) or int(rows[0][-1, 0]) >= G_MAXT:
                break
        out[key] = (chunks, [e.received() for e in es], [e.crashed() for e in es])
    return out


G_CASES = [(n, T, d, c) for n in G_N for T in (3, 6) for d in ((10, 20), (1, 2)) for c in (0.0, 0.05)]


@pytest.mark.parametrize("n,T,delays,crash", G_CASES)
def test_oracle_flood_masks_matter(n, T, delays, crash):
    c = case_g(n, T, delays, crash)
    rows = lambda key, t: np.concatenate([ch[t] for ch in c[key][0]])  # noqa: E731
    some = False
    for t in range(T):
        if c["masks"][t].any():
            some = True
            m, p = rows("masked", t), rows("plain", t)
            k = min(len(m), len(p))
            assert len(m) != len(p) or not np.array_equal(m[:k], p[:k]), f"trial {t}'s mask changes no row"
            assert int(c["masked"][0][-1][t][-1, 6]) == 0  # ran to its end
    assert some


@pytest.mark.gpu
@pytest.mark.parametrize("n,T,delays,crash", G_CASES)
def test_flood_per_tick_bit_exact(gs, n, T, delays, crash):
    c = case_g(n, T, delays, crash)
    chunks, recv, crashed = c["masked"]
    with gs.Simulator(config(gs, n, T, model="flood", crash=crash, dlo=delays[0], dhi=delays[1])) as sim:
        sim.load_peers(*stacked(c["tabs"]))
        sim.set_failed(np.array(c["masks"]))
        sim.broadcast_begin(-1)
        assert sim.totals()["pending"] == T
        for k, rows in enumerate(chunks):
            got = sim.step(G_CHUNK).astype(np.int64)
            want = batch_rows(rows)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, f"chunk {k}, tick {want[bad[0], 0]}:\n{got[bad[0]]}\n{want[bad[0]]}"
        assert np.array_equal(sim.received(), np.array(recv))
        assert np.array_equal(sim.crashed(), np.array(crashed))


@functools.lru_cache(maxsize=None)
def case_g_run():
    n, T = 4099, 6
    tabs = [table(n, 6, 5, 6, seed=700 + t) for t in range(T)]
    masks = flood_masks(n, T, seed=710, crash=0.0)
    s4 = O().pick_sender(params(n, 4, 0, crash=0.0))
    masks[4] = masks[4] | words_of(n, [s4])  # trial 4's keyed sender is failed
    want = [trial_row(params(n, t, 0, crash=0.0), tabs[t], masks[t])[0] for t in range(T)]
    return n, T, tabs, np.array(masks), np.array(want)


def test_oracle_flood_run_case():
    n, T, _, masks, want = case_g_run()
    assert list(want[4, 2:9]) == [10, 0, 0, 0, 0, 0, QUIESCENT]  # a failed sender: stops at the first poll
    assert (want[[0, 1, 2, 3, 5], 6] > 0.5 * n).all()
    assert COVERED in want[:, 8] and QUIESCENT in want[[0, 1, 2, 3, 5], 8]  # the 30 % masks cannot be covered


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_flood_run_failed_sender_and_members(gs, devices):
    """gs_run: a batch with a failed keyed sender in trial 4 equals the oracle
    and one-trial GPU contexts (window and tick engine) with the same masks;
    also split over two members."""
    n, T, tabs, masks, want = case_g_run()
    with gs.Simulator(config(gs, n, T, model="flood", crash=0.0), devices=devices) as sim:
        sim.load_peers(*stacked(tabs))
        sim.set_failed(masks)
        sim.broadcast_begin(-1)
        assert sim.totals()["pending"] == T - 1
        sim.run(poll=10)
        got = sim.trial_results()
        assert np.array_equal(sim.crashed()[4], masks[4]) and not sim.received()[4].any()
    assert np.array_equal(got, want), f"\n{got}\n{want}"
    if devices is None:
        for eng in ("window", "tick"):
            for t in range(T):
                with gs.Simulator(config(gs, n, 1, model="flood", crash=0.0, trial=t, engine=eng)) as one:
                    one.load_peers(*tabs[t])
                    one.set_failed(masks[t])
                    one.broadcast_begin(-1)
                    one.run(poll=10)
                    assert np.array_equal(one.trial_results()[0], got[t]), f"{eng} engine, trial {t}"


@pytest.mark.gpu
def test_tick_engine_still_refuses_batches(gs):
    with pytest.raises(gs.GossipError) as ei:
        gs.Simulator(config(gs, 257, 3, model="flood", engine="tick"))
    assert ei.value.code == -1


# ---- CPU: the LDS plan ------------------------------------------------------------------------
PLAN_MAIN = r"""
#include <cstdio>
#include "gs_ppt_plan.h"
using namespace gs;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  const unsigned long long big = 1ull << 40;
  // three bitsets of ceil(n / 64) 8-byte words + 256 B of reduction scratch
  CHECK(ppt_plan_masked(1, big).lds_bytes == 3 * 8 + 256);
  CHECK(ppt_plan_masked(65, big).lds_bytes == 3 * 2 * 8 + 256);
  CHECK(ppt_plan_masked(16385, big).lds_bytes == 3 * 257 * 8 + 256);
  CHECK(!ppt_plan_masked(0, big).fits);
  CHECK(ppt_max_n_masked(65536) == (65536 - 256) / 24 * 64 && ppt_max_n_masked(65536) == 174080);
  CHECK(ppt_max_n_masked(163840) == (163840 - 256) / 24 * 64 && ppt_max_n_masked(163840) == 436224);
  CHECK(ppt_max_n_masked(279) == 0 && ppt_max_n_masked(280) == 64 && ppt_max_n_masked(0) == 0);
  const unsigned long long limits[] = {65536, 163840, 280, 300};
  for (unsigned long long lim : limits) {
    const unsigned long long m = ppt_max_n_masked(lim);
    CHECK(m >= 64 && m % 64 == 0 && m <= ppt_max_n(lim));
    if (lim >= 65536) CHECK(m < ppt_max_n(lim));
    const PptPlan p = ppt_plan_masked(m, lim);
    CHECK(p.fits && p.lds_bytes <= lim && p.lds_bytes == 3 * p.words * 8 + kPptScratchBytes);
    CHECK(!ppt_plan_masked(m + 1, lim).fits && ppt_plan_masked(m + 1, lim).lds_bytes > lim);
    if (lim >= 65536) CHECK(ppt_plan(m + 1, lim).fits);  // the unmasked layout still takes it
  }
  // the block rule is the unmasked plan's
  for (unsigned long long n = 1; n <= 700000; n += (n < 4096 ? 1 : 997)) {
    const PptPlan a = ppt_plan(n, big), b = ppt_plan_masked(n, big);
    CHECK(a.block == b.block && a.words == b.words && b.lds_bytes == a.lds_bytes + a.words * 8);
  }
  // the unmasked functions keep their pinned values
  CHECK(ppt_max_n(65536) == 261120 && ppt_max_n(163840) == 654336 && ppt_max_n(271) == 0);
  CHECK(ppt_plan(16385, big).lds_bytes == 2 * 257 * 8 + 256);
  CHECK(ppt_plan(1, big).block == 64 && ppt_plan(1025, big).block == 128 && ppt_plan(100000, big).block == 1024);
  std::printf("ok\n");
  return 0;
}
"""


def test_masked_plan_header_on_the_host(tmp_path):
    """gs_ppt_plan.h alone under the host compiler, as a stand-alone sanitized program."""
    assert shutil.which("g++"), "g++ is needed to build the plan check"
    src = tmp_path / "ppt_plan_masked_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = str(tmp_path / "ppt_plan_masked_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr or "unsupported" in r.stderr):
        r = subprocess.run(base, capture_output=True, text=True)  # no sanitizer runtime on this toolchain
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
