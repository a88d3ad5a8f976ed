"""One family of the poison sweep in a fresh process (GS_DEVMEM_POISON is read
once per process, so tests/test_poison_sweep.py starts one child per family and
poison byte with the variable set): every device block the library gets is
filled with the byte before it is handed out, and every case must still be
bit-exact against the checker the project already has for that engine
(oracle.Engine / oracle.overlay, PyRumorModes, PyMedian, PyRumorSet).

A case walks one context through its life:
  1. fresh: after create, and again after the table is loaded, every read-back
     legal before broadcast_begin gives the documented empty value, and
     read_peers the loaded table;
  2. begin, then step(1) per round: the stats row and every set or state array
     the engine exposes, against the reference;
  3. reset, another mask, begin from another sender;
  4. reset, set_trial, a table of more slots per row (more bytes than grow()'s
     slack covers) and the first sender again.

The case lists (CASES) hold data only; reference(case, phase) builds the
checker alone, which the CPU test uses to see that a case is worth running.

Usage: python tests/poison_worker.py <family>      one JSON line; exit 1 on a mismatch
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BASE = dict(fanout=5, fanin=6, delay_low=10, delay_high=20, drop_rate=0.1, crash_rate=0.0, seed=0x5EED, trial=0)
NS = (65, 4133)  # one word and one bit; a ragged last word after 64 full ones
STAT = ("tick", "fired", "sent", "messages", "received", "crashed", "pending")


def _case(family, n, **more):
    c = dict(family=family, n=n, strides=(6, 9), rounds=30, kw={}, cfg={})
    c.update(more)
    c["name"] = more.get("name", f"{family}-n{n}")
    return c


def _grid1(m):
    """GS_RUMOR_GRID=1: one block, so a list or a table takes several passes of the kernel's loop."""
    return _case("rumor", 4133, name=f"rumor-grid1-mode{m}", mode=m, k=2, rounds=40, kw=dict(model=2),
                 env=dict(GS_RUMOR_GRID="1"))


CASES = {
    # the window engine, injected rows of 6 slots; short delays so 30 ticks spread it
    "flood_window": [_case("flood_window", n, kw=dict(delay_low=1, delay_high=3, crash_rate=0.01)) for n in NS] +
                    # the same table from a buffer the caller owns (gs_load_peers_device)
                    [_case("flood_window", 4133, name="flood_window-devload-n4133", device_load=True,
                           kw=dict(delay_low=1, delay_high=3, crash_rate=0.01))],
    # a ring of 257 slots is too long for the window engine: the tick engine without the flag
    "flood_ring257": [_case("flood_tick", n, name=f"flood_ring257-n{n}", rounds=rounds,
                            kw=dict(delay_low=1, delay_high=257, crash_rate=0.01, drop_rate=0.0))
                      for n, rounds in ((65, 1500), (4133, 2000))],
    # a batched context: 3 trials, a mask per trial
    "flood_batch": [_case("flood_window", n, name=f"flood_batch-n{n}", trials=3,
                          kw=dict(delay_low=1, delay_high=3, crash_rate=0.01)) for n in NS],
    # 2 in-process shards: whole 16384-node buckets, one node into the second
    "flood_shards": [_case("flood_window", 16385, name="flood_shards-n16385", devices=[0, 0],
                           kw=dict(delay_low=1, delay_high=3, crash_rate=0.01))],
    # the tick engine: rows wider than the window engine takes
    # (at n = 65 node 64 crashes at its own first receipt under this key: the second sender is 63)
    "flood_tick": [_case("flood_tick", n, strides=(33, 42), cfg=dict(engine="tick"), sender2=n - 2,
                         kw=dict(fanout=33, fanin=42, delay_low=1, delay_high=3, crash_rate=0.01, drop_rate=0.3, seed=12))
                   for n in NS],
    # the GPU-built table and its packed view (fanout 5, fanin 6), and one wide pair
    "overlay": [_case("overlay", 4133, name="overlay-5-6", rounds=40, kw=dict(delay_low=1, delay_high=3)),
                _case("overlay", 4133, name="overlay-18-19", rounds=40,
                      kw=dict(fanout=18, fanin=19, delay_low=1, delay_high=3, drop_rate=0.5))],
    # push-pull: the default selection (early then dense bottom-up), each forced path, and dense-only
    "pushpull": [_case("pushpull", n, name=f"pushpull-{r}-n{n}", rounds=16, kw=dict(model=1), cfg=dict(pp_rounds=r))
                 for n in NS for r in ("auto", "early", "bottom", "answer", "dense")],
    "pushpull_batch": [_case("pushpull", n, name=f"pushpull_batch-n{n}", trials=3, rounds=16, kw=dict(model=1))
                       for n in NS],
    # (a sharded push-pull context takes a failure mask with rows of at most 8 slots)
    "pushpull_shards": [_case("pushpull", 16385, name="pushpull_shards-n16385", devices=[0, 0], rounds=18,
                              strides=(6, 8), kw=dict(model=1))],
    # all 8 modes: the list engine (push) and the dense engine (pull)
    "rumor_push": [_case("rumor", n, name=f"rumor-mode{m}-n{n}", mode=m, k=60 if m & 3 else 2, rounds=40,
                         kw=dict(model=2)) for n in NS for m in range(4)] + [_grid1(0)],
    "rumor_pull": [_case("rumor", n, name=f"rumor-mode{m}-n{n}", mode=m, k=60 if m & 3 else 2, rounds=40,
                         kw=dict(model=2)) for n in NS for m in range(4, 8)] + [_grid1(4)],
    # the trial-resident batch: modes 0, pull, and pull+blind+coin
    "rumor_batch": [_case("rumor", n, name=f"rumor_batch-mode{m}-n{n}", mode=m, k=200 if m & 3 else 2, rounds=40,
                          trials=3, kw=dict(model=2)) for n in NS for m in (0, 4, 7)],
    "median": [_case("median", n, k=2, rounds=30, kw=dict(model=3)) for n in NS],
    "median_batch": [_case("median", n, name=f"median_batch{'-packed' if pk else ''}-n{n}", k=2, rounds=30, trials=3,
                           kw=dict(model=3), cfg=dict(median_packed=pk)) for n in NS for pk in (False, True)],
    "rumorset": [_case("rumorset", n, name=f"rumorset-R{R}-n{n}", R=R, rounds=14, kw=dict(model=1))
                 for n in NS for R in (63, 64)],
    # a cap of 2 per message, rotate, late starts (two of them at one node)
    "rumorset_cap": [_case("rumorset", n, name=f"rumorset_cap-n{n}", R=9, rounds=16, kw=dict(model=1),
                           cap=dict(B=2, pick="rotate", starts=[0, 3, 0, 1, 2, 3, 5, 5, 8])) for n in NS],
}
FAMILIES = sorted(CASES)


# ---- the data of a case: tables, masks, senders ------------------------------
def tables(case):
    from test_gpu_parity import random_table
    n, (s1, s2) = case["n"], case["strides"]
    t1 = random_table(n, s1, 1, s1, seed=n)        # ragged rows: slots past deg are never the engine's to read
    t2 = random_table(n, s2, s2 - 1, s2, seed=n + 1)
    for _, ids in (t1, t2):  # a ring in slot 0: every sender reaches everyone, node n - 1 is named
        ids[:, 0] = (np.arange(n) + 1) % n
    return t1, t2


def masks(case):
    n = case["n"]
    a = np.random.default_rng(3).random(n) < 0.05
    b = np.random.default_rng(4).random(n) < 0.10
    for m in (a, b):
        m[[n // 2, n - 2, n - 1]] = False    # the senders live
        m[n // 3] = True              # and somebody dies, at either n
    return a, b


def phases(case):
    """(phase, trial, table index, mask index, sender)"""
    n = case["n"]
    return [("begin", 0, 0, 0, n // 2), ("reset", 0, 0, 1, case.get("sender2", n - 1)), ("set_trial", 3, 1, 1, n // 2)]


def kw_of(case, trial=0):
    return dict(BASE, n=case["n"], **case["kw"], trial=trial)


# ---- the references, behind one face: step() -> row, sets() -> arrays --------
class OracleRef:
    def __init__(self, oracle, case, kw, deg, ids, dead, sender):
        from test_pushpull import words_of
        self.e = oracle.Engine(oracle.make_params(**kw), deg, ids)
        self.dead = words_of(dead)
        self.e.set_failed(self.dead)
        self.e.begin(sender)

    def step(self):
        return [int(x) for x in self.e.step(1)[0]]

    def sets(self):
        return dict(received=self.e.received(), crashed=self.e.crashed())


class PyRef:
    def __init__(self, oracle, case, kw, deg, ids, dead, sender):
        from test_gpu_parity import masked
        from test_pushpull import words_of
        p, f = oracle.make_params(**kw), case["family"]
        self.w, self.f, self.dead = words_of, f, dead
        if f == "rumor":
            from test_rumor_modes import PyRumorModes
            self.e = PyRumorModes(oracle, p, deg, masked(deg, ids), sender, case["k"], dead, case["mode"])
        elif f == "median":
            from test_median import PyMedian
            self.e = PyMedian(oracle, p, deg, masked(deg, ids), sender, case["k"], dead)
        elif case.get("cap"):
            from test_rumorset_cap import POLICIES, PyCappedSet
            cap = case["cap"]
            self.e = PyCappedSet(oracle, p, deg, masked(deg, ids), senders_of(case, sender), cap["starts"], cap["B"],
                                 POLICIES[cap["pick"]], dead)
        else:
            from test_rumorset import PyRumorSet
            self.e = PyRumorSet(oracle, p, deg, masked(deg, ids), senders_of(case, sender), dead)

    def step(self):
        row = self.e.step()
        if self.f == "rumorset":
            self.e.poll()
        return [int(x) for x in row]

    def sets(self):
        e, w = self.e, self.w
        if self.f == "rumorset":
            out = dict(rumor_words=e.have, received=w(e.holds_all), crashed=w(self.dead),
                       counts=np.array(e.counts, np.int64), tick_99=np.array(e.tick_99, np.int64))
            if hasattr(e, "traffic"):
                out["traffic"] = np.array([e.traffic[k] for k in ("wanted", "carried", "bound")], np.int64)
            return out
        out = dict(received=w(e.inf), removed=w(e.removed), crashed=w(self.dead))
        if self.f == "median":
            out["median_state"] = e.st
        return out


def senders_of(case, sender):
    n, R = case["n"], case["R"]
    if case.get("cap"):  # a few nodes apart, so that rumors meet and the cap binds early
        s = [(sender + 3 * j) % n for j in range(R)]
        s[7] = s[6]      # two late starts at one node
        return s
    s = [(sender + (j * n) // R) % n for j in range(R)]
    s[1] = s[0]  # two rumors at one node
    return s


class BatchRef:
    """A batch: one checker per trial (trial + i, its own table and mask); the
    row is the trials' sum with the tick, the sets are stacked trial-major."""

    def __init__(self, refs):
        self.refs = refs

    def step(self):
        rows = np.array([r.step() for r in self.refs], dtype=np.int64)
        out = rows.sum(0)
        out[0] = rows[0][0]
        return [int(x) for x in out]

    def sets(self):
        per = [r.sets() for r in self.refs]
        return {k: np.stack([p[k] for p in per]) for k in per[0]}


def trial_tables(case, ti, i):
    """Trial i's table: the case's, its rows rolled by i (ids stay in range)."""
    deg, ids = tables(case)[ti]
    return np.roll(deg, i), np.roll(ids, i, axis=0)


def trial_mask(case, mi, i):
    m = np.roll(masks(case)[mi], 7 * i).copy()
    n = case["n"]
    m[[n // 2, n - 2, n - 1]] = False
    return m


def reference(oracle, case, phase_index):
    """The checker of one phase of a case, begun; no GPU."""
    ph, trial, ti, mi, sender = phases(case)[phase_index]
    deg, ids = tables(case)[ti]
    kw = kw_of(case, trial)
    if case["family"] == "overlay":
        deg, ids, _, _ = oracle.overlay(oracle.make_params(**kw))
    cls = OracleRef if case["family"] in ("flood_window", "flood_tick", "overlay", "pushpull") else PyRef
    T = case.get("trials", 1)
    if T > 1:
        return BatchRef([cls(oracle, case, kw_of(case, trial + i), *trial_tables(case, ti, i), trial_mask(case, mi, i),
                             sender) for i in range(T)])
    return cls(oracle, case, kw, deg, ids, masks(case)[mi], sender)


# ---- the GPU side ---------------------------------------------------------------
def make_sim(gs, case):
    kw = kw_of(case)
    model = {0: "flood", 1: "pushpull", 2: "rumor", 3: "median"}[kw.get("model", 0)]
    more = dict(case["cfg"])
    if model == "rumor":
        m = case["mode"]
        more.update(rumor_k=case["k"], rumor_blind=bool(m & 1), rumor_coin=bool(m & 2), rumor_pull=bool(m & 4))
    if model == "median":
        more.update(rumor_k=case["k"])
    fo, fi = kw["fanout"], kw["fanin"]
    if case["family"] != "overlay":  # rows as wide as the widest table of the case
        fi = max(fi, max(case["strides"]))
    cfg = gs.Config(n=kw["n"], fanout=fo, fanin=fi, delaylow=kw["delay_low"], delayhigh=kw["delay_high"],
                    droprate=kw["drop_rate"], crashrate=kw["crash_rate"], seed=kw["seed"], trial=kw["trial"],
                    model=model, trials=case.get("trials", 1), **more)
    if case["family"] == "rumorset":
        return gs.Simulator.rumor_set(cfg, case["R"])
    if case.get("trials") and model == "rumor":
        return gs.Simulator.batch(cfg)
    if case.get("trials") and model == "median":
        return gs.Simulator.median_batch(cfg)
    return gs.Simulator(cfg, devices=case.get("devices"))


def sim_sets(sim, case, begun=True):
    f = case["family"]
    out = dict(received=sim.received(), crashed=sim.crashed())
    if f in ("rumor", "median"):
        out["removed"] = sim.removed()
    if f == "median":
        out["median_state"] = sim.median_state()
    if f == "rumorset":
        res = sim.rumor_results()
        out.update(rumor_words=sim.rumor_words(), counts=np.array([r["received"] for r in res], np.int64),
                   tick_99=np.array([r["tick_99"] for r in res], np.int64))
        if case.get("cap") and begun:
            t = sim.rumor_traffic()
            out["traffic"] = np.array([t[k] for k in ("wanted", "carried", "bound")], np.int64)
    return out


def check_empty(sim, case, where, fresh=True):
    """fresh=False: the context has a failure mask from the phase before, which
    the next set_failed replaces; every other read-back is empty again."""
    got = sim_sets(sim, case, begun=False)
    for k, v in got.items():
        if k == "crashed" and not fresh:
            continue
        want = np.zeros_like(v)
        assert np.array_equal(v, want), f"{where}: {k} is not empty: {np.count_nonzero(v != want)} element(s) differ"
    tot = sim.totals()
    assert all(tot[f] == 0 for f in STAT), f"{where}: totals {tot}"
    tr = sim.trial_results()
    assert tr.shape[0] == (case.get("trials", 1) if not case.get("devices") else tr.shape[0]) and \
        not tr[:, 1:8].any(), f"{where}: trial_results {tr.tolist()}"


def compare(sim, case, ref, where):
    want, got = ref.sets(), sim_sets(sim, case)
    for k in want:
        if not np.array_equal(got[k], want[k]):
            g, w = np.asarray(got[k]).ravel(), np.asarray(want[k]).ravel()
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{where}: {k} differs in {bad.size} element(s); first at {bad[:4].tolist()}: "
                                 f"got {[hex(int(x)) for x in g[bad[:4]]]}, reference {[hex(int(x)) for x in w[bad[:4]]]}")


def run_case(gs, oracle, case):
    from test_gpu_parity import masked
    from test_pushpull import words_of
    name, T, last_mask = case["name"], case.get("trials", 1), None
    with make_sim(gs, case) as sim:
        check_empty(sim, case, f"{name}: after create")
        for pi, (ph, trial, ti, mi, sender) in enumerate(phases(case)):
            where = f"{name}: {ph}"
            if pi:
                sim.reset()
                check_empty(sim, case, f"{where}: after reset", fresh=False)
                assert np.array_equal(np.asarray(sim.crashed()).ravel(), np.asarray(last_mask).ravel()), \
                    f"{where}: after reset: crashed is not the mask set before"
            if ph == "set_trial":
                sim.set_trial(trial)
            if pi == 0 or ph == "set_trial":
                if case["family"] == "overlay":
                    wins, final = sim.build_overlay()
                    odeg, oids, owins, ofinal = oracle.overlay(oracle.make_params(**kw_of(case, trial)))
                    assert final == ofinal and [tuple(w) for w in wins] == [tuple(w) for w in owins], \
                        f"{where}: overlay windows differ"
                    deg, ids = odeg, oids
                else:
                    tabs = [trial_tables(case, ti, i) for i in range(T)]
                    deg, ids = np.concatenate([d for d, _ in tabs]), np.concatenate([x for _, x in tabs])
                    if case.get("device_load"):
                        import devbuf
                        with devbuf.device_copy(deg, ids) as (pdeg, pids):
                            sim.load_peers_device(pdeg, pids, ids.shape[1])
                    else:
                        sim.load_peers(deg, ids)
                if not case.get("devices"):  # (a sharded context keeps only its partitions)
                    gdeg, gids = sim.read_peers()
                    assert np.array_equal(gdeg, deg), f"{where}: read_peers degrees differ"
                    assert np.array_equal(masked(gdeg, gids)[:, :ids.shape[1]], masked(deg, ids)), \
                        f"{where}: read_peers rows differ"
                check_empty(sim, case, f"{where}: after the table", fresh=pi == 0)
            last_mask = np.stack([words_of(trial_mask(case, mi, i)) for i in range(T)]) if T > 1 \
                else words_of(masks(case)[mi])
            sim.set_failed(last_mask)
            ref = reference(oracle, case, pi)
            if case.get("cap"):
                sim.set_payload(case["cap"]["B"], case["cap"]["pick"])
                sim.begin_rumors(senders_of(case, sender), case["cap"]["starts"])
            elif case["family"] == "rumorset":
                sim.begin_rumors(senders_of(case, sender))
            else:
                sim.broadcast_begin(sender)
            compare(sim, case, ref, f"{where}: round 0")
            for t in range(1, case["rounds"] + 1):
                row, got = ref.step(), [int(x) for x in sim.step(1)[0]]
                assert got == row, f"{where}: round {t}: stats row {got}, reference {row}"
                compare(sim, case, ref, f"{where}: round {t}")
            tot = sim.totals()
            assert tot["tick"] == case["rounds"] and tot["received"] == row[4] and tot["pending"] == row[6] and \
                tot["crashed"] == row[5], f"{where}: totals {tot}, last row {row}"


def main():
    family = sys.argv[1]
    import gossip_simulator_amd as gs
    from gossip_simulator_amd import _lib
    from oracle import pyoracle
    pyoracle.build()
    gs.load()
    failures, device_error, t0 = [], None, time.time()
    for case in CASES[family]:
        os.environ.update(case.get("env", {}))  # (read per broadcast)
        try:
            run_case(gs, pyoracle, case)
        except AssertionError as e:  # a wrong value: the other cases still run
            failures.append(str(e)[:600])
        except gs.GossipError as e:  # the library refused or the device failed: nothing more runs here
            failures.append(f"{case['name']}: {e}"[:600])
            if e.code == _lib.GS_EDEVICE:
                device_error = str(e)[:300]
            break
        finally:
            for k in case.get("env", {}):
                os.environ.pop(k, None)
    print(json.dumps(dict(family=family, poison=os.environ.get("GS_DEVMEM_POISON"), cases=len(CASES[family]),
                          failures=failures, device_error=device_error, seconds=round(time.time() - t0, 2))))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
