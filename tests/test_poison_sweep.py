"""Every engine bit-exact on dirty device allocations.

GS_DEVMEM_POISON=<byte> makes gs_dev_malloc fill every block it hands out
(gs_devmem.cpp), so a kernel or read-back that consumes a
byte nobody wrote sees the same wrong value in every process, not whatever the
driver happened to return.  The variable is read once per process:
tests/poison_worker.py runs one family at one byte in a child, and walks each
context through create, table, begin, rounds, reset, set_trial and a larger
table, checking every read-back against the project's references.

Two bytes, since one can coincide with a legal state: 0xFF is the median
model's "done", an empty slot id and a full bitset; 0x01 is B-1, degree 1 and
true.

Children run one at a time and the pytest process never has the variable set.
A child that ends by a signal or at its time limit is reported failed with its
last stderr lines, and every later case of the module skips: after a fault or
a hang nothing more starts on the card.

The time limit is a safety net, not an assertion.  Measured wall time per
child on an MI355X, process start to exit, the same at both bytes: 0.5 to
0.9 s for every family but flood_ring257 (2 x 3 x up to 2,000 ticks), 1.6 s.
TIMEOUT is about 40 times the slowest, for a cold start on a busy host.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import poison_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "poison_worker.py")
BYTES = ["0xFF", "0x01"]
TIMEOUT = 60  # seconds per child; measured: 0.5 to 1.6 s

_stopped: list = []   # why nothing more may start on the card


def test_at_most_16_children_per_byte():
    assert len(W.FAMILIES) <= 16 and all(W.CASES[f] for f in W.FAMILIES)
    for f in W.FAMILIES:  # a one-word case and a ragged multi-word case in every family with injected tables
        ns = {c["n"] for c in W.CASES[f]}
        if f.endswith("_shards"):  # two shards need whole 16384-node buckets: one node into the second
            assert ns == {16385}
        else:
            assert 4133 in ns and (65 in ns or f == "overlay"), (f, ns)


@pytest.mark.parametrize("family", W.FAMILIES)
def test_cases_are_worth_running(oracle, family):
    """The references alone: every phase of every case spreads past half of n
    (per rumor, for a set), its mask kills someone the broadcast would reach,
    and the table of phase 4 is bigger than the first by more than the 25 %
    slack grow() leaves, so a buffer sized by the table reallocates."""
    for case in W.CASES[family]:
        n, R = case["n"], case.get("R", 1)
        for pi, (ph, trial, ti, mi, sender) in enumerate(W.phases(case)):
            ref = W.reference(oracle, case, pi)
            row = None
            for _ in range(case["rounds"]):
                row = ref.step()
            T = case.get("trials", 1)
            assert row[4] > T * R * (n // 2), f"{case['name']}: {ph}: only {row[4]} received"
            got = ref.sets()
            for i in range(T):
                dead = W.trial_mask(case, mi, i) if T > 1 else W.masks(case)[mi]
                assert dead.any() and not dead[sender]
                words = got["received"][i] if T > 1 else got["received"]
                recv = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
                if R == 1:
                    assert not (recv & dead).any(), case["name"]
                    assert T > 1 or recv.sum() == row[4], case["name"]
                else:  # no dead node holds a rumor
                    assert not got["rumor_words"][dead].any(), case["name"]
                # somebody live names a dead node: the mask changes the run
                deg, ids = (W.trial_tables(case, ti, i) if case["family"] != "overlay"
                            else oracle.overlay(oracle.make_params(**W.kw_of(case, trial)))[:2])
                named = np.zeros(n, bool)
                m = (np.arange(ids.shape[1])[None, :] < deg[:, None]) & ~dead[:, None]
                named[ids[m]] = True
                assert (named & dead).any(), case["name"]
            if case.get("cap"):  # the cap binds: messages wanted more than they carried
                e = ref.e
                assert e.bound > 0 and e.carried < e.wanted, f"{case['name']}: {ph}: the cap never bound"
                assert max(case["cap"]["starts"]) > 0 and len(set(W.senders_of(case, sender))) < R
        if case["family"] != "overlay":
            (d1, i1), (d2, i2) = W.tables(case)
            assert i2.nbytes > i1.nbytes * 1.25 and i2.shape[1] != i1.shape[1]
            assert int(d2.astype(np.int64).sum()) > int(d1.astype(np.int64).sum()) * 1.25  # and so are its edges


def test_rumor_set_leaves_a_bit_unset(oracle):
    """R = 63: bit 63 of every word must stay 0 whatever the buffers held."""
    case = [c for c in W.CASES["rumorset"] if c["R"] == 63 and c["n"] == 4133][0]
    ref = W.reference(oracle, case, 0)
    for _ in range(case["rounds"]):
        ref.step()
    have = ref.sets()["rumor_words"]
    assert int(have.max()) >> 63 == 0 and (have >> np.uint64(62)).any()  # its neighbour, bit 62, is in use


def _env(byte):
    env = {k: v for k, v in os.environ.items() if k != "GS_DEVMEM_POISON"}
    env["GS_DEVMEM_POISON"] = byte
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("byte", BYTES)
def test_poisoned(byte, family):
    assert "GS_DEVMEM_POISON" not in os.environ, "the pytest process itself must run unpoisoned"
    if _stopped:
        pytest.skip(_stopped[0])
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, WORKER, family], capture_output=True, text=True, timeout=TIMEOUT,
                           env=_env(byte), cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        _stopped.append(f"{family} at {byte} was still running after {TIMEOUT} s: nothing more starts on the card")
        pytest.fail(_stopped[0] + "\n" + "\n".join(err.splitlines()[-15:]))
    wall = time.time() - t0
    tail = "\n".join(p.stderr.splitlines()[-15:])
    if p.returncode < 0 or p.returncode in (134, 139):
        _stopped.append(f"{family} at {byte} ended by a signal (exit {p.returncode}): nothing more starts on the card")
        pytest.fail(_stopped[0] + "\n" + tail)
    assert ("[devmem] poison 0x%02X" % int(byte, 0)) in p.stderr, f"the child ran unpoisoned\n{tail}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, f"no result line (exit {p.returncode})\n{tail}"  # (a Python error before any case: no fault)
    res = json.loads(lines[-1])
    print(f"{family} at {byte}: {res['cases']} cases, {res['seconds']} s of cases, {wall:.1f} s wall")
    if res.get("device_error"):  # the library reported a HIP error: a fault, whatever the exit status
        _stopped.append(f"{family} at {byte}: {res['device_error']}: nothing more starts on the card")
        pytest.fail(_stopped[0] + "\n" + tail)
    assert res["poison"] == byte and res["cases"] == len(W.CASES[family])
    assert p.returncode == 0 and not res["failures"], "\n".join(res["failures"]) + "\n" + tail
