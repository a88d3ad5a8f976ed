"""bench.py's plain run and `--dump-outputs`.

CPU: the bitset digests of dump_outputs against numpy's own bit unpacking, and
the option table (`--full` off by default, `--steps` at least 1).  GPU: two
plain runs with the same arguments write the same arrays, the arrays agree
with the line, `--steps` sets the number of timed steps, and a plain run's
line carries the headline keys with nothing behind `--full` in it.
"""
from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("poll_stats", "totals", "status", "sample_nodes", "received_sample", "crashed_sample",
         "received_per_block", "crashed_per_block")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [1, 63, 64, 4096, 4097, 3 * 4096 + 65])
def test_bitset_views_match_unpackbits(n):
    b = _bench()
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2, size=n, dtype=np.uint8)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = bits
    words = np.packbits(padded, bitorder="little").view("<u8")
    ids = np.unique(rng.integers(0, n, size=min(n, 500), dtype=np.int64))
    sample, per_block = b.bitset_views(words, n, ids)
    assert sample.dtype == np.float32 and per_block.dtype == np.float32
    assert np.array_equal(sample, bits[ids].astype(np.float32))
    blocks = (n + b.DUMP_BLOCK - 1) // b.DUMP_BLOCK
    full = np.zeros(blocks * b.DUMP_BLOCK, dtype=np.uint8)
    full[:n] = bits
    assert np.array_equal(per_block, full.reshape(blocks, b.DUMP_BLOCK).sum(axis=1).astype(np.float32))


def _parse(b, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return b.parse()


def test_full_is_off_by_default_and_steps_must_be_positive(monkeypatch):
    b = _bench()
    a = _parse(b, ["--gpus", "1", "--steps", "4", "--warmup", "2"], monkeypatch)
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    a = _parse(b, ["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        _parse(b, ["--steps", "0"], monkeypatch)


def _run(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_arrays_twice(tmp_path):
    n = 300_001  # more than one block of the digests, not a multiple of 64
    args = ["--nodes", str(n), "--warmup", "1"]
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    one = _run(args + ["--steps", "3", "--dump-outputs", d1])
    two = _run(args + ["--steps", "1", "--dump-outputs", d2])
    for line, steps in ((one, 3), (two, 1)):
        assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "msgs/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
        assert line["metric"].startswith("gossip messages delivered/sec")
        # nothing that --full adds ran
        assert line["roofline"] is None and line["extensions"] is None and line["cpu_baseline"] is None
        assert "strong_scaling" not in line
    # value = counted messages of all timed steps / their time
    msgs = one["config"]["messages_per_step"]
    assert one["value"] == pytest.approx(msgs * 3 / (one["ms_per_step"] * 3e-3), rel=1e-3)
    assert sorted(os.listdir(d1)) == sorted(f"{k}.npy" for k in NAMES)
    a = {k: np.load(os.path.join(d1, f"{k}.npy")) for k in NAMES}
    b = {k: np.load(os.path.join(d2, f"{k}.npy")) for k in NAMES}
    for k in NAMES:
        assert a[k].dtype in (np.float32, np.float64)
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    # the arrays are the step the line reports
    tick, _fired, sent, messages, received, crashed, _pending = a["totals"]
    assert messages == msgs and sent == one["config"]["delivered_per_step"] and tick == one["config"]["ticks"]
    last = a["poll_stats"][-1]  # one row per 10-tick poll; tick, received and crashed are running figures
    assert a["poll_stats"].ndim == 2 and a["poll_stats"].shape[1] == 7
    assert (last[0], last[4], last[5]) == (tick, received, crashed)
    assert np.array_equal(a["sample_nodes"], np.arange(n))  # n below the sample size: every node
    assert a["received_sample"].sum() == received == a["received_per_block"].sum()
    assert a["crashed_sample"].sum() == crashed == a["crashed_per_block"].sum()
    assert a["received_per_block"].shape == ((n + 4095) // 4096,)
