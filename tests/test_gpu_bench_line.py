"""bench.py's contract on a small C2 shape: one JSON line with the metric, roofline and CPU baseline
fields the driver and the judge read (run as a child process, as the driver runs it)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_bench_emits_one_contract_line():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch",
           str(1 << 18), "--keys", str(1 << 12), "--full", "--cpu-seconds", "0.5", "--no-extra"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    assert len(lines[0]) <= 8192   # the driver parses the line from a bounded stdout tail
    d = json.loads(lines[0])
    assert os.path.exists(os.path.join(ROOT, d["detail"]))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert d["unit"] == "events/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1
    assert d["cpu_baseline"]["value"] > 0
    # events/s = events of the timed steps over the timed wall time
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - (1 << 18)) / (1 << 18) < 1e-6


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """without --full: the headline line only (no other leg, no record beside it); --dump-outputs writes the
    matches of the last timed step, equal to those an engine fed the same stream batch by batch hands out"""
    import importlib

    import numpy as np
    B, K, steps, warm = 1 << 18, 1 << 12, 3, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warm), "--batch", str(B), "--keys", str(K), "--dump-outputs", str(tmp_path / "out")]
    # (two slices resident at a time: the timed steps run in two segments, the slices are dropped and refilled)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110,
                       env=dict(os.environ, SG_BENCH_WINDOW="2"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warm and d["value"] > 0 and d["dtype"] == "f32"
    assert d["unit"] == "events/s" and d["higher_is_better"] is True
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - B) / B < 1e-6
    assert 0 < d["roofline"]["frac"] < 1
    assert d["detail"] is None and "cpu_baseline" not in d and "extra" not in d and "stages_ms_isolated" not in d

    sa = importlib.import_module("siddhi-1_amd")
    synth = importlib.import_module("siddhi-1_amd.synth")
    app = sa.parse_app(synth.C2_QUERY)
    cq = sa.compile_query(app, app.queries[0], sa.StringDictionary())
    eng = sa.NativeEngine(sa.load_hip_library(), "sg_", cq.ir, n_keys=K, max_batch=B, partial_capacity=64,
                          match_capacity=2 * B)
    for s in range(warm + steps):
        t = synth.stock_ticks(s * B, B, K)
        eng.push(0, s * B, t["ts"], [t["symbol"], t["price"], t["volume"]], None, t["key"])
        m = eng.poll()
    eng.close()
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("n_matches", "trigger_seq", "key", "ts", "slot_seq",
                                                                "chain_len")}
    assert len(m) > 1000 and got["n_matches"].tolist() == [len(m)]
    assert int(m.trigger_seq.min()) >= (warm + steps - 1) * B
    for n in ("trigger_seq", "key", "ts", "slot_seq", "chain_len"):
        assert got[n].dtype == np.float64
        np.testing.assert_array_equal(got[n], getattr(m, n).astype(np.float64))
