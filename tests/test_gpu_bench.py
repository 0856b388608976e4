"""GPU: bench.py's command line itself.  A plain run prints the headline line without the
figures that need passes of their own and, with --dump-outputs, writes what its last timed
step computed; --full reports the per-stage pass, the roofline and the step detail as well."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4"]


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, capture_output=True,
                       text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    d = _bench(["--dump-outputs", str(tmp_path / "out")])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and not d["stages_ms"]
    assert d["steps_detail"] is None and d["batches_detail"] is None
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["conf.npy", "count.npy", "desc.npy", "matches.npy", "nmatch.npy", "xy.npy"]
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= 64 * 1000 * 1000
    a = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert {k: v.size for k, v in a.items()} == d["dumped_outputs"]
    cap = a["desc"].shape[1]
    assert a["count"].shape == (4,) and a["xy"].shape == (4, cap, 2) and a["desc"].shape == (4, cap, 128)
    assert a["nmatch"].shape == (3,) and a["matches"].shape == (3, cap, 2) and a["conf"].shape == (3, cap)
    assert (a["count"] > 0).all() and (a["count"] <= cap).all()
    assert (a["desc"] >= 0).all() and (a["desc"] <= 1).all()  # sqrt of an L2-normalised histogram
    for i, c in enumerate(a["count"].astype(int)):
        assert a["desc"][i, :c].any(axis=1).sum() > c // 2
        assert not a["desc"][i, c:].any() and not a["xy"][i, c:].any()
        assert (a["xy"][i, :c] >= 0).all() and (a["xy"][i, :c] < 1920).all()
    for p, n in enumerate(a["nmatch"].astype(int)):
        assert 0 < n <= min(a["count"][p], a["count"][p + 1])
        assert (a["matches"][p, :n, 0] < a["count"][p]).all() and (a["matches"][p, :n, 1] < a["count"][p + 1]).all()
        assert (np.diff(a["conf"][p, :n]) >= 0).all() and (a["conf"][p, :n] <= np.float32(0.85)).all()
        assert not a["matches"][p, n:].any() and not a["conf"][p, n:].any()


def test_full_run_reports_what_a_plain_run_leaves_out():
    d = _bench(["--full", "--cpu-sample", "0"])
    assert d["full"] is True and d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["roofline"]["kernel"] == "k_harris<7>" and d["roofline"]["launches"] == 3 * 4
    assert 0 < d["roofline"]["ms_per_step"] <= d["ms_per_step"] * 1.01
    assert {"harris", "nms", "describe", "match"} <= set(d["stages_ms"])
    assert len(d["steps_detail"]["end_ms"]) == 3
    assert d["batches_detail"]["value_same_batch_every_step"] > 0
    assert d["cpu_baseline"] is None
