"""bench.py's plain run: exactly --steps timed steps, the headline line without the legs of --full, and --dump-outputs writing what the last
timed step returned to its caller (solved state and summary), float64, consistent with the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    rows = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and rows, out.stdout[-2000:] + out.stderr[-4000:]
    r = json.loads(rows[-1])
    assert r["steps"] == 3 and r["value"] > 0 and r["ms_per_step"] > 0 and r["unit"] == "iterations/s" and r["dtype"] == "f64" and r["higher_is_better"] is True, r
    assert not {"repeats", "roofline", "pcie_inclusive", "configs2_window", "configs3_window", "cpu_baseline"} & set(r), sorted(r)
    a = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(a) == {"pose", "speedbias", "ex_pose", "td", "inv_depth", "summary", "cost_trace", "radius_trace"}, sorted(a)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) < 64 << 20
    assert a["pose"].shape == (10, 7) and a["speedbias"].shape == (10, 9) and a["inv_depth"].shape == (1000,)
    assert np.allclose(np.linalg.norm(a["pose"][:, 3:], axis=1), 1.0, atol=1e-6)
    its, succ, term, c0, c1 = a["summary"]
    cfg = r["config"]
    assert its == cfg["iterations_per_solve"] and c1 == cfg["final_cost"] and c1 < c0, (a["summary"], cfg)
    assert len(a["cost_trace"]) == len(a["radius_trace"]) == its
