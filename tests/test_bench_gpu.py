"""bench.py on one GPU: a plain run prints its headline and measures nothing else; `--full` adds the roofline after the SAME timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True, timeout=240,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_and_full_measures_after_the_same_steps(tmp_path):
    # (three warm-up steps: the engine captures its graphs at the third, so the timed steps are replays in both runs)
    plain = _bench("--steps", "3", "--warmup", "3", "--dump-outputs", str(tmp_path / "plain"))
    assert plain["full"] is False and plain["roofline"] is None and plain["executed_tflop_per_step"] is None and plain["ranks"] is None
    assert "cpu_baseline" not in plain and plain["hip_graph"] is True
    assert plain["unit"] == "train-steps/sec" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and plain["value"] * plain["ms_per_step"] == pytest.approx(1e3)
    full = _bench("--steps", "3", "--warmup", "3", "--full", "--no-cpu-baseline", "--prof-steps", "1", "--dump-outputs", str(tmp_path / "full"))
    assert full["full"] is True and full["roofline"]["kernel"] and full["executed_tflop_per_step"] > 0 and "cpu_baseline" not in full
    # what the timed steps computed does not depend on --full: the instrumented steps come after the outputs are taken
    assert plain["losses"] == full["losses"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)), n
