"""bench.py's command line: a plain run times exactly --steps steps, leaves
the --full legs out, and --dump-outputs writes the last step's emissions.
One run (the setup dominates: a 512 MiB replay ring); needs an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_steps_fields_and_dump(tmp_path):
    dump = tmp_path / "dump"
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "250", "--warmup", "50", "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    r = json.loads(lines[0])
    assert r["metric"] == "nexmark_q5_rows_per_sec"
    assert r["unit"] == "rows/s" and r["higher_is_better"] is True
    assert r["dtype"] == "int64"
    assert r["steps"] == 250 and r["warmup"] == 50
    assert r["ms_per_step"] == pytest.approx(r["timed_s"] * 1000 / 250)
    assert r["value"] == pytest.approx(250 * 65536 / r["timed_s"])
    # legs that take runs of their own are behind --full
    assert r["cpu_baseline"] is None and r["boundary_host"] is None

    files = sorted(os.listdir(dump))
    assert files == ["emitted_rows.npy", "last_windows.npy"]
    assert sum(os.path.getsize(dump / f) for f in files) <= 64 << 20
    win = np.load(dump / "last_windows.npy")
    emitted = np.load(dump / "emitted_rows.npy")
    assert win.dtype == np.float64 and emitted.dtype == np.float64
    # [key, count, window_start, window_end, _timestamp]: 10 s windows that
    # have fired, every key counted at least once, no key twice per window
    assert win.ndim == 2 and win.shape[1] == 5 and win.shape[0] > 0
    assert np.all(win[:, 3] - win[:, 2] == 10e9)
    assert np.all(win[:, 1] >= 1)
    assert len(np.unique(win[:, [0, 2]], axis=0)) == win.shape[0]
    assert emitted.shape == (1,) and emitted[0] >= win.shape[0]
