"""bench.py without --full: the timed leg and the headline only (no kernel timing, roofline, box probe, extra legs or CPU baselines), and
--dump-outputs: what the timed path computed in its last step, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    K, Wm = 6, 2
    runs = []
    for i in range(2):
        out = tmp_path / ("out%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(Wm),
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["unit"] == "triplets/s" and d["higher_is_better"] is True and d["dtype"] == "f16" and d["metric"].startswith("triplets/sec")
        assert d["steps"] == K and d["warmup"] == Wm and 0 < d["final_loss"] < 16
        assert abs(d["value"] - 1024 * 50 * K / (d["ms_per_step"] * K * 1e-3)) <= 1e-6 * d["value"]
        assert d["roofline"] is None and d["kernels_ms"] is None and d["box"] is None
        for k in ("cpu_baseline", "gpu_path_only", "step_ms_stats", "dense_execution", "bf16_execution", "dropout_execution"):
            assert k not in d, k
        names = sorted(os.listdir(out))
        assert names == sorted(n + ".npy" for n in ("loss", "violations", "W", "b", "W_history", "b_history"))
        assert sum(os.path.getsize(out / n) for n in names) <= 64 << 20
        a = {n[:-4]: np.load(out / n) for n in names}
        assert all(v.dtype in (np.float32, np.float64) for v in a.values())
        assert a["W"].shape == a["W_history"].shape == (512, 4096) and a["b"].shape == (512,)
        assert a["loss"][0] == d["final_loss"] and a["violations"][0] == d["final_violations"]
        assert np.isfinite(a["W"]).all() and np.abs(a["W_history"]).max() > 0
        runs.append(a)
    for n, v in runs[0].items():
        assert np.array_equal(v, runs[1][n]), n
