"""bench.py without --full: exactly one JSON line with the headline fields over --steps timed steps and none of the --full legs; with
--dump-outputs DIR the last timed step's outputs as float32 / float64 .npy files, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"roofline", "g1_like_session_lengths", "native_fp32_mfma_arm", "through_boundary", "dp_self_exchange_ms", "bf16_arm",
             "adressa_arm", "stress_arm", "cpu_baseline", "accuracy_vs_cpu_ref", "dp"}


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-3000:])
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), "stdout must carry exactly one JSON line: %r" % lines[:5]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(gpu, tmp_path):
    a, b = _run(tmp_path / "a", 3), _run(tmp_path / "b", 3)
    for d in (a, b):
        assert d["metric"] == "NAR training sessions/sec" and d["unit"] == "sessions/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
        assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
        assert not FULL_ONLY & set(d), FULL_ONLY & set(d)
    arrays = a["dumped_outputs"]["arrays"]
    assert {"loss", "logits", "probs", "neg_items", "params", "grads", "recent_pop_norm", "recent_clicks_buffer"} <= set(arrays)
    total = 0
    for name, shape in arrays.items():
        x, y = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert x.dtype in (np.float32, np.float64) and list(x.shape) == shape and np.isfinite(x).all(), name
        total += x.nbytes
        if name in ("neg_items", "recent_pop_norm", "recent_clicks_buffer"):      # integer-valued / counts: exact
            assert np.array_equal(x, y), name
        else:
            np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-5, err_msg=name)
    assert total <= 64e6
    assert np.allclose(np.load(str(tmp_path / "a" / "loss.npy")), a["config"]["final_loss"], atol=1e-5)
    assert arrays["logits"] == [256, 19, 51] and arrays["neg_items"] == [256, 19, 50]
