"""bench.py without --full: one JSON line whose check, roofline and CPU-baseline fields are null, --steps timed steps, and
--dump-outputs DIR: the lists the last timed step returned, as float .npy files that are the same from one run to the next
(same arguments, same seeded inputs), whatever the number of steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--steps", str(steps), "--warmup", "1",
           "--streams", "3", "--recall-queries", "512", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_lists(cuda, tmp_path):
    a = _run(tmp_path / "a", 2)
    b = _run(tmp_path / "b", 5)
    assert (a["steps"], b["steps"]) == (2, 5) and a["ms_per_step"] > 0 and a["value"] > 0
    c = a["config"]
    assert c["check_ok"] is None and c["recall_at_10_vs_fp32"] is None and a["roofline"] is None and a["cpu_baseline"] is None
    k, nq = c["top_k"], c["queries_per_step"]
    got = {}
    for name in ("scores", "ids", "status"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        got[name] = x
    s, i = got["scores"], got["ids"]
    assert s.shape == (nq, k) and i.shape == (nq, k) and got["status"].shape == (nq,)
    assert (i >= 0).all() and (i < c["corpus_rows"]).all() and (i == np.round(i)).all()
    assert (np.diff(s, axis=1) <= 0).all() and (s <= 1 + 1e-5).all()
    assert set(np.unique(got["status"]).tolist()) <= {0.0, 1.0}      # every list proven or escalated
