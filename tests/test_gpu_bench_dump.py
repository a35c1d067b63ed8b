"""bench.py --dump-outputs: the scores its last timed step returned, saved as DIR/scores.npy.  The inputs are seeded, so the
dump is the same from run to run; `--steps` is the number of timed steps (the line says so), and the last of 3 steps and the
last of 7 score the same seeded buffer (bufs[2]: 3 buffers at 3 steps, 4 at 7, drawn from one generator)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, steps):
    out = tmp_path / f"steps{steps}"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--ckpt", "tiny", "--batch", "48", "--prompts", "20",
                        "--quick", "--no-profile", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out),
                        "--detail", str(tmp_path / f"detail{steps}.json")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    return line, np.load(out / "scores.npy")


def test_dump_outputs_is_the_last_step_and_repeats(tmp_path):
    line3, a = _bench(tmp_path, 3)
    line7, b = _bench(tmp_path, 7)
    assert line3["steps"] == 3 and line7["steps"] == 7
    assert a.dtype == np.float32 and a.shape == (48,) and np.isfinite(a).all()
    assert np.array_equal(a, b)
    assert len(np.unique(a)) > 1   # 48 different images, not one value broadcast
