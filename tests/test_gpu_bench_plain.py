"""bench.py's plain run next to --full: a plain run times the `value` region and reports it, nothing else (no `resident` region, no
verification, no CPU baseline); `--dump-outputs DIR` writes the proofs of the last timed step as DIR/proofs.npy.  With the same arguments
both runs prove the same statements with the same blinding scalars, so their dumps are the same bytes — and the --full run has checked
every one of its timed proofs with the batch verifier and the last one against the oracle's closed form.  Run with `-m gpu`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3


def _bench(extra_args, out_dir):
    env = dict(os.environ, MASP_BENCH_E2E="0", MASP_BENCH_OTHER="0", MASP_BENCH_LONE="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                          "--dump-outputs", str(out_dir)] + extra_args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_value_only_and_dumps_the_proofs_a_full_run_verifies(tmp_path):
    plain = _bench([], tmp_path / "plain")
    full = _bench(["--full", "--no-cpu-baseline"], tmp_path / "full")
    for d in (plain, full):
        assert d["metric"] == "Spend proofs/sec" and d["unit"] == "proofs/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
        assert d["steps"] == STEPS and d["warmup"] == 1 and d["n_gpus"] == 1 and d["value"] > 0
        assert abs(d["ms_per_step"] - 256e3 / d["value"]) <= 1e-3 * d["ms_per_step"]      # one step = 256 proofs
    assert plain["full"] is False and not {"resident", "verified", "cpu_baseline", "roofline", "end_to_end"} & set(plain)
    assert full["full"] is True and full["verified"] == STEPS * 256 and full["closed_form_equal"] == 4 and full["resident"]["value"] > 0
    a, b = np.load(tmp_path / "plain" / "proofs.npy"), np.load(tmp_path / "full" / "proofs.npy")
    assert a.dtype == np.float32 and a.shape == (256, 192) and np.array_equal(a, b)
    assert a.min() >= 0 and a.max() <= 255 and np.array_equal(a, np.round(a))
    assert len({row.tobytes() for row in a.astype(np.uint8)}) == 256                          # 256 distinct proofs
