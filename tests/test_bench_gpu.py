"""GPU: the plain one-GPU run of bench.py -- exactly `--steps` timed steps, the headline fields and nothing of `--full` -- and
`--dump-outputs`: the proof of the last timed step, equal to the proof of the same seeded step proven in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_proof(ctx, tmp_path):
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload

    k, steps = 14, 3
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--k", str(k),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and len(line["step_ms_all_this_rank"]) == steps
    assert line["unit"] == "Mscalar/s" and line["higher_is_better"] is True and line["dtype"] == "u256-montgomery"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] - line["config"]["msm_scalars_per_proof"] / (line["ms_per_step"] / 1e3) / 1e6) < 1e-6 * line["value"]
    for key in ("roofline", "roofline_ntt", "config3_k20", "cpu_baseline", "batched", "generic_rng"):
        assert key not in line, key  # --full only
    assert sorted(os.listdir(out)) == ["proof.npy"]
    got = np.load(out / "proof.npy")
    assert got.dtype == np.float64 and got.ndim == 1
    wl = ShaCqWorkload(ctx, k, seed=0x5348413243515F)
    wl.fill_witness()
    expected = wl.prove(seed=1000 + steps - 1)
    wl.close()
    assert got.size == len(expected) and bytes(got.astype(np.uint8)) == expected
