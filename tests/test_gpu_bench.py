"""bench.py's plain run on the engine: `--gpus 1 --steps K --warmup W` prints the headline line and
nothing that takes runs of its own (those are --full's), K is the number of timed steps, and
--dump-outputs writes the last step's records -- checked here against the oracle on every row of
a 5 % cfg4 workload (50 000 loci: from 32 768 loci up the engine picks the lane kernel, as on
the full workload)."""
import json
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "index_build", "cpu_baseline", "work", "records_verified", "parity_sample")


def test_plain_run_is_lean_and_dumps_the_records(tmp_path):
    import oracle_ffi as O
    from svtrek_amd import sim
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--scale", "0.05", "--dump-outputs", str(tmp_path / "d")], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["full"] is False and not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 4 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["metric"] == "refined SV loci/sec (whole node)" and out["unit"] == "loci/s"
    assert out["higher_is_better"] is True and out["dtype"] == "int32"
    n = out["config"]["loci_total"]
    assert 32768 <= n <= 50000 and out["ms_per_step"] > 0
    # value = loci / step time; ms_per_step is printed to 1e-4 ms, 1 % of a 0.01 ms step (this one takes longer)
    assert out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3), rel=1e-2)
    assert out["engine_lib"]["path"] == os.path.join("svtrek_amd", "libsvtrek_hip.so")
    rec = np.load(tmp_path / "d" / "records.npy")
    assert rec.dtype == np.float64 and rec.shape == (n, 3) and out["outputs"]["records.npy"]["rows"] == n
    cfg = sim.WORKLOADS["cfg4_1m_delins_30x_hifi"]
    res = sim.generate(replace(cfg, n_loci=n))
    want = O.refine_batch(res.pileup, res.loci, threads=8)
    idx = rec[:, 0].astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(n))
    np.testing.assert_array_equal(rec[:, 1], want["start"][idx].astype(np.float64))
    np.testing.assert_array_equal(rec[:, 2], want["end"][idx].astype(np.float64))
