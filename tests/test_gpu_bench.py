"""A plain `bench.py` run as the driver makes it (a child process, one GPU): the result line
holds the headline figures and nothing that takes a run of its own, --steps sets the timed steps,
and --dump-outputs writes what the timed path computed -- checked bit for bit against a
general-kernel plan of the same workload built here (C4 reduced: 8k peaks x 1000 bins, 2M reads;
the matrix is 64 MB, so the dump holds a sample of its rows)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from recoup_amd.engine import Plan, ReadSet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS, REGIONS, STEPS, SEED = 2_000_000, 8_000, 5, 7
FULL_ONLY = ("roofline", "cpu_baseline", "e2e", "gather", "kernel_ms", "heavy_rows", "n_overlaps", "parity_sample",
             "inflight_check")


def test_plain_run_line_and_dump(gpu, tmp_path):
    dump = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--reads", str(READS), "--regions", str(REGIONS),
                        "--seed", str(SEED), "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == "region-bins/sec (profileMatrix)" and res["unit"] == "region-bins/s"
    assert res["higher_is_better"] is True and res["dtype"] == "int32" and res["n_gpus"] == 1
    assert res["steps"] == STEPS and res["full"] is False
    B = res["config"]["bins"]
    assert (res["config"]["regions"], B, res["config"]["reads"]) == (REGIONS, 1000, READS)
    # value = region-bins of the timed steps / their time; ms_per_step = that time / steps
    assert res["ms_per_step"] > 0
    assert res["value"] * res["ms_per_step"] * 1e-3 == pytest.approx(REGIONS * B, rel=1e-9)
    assert all(res[k] is None for k in FULL_ONLY), {k: res[k] for k in FULL_ONLY if res[k] is not None}

    prof = np.load(dump / "profile.npy")
    rows = np.load(dump / "profile_rows.npy")
    valid = np.load(dump / "valid.npy")
    assert prof.dtype == np.float64 and rows.dtype == np.float64 and valid.dtype == np.float32
    assert sorted(os.listdir(dump)) == ["profile.npy", "profile_rows.npy", "valid.npy"]
    assert prof.nbytes + rows.nbytes + valid.nbytes <= 64_000_000
    n = bench.DUMP_BYTES // (8 * B)
    assert n < REGIONS and prof.shape == (n, B) and rows.shape == (n,) and valid.shape == (n,)
    idx = rows.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < REGIONS

    # the same workload here (sample 0), on the general pileup kernel
    args = argparse.Namespace(config="c4", seed=SEED, reads=READS, regions=REGIONS)
    data, table, bins, _ = bench.workload(args, "cuda:0", counts=False)
    plan = Plan(ReadSet(*data["reads"], data["seqlen"], device=0), table, bins, kernel="general")
    mat, v = plan.run()
    assert v.any() and mat[idx].any()
    np.testing.assert_array_equal(valid, v[idx].astype(np.float32))
    np.testing.assert_array_equal(prof.view(np.int64), np.ascontiguousarray(mat[idx]).view(np.int64))

