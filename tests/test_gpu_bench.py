"""bench.py as a plain run: --steps sets the number of timed steps the line reports, and --dump-outputs writes
exactly what the timed path computed in its last step for the benchmark's own seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_reports_its_steps_and_dumps_the_last_step(tmp_path):
    import torch

    from kyber_amd.group import edwards25519 as ed

    n, d = 4096, tmp_path / "out"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--n", str(n),
        "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "scalar-muls/s" and line["higher_is_better"] is True and line["value"] > 0
    assert "cpu_baseline" not in line and "bls12381_pairings_per_s" not in line
    assert not os.path.exists(tmp_path / "bench_detail.json")
    s, h = bench.make_inputs(n, 0)
    d_s = torch.from_numpy(s).cuda()
    fix = ed.batch_mul_base(d_s)
    var, st = ed.batch_mul(d_s, ed.batch_mul_base(torch.from_numpy(h).cuda()))
    for name, want in (("ed25519_fixed_base_points", fix), ("ed25519_var_base_points", var), ("ed25519_var_base_status", st)):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, want.cpu().numpy().astype(np.float32)), name
    assert not np.load(d / "ed25519_var_base_status.npy").any()
