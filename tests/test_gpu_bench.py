"""bench.py on the GPU at a small shape: a plain run carries the headline only, and
`--dump-outputs` holds what the timed step computed (the same seeded workload rebuilt
in this process gives the same arrays)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--arch", "ECAPA_TDNN_c512", "--batch", "3", "--seconds", "1"]


def test_plain_run_is_headline_only_and_dumps_last_step(tmp_path, monkeypatch):
    import torch
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", out] + SHAPE, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "emb/s" and res["higher_is_better"] is True
    assert abs(res["value"] - 3 / (res["ms_per_step"] * 1e-3)) / res["value"] < 0.01
    # the side measurements are --full's
    assert "configs" not in res
    for key in ("value_sustained", "value_exact_f32", "cpu_baseline", "kernel_roofline", "value_batch64"):
        assert res[key] is None, key

    emb, feats = np.load(os.path.join(out, "emb.npy")), np.load(os.path.join(out, "feats.npy"))
    assert sorted(os.listdir(out)) == ["emb.npy", "feats.npy"]
    assert emb.dtype == np.float32 and emb.shape == (3, 192)
    assert feats.dtype == np.float32 and feats.shape == (3, 98, 80)

    # the same workload, seeds and options in this process
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + SHAPE)
    w = bench.build_workload(bench.parse(), "ECAPA_TDNN_c512", 3, 0, torch.device("cuda", 0))
    w["step"]()
    torch.cuda.synchronize()
    # same kernels on the same inputs; the project's parity bound against the oracle
    # (|d emb| < 1e-4, fbank 1e-5) is the tolerance here too
    assert np.abs(w["feats"].cpu().numpy() - feats).max() < 1e-5
    assert np.abs(w["emb"].cpu().numpy() - emb).max() < 1e-4
    assert np.isfinite(emb).all() and np.abs(emb).max() > 0
    w["model"]._release()
