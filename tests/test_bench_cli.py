"""bench.py command line: ``--full`` / ``--dump-outputs`` parsing and the output dump (CPU only)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_defaults(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_is_float32_seeded_and_bounded(tmp_path):
    torch.manual_seed(0)
    params = [torch.randn(300, 200, dtype=torch.bfloat16), torch.randn(5), torch.randn(64, 64)]
    losses = [torch.tensor(2.5, dtype=torch.bfloat16), torch.tensor(1.25)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, losses[-1], losses, params)
    out = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(out) == ["loss.npy", "loss_curve.npy", "params_sample.npy"]
    assert all(v.dtype == np.float32 for v in out.values())
    assert out["loss.npy"].tolist() == [1.25] and out["loss_curve.npy"].tolist() == [2.5, 1.25]
    k = bench.DUMP_SAMPLE_PER_PARAM
    assert out["params_sample.npy"].shape == (k + 5 + min(k, 64 * 64),)
    # every sampled value is an element of its parameter; the same indices on every call
    assert np.isin(out["params_sample.npy"][:k], params[0].float().numpy()).all()
    assert np.array_equal(out["params_sample.npy"], np.load(tmp_path / "b" / "params_sample.npy"))
    assert bench.DUMP_SAMPLE_PER_PARAM * 4 <= bench.DUMP_MAX_BYTES < 64 << 20
