"""CPU: bench.py's --dump-outputs writer and option checks (no GPU: the writer takes any torch tensors)."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_samples_large_arrays_within_budget_and_repeats(tmp_path):
    """arrays shaped like a C2 step's outputs (32 volumes of 64^3, T = 10): every file float32 unless float64, the whole dump
    under 64 MB, small arrays whole and in shape, large ones a sample that is the same on every call"""
    bench = _bench()
    V, S, T = 32, 64, 10
    g = torch.Generator().manual_seed(0)
    out = {"pred_entropy": torch.rand((V, S, S, S), generator=g),
           "mean_softmax": torch.rand((V, 2, S, S, S), generator=g),
           "pred_seg_mean": (torch.rand((V, S, S, S), generator=g) > 0.5).to(torch.uint8),
           "logits": torch.randn((V * T, 2, S, S, S), generator=g),
           "extra": [torch.arange(10, dtype=torch.float64).view(2, 5), None]}
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(argparse.Namespace(dump_outputs=str(d)), 0, out)
    names = sorted(os.listdir(dirs[0]))
    assert names == ["extra.0.npy", "logits.npy", "mean_softmax.npy", "pred_entropy.npy", "pred_seg_mean.npy"]
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64 * 10 ** 6
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype == (np.float64 if n == "extra.0.npy" else np.float32)
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(dirs[0] / "extra.0.npy"), out["extra"][0].numpy())
    # a sampled array holds elements of its source: the seg mask stays 0 / 1, the probabilities in [0, 1)
    seg = np.load(dirs[0] / "pred_seg_mean.npy")
    assert seg.ndim == 1 and 0 < seg.size < V * S ** 3 and set(np.unique(seg)) <= {0.0, 1.0}
    # only rank 0 writes
    bench.dump_outputs(argparse.Namespace(dump_outputs=str(tmp_path / "r1")), 1, out)
    assert not os.path.exists(tmp_path / "r1")


def test_detail_needs_the_full_run():
    """--detail is the roofline leg's per-kernel table: a plain run has no roofline leg, so the option is refused at parse time"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--detail", "x.json"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 2 and "--full" in p.stderr
