"""bench.py --dump-outputs: what it writes for arrays of the headline workload's shapes (CPU tensors; no GPU needed)."""
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def headline_arrays():
    P, W, H = 500_000, 1920, 1080
    g = torch.Generator().manual_seed(3)
    return {"out_color": torch.rand(3, H, W, generator=g), "out_radii": torch.randint(0, 40, (P,), dtype=torch.int32, generator=g),
            "out_depth": torch.rand(1, H, W, generator=g), "grad_shs": torch.randn(P, 16, 3, generator=g),
            "grad_means3D": torch.randn(P, 3, generator=g), "grad_viewmatrix": torch.randn(4, 4, generator=g)}


def test_dump_stays_in_budget_and_repeats(tmp_path):
    t = headline_arrays()
    r1 = bench.dump_outputs(str(tmp_path / "a"), t)
    r2 = bench.dump_outputs(str(tmp_path / "b"), t)
    files = sorted(glob.glob(str(tmp_path / "a" / "*.npy")))
    assert [os.path.basename(f)[:-4] for f in files] == sorted(t)
    assert sum(os.path.getsize(f) for f in files) == r1["bytes"] <= bench.DUMP_BUDGET_BYTES < 64_000_000
    assert r1["arrays"] == r2["arrays"]
    for f in files:
        a, b = np.load(f), np.load(f.replace(os.sep + "a" + os.sep, os.sep + "b" + os.sep))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    # small arrays are written whole, in their shape; integer outputs exactly, as float64
    assert np.array_equal(np.load(tmp_path / "a" / "grad_viewmatrix.npy"), t["grad_viewmatrix"].numpy())
    radii = np.load(tmp_path / "a" / "out_radii.npy")
    assert radii.dtype == np.float64 and np.array_equal(radii, t["out_radii"].numpy())
    # a large array is a sample of its own values, at the seeded indices the docstring names
    sh = np.load(tmp_path / "a" / "grad_shs.npy")
    n = r1["arrays"]["grad_shs"]["sampled_elements"]
    assert sh.shape == (n,) and 0 < n < t["grad_shs"].numel()
    idx = np.sort(np.random.default_rng(0).choice(t["grad_shs"].numel(), n, replace=False))
    assert np.array_equal(sh, t["grad_shs"].numpy().reshape(-1)[idx])
