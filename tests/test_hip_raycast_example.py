"""examples/mapping.py --tsdf VOXEL --raycast at a small size: after the fusion the volume is ray-cast at the fused keyframes' poses
(slam.tsdf_raycast); the run logs one line with the share of pixels that hit the surface and the mean |rendered depth - ray-cast
depth| over the pixels where both are valid, keeps both on the model's `tsdf` attribute, and the difference stays below a voxel."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

P, W, H, KEYFRAMES, ITERS, VOXEL = 2000, 64, 48, 2, 8, 0.05


def test_raycast_reports_the_hit_share_and_the_depth_difference(monkeypatch):
    from mapping import mapping_loop
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    lines = []
    (first, last), pc, _ = mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, views_in_flight=1, log=lines.append, tsdf=VOXEL,
                                        raycast=True)
    t = pc.tsdf
    report = [ln for ln in lines if ln.startswith("raycast: ")]
    print(report)
    assert report == [f"raycast: hit share {t['hit_share']:.4f}, mean |rendered - ray-cast depth| {t['depth_diff']:.5f}"]
    assert math.isfinite(last) and 0.0 < t["hit_share"] <= 1.0 and 0.0 <= t["depth_diff"] < VOXEL
    assert lines.index(report[0]) == lines.index([ln for ln in lines if ln.startswith("tsdf: ")][0]) + 1


def test_raycast_needs_tsdf(monkeypatch, capsys):
    from mapping import main, mapping_loop
    with pytest.raises(ValueError, match="raycast"):
        mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, raycast=True)
    monkeypatch.setattr(sys, "argv", ["mapping.py", "--raycast", "--iters", "4"])
    with pytest.raises(SystemExit) as exit_:
        main()
    assert exit_.value.code == 2 and "--raycast looks at the volume that --tsdf VOXEL fuses" in capsys.readouterr().err
