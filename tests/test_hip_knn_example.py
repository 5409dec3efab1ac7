"""examples/mapping.py --seed --knn-scale at its smallest size, through the example's own main(): the run reaches its end, and the
log-scales each seeding set equal the twin's 0.5 log(max(dist2, 1e-7)) over the map as it was then (tests/knn_model.py) within
4 ulp -- the bar seed_from_frame's logf already has in tests/test_hip_seed.py, for the same reason: logf is a 1-ulp function of an
argument that already carries a rounding (here the mean's: a relative 2^-24 of the argument moves 0.5 log by 2^-25, half an ulp
of a result of magnitude >= 0.5, which the test asserts of its scene)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import knn_model as M

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

P, W, H, KEYFRAMES, ITERS = 2000, 64, 48, 2, 12
SMALL = ["--gaussians", str(P), "--width", str(W), "--height", str(H), "--keyframes", str(KEYFRAMES), "--iters", str(ITERS),
         "--views-in-flight", "1"]


def test_the_seeded_rows_get_the_scale_of_their_three_nearest_neighbours(monkeypatch, capsys):
    import mapping
    seeds = []  # per seeding: rows before, the map's xyz then, the new rows' log-scales as set
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    monkeypatch.setattr(mapping, "mapping_loop", functools.partial(
        mapping.mapping_loop, on_knn_scale=lambda before, xyz, scaling: seeds.append((before, xyz.clone(), scaling.clone()))))
    monkeypatch.setattr(sys, "argv", ["mapping.py", "--seed", "--knn-scale", *SMALL])
    threaded = torch.autograd.is_multithreading_enabled()  # (main() turns it off for its process)
    try:
        mapping.main()
    finally:
        torch.autograd.set_multithreading_enabled(threaded)
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1].startswith("loss ") and "nan" not in lines[-1] and f"P 0 -> {len(seeds[-1][1])}" in lines[-1]
    assert len(seeds) == KEYFRAMES == len([ln for ln in lines if ln.startswith("knn-scale:")])
    rows_before = 0
    for before, xyz, scaling in seeds:
        xyz, got = xyz.cpu().numpy(), scaling.cpu().numpy()
        assert before == rows_before and len(xyz) - before == len(got) > 0 and got.shape[1] == 3
        rows_before = len(xyz)
        d2 = M.knn32(xyz, None, 3)[3].astype(np.float64)
        assert np.isfinite(d2).all()
        want = (0.5 * np.log(np.maximum(d2, np.float64(np.float32(1e-7)))))[before:].astype(np.float32)
        ulp = np.abs(got.astype(np.float64) - want.astype(np.float64)[:, None]) / np.spacing(np.abs(want)).astype(np.float64)[:, None]
        print(f"knn-measured: keyframe rows {before} -> {len(xyz)}: worst log-scale error {ulp.max():.2f} ulp (bound 4), scales "
              f"{np.exp(want.min()):.5f} .. {np.exp(want.max()):.5f}")
        assert ulp.max() <= 4.0 and float(np.abs(want).min()) >= 0.5
        assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()


def test_the_flag_needs_seeding(monkeypatch, capsys):
    import mapping
    with pytest.raises(ValueError, match="knn_scale"):
        mapping.mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, knn_scale=True)
    monkeypatch.setattr(sys, "argv", ["mapping.py", "--knn-scale", *SMALL])
    with pytest.raises(SystemExit):
        mapping.main()
    assert "--knn-scale sets the scale" in capsys.readouterr().err
