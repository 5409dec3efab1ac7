"""examples/mapping.py --tsdf VOXEL [--mesh-out PATH] at a small size: after the last iteration the window's keyframes are
rendered once more, fused into a TSDF volume around the map in one slam.tsdf_integrate call and extracted with
slam.extract_mesh; the run reports a positive triangle count and a finite area, and the PLY's header counts match."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

P, W, H, KEYFRAMES, ITERS = 2000, 64, 48, 2, 8


def test_tsdf_reports_a_mesh_and_writes_it(monkeypatch, tmp_path):
    from mapping import mapping_loop
    monkeypatch.setenv("DGR_SYNC_MODE", "strict")
    lines, path = [], tmp_path / "mesh.ply"
    (first, last), pc, _ = mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, views_in_flight=1, log=lines.append, tsdf=0.05,
                                        mesh_out=str(path))
    t = pc.tsdf
    report = [ln for ln in lines if ln.startswith("tsdf: ")]
    print(report)
    assert math.isfinite(last) and t["triangles"] > 0 and math.isfinite(t["area"]) and t["area"] > 0
    assert report == [f"tsdf: {t['dims'][0]}x{t['dims'][1]}x{t['dims'][2]} voxels, {t['triangles']} triangles, area {t['area']:.4f}"]
    assert t["mesh"].count.tolist() == [t["triangles"]] and tuple(t["mesh"].colors.shape) == (3 * t["triangles"], 3)
    text = path.read_text().split("\n")
    head = text[:text.index("end_header")]
    assert head[0] == "ply" and f"element vertex {3 * t['triangles']}" in head and f"element face {t['triangles']}" in head
    body = [ln for ln in text[len(head) + 1:] if ln]
    assert len(body) == 4 * t["triangles"] and len(body[0].split()) == 6 and body[-1].split()[0] == "3"


def test_mesh_out_needs_tsdf():
    from mapping import mapping_loop
    with pytest.raises(ValueError, match="mesh_out"):
        mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, mesh_out="mesh.ply")
    with pytest.raises(ValueError, match="tsdf"):
        mapping_loop(torch.device("cuda:0"), P, W, H, KEYFRAMES, ITERS, tsdf=-0.05)
