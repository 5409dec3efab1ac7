"""Time per call of slam.contribution_stats (its three launches: clear, tiles, fold) replayed from a hipGraph, beside the time of
the forward blend kernel of the same frame from the library's own stage profiler:
    python profiles/contrib/timing.py [P:W:H[:variant] ...]      (default 100000:640:480 500000:1920:1080, light and full)
synth-v1 scenes as bench.py renders them (make_scene, seed 3)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import hip_helpers as hh  # noqa: E402
from dgr_amd import _capi, slam  # noqa: E402
from dgr_amd.synth import make_scene  # noqa: E402


def one(P, W, H, variant, replays=50, forwards=10):
    s = make_scene(P, W, H, 3)
    forward = (lambda: hh.hip_forward(s, 3)[0]) if variant == "light" else (lambda: hh.hip_full_forward(s, 3)[0])
    forward()
    torch.cuda.synchronize()
    _capi.profile_select("render_fwd")
    _capi.profile_read("render_fwd")
    for _ in range(forwards):
        out = forward()
    torch.cuda.synchronize()
    blend_ms, launches = _capi.profile_read("render_fwd")
    _capi.profile_select("")
    blend_ms /= max(launches, 1)
    geom, binning, img = out[7:10] if variant == "light" else out[6:9]
    acc = slam.ContributionAccumulator(P, hh.dev())
    stats = lambda: slam.contribution_stats(geom, binning, img, P, H, W, out[0], into=acc, frame_id=1)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stats()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = stats()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):  # five windows: their spread stands beside the mean
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(replays):
            graph.replay()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / replays)
    ms = sum(times) / len(times)
    touched, observed, overflowed, _ = st.counts.tolist()
    pairs = int(st.n_touched.long().sum())
    tags = hh.hip_state("contribution_tags", s, dict(num_rendered=out[0], geom=geom, binning=binning, img=img))
    live = int((tags != 0).sum())
    print(f"{variant} P={P} {W}x{H}: contribution_stats {ms * 1e3:.1f} us per call (hipGraph replay, 5 x {replays} replays, windows "
          f"{min(times) * 1e3:.1f} .. {max(times) * 1e3:.1f} us); forward blend (render_fwd, stage profiler, {launches} launches) "
          f"{blend_ms * 1e3:.1f} us; ratio {ms / blend_ms:.2f}; num_rendered {out[0]}, live (tile, Gaussian) instances {live} "
          f"({16 * live / (ms * 1e-3) / 1e9:.2f} GB/s of atomic payload over the whole call), blended pairs {pairs}, "
          f"Gaussians touched {touched} of {P}, overflowed {overflowed}")


if __name__ == "__main__":
    specs = sys.argv[1:] or ["100000:640:480:light", "100000:640:480:full", "500000:1920:1080:light", "500000:1920:1080:full"]
    for spec in specs:
        f = spec.split(":")
        one(int(f[0]), int(f[1]), int(f[2]), f[3] if len(f) > 3 else "light")
