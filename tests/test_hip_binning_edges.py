"""The designed frames of tests/binning_frames.py through the real forward: the binning state must be the oracle's bit for bit,
the segment binning, the global-counter binning ("lds_count" = 0) and the callback entry must agree on state and images, and
dgr_debug_bin_tiles_trace must show that every segment took the path it was designed for -- the designed instance count, pair
count and longest list, dense exactly where the design says so, and the segment size intended.  No expectation comes from the
kernels' own lists: the designs are verified against the oracle on the CPU (tests/test_binning_frames.py).

Edge -> frame: register networks 64/65 .. 512/513 and one wave up to 1024: rule, rule_flat; parts of 512 and the rank merge, 2048/2049
of the global-counter path: parts; segment total 6144/6145: budget (16-tile segments), groups; the dense group loop, a group of exactly
6144, a group of one, an empty tile, 6145 and 8193 in global memory: groups; short last segments and helpers without tiles: ragged*,
groups; coverage bytes and pairs << instances: spans; empty runs: runs; 24/25 pairs and the float division by 3, 5, 6, 7, 11, 13
segments: rectangles; a full queue: queue; more than 4096 Gaussians per bin_segments workgroup: reread.

(`!in_regs` -- more pairs than bin_tiles' registers hold -- implies gcount > K2_CAP, because every pair carries at least one
instance: there is no frame that is dense "by pairs" alone, so none is looked for.)

DGR_SEG_SHIFT is read once per process: in this process policy gives 4-tile segments for frames this small (asserted from the
trace); 8- and 16-tile segments run in a fresh child interpreter each, which calls the same binning_frames.check_frame."""
import json
import os
import subprocess
import sys

import pytest

import binning_frames as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(B.FRAMES))
def test_frame_at_four_tiles_per_segment(oracle, name):
    forced = os.environ.get("DGR_SEG_SHIFT", "")   # (a suite run under the A/B switch: that size, asserted all the same)
    assert B.check_frame(name, oracle, 1 << int(forced) if forced in ("2", "3", "4") else 4) == []


def test_frames_at_eight_and_sixteen_tiles_per_segment():
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binning_frames_child.py")
    for shift in (3, 4):   # one after the other; a child that does not end well is the end of the test
        env = dict(os.environ, DGR_SEG_SHIFT=str(shift))
        try:
            r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"DGR_SEG_SHIFT={shift}: the child did not finish in 300 s")
        if r.returncode != 0:
            pytest.fail(f"DGR_SEG_SHIFT={shift}: the child ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert res["tiles_per_segment"] == 1 << shift and set(res["failures"]) == set(B.FRAMES)
        assert {k: v for k, v in res["failures"].items() if v} == {}, shift
