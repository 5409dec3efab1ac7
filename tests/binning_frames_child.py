"""The child process of tests/test_hip_binning_edges.py: DGR_SEG_SHIFT is read once per process, so the frames of
tests/binning_frames.py meet the 8- and 16-tile segment kernels in a fresh interpreter each.  Prints one JSON line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "diff-gaussian-rasterization_amd", "light"),
          os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import binning_frames  # noqa: E402

if __name__ == "__main__":
    sys.exit(binning_frames.child_main(sys.argv[1:]))
