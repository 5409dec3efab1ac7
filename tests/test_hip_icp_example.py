"""examples/tracking.py --icp: the pose is aligned by slam.icp_align before the Adam loop and the example prints the pose error at
the start, after ICP and at the end; without the flag it prints what it always did.  Each run is a fresh child process under a
time limit."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--iters", "5", "--width", "96", "--height", "80", "--gaussians", "2000"]
ERRORS = r"rotation error (\S+), translation error ([^\s,]+)"


def run(*more):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tracking.py"), *more, *SMALL], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.strip().splitlines()


def errors_of(line):
    rot, trans = (float(x) for x in re.search(ERRORS, line).groups())
    assert math.isfinite(rot) and math.isfinite(trans) and rot >= 0 and trans >= 0
    return rot, trans


def test_tracking_with_icp_prints_its_three_pose_errors():
    lines = run("--icp", "5")
    assert [ln.split(":")[0].strip() for ln in lines[:3]] == ["start", "icp", "finish"]
    start, icp, finish = (errors_of(ln) for ln in lines[:3])
    assert start[0] > 0 and start[1] > 0
    m = re.search(r"(\d+) of 5 steps accepted, (\d+) pairs, (\S+) us per ICP iteration", lines[1])
    assert m and 0 <= int(m.group(1)) <= 5 and int(m.group(2)) >= 0 and math.isfinite(float(m.group(3))) and float(m.group(3)) > 0
    assert re.match(r"5 iterations in \S+ ms = \S+ ms per tracking iteration \(eager\)$", lines[3]) and len(lines) == 4


def test_tracking_without_icp_prints_what_it_always_did():
    lines = run()
    assert len(lines) == 3
    assert re.match(r"start : " + ERRORS + "$", lines[0])
    assert re.match(r"finish: " + ERRORS + r", loss \S+$", lines[1])
    assert re.match(r"5 iterations in \S+ ms = \S+ ms per tracking iteration \(eager\)$", lines[2])
    errors_of(lines[0]), errors_of(lines[1])
