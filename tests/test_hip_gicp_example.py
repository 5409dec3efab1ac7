"""examples/registration.py at its smallest size, through the example's own main(): the run reaches its end, every measured edge is
closer to the truth than the drifted estimate it started from, and the trajectory's error after pose_graph_optimize is below the
one before."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

K = 5
SMALL = ["--keyframes", str(K), "--width", "64", "--height", "48", "--stride", "2", "--iterations", "10"]


def test_measured_edges_beat_the_drift_and_the_pose_graph_takes_them(monkeypatch, capsys):
    import registration
    monkeypatch.setattr(sys, "argv", ["registration.py", *SMALL])
    r = registration.main()
    lines = capsys.readouterr().out.splitlines()
    print("\n".join(lines))
    assert lines[-1].startswith("trajectory error ") and "nan" not in " ".join(lines)
    assert len([ln for ln in lines if ln.startswith("edge ")]) == K == len(r["edges"]) and r["points"] == 32 * 24
    assert r["edges"][-1]["edge"] == (0, K - 1)  # the loop
    for e in r["edges"]:
        assert e["ok"] and e["pairs"] > 0.9 * r["points"], e
        assert e["after"][0] < e["before"][0] and e["after"][1] < e["before"][1], e
    assert r["pgo_ok"] and r["trajectory_after"] < r["trajectory_before"], r


def test_a_loop_needs_three_keyframes(monkeypatch, capsys):
    import registration
    monkeypatch.setattr(sys, "argv", ["registration.py", "--keyframes", "2"])
    with pytest.raises(SystemExit):
        registration.main()
    assert "at least 3" in capsys.readouterr().err
