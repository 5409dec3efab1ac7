"""Time per call of slam.pose_graph_optimize from a hipGraph replay, beside the float64 model (tests/pgo_model.py) in torch ops on
the same GPU: python profiles/pgo/timing.py [K:E ...] (default 200:203 1000:1050).  Ring graphs as in tests/test_hip_pgo.py."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "diff-gaussian-rasterization_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pgo_model as M  # noqa: E402
from dgr_amd import slam  # noqa: E402


def one(K, E, replays=20):
    dev = torch.device("cuda:0")
    g = M.ring_graph(K, E - (K - 1))
    vm, Z = M.to_viewmatrices(g["T0"]).to(dev), M.to_viewmatrices(g["Z"]).to(dev)
    edges, info = g["edges"].to(torch.int32).to(dev), g["Omega"].float().to(dev)
    plan = slam.pose_graph_plan(edges, K)
    solve = lambda: slam.pose_graph_optimize(vm, edges, Z, information=info, plan=plan)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solve()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = solve()
    graph.replay()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        graph.replay()
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / replays
    s = res.stats.tolist()
    plan_start, plan_stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plan_start.record()
    for _ in range(replays):
        slam.pose_graph_plan(edges, K)
    plan_stop.record()
    torch.cuda.synchronize()
    T0, Zm = M.from_viewmatrices(vm.cpu()).to(dev), M.from_viewmatrices(Z.cpu()).to(dev)
    args = (T0, g["edges"].to(dev), Zm, g["Omega"].to(dev), g["fixed"].to(dev))
    M.solve(*args, iterations=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = M.solve(*args, iterations=10)
    torch.cuda.synchronize()
    model_ms = (time.perf_counter() - t0) * 1e3
    print(f"K={K} E={E}: solve {ms:.3f} ms per call (hipGraph replay, {replays} replays), {s[3]:.0f} trials ({s[4]:.0f} accepted), "
          f"{s[6]:.0f} CG iterations in total, cost {s[0]:.5g} -> {s[1]:.5g}, converged {s[14]:.0f}; plan {plan_start.elapsed_time(plan_stop) / replays:.3f} ms "
          f"per eager call; float64 model in torch ops on the same GPU: {model_ms:.1f} ms, {len(ref['trials'])} trials, cost -> {ref['costs'][-1]:.5g}")


if __name__ == "__main__":
    for spec in sys.argv[1:] or ["200:203", "1000:1050"]:
        one(*(int(x) for x in spec.split(":")))
