"""The densify apply kernel by tensor group at measure.py's size: all 18 tensors, then each leaf with its two moments alone.
  python profiles/densify/apply_breakdown.py"""
import importlib.util, os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "diff-gaussian-rasterization_amd")]
spec = importlib.util.spec_from_file_location("measure", os.path.join(ROOT, "profiles", "densify", "measure.py"))
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
import torch
from dgr_amd import _capi
dev = torch.device("cuda:0")
P = 500000
L, M, accum, denom, maxr = m.make(P, dev)
noise = torch.randn((P, 2, 3), device=dev)
thr = m.densify_thresholds(grad_threshold=2e-4, extent=10.0, percent_dense=0.01, min_opacity=0.005, max_screen_size=20.0)
lib, st = _capi.load(), _capi.stream_handle()
plan = torch.empty(lib.dgr_densify_plan_bytes(P), dtype=torch.uint8, device=dev)
cdev = torch.empty(8, dtype=torch.int32, device=dev)
assert lib.dgr_densify_plan(st, P, accum.data_ptr(), denom.data_ptr(), maxr.data_ptr(), L["opacity"].data_ptr(), L["scaling"].data_ptr(), *thr, plan.data_ptr(), cdev.data_ptr()) == 0
c = cdev.tolist(); P_new = c[0]
mode_of = {"xyz": 3, "scaling": 4}
def table_for(names, with_acc):
    t, keep = [], []
    for n in names:
        k = L[n].numel() // P
        for src, mode in ((L[n], mode_of.get(n, 0)), (M[n][0], 1), (M[n][1], 1)):
            d = torch.empty((P_new, k), device=dev); keep.append(d); t.append((src.data_ptr(), d.data_ptr(), k, mode))
    for _ in range(3 if with_acc else 0):
        d = torch.empty((P_new, 1), device=dev); keep.append(d); t.append((None, d.data_ptr(), 1, 2))
    descs = (_capi.DensifyTensor * len(t))()
    for d, (s, dd, k, mode) in zip(descs, t):
        d.src, d.dst, d.k, d.mode = s, dd, k, mode
    return descs, len(t), keep
for label, names, acc in (("all", m.NAMES, True), ("features", ("features",), False), ("rotation", ("rotation",), False), ("xyz", ("xyz",), False),
                          ("scaling", ("scaling",), False), ("opacity+acc", ("opacity",), True)):
    descs, n, keep = table_for(names, acc)
    def f():
        assert lib.dgr_densify_apply(st, P, P_new, plan.data_ptr(), n, descs, L["scaling"].data_ptr(), L["rotation"].data_ptr(), noise.data_ptr(), 0) == 0
    r = m.timed(f, 20)
    floats = sum(d.k for d in descs)
    print(label, n, "tensors", floats, "floats/row", json.dumps(r), "us per float/row: %.2f" % (r["median_ms"] * 1e3 / floats))
