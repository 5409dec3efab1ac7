#!/usr/bin/env python3
"""Writes profiles/ref_parity/measured.txt from the lines that tests/test_hip_reference_light.py and test_hip_reference_full.py
append to $DGR_REF_PARITY_LOG (tests/ref_parity.judge / log_flips):

    DGR_REF_PARITY_LOG=raw.txt python -m pytest tests/test_hip_reference_light.py tests/test_hip_reference_full.py -m gpu
    python profiles/ref_parity/summarize.py raw.txt > profiles/ref_parity/measured.txt

The raw lines are kept as they are; a summary follows: per variant and tensor the worst distance of each side from float64 over
the cases and modes, and the worst ratio e_x / max(2 e_ref, bar) (a side passes at <= 1)."""
import collections
import re
import sys

HEAD = """The reference rasterizer's own source compiled for gfx950 (oracle/build_ref.py), the HIP kernels and both oracle builds on an MI355X;
arbiter: the float64 formulation of tests/fp64_model.py on the reference's decisions (tests/ref_parity.py).
e_x = distance of side x from float64 at pixels / Gaussians no counted flip touches: images and per-Gaussian forward values
max |d| / max(1, |f64|) (gau_uncertainty: / (1 + |f64|)), gradients max |d| / max |f64|.  Rule: e_x <= max(2 e_ref, bar), bar 1e-6
(images, preprocess), 1e-5 (gradients, gau_uncertainty).  Modes: 'mapping' = track_off, 'tracking' = map_off (switched-off tensors
are exactly zero on every side), 'end-to-end' = mapping+pose with every side on its own forward's alpha image.
"""


def main(path):
    lines = [l.rstrip("\n") for l in open(path)]
    print(HEAD)
    print("== counted flips and masks")
    for l in lines:
        if " e_ref " not in l:
            print(l)
    print("\n== distances from float64")
    summ = collections.OrderedDict()
    for l in lines:
        if " e_ref " not in l:
            continue
        print(l)
        case, tensor, eref, rest = re.match(r"(.*?)\s+(\S+)\s+e_ref\s+(\S+)\s+(.*)", l).groups()
        eref = float(eref)
        bar = 1e-5 if ("dL_" in tensor or "uncert" in tensor) else 1e-6
        s = summ.setdefault((case.split()[0], tensor), collections.defaultdict(float))
        s["ref"] = max(s["ref"], eref)
        for n, v in re.findall(r"e_(\w+)\s+(\S+)", rest):
            s[n] = max(s[n], float(v))
            s["ratio"] = max(s["ratio"], float(v) / max(2 * eref, bar))
    print("\n== summary: worst over the cases and modes: e_ref  e_hip  e_oracle  e_oracle_cmath   worst e_x / max(2 e_ref, bar)")
    for (v, t), s in summ.items():
        print(f"{v:<6}{t:<18} {s['ref']:9.2e} {s['hip']:9.2e} {s['oracle']:9.2e} {s['oracle_cmath']:9.2e}   {s['ratio']:.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
