#!/usr/bin/env python3
"""Writes sh_rotation_table.h: the constants csrc/transform.hip needs to turn a rotation R into the matrices M_l (l = 1, 2, 3) with
B_l(R d) = M_l B_l(d), B_l being gaussian_math.h's band-l basis (SH_C1, SH_C2[], SH_C3[], its signs and its order).

Band l has n = 2 l + 1 functions.  With n fixed unit directions d_k, Y_l = [B_l(d_0) .. B_l(d_{n-1})] (one column per direction) and
Y'_l the same at R d_k, M_l = Y'_l Y_l^-1.  The table holds seven directions (band l uses the first 2 l + 1) and the three inverses.
The directions are the best of a seeded random search for the smallest condition number of the worst Y_l; the numbers are printed
with 17 significant digits, so the header is reproduced bit for bit:

    python3 gen_sh_rotation_table.py > sh_rotation_table.h
"""
import numpy as np

SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)
# the basis is the one the kernels evaluate: their constants are these literals rounded to fp32
SH_C1 = float(np.float32(SH_C1))
SH_C2 = tuple(float(np.float32(c)) for c in SH_C2)
SH_C3 = tuple(float(np.float32(c)) for c in SH_C3)
TRIALS, SEED = 4000, 20240607


def band(l, d):
    """B_l at the unit direction d = (x, y, z), as computeColorFromSH / gaussian_math.h evaluate it"""
    x, y, z = d
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if l == 1:
        return np.array([-SH_C1 * y, SH_C1 * z, -SH_C1 * x])
    if l == 2:
        return np.array([SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)])
    return np.array([SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
                     SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy),
                     SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3.0 * yy)])


def sample_matrix(l, dirs):
    return np.stack([band(l, d) for d in dirs[:2 * l + 1]], axis=1)


def search():
    rng = np.random.RandomState(SEED)
    best, best_cond = None, np.inf
    for _ in range(TRIALS):
        dirs = rng.standard_normal((7, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        cond = max(np.linalg.cond(sample_matrix(l, dirs)) for l in (1, 2, 3))
        if cond < best_cond:
            best, best_cond = dirs, cond
    return best


def rows(a):
    return ",\n".join("    " + ", ".join("%.17g" % v for v in r) for r in np.atleast_2d(a))


def main():
    dirs = search()
    print("// sh_rotation_table.h -- written by gen_sh_rotation_table.py; do not edit.  Seven unit directions and, per band l = 1, 2, 3,")
    print("// the inverse of Y_l = [B_l(d_0) .. B_l(d_2l)] (row-major): M_l = Y_l(R d) Y_l^-1 is the band's rotation matrix.")
    conds = ", ".join("%.2f" % np.linalg.cond(sample_matrix(l, dirs)) for l in (1, 2, 3))
    print("// condition numbers of Y_1, Y_2, Y_3: " + conds)
    print("#pragma once")
    print("namespace dgr {")
    print("__device__ const double SH_ROT_DIRS[7][3] = {\n" + rows(dirs).replace("    ", "    {").replace(",\n", "},\n") + "}};")
    for l in (1, 2, 3):
        n = 2 * l + 1
        inv = np.linalg.inv(sample_matrix(l, dirs))
        print("__device__ const double SH_ROT_YINV%d[%d] = {\n%s};" % (l, n * n, rows(inv)))
    print("}  // namespace dgr")


if __name__ == "__main__":
    main()
