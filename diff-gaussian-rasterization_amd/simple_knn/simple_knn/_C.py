"""`simple_knn._C`: distCUDA2(points) -> float32 [P], the mean squared distance of every point to its three nearest other
points, from the exact search of dgr_amd.knn.  +inf (simple-knn: a FLT_MAX-derived value) with fewer than four valid points; the
yardstick is the brute-force model of the rule in include/dgr_hip.h, no bit parity with simple-knn is claimed."""
from dgr_amd.knn import dist2 as distCUDA2  # noqa: F401
