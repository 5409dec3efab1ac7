"""The kNN entry points (include/dgr_hip.h: dgr_knn_index_bytes, dgr_knn_scratch_bytes, dgr_knn_build, dgr_knn_search) and their
Python surface without a GPU: declared, exported and bound; the params struct against the header text; the size functions; every
argument error refused with its message before any device call (FAKE pointers: nothing is dereferenced); the wrappers' refusals."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest
import torch

from dgr_amd import _capi, knn, slam

from abi_checks import FAKE, ROOT, assert_entry_points, header_text, keyword_only, refused

NAMES = ("dgr_knn_index_bytes", "dgr_knn_scratch_bytes", "dgr_knn_build", "dgr_knn_search")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_declared_exported_and_bound():
    assert_entry_points(NAMES, {"dgr_knn_index_bytes": 1, "dgr_knn_scratch_bytes": 2, "dgr_knn_build": 5, "dgr_knn_search": 12})
    assert _capi._SIGS["dgr_knn_index_bytes"][0] is C.c_size_t and _capi._SIGS["dgr_knn_scratch_bytes"][0] is C.c_size_t


def test_the_params_struct_matches_the_header_text():
    body = header_text().split("} dgr_knn_params;")[0].rsplit("typedef struct dgr_knn_params {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.strip().split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("k", "int"), ("exclude_self", "int"), ("max_dist2", "float")]
    P = _capi.KnnParams
    assert [(n, {C.c_int: "int", C.c_float: "float"}[t]) for n, t in P._fields_] == fields
    assert C.sizeof(P) == 12 and [getattr(P, n).offset for n, _ in fields] == [0, 4, 8]
    assert "#define DGR_KNN_MAX_K 16\n" in header_text() and _capi.KNN_MAX_K == 16


def test_the_header_names_the_rounded_operations_and_the_distcuda2_convention():
    """what the issue wants said in the header, by identifier: the four rounded operations of the rule, distCUDA2 and what it
    returns in place of simple-knn's FLT_MAX-derived value"""
    text = header_text()
    doc = text[text.index("Exact k-nearest-neighbour search"):text.index("typedef struct dgr_knn_params")]
    for word in ("__fsub_rn", "__fmul_rn", "__fadd_rn", "__fdiv_rn", "distCUDA2", "FLT_MAX", "+inf", "DGR_KNN_MAX_K"):
        assert word in doc, word


def test_the_size_functions_refuse_bad_shapes_and_give_16_byte_multiples():
    lib = _capi.load()
    for bad in (0, -1, (1 << 24) + 1, -(1 << 31)):
        assert lib.dgr_knn_index_bytes(bad) == 0
        assert lib.dgr_knn_scratch_bytes(bad, 10) == 0 and lib.dgr_knn_scratch_bytes(10, bad) == 0
    last = 0
    for n in (1, 2, 255, 256, 257, 4096, 4097, 16385, 100000, 1 << 24):
        b = lib.dgr_knn_index_bytes(n)
        assert b % 16 == 0 and b >= 16 * n + 32 * -(-n // 256) and b > last
        last = b
        for q in (1, 63, n, 5000):
            s = lib.dgr_knn_scratch_bytes(n, q)
            assert s % 16 == 0 and s >= 16 * max(n, q)
            # a build's and a self search's need never depends on the queries; more queries never need less
            assert s >= lib.dgr_knn_scratch_bytes(n, 1) and lib.dgr_knn_scratch_bytes(n, max(q - 1, 1)) <= s


def _build(P=100, points=FAKE, index=FAKE, scratch=FAKE):
    return _capi.load().dgr_knn_build(None, P, points, index, scratch)


@pytest.mark.parametrize("case, text", [
    (dict(P=0), "n_points must be 1 .. 2^24"), (dict(P=-5), "n_points must be 1 .. 2^24"), (dict(P=(1 << 24) + 1), "n_points must be 1 .. 2^24"),
    (dict(points=None), "points is NULL"), (dict(points=FAKE + 2), "points is not 4-byte aligned"),
    (dict(index=None), "index is NULL or not 16-byte aligned"), (dict(index=FAKE + 8), "index is NULL or not 16-byte aligned"),
    (dict(scratch=None), "scratch is NULL or not 16-byte aligned"), (dict(scratch=FAKE + 4), "scratch is NULL or not 16-byte aligned"),
])
def test_build_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_build(**case), "dgr_knn_build", text)


def _search(index=FAKE, P=100, points=FAKE, Q=None, queries=None, params=True, k=3, exclude_self=0, max_dist2=INF, scratch=FAKE,
            dist2=FAKE, idx=FAKE, count=FAKE, mean=FAKE):
    p = _capi.KnnParams(k, exclude_self, max_dist2) if params else None
    return _capi.load().dgr_knn_search(None, index, P, points, P if Q is None else Q, queries, p, scratch, dist2, idx, count, mean)


@pytest.mark.parametrize("case, text", [
    (dict(P=0), "n_points must be 1 .. 2^24"), (dict(P=-1), "n_points must be 1 .. 2^24"), (dict(P=(1 << 24) + 1), "n_points must be 1 .. 2^24"),
    (dict(Q=0, queries=FAKE), "n_queries must be 1 .. 2^24"), (dict(Q=-3, queries=FAKE), "n_queries must be 1 .. 2^24"),
    (dict(Q=(1 << 24) + 1, queries=FAKE), "n_queries must be 1 .. 2^24"),
    (dict(Q=99), "n_queries must equal n_points in self mode"),
    (dict(params=False), "params is NULL"),
    (dict(k=0), "k must be 1 .. 16"), (dict(k=17), "k must be 1 .. 16"), (dict(k=-2), "k must be 1 .. 16"),
    (dict(max_dist2=NAN), "max_dist2 is NaN or negative"), (dict(max_dist2=-1.0), "max_dist2 is NaN or negative"),
    (dict(max_dist2=-INF), "max_dist2 is NaN or negative"),
    (dict(queries=FAKE, Q=7, exclude_self=1), "exclude_self with queries given"),
    (dict(index=None), "index is NULL or not 16-byte aligned"), (dict(index=FAKE + 4), "index is NULL or not 16-byte aligned"),
    (dict(points=None), "points is NULL"),
    (dict(scratch=None), "scratch is NULL or not 16-byte aligned"), (dict(scratch=FAKE + 8), "scratch is NULL or not 16-byte aligned"),
    (dict(dist2=None, idx=None, count=None, mean=None), "no output given"),
    (dict(queries=FAKE + 1, Q=7), "not 4-byte aligned"), (dict(idx=FAKE + 2), "not 4-byte aligned"), (dict(mean=FAKE + 3), "not 4-byte aligned"),
])
def test_search_refuses_bad_arguments_before_touching_the_gpu(case, text):
    refused(_search(**case), "dgr_knn_search", text)


def test_python_surface():
    keyword_only(knn.knn_search, ["index", "queries", "k"], dict(exclude_self=None, max_distance=INF, return_count=False, return_mean=False))
    assert knn.KnnResult._fields == ("dist2", "idx", "count", "mean_dist2") and knn.KnnIndex._fields == ("points", "index", "scratch")
    for name in ("knn_build", "knn_search", "dist2", "KnnIndex", "KnnResult"):
        assert getattr(slam, name) is getattr(knn, name), name


def test_the_drop_in_package_exports_distcuda2(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "diff-gaussian-rasterization_amd", "simple_knn"))
    for name in ("simple_knn", "simple_knn._C"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    mod = importlib.import_module("simple_knn._C")
    assert mod.distCUDA2 is knn.dist2


def test_python_surface_refuses_what_it_cannot_read():
    """every check runs on the host, the device check last: CPU tensors reach each of them and never the library"""
    p = torch.rand(10, 3)
    fake = knn.KnnIndex(p, torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8))
    for f in (knn.knn_build, knn.dist2):
        with pytest.raises(ValueError, match="GPU tensors"):
            f(p)
        with pytest.raises(ValueError, match="points must be a tensor"):
            f(p.numpy())
        with pytest.raises(ValueError, match="points must be float32"):
            f(p.double())
        with pytest.raises(ValueError, match="points must be float32"):
            f(p.half())
        with pytest.raises(ValueError, match=r"points is \[N,3\]"):
            f(torch.rand(10, 4))
        with pytest.raises(ValueError, match=r"points is \[N,3\]"):
            f(torch.rand(30))
        with pytest.raises(ValueError, match="1 .. 2\\^24 rows"):
            f(torch.rand(0, 3))
    s = knn.knn_search
    with pytest.raises(ValueError, match="GPU tensors"):
        s(fake)
    with pytest.raises(ValueError, match="GPU tensors"):
        s(fake, torch.rand(4, 3), k=2, return_count=True, return_mean=True, max_distance=0.5)
    with pytest.raises(ValueError, match="index must be what knn_build returned"):
        s(p)
    with pytest.raises(ValueError, match="queries must be float32"):
        s(fake, torch.rand(4, 3).double())
    with pytest.raises(ValueError, match="queries must be a tensor"):
        s(fake, [[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"queries is \[N,3\]"):
        s(fake, torch.rand(4, 2))
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="k must be 1 .. 16"):
            s(fake, k=bad)
    with pytest.raises(ValueError, match="exclude_self is defined in self mode only"):
        s(fake, torch.rand(4, 3), exclude_self=True)
    for bad in (NAN, -0.5, -INF):
        with pytest.raises(ValueError, match="max_distance must not be NaN or negative"):
            s(fake, max_distance=bad)


def test_max_distance_is_squared_in_float64_and_rounded_once():
    import numpy as np
    for d in (0.0, 1.0, 0.1, 2.0 ** 0.5, 3.3333333, 1e-30, 1e19, 1e20, INF):
        with np.errstate(over="ignore"):
            want = np.float32(np.float64(d) * np.float64(d))
        assert knn._square(d) == float(want), d
