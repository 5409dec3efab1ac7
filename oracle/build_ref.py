"""Builds the reference rasterizer's own source for gfx950 into oracle/_ref/ (test infrastructure; nothing under _ref/ is committed).

    python oracle/build_ref.py            # or __graft_entry__.build(), which calls build_reference()

Reads the reference checkout at $DGR_REFERENCE_DIR (default: a directory `reference` next to this repository, or further up, or
in the home directory: see reference_dir).  For each variant
(light, full) it
  1. copies cuda_rasterizer/*.{cu,h} to oracle/_ref/src_<variant>/;
  2. rewrites nvcc's spaced launch brackets (`<< <`, `>> >`), which clang rejects, in the copies;
  3. full only: deletes the dead older `int Rasterizer::forward` of rasterizer_impl.cu -- from its leading
     `// Forward rendering procedure` comment through the line `comment end*/` (its opening comment mark is missing, so the file
     compiles under no compiler as shipped); the live std::tuple<int,int> forward below it is untouched;
  4. compiles forward.cu, backward.cu, rasterizer_impl.cu and oracle/ref_capi.hip with FLAGS below -- the forwarding headers of
     oracle/ref_shim/, the reference's third_party/glm and the copies on the include path, FP contraction at the compiler's
     default (nvcc fuses by default too) -- and links oracle/_ref/libdgr_ref_<variant>.so.
Without a checkout it prints one line and leaves oracle/_ref/ as it is.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
SHIM = os.path.join(HERE, "ref_shim")
CAPI = os.path.join(HERE, "ref_capi.hip")
VARIANTS = {"light": "diff-gaussian-rasterization-light", "full": "diff-gaussian-rasterization-full"}
FLAGS = ["--offload-arch=gfx950", "-O2", "-fPIC", "-std=c++17"]
UNITS = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
MAX_JOBS = 8  # two variants x four translation units; never more than 16


def _is_checkout(path):
    return all(os.path.isdir(os.path.join(path, d, "cuda_rasterizer")) for d in VARIANTS.values())


def reference_dir():
    """$DGR_REFERENCE_DIR; else a directory `reference` next to this repository, next to one of its parent directories, or in
    the home directory -- the first that holds both variants; else the sibling, for the message."""
    if os.environ.get("DGR_REFERENCE_DIR"):
        return os.environ["DGR_REFERENCE_DIR"]
    repo = os.path.dirname(HERE)
    candidates, d = [], os.path.dirname(repo)
    while True:
        candidates.append(os.path.join(d, "reference"))
        if os.path.dirname(d) == d:
            break
        d = os.path.dirname(d)
    candidates.append(os.path.join(os.path.expanduser("~"), "reference"))
    for c in candidates:
        if _is_checkout(c):
            return c
    return candidates[0]


def have_reference():
    return _is_checkout(reference_dir())


def library(variant):
    return os.path.join(OUT, f"libdgr_ref_{variant}.so")


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def _shim_files():
    return [os.path.join(d, f) for d, _, fs in os.walk(SHIM) for f in fs]


def _prepare_sources(variant, ref_src):
    """steps 1-3; returns the directory of the copies"""
    dst = os.path.join(OUT, f"src_{variant}")
    os.makedirs(dst, exist_ok=True)
    for name in sorted(os.listdir(ref_src)):
        if not name.endswith((".cu", ".h")):
            continue
        with open(os.path.join(ref_src, name), encoding="utf-8", errors="surrogateescape") as f:
            lines = f.read().replace("<< <", "<<<").replace(">> >", ">>>").split("\n")
        if variant == "full" and name == "rasterizer_impl.cu":
            ends = [i for i, l in enumerate(lines) if l.strip() == "comment end*/"]
            if ends:
                start = next(i for i, l in enumerate(lines) if "// Forward rendering procedure" in l)
                assert start < ends[0], "rasterizer_impl.cu: the dead span is not where it is expected"
                del lines[start:ends[0] + 1]
        text = "\n".join(lines)
        path = os.path.join(dst, name)
        old = None
        if os.path.exists(path):
            with open(path, encoding="utf-8", errors="surrogateescape") as f:
                old = f.read()
        if old != text:  # (an unchanged copy keeps its time stamp)
            with open(path, "w", encoding="utf-8", errors="surrogateescape") as f:
                f.write(text)
    return dst


def _compile(job):
    src, obj, cmd = job
    subprocess.check_call(cmd)
    return obj


def build_reference(force=False, verbose=True):
    """Returns the libraries built or found up to date ({} without a reference checkout)."""
    ref = reference_dir()
    if not have_reference():
        print(f"oracle/build_ref.py: no reference checkout at {ref} (set DGR_REFERENCE_DIR): oracle/_ref/ left as it is")
        return {}
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    jobs, links = [], []
    for variant, d in VARIANTS.items():
        src = _prepare_sources(variant, os.path.join(ref, d, "cuda_rasterizer"))
        inputs = [os.path.join(src, n) for n in os.listdir(src)] + _shim_files() + [CAPI, os.path.abspath(__file__)]
        lib = library(variant)
        if not force and os.path.exists(lib) and os.path.getmtime(lib) >= _newest(inputs):
            continue
        objdir = os.path.join(OUT, f"obj_{variant}")
        os.makedirs(objdir, exist_ok=True)
        inc = ["-I", SHIM, "-I", os.path.join(ref, d, "third_party", "glm"), "-I", src]
        defs = ["-DDGR_REF_FULL=1"] if variant == "full" else []
        objs = []
        for unit in [os.path.join(src, u) for u in UNITS] + [CAPI]:
            obj = os.path.join(objdir, os.path.splitext(os.path.basename(unit))[0] + ".o")
            objs.append(obj)
            jobs.append((unit, obj, [hipcc, *FLAGS, "-x", "hip", *defs, *inc, "-c", unit, "-o", obj]))
        links.append((lib, [hipcc, *FLAGS, "-shared", "-o", lib + ".tmp", *objs]))
    if jobs and verbose:
        print(f"oracle/build_ref.py: compiling {len(jobs)} translation units of the reference for gfx950 ({' '.join(FLAGS)})")
    with ThreadPoolExecutor(max_workers=MAX_JOBS) as pool:
        list(pool.map(_compile, jobs))
    for lib, cmd in links:
        subprocess.check_call(cmd)
        os.replace(lib + ".tmp", lib)
    return {v: library(v) for v in VARIANTS}


if __name__ == "__main__":
    build_reference(force="--force" in sys.argv[1:])
