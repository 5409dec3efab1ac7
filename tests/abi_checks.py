"""What the C-ABI tests that need no GPU (tests/test_*_abi.py, tests/test_capi_symbols.py) share: the header's text and the
symbols it declares, the stand-in pointers, and the checks every family of entry points gets -- declared, exported and bound; a
descriptor's layout and constants; a refusal and its message; a neutral argument list; a Python surface's keyword-only arguments."""
import ctypes as C
import functools
import inspect
import os
import re

from dgr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dgr_hip.h")
FAKE = 1 << 20   # a non-NULL, 16-byte aligned "device" pointer: every call made with it is refused before anything dereferences it
OTHER = 1 << 21  # a second one, where two arguments must (or must not) be the same tensor


@functools.lru_cache(maxsize=None)
def header_text():
    with open(HEADER) as f:
        return f.read()


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(dgr_[a-z0-9_]+)\s*\(", text)))


def assert_entry_points(names, n_args=None):
    """every name is declared in the header, bound by _capi and exported by the library itself (a fresh CDLL, not the binding's);
    `n_args` = {name: the argument count _capi._SIGS gives it}"""
    lib = C.CDLL(_capi.LIB_PATH)
    declared, bound = declared_symbols(), _capi.exported_symbols()
    for name in names:
        assert name in declared, name
        assert name in bound, name
        assert hasattr(lib, name), name
    for name, n in (n_args or {}).items():
        assert name in names and len(_capi._SIGS[name][1]) == n, name


def assert_descriptor(cls, size, offsets, prefix, defines):
    """the ctypes struct `cls` has `size` bytes and exactly the fields of `offsets` = {field: byte offset}; every NAME of `defines`
    = {NAME: value} is `_capi.<prefix>_<NAME>` and `#define DGR_<prefix>_<NAME> <value>` in the header"""
    assert C.sizeof(cls) == size
    assert {name: getattr(cls, name).offset for name, _ in cls._fields_} == offsets
    for name, value in defines.items():
        assert getattr(_capi, f"{prefix}_{name}") == value, name
        assert f"#define DGR_{prefix}_{name} {value}\n" in header_text(), name


def refused(rc, who, text):
    """the call was refused as a bad argument, with `text` in a message that starts "<who>: " (the entry point's name).  who=None
    only for the messages the library leaves without such a prefix."""
    err = _capi.last_error()
    assert rc == _capi.DGR_ERR_BAD_ARGUMENT and text in err, (rc, err)
    assert who is None or err.startswith(who + ": "), (who, err)


def neutral_args(entry, pointer=None, **at):
    """one argument per parameter of `entry` (_capi._SIGS): `pointer` (NULL) for a void pointer, NULL for every typed pointer, an
    empty callback, 0 for an integer, 1.0 for a float; then `at` = {"i<index>": value} on top"""
    out = []
    for t in _capi._SIGS[entry][1]:
        if t is _capi.ALLOC_FN:
            out.append(t())
        elif t is C.c_void_p:
            out.append(pointer)
        elif t in (C.c_float, C.c_double):
            out.append(1.0)
        elif t in (C.c_int, C.c_long, C.c_size_t, C.c_ulonglong):
            out.append(0)
        else:
            assert t is C.c_char_p or hasattr(t, "contents"), (entry, t)
            out.append(None)
    for i, v in at.items():
        out[int(i[1:])] = v
    return out


def keyword_only(fn, leading, defaults, required=()):
    """`fn` starts with the positional parameters `leading`; every name of `defaults` = {name: default} is keyword-only with that
    default, every name of `required` keyword-only without one"""
    p = inspect.signature(fn).parameters
    assert list(p)[:len(leading)] == list(leading)
    for name, default in defaults.items():
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert p[name].default is None if default is None else p[name].default == default, name
    for name in required:
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is inspect.Parameter.empty, name
