"""The SH degree at the C ABI, without a GPU: every entry point that takes `D` refuses a value outside 0 .. 3 with
DGR_ERR_BAD_ARGUMENT and a message, before it touches a pointer or the device (include/dgr_hip.h: the SH layout).  The SH basis is
written out for degrees 0 .. 3; the reference's kernels have no other degree either.  The calls carry NULL for every device
pointer: a refusal that came after the first launch would not return here."""
import ctypes as C

import pytest

from dgr_amd import _capi

from abi_checks import neutral_args, refused

# entry point -> the positions of (P, D, M, W, H) in its argument list, n_views' position (batches) and the value of P
ONE_VIEW_FORWARD = dict(P=5, D=6, M=7, W=9, H=10)            # (stream, three callbacks, user, P, D, M, background, W, H, ...)
PRESIZED_FORWARD = dict(P=6, D=7, M=8, W=10, H=11)           # (stream, three buffers + capacity, status, P, D, M, background, W, H, ...)
ONE_VIEW_BACKWARD = dict(P=1, D=2, M=3, W=6, H=7)            # (stream, P, D, M, R, background, W, H, ...)
BATCH = dict(P=3, D=4, M=5, W=7, H=8, n_views=1)             # (stream, n_views, views, P, D, M, background, W, H, ...)
ENTRIES = {name: where for names, where in (
    (("dgr_light_forward", "dgr_full_forward"), ONE_VIEW_FORWARD),
    (("dgr_light_forward_presized", "dgr_full_forward_presized"), PRESIZED_FORWARD),
    (("dgr_light_backward", "dgr_light_backward_absgrad", "dgr_light_backward_silhouette", "dgr_full_backward",
      "dgr_full_backward_absgrad", "dgr_full_backward_silhouette"), ONE_VIEW_BACKWARD),
    (("dgr_light_forward_batch", "dgr_full_forward_batch", "dgr_light_backward_batch", "dgr_light_backward_batch_absgrad",
      "dgr_light_backward_batch_silhouette", "dgr_full_backward_batch", "dgr_full_backward_batch_absgrad",
      "dgr_full_backward_batch_silhouette"), BATCH)) for name in names}

_HOST = (C.c_float * 64)()  # stands for a view's camera and output pointers (a batch forward looks at them being there first)


def _arguments(name, fn, where, D, P):
    """neutral arguments (NULL for every pointer: num_related and a batch's array of images as well) with the sizes at `where`"""
    at = {f"i{where[key]}": value for key, value in dict(P=P, D=D, M=16, W=64, H=48, n_views=1).items() if key in where}
    if "n_views" in where:  # a batch's views: one view, every pointer "there", every number 0
        struct = fn.argtypes[where["n_views"] + 1]._type_
        assert issubclass(struct, C.Structure)
        view = struct()
        for field, ft in view._fields_:
            if ft is C.c_void_p:
                setattr(view, field, C.addressof(_HOST))
        at[f"i{where['n_views'] + 1}"] = (struct * 1)(view)
    return neutral_args(name, **at)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_entry_point_refuses_a_degree_outside_0_to_3(name):
    lib = _capi.load()
    fn = getattr(lib, name)
    where = ENTRIES[name]
    assert len(fn.argtypes) > max(v for k, v in where.items() if k != "n_views")
    # (a batch forward asks for every view's state buffers first when P > 0; the degree is judged the same for an empty scene)
    P = 0 if name.endswith("forward_batch") else 10
    for D in (-1, 4, 16, -2 ** 31):
        lib.dgr_set_option(b"no_such_option", 0)  # (leaves another message behind)
        assert b"SH degree" not in lib.dgr_last_error()
        refused(fn(*_arguments(name, fn, where, D, P)), None, "SH degree must be 0 .. 3")  # (csrc/api.hip: a message without a prefix)
