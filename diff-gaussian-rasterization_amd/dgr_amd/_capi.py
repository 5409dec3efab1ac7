"""ctypes binding of lib/libdgr_hip.so (C ABI declared in include/dgr_hip.h).

torch is used for device memory and the current HIP stream only; every compute call goes through
the C ABI.  `import torch` must precede loading the library so that it binds to the HIP runtime
torch already mapped (same SONAME, libamdhip64.so.7).
"""
import ctypes as C
import os

import torch  # noqa: F401  (must be imported before the HIP library is mapped)

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# DGR_HIP_LIB points at another build of the same ABI (kernel experiments); the default is the in-tree library
LIB_PATH = os.environ.get("DGR_HIP_LIB") or os.path.join(_PKG, "lib", "libdgr_hip.so")

DGR_OK = 0
DGR_ERR_BAD_ARGUMENT = -1
DGR_ERR_PREFILTERED = -2
DGR_ERR_BINNING_OVERFLOW = -3
DGR_ERR_HIP = -4
DGR_ERR_ALLOC = -5

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t



class LightView(C.Structure):  # dgr_light_view (include/dgr_hip.h): the per-camera arguments of a batched forward
    _fields_ = [("geometry_buffer", _vp), ("binning_buffer", _vp), ("binning_capacity", _i), ("image_buffer", _vp),
                ("status", _vp), ("viewmatrix", _vp), ("projmatrix", _vp), ("cam_pos", _vp), ("out_color", _vp),
                ("out_depth", _vp), ("out_median_depth", _vp), ("out_alpha", _vp), ("gt_depth", _vp),
                ("out_depth_var", _vp), ("gau_uncertainty", _vp), ("gau_related_pixels", _vp), ("radii", _vp)]


class LightViewGrad(C.Structure):  # dgr_light_view_grad: the per-camera arguments of a batched backward
    _fields_ = [("geometry_buffer", _vp), ("binning_buffer", _vp), ("image_buffer", _vp), ("viewmatrix", _vp),
                ("projmatrix", _vp), ("cam_pos", _vp), ("perspec_matrix", _vp), ("alphas", _vp), ("gt_depth", _vp),
                ("radii", _vp), ("dL_dpix", _vp), ("dL_dpix_depth", _vp), ("dL_dpix_median_depth", _vp),
                ("dL_dpix_depth_var", _vp), ("dL_dmean2D", _vp), ("dL_dview", _vp), ("scratch", _vp),
                ("scratch_bytes", _sz), ("num_rendered", _i)]


class FullView(C.Structure):  # dgr_full_view: the per-camera arguments of a batched forward of the full variant
    _fields_ = [("geometry_buffer", _vp), ("binning_buffer", _vp), ("binning_capacity", _i), ("image_buffer", _vp),
                ("status", _vp), ("viewmatrix", _vp), ("projmatrix", _vp), ("cam_pos", _vp), ("out_color", _vp),
                ("out_depth", _vp), ("gt_depth", _vp), ("out_uncertainty", _vp), ("radii", _vp)]


class FullViewGrad(C.Structure):  # dgr_full_view_grad: the per-camera arguments of a batched backward of the full variant
    _fields_ = [("geometry_buffer", _vp), ("binning_buffer", _vp), ("image_buffer", _vp), ("viewmatrix", _vp),
                ("projmatrix", _vp), ("cam_pos", _vp), ("perspec_matrix", _vp), ("gt_depth", _vp), ("radii", _vp),
                ("dL_dpix", _vp), ("dL_depths", _vp), ("dL_duncertainties", _vp), ("dL_dmean2D", _vp), ("dL_dview", _vp),
                ("scratch", _vp), ("scratch_bytes", _sz), ("num_rendered", _i)]


class DensifyTensor(C.Structure):  # dgr_densify_tensor: one per-Gaussian tensor of a dgr_densify_apply call
    _fields_ = [("src", _vp), ("dst", _vp), ("k", _i), ("mode", _i)]


assert C.sizeof(DensifyTensor) == 24  # two pointers, two ints: the C layout


class SeedTensor(C.Structure):  # dgr_seed_tensor: one per-Gaussian tensor of a dgr_seed_apply call
    _fields_ = [("src", _vp), ("dst", _vp), ("k", _i), ("mode", _i), ("value", _f)]


assert C.sizeof(SeedTensor) == 32  # two pointers, two ints, a float, padded to the pointers' alignment


class RelocateTensor(C.Structure):  # dgr_relocate_tensor: one per-Gaussian tensor of a dgr_relocate_apply call (rewritten in place)
    _fields_ = [("data", _vp), ("k", _i), ("mode", _i)]


assert C.sizeof(RelocateTensor) == 16  # a pointer, two ints: the C layout


class TransformTensor(C.Structure):  # dgr_transform_tensor: one per-Gaussian tensor of a dgr_transform_apply call (rewritten in place)
    _fields_ = [("data", _vp), ("k", _i), ("mode", _i), ("skip", _i)]


assert C.sizeof(TransformTensor) == 24  # a pointer, three ints, padded to the pointer's alignment


class MaskedLossParams(C.Structure):  # dgr_masked_loss_params
    _fields_ = [("depth_lo", _f), ("depth_hi", _f), ("silhouette_threshold", _f), ("outlier_factor", _f),
                ("reject_outliers", _i), ("mask_color", _i), ("reduction", _i), ("w_color", _f), ("w_depth", _f)]


assert C.sizeof(MaskedLossParams) == 36  # nine four-byte fields: the C layout


class KeyframeOverlapParams(C.Structure):  # dgr_keyframe_overlap_params
    _fields_ = [("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f), ("depth_min", _f), ("depth_max", _f), ("edge", _f), ("near_z", _f),
                ("depth_tolerance", _f), ("stride", _i)]


assert C.sizeof(KeyframeOverlapParams) == 40  # ten four-byte fields: the C layout


class IcpParams(C.Structure):  # dgr_icp_params
    _fields_ = [("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f), ("depth_min", _f), ("depth_max", _f), ("dist_max", _f),
                ("normal_cos_min", _f), ("huber_delta", _f), ("damping", _f), ("rcond", _f), ("min_points", _i), ("stride", _i)]


assert C.sizeof(IcpParams) == 52  # thirteen four-byte fields: the C layout


class RgbdParams(C.Structure):  # dgr_rgbd_params: dgr_icp_params' fields, then the two class weights and the photometric bounds
    _fields_ = IcpParams._fields_ + [("geo_weight", _f), ("photo_weight", _f), ("photo_max", _f), ("photo_huber", _f)]


assert C.sizeof(RgbdParams) == 68  # seventeen four-byte fields: the C layout


class PgoParams(C.Structure):  # dgr_pgo_params
    _fields_ = [("iterations", _i), ("cg_iterations", _i), ("cg_tolerance", _f), ("huber_delta", _f), ("damping", _f),
                ("rcond", _f), ("step_tolerance", _f), ("cost_tolerance", _f)]


assert C.sizeof(PgoParams) == 32  # eight four-byte fields: the C layout


class ContributionParams(C.Structure):  # dgr_contribution_params
    _fields_ = [("min_pixels", _i), ("weight_min", _f), ("frame_id", _i)]


assert C.sizeof(ContributionParams) == 12  # three four-byte fields: the C layout


class TsdfGrid(C.Structure):  # dgr_tsdf_grid
    _fields_ = [("nx", _i), ("ny", _i), ("nz", _i), ("origin", _f * 3), ("voxel_size", _f)]


assert C.sizeof(TsdfGrid) == 28  # seven four-byte fields: the C layout


class TsdfParams(C.Structure):  # dgr_tsdf_params
    _fields_ = [("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f), ("truncation", _f), ("weight", _f), ("max_weight", _f),
                ("depth_min", _f), ("depth_max", _f), ("near_z", _f), ("mask_threshold", _f)]


assert C.sizeof(TsdfParams) == 44  # eleven four-byte fields: the C layout


class RaycastParams(C.Structure):  # dgr_raycast_params
    _fields_ = [("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f), ("depth_min", _f), ("depth_max", _f), ("step", _f), ("min_weight", _f)]


assert C.sizeof(RaycastParams) == 32  # eight four-byte fields: the C layout


class KnnParams(C.Structure):  # dgr_knn_params
    _fields_ = [("k", _i), ("exclude_self", _i), ("max_dist2", _f)]


assert C.sizeof(KnnParams) == 12  # three four-byte fields: the C layout
KNN_MAX_K = 16  # DGR_KNN_MAX_K


class CovarianceParams(C.Structure):  # dgr_covariance_params
    _fields_ = [("mode", _i), ("epsilon", _f), ("min_neighbours", _i), ("scale_floor", _f), ("viewpoint", _f * 3), ("has_viewpoint", _i)]


assert C.sizeof(CovarianceParams) == 32  # eight four-byte fields: the C layout
COV_RAW, COV_PLANE = 0, 1  # DGR_COV_*


class GicpParams(C.Structure):  # dgr_gicp_params
    _fields_ = [("dist_max", _f), ("huber_delta", _f), ("damping", _f), ("rcond", _f), ("min_points", _i)]


assert C.sizeof(GicpParams) == 20  # five four-byte fields: the C layout

RELOCATE_MAX_TENSORS = 24  # DGR_RELOCATE_MAX_TENSORS
RELOCATE_COPY, RELOCATE_OPACITY, RELOCATE_LOG_SCALE, RELOCATE_ZERO_TOUCHED, RELOCATE_ZERO_RELOCATED = range(5)  # DGR_RELOCATE_*
TRANSFORM_MAX_TENSORS = 24  # DGR_TRANSFORM_MAX_TENSORS
TRANSFORM_VALUE, TRANSFORM_MOMENT1, TRANSFORM_MOMENT2 = range(3)  # DGR_TRANSFORM_<order>; a mode is kind + order
TRANSFORM_XYZ, TRANSFORM_QUAT, TRANSFORM_LOG_SCALE, TRANSFORM_SH = 0, 4, 8, 12  # DGR_TRANSFORM_<kind>
MASKED_LOSS_SUM, MASKED_LOSS_MEAN = 0, 1  # DGR_MASKED_LOSS_*
MAX_BATCH_VIEWS = 8  # DGR_MAX_BATCH_VIEWS
DENSIFY_MAX_TENSORS = 24  # DGR_DENSIFY_MAX_TENSORS
DENSIFY_COPY, DENSIFY_ZERO_NEW, DENSIFY_ZERO, DENSIFY_XYZ, DENSIFY_LOG_SCALE = range(5)  # DGR_DENSIFY_*
SEED_MAX_TENSORS = 24  # DGR_SEED_MAX_TENSORS
SEED_XYZ, SEED_LOG_SCALE, SEED_RGB_DC, SEED_QUAT_IDENTITY, SEED_CONST = range(5)  # DGR_SEED_*

# argument lists follow include/dgr_hip.h one to one
_SIGS = {
    "dgr_light_forward_batch": (_i, [_vp, _i, C.POINTER(LightView), _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp,
                                     _vp, _f, _f, _i]),
    "dgr_light_backward_batch": (_i, [_vp, _i, C.POINTER(LightViewGrad), _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp,
                                      _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i]),
    "dgr_full_forward_batch": (_i, [_vp, _i, C.POINTER(FullView), _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp,
                                    _vp, _f, _f, _i]),
    "dgr_full_backward_batch": (_i, [_vp, _i, C.POINTER(FullViewGrad), _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp,
                                     _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_last_error": (C.c_char_p, []),
    "dgr_status_post": (C.c_long, [_vp, _vp]),
    "dgr_status_poll": (_i, [C.c_long, _i, _vp]),
    "dgr_status_arm": (C.c_long, []),
    "dgr_stream_is_capturing": (_i, [_vp]),
    "dgr_early_status_arm": (_i, []),
    "dgr_backward_scratch_clean_arm": (_i, []),
    "dgr_early_status_wait": (_i, [_vp]),
    "dgr_pose_forward": (_i, [_vp] * 7),
    "dgr_pose_backward": (_i, [_vp] * 5),
    "dgr_l1_loss_scratch_floats": (_i, []),
    "dgr_l1_loss_forward": (_i, [_vp, C.c_long, _vp, _vp, C.c_long, _vp, _vp, _f, _f, _vp, _vp]),
    "dgr_l1_loss_backward": (_i, [_vp, C.c_long, _vp, _vp, C.c_long, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "dgr_ssim_scratch_floats": (C.c_long, [_i, _i, _i, _i]),
    "dgr_ssim_loss_forward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, C.c_long, _vp, _vp, _f, _f, _f, _vp, _i, _vp]),
    "dgr_ssim_loss_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, C.c_long, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "dgr_masked_loss_scratch_bytes": (_sz, [_i, _i, _i]),
    "dgr_masked_loss_forward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(MaskedLossParams), _vp, _vp]),
    "dgr_masked_loss_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(MaskedLossParams), _vp, _vp,
                                      _vp, _vp]),
    "dgr_keyframe_overlap_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "dgr_keyframe_overlap": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, C.POINTER(KeyframeOverlapParams), _vp, _vp, _vp, _vp, _vp,
                                  _vp]),
    "dgr_depth_normals": (_i, [_vp, _i, _i, _vp, _vp, _f, _f, _f, _f, _f, _f, _f, _f, _vp]),
    "dgr_icp_scratch_bytes": (_sz, [_i, _i, _i]),
    "dgr_icp_step": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(IcpParams), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_intensity_map": (_i, [_vp, _i, _i, _i, _vp, _vp, _f, _vp, _vp]),
    "dgr_frame_halve": (_i, [_vp, _i, _i, _i, _vp, _vp, _f, _f, _f, _vp, _vp]),
    "dgr_rgbd_scratch_bytes": (_sz, [_i, _i, _i]),
    "dgr_rgbd_step": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(RgbdParams), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_pgo_scratch_bytes": (_sz, [_i, _i]),
    "dgr_pgo_plan": (_i, [_vp, _i, _i, _vp, _vp]),
    "dgr_pgo_solve": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, C.POINTER(PgoParams), _vp, _vp, _vp, _vp, _vp]),
    "dgr_contribution_scratch_bytes": (_sz, [C.c_long]),
    "dgr_contribution_stats": (_i, [_vp, C.c_long, _i, _i, _i, _vp, _vp, _vp, C.POINTER(ContributionParams), _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp]),
    "dgr_tsdf_integrate": (_i, [_vp, C.POINTER(TsdfGrid), _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(TsdfParams)]),
    "dgr_mesh_scratch_bytes": (_sz, [C.POINTER(TsdfGrid)]),
    "dgr_mesh_plan": (_i, [_vp, C.POINTER(TsdfGrid), _vp, _f, _i, _vp, _vp, _vp]),
    "dgr_mesh_emit": (_i, [_vp, C.POINTER(TsdfGrid), _vp, _vp, _f, _i, _vp, _vp, _vp]),
    "dgr_tsdf_brick_bytes": (_sz, [C.POINTER(TsdfGrid)]),
    "dgr_tsdf_bricks": (_i, [_vp, C.POINTER(TsdfGrid), _vp, _f, _vp]),
    "dgr_tsdf_raycast": (_i, [_vp, C.POINTER(TsdfGrid), _vp, _vp, _vp, _i, _i, _i, _vp, C.POINTER(RaycastParams), _vp, _vp, _vp, _vp]),
    "dgr_knn_index_bytes": (_sz, [_i]),
    "dgr_knn_scratch_bytes": (_sz, [_i, _i]),
    "dgr_knn_build": (_i, [_vp, _i, _vp, _vp, _vp]),
    "dgr_knn_search": (_i, [_vp, _vp, _i, _vp, _i, _vp, C.POINTER(KnnParams), _vp, _vp, _vp, _vp, _vp]),
    "dgr_point_covariances": (_i, [_vp, _i, _vp, _i, _vp, C.POINTER(CovarianceParams), _vp, _vp, _vp, _vp, _vp]),
    "dgr_gicp_scratch_bytes": (_sz, [_i, _i]),
    "dgr_gicp_step": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(GicpParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_densification_stats": (_i, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp]),
    "dgr_densify_plan_bytes": (_sz, [C.c_long]),
    "dgr_densify_plan": (_i, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _vp, _vp]),
    "dgr_densify_apply": (_i, [_vp, C.c_long, C.c_long, _vp, _i, C.POINTER(DensifyTensor), _vp, _vp, _vp, C.c_ulonglong]),
    "dgr_seed_plan_bytes": (_sz, [_i, _i, _i]),
    "dgr_seed_plan": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _f, _f, _f, _f, _vp, C.c_long, _vp, _vp]),
    "dgr_seed_apply": (_i, [_vp, _i, _i, _i, C.c_long, C.c_long, _vp, _i, C.POINTER(SeedTensor), _vp, _vp, _vp, _f, _f, _f, _f,
                            _f]),
    "dgr_relocate_scratch_bytes": (_sz, [C.c_long]),
    "dgr_relocate_plan": (_i, [_vp, C.c_long, _vp, _f, _vp, C.c_ulonglong, _i, _vp, _vp, _vp, _vp]),
    "dgr_relocate_apply": (_i, [_vp, C.c_long, _vp, _i, C.POINTER(RelocateTensor), _vp, _vp, C.c_double]),
    "dgr_position_noise": (_i, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp, C.c_ulonglong, _i, _vp, _f, _vp, _f, _f, _f]),
    "dgr_transform_scratch_bytes": (_sz, [C.c_long]),
    "dgr_transform_plan": (_i, [_vp, C.c_long, _vp, _vp, _vp]),
    "dgr_transform_apply": (_i, [_vp, C.c_long, C.c_long, _vp, _vp, _i, C.POINTER(TransformTensor), _vp]),
    "dgr_sparse_adam": (_i, [_vp, C.c_long, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i]),
    "dgr_sparse_adam_capturable": (_i, [_vp, C.c_long, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _vp]),
    "dgr_set_option": (_i, [C.c_char_p, _i]),
    "dgr_get_option": (_i, [C.c_char_p]),
    "dgr_set_thread_option": (_i, [C.c_char_p, _i]),
    "dgr_get_thread_option": (_i, [C.c_char_p]),
    "dgr_thread_options_effective": (_i, []),
    "dgr_thread_options_swap": (_i, [_i]),
    "dgr_version": (C.c_char_p, []),
    "dgr_geometry_bytes": (_sz, [_i]),
    "dgr_image_bytes": (_sz, [_i, _i]),
    "dgr_binning_bytes": (_sz, [_i, _i, _i]),
    "dgr_light_backward_scratch_bytes": (_sz, [_i, _i, _i]),
    "dgr_light_backward_scratch_bytes_r": (_sz, [_i, _i, _i, _i]),
    "dgr_mark_visible": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "dgr_light_forward": (_i, [_vp, ALLOC_FN, ALLOC_FN, ALLOC_FN, _vp, _i, _i, _i, _vp, _i, _i,
                               _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _i,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "dgr_light_forward_presized": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i,
                                        _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _i,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_light_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp,
                                _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                _vp, _i, _i, _vp, _sz]),
    "dgr_full_forward": (_i, [_vp, ALLOC_FN, ALLOC_FN, ALLOC_FN, _vp, _i, _i, _i, _vp, _i, _i,
                              _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _i,
                              _vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "dgr_full_forward_presized": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i,
                                       _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _i,
                                       _vp, _vp, _vp, _vp, _vp]),
    "dgr_full_backward": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "dgr_state_export": (C.c_long, [_vp, C.c_char_p, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "dgr_cov3d_forward": (_i, [_vp, _i, _vp, _vp, _f, _vp]),
    "dgr_cov3d_backward": (_i, [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp]),
    "dgr_debug_wave_reduce": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_debug_exact_math": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "dgr_debug_half_reduce": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_debug_half_reduce16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "dgr_debug_lane_lists": (_i, [_vp, _vp, _vp, _vp]),
    "dgr_debug_bin_tiles_trace": (_i, [_vp]),
    "dgr_debug_tile_sort": (_i, [_vp, _i, _i, _vp, C.POINTER(_i), _vp, _vp]),
    "dgr_profile_select": (_i, [C.c_char_p]),
    "dgr_profile_stage_count": (_i, []),
    "dgr_profile_stage_name": (C.c_char_p, [_i]),
    "dgr_profile_read": (_i, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(_i)]),
}
# absgrad (dgr_hip.h): each takes its namesake's arguments plus the absgrad output -- one device pointer, or (batches) a host array
# of n_views device pointers
_SIGS["dgr_light_backward_absgrad"] = (_i, _SIGS["dgr_light_backward"][1] + [_vp])
_SIGS["dgr_full_backward_absgrad"] = (_i, _SIGS["dgr_full_backward"][1] + [_vp])
_SIGS["dgr_light_backward_batch_absgrad"] = (_i, _SIGS["dgr_light_backward_batch"][1] + [C.POINTER(_vp)])
_SIGS["dgr_full_backward_batch_absgrad"] = (_i, _SIGS["dgr_full_backward_batch"][1] + [C.POINTER(_vp)])
# the exact silhouette gradient (dgr_hip.h): each takes its _absgrad namesake's arguments plus dL_dpix_silhouette -- one device
# pointer, or (batches) a host array of n_views device pointers
_SIGS["dgr_light_backward_silhouette"] = (_i, _SIGS["dgr_light_backward_absgrad"][1] + [_vp])
_SIGS["dgr_full_backward_silhouette"] = (_i, _SIGS["dgr_full_backward_absgrad"][1] + [_vp])
_SIGS["dgr_light_backward_batch_silhouette"] = (_i, _SIGS["dgr_light_backward_batch_absgrad"][1] + [C.POINTER(_vp)])
_SIGS["dgr_full_backward_batch_silhouette"] = (_i, _SIGS["dgr_full_backward_batch_absgrad"][1] + [C.POINTER(_vp)])

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def load():
    """Maps the HIP library; raises (never falls back) when it is missing or incomplete."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `make -C {_PKG}` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the rasterizer.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def last_error():
    return load().dgr_last_error().decode()


def ptr(t):
    """Device pointer of a tensor; NULL for None / empty tensors (the reference's nullptr convention)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def row_ptr(t, v):
    """Device pointer of view v's slice of a contiguous [V, ...] tensor (NULL for None / empty)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr() + v * t.stride(0) * t.element_size()


def call_backward(variant, n_views, args, abs_out=None, silhouette=None):
    """The one place that knows the three entry points of a backward (include/dgr_hip.h): dgr_<variant>_backward (n_views = 0)
    or dgr_<variant>_backward_batch with `args`; the _absgrad namesake, which takes one more argument, when only `abs_out` is
    given (the tensor that receives the absolute screen-space gradient, [P,3] or [V,P,3]); the _silhouette one, which takes
    both, when `silhouette` is (the silhouette gradient image [1,H,W] or [V,1,H,W], contiguous fp32 on the device).  Each goes
    in as one device pointer, or (batches) as a host array of n_views device pointers.  Returns the entry point's result."""
    def arg(t):
        if t is None or not n_views:
            return ptr(t)
        return (C.c_void_p * n_views)(*(row_ptr(t, v) for v in range(n_views)))
    name = f"dgr_{variant}_backward" + ("_batch" if n_views else "")
    if silhouette is not None:
        name, args = name + "_silhouette", (*args, arg(abs_out), arg(silhouette))
    elif abs_out is not None:
        name, args = name + "_absgrad", (*args, arg(abs_out))
    return getattr(load(), name)(*args)


def stream_handle(device_index=None):
    """Raw handle of torch's current HIP stream ON THE GIVEN DEVICE -- pass the index of the device the tensors live on
    (the private torch binding is ~20x cheaper than building a Stream object)."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if device_index is None else device_index)
    except AttributeError:  # pragma: no cover -- other torch builds
        return torch.cuda.current_stream(device_index).cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_GUARD = _NoGuard()


def on_device(dev):
    """Context manager that makes `dev` the current HIP device for the C-ABI calls inside it (kernels are launched on
    a stream of `dev` against pointers of `dev`; the library's events and workspaces are created on the current
    device).  Free when `dev` already is current."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


class StepCalls:
    """The one way a step enters the C ABI, for the calls of one invocation (an Adam step's call per tensor, a plan call and its
    apply calls): `with StepCalls(device) as abi: abi.call("dgr_<name>", *args)`.  The device rule: `device` (the tensors') is
    made current for the block and `stream` is ITS current stream, whichever device was current; both are looked up once."""
    __slots__ = ("device", "lib", "stream", "_guard")

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        self.lib = load()
        self._guard = on_device(self.device)
        self._guard.__enter__()
        self.stream = stream_handle(self.device.index)
        return self

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)

    def call(self, name_or_fn, *args):
        """`dgr_<name>(stream, *args)`; RuntimeError with the library's message on a non-zero result"""
        fn = getattr(self.lib, name_or_fn) if isinstance(name_or_fn, str) else name_or_fn
        if fn(self.stream, *args):
            raise RuntimeError(last_error())

    def capturing(self):
        """whether the stream is being recorded into a hipGraph"""
        return bool(self.lib.dgr_stream_is_capturing(self.stream))


def call(name_or_fn, device, *args):
    """One step call into the C ABI: `StepCalls(device)` used once."""
    with StepCalls(device) as abi:
        abi.call(name_or_fn, *args)


def set_option(name, value):
    """Process-wide library option (include/dgr_hip.h: dgr_set_option), e.g. set_option("tight_cull", 1)."""
    if load().dgr_set_option(name.encode(), int(value)):
        raise ValueError(last_error())


def get_option(name):
    return load().dgr_get_option(name.encode())


class thread_options:
    """`with thread_options(alpha_mode=1, tight_cull=1): ...` -- the calling THREAD's rasterizer calls inside the block use these
    values of the per-call options (include/dgr_hip.h: dgr_set_thread_option) whatever the process-wide ones are; other threads
    are not affected, and a backward runs under its forward's options wherever autograd runs it.  Names: alpha_mode (fast_alpha),
    tight_cull, deterministic_grads, pose_grad (1: the complete pose gradient, include/dgr_hip.h), silhouette_grad (1: the bindings
    pass the exact silhouette gradient of opacity_map / uncertainty)."""

    def __init__(self, **options):
        self.options = options
        self.prev = None

    def __enter__(self):
        lib = load()
        self.prev = lib.dgr_thread_options_swap(-1)
        for k, v in self.options.items():
            if lib.dgr_set_thread_option(k.encode(), int(v)):
                lib.dgr_thread_options_swap(self.prev)
                raise ValueError(last_error())
        return self

    def __exit__(self, *exc):
        load().dgr_thread_options_swap(self.prev)
        return False


def silhouette_on(word):
    """Whether a dgr_thread_options_effective() word has the option "silhouette_grad" on (bits 16-19: value + 1)."""
    return ((int(word) >> 16) & 15) == 2  # 16 = DGR_OPT_SHIFT_SILHOUETTE_GRAD (include/dgr_hip.h)


class under_options:
    """Runs a block under a word of dgr_thread_options_effective() (a backward under its forward's options)."""

    def __init__(self, word):
        self.word = word

    def __enter__(self):
        self.prev = load().dgr_thread_options_swap(self.word)

    def __exit__(self, *exc):
        load().dgr_thread_options_swap(self.prev)
        return False


def profile_select(stage=""):
    rc = load().dgr_profile_select(stage.encode())
    if rc:
        raise ValueError(f"unknown stage {stage!r}")


def profile_stages():
    lib = load()
    return [lib.dgr_profile_stage_name(i).decode() for i in range(lib.dgr_profile_stage_count())]


def profile_read(stage):
    """(total milliseconds, launches) recorded for `stage` since the last read."""
    tot, n = C.c_double(0), C.c_int(0)
    rc = load().dgr_profile_read(stage.encode(), C.byref(tot), C.byref(n))
    if rc:
        raise ValueError(f"unknown stage {stage!r}")
    return tot.value, n.value
