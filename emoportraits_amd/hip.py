"""ctypes binding of libemoportraits_hip.so -- the C ABI declared in include/emo_hip.h.

The product path has NO fallback: if the library is missing or a kernel call fails, a RuntimeError is raised.
PyTorch is only plumbing here (device memory, streams): tensors are passed as raw device pointers.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EMO_HIP_LIB selects an alternative build of the same library (A/B measurements of kernel variants only)
LIB_PATH = os.environ.get("EMO_HIP_LIB") or os.path.join(_HERE, "lib", "libemoportraits_hip.so")

PAD_MODES = {"zeros": 0, "border": 1, "reflection": 2}
LAYOUT_NCDHW, LAYOUT_NDHWC, LAYOUT_P4 = 0, 1, 3
ACT = {"none": 0, "relu": 1, "tanh": 2, "sigmoid": 3}

_c_int, _c_i64, _c_void, _c_float, _c_double = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double

# name -> argtypes; restype is int unless listed in _RESTYPES.  Mirrors include/emo_hip.h one to one
# (tests/test_abi.py checks header <-> this table <-> exported symbols).
SIGNATURES = {
    "emo_abi_version": [],
    "emo_build_info": [],
    "emo_device_cu_count": [],
    "emo_mfma_stream_f16": [_c_void, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_void],
    "emo_grid_sample3d_f32": [_c_void] * 7 + [_c_int] * 8 + [_c_i64] + [_c_int] * 5 + [_c_void],
    "emo_grid_sample3d_indexed_f32": [_c_void, _c_void, _c_int] + [_c_void] * 6 + [_c_int] * 13 + [_c_void],
    "emo_grid_sample3d_launch_form": [_c_void, _c_void] + [_c_int] * 9 + [_c_i64] + [_c_int] * 5 + [ctypes.POINTER(_c_i64)],
    "emo_volume_repack_launch_form": [_c_void, _c_void] + [_c_int] * 5 + [ctypes.POINTER(_c_i64)],
    "emo_affine_grid3d_f32": [_c_void] * 5 + [_c_int] * 4 + [_c_void],
    "emo_volume_repack_f32": [_c_void, _c_void, _c_int, _c_int, _c_int, _c_int, _c_void],
    "emo_volume_repack_indexed_f32": [_c_void, _c_void, _c_void, _c_int, _c_int, _c_int, _c_int, _c_void],
    "emo_groupnorm_workspace_bytes": [_c_int, _c_int],
    "emo_groupnorm_affine_f32": [_c_void, _c_int, _c_int, _c_i64, _c_int, _c_float] + [_c_void] * 4 + [_c_i64]
                                + [_c_void] * 5 + [_c_i64, _c_void],
    "emo_groupnorm_affine_from_tiles_f32": [_c_void, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_float] + [_c_void] * 4
                                           + [_c_i64] + [_c_void] * 5,
    "emo_groupnorm_affine_from_sums_f32": [_c_void, _c_int, _c_int, _c_int, _c_i64, _c_int, _c_float] + [_c_void] * 4
                                          + [_c_i64] + [_c_void] * 5,
    "emo_conv_pack_info": [_c_int, _c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)],
    "emo_conv_tile_positions": [_c_int],
    "emo_conv_igemm_f32": [_c_void] * 7 + [_c_int] * 15 + [_c_void, _c_void, _c_void],
    "emo_conv_igemm_ksplit": [_c_int] * 11,
    "emo_conv_pack_info_f16": [_c_int, _c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)],
    "emo_conv_igemm_f16acc32": [_c_void] * 7 + [_c_int] * 15 + [_c_void, _c_void, _c_void],
    "emo_conv_igemm_f16w8": [_c_void] * 7 + [_c_int] * 15 + [_c_void, _c_void, _c_void, ctypes.c_float],
    "emo_conv_igemm_f16w8_rest": [_c_void] * 8 + [_c_int] * 15 + [_c_void, _c_void, _c_void, ctypes.c_float],
    "emo_conv_accepts": [_c_int, ctypes.POINTER(_c_int)] + [_c_int] * 15 + [_c_float, _c_float, _c_int],
    "emo_conv_pack_info_bf16x3": [_c_int, _c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)],
    "emo_conv_igemm_bf16x3": [_c_void] * 7 + [_c_int] * 15 + [_c_void, _c_void, _c_void, _c_void],
    "emo_conv_igemm_f16x2": [_c_void] * 7 + [_c_int] * 15 + [_c_void, _c_void, _c_void, ctypes.c_float, ctypes.c_float, _c_void],
    "emo_conv_igemm_f32_guarded": [_c_void] * 7 + [_c_int] * 15 + [_c_void, _c_void, _c_void, _c_void],
    "emo_conv_head_f32": [_c_void] * 6 + [_c_int, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_void],
    "emo_stage2_head_f32": [_c_void] * 10 + [_c_int, _c_int, _c_i64, _c_int, _c_void],
    "emo_upsample_trilinear_f32": [_c_void, _c_void, _c_i64] + [_c_int] * 6 + [_c_void],
    "emo_upsample_trilinear_gn_sums_f32": [_c_void, _c_void] + [_c_int] * 9 + [_c_void, _c_i64, ctypes.POINTER(_c_int), _c_void],
    "emo_avgpool_f32": [_c_void, _c_void, _c_i64] + [_c_int] * 6 + [_c_void],
    "emo_add_f32": [_c_void, _c_void, _c_void, _c_i64, _c_i64, _c_float, _c_void],
    "emo_add_rows_indexed_f32": [_c_void] * 4 + [_c_int, _c_int, _c_i64, _c_float, _c_void],
    "emo_op_launch_form": [_c_int, _c_void, _c_void, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)],
    "emo_resize2d_f32": [_c_void, _c_i64, _c_i64, _c_void, _c_i64] + [_c_int] * 6 + [_c_void],
    "emo_resize2d_windows_f32": [_c_void, _c_i64, _c_i64, _c_void, _c_void] + [_c_int] * 6 + [_c_void],
    "emo_conv2d_generic_f32": [_c_void] * 6 + [_c_int] * 11 + [_c_void, _c_void],
    "emo_conv2d_generic_splits": [_c_int] * 9,
    "emo_maxpool2d_f32": [_c_void] * 4 + [_c_i64] + [_c_int] * 6 + [_c_void],
    "emo_affine_add_relu_f32": [_c_void] * 7 + [_c_i64, _c_i64, _c_int, _c_void],
    "emo_grid_sample2d_f32": [_c_void] * 6 + [_c_int] * 6 + [_c_void],
    "emo_mat4_inverse_f32": [_c_void, _c_void, _c_int, _c_void],
    "emo_mixing_theta_f32": [_c_void, _c_void, _c_void, _c_int, _c_int, _c_int, _c_void, _c_void],
    "emo_theta_ema_scan_f32": [_c_void] * 4 + [_c_int, _c_int, _c_float, _c_float, _c_void, _c_void],
    "emo_expr_controls_f32": [_c_void] * 9 + [_c_int] * 5 + [_c_float, _c_float, _c_void, _c_void],
    "emo_head_pose_controls_f32": [_c_void, _c_int] + [_c_void] * 10 + [_c_int] * 4 + [_c_void] * 3,
    "emo_theta_ema_scan_tracks_f32": [_c_void] * 4 + [_c_int, _c_int, _c_float, _c_float] + [_c_void] * 4,
    "emo_expr_controls_tracks_f32": [_c_void] * 9 + [_c_int] * 5 + [_c_float, _c_float] + [_c_void] * 4,
    "emo_head_pose_controls_tracks_f32": [_c_void, _c_int] + [_c_void] * 10 + [_c_int] * 4 + [_c_void] * 5,
    "emo_crop_track_f64": [_c_void] * 3 + [_c_int, _c_int] + [_c_void] * 3 + [_c_int, _c_int, _c_double, _c_double, _c_int, _c_int,
                           _c_double] + [_c_int] * 3 + [_c_void] * 4,
    "emo_crop_track_restarts_f64": [_c_void] * 3 + [_c_int, _c_int] + [_c_void] * 3 + [_c_int, _c_int, _c_double, _c_double, _c_int,
                                    _c_int, _c_double] + [_c_int] * 3 + [_c_void] * 5,
    "emo_track_assign_f64": [_c_void, _c_void] + [_c_int] * 4 + [_c_void, _c_void, _c_double, _c_int, _c_int] + [_c_void] * 4,
    "emo_present_rows_i32": [_c_void, _c_void, _c_int, _c_int] + [_c_void] * 6,
    "emo_mul_mask_f32": [_c_void, _c_void, _c_void, _c_int, _c_int, _c_i64, _c_void],
    "emo_stage2_compose_f32": [_c_void] * 5 + [_c_int, _c_int, _c_i64, _c_void],
    "emo_small_gemm_f32": [_c_void] * 3 + [_c_int] * 4 + [_c_i64, _c_i64, _c_void],
    "emo_projector_finalize_f32": [_c_void] * 7 + [_c_int] * 3 + [_c_void],
    "emo_pose_theta_f32": [_c_void, _c_int, _c_void, _c_void, _c_void, _c_int, _c_void],
    "emo_pack_rgb8": [_c_void, _c_void, _c_int, _c_int, _c_int, _c_void],
    "emo_unpack_rgb8": [_c_void, _c_void, _c_int, _c_int, _c_int, _c_void],
    "emo_paste_windows_rgb8": [_c_void] * 5 + [_c_int] * 4 + [_c_float, _c_void],
    "emo_nv12_windows_f32": [_c_void, _c_void, _c_i64, _c_i64, _c_int, _c_int, _c_void, _c_void, _c_void] + [_c_int] * 5 + [_c_void],
    "emo_pack_nv12": [_c_void, _c_void, _c_void, _c_i64, _c_i64] + [_c_int] * 5 + [_c_void],
    "emo_paste_windows_nv12": [_c_void] * 6 + [_c_i64, _c_i64] + [_c_int] * 4 + [_c_float, _c_int, _c_int, _c_void],
    "emo_resize2d_faces_f32": [_c_void, _c_i64, _c_i64, _c_void, _c_void, _c_void] + [_c_int] * 7 + [_c_void],
    "emo_nv12_faces_f32": [_c_void, _c_void, _c_i64, _c_i64, _c_int, _c_int] + [_c_void] * 5 + [_c_int] * 6 + [_c_void],
    "emo_paste_faces_rgb8": [_c_void] * 7 + [_c_int] * 5 + [_c_float, _c_void],
    "emo_paste_faces_nv12": [_c_void] * 8 + [_c_i64, _c_i64] + [_c_int] * 5 + [_c_float, _c_int, _c_int, _c_void],
    "emo_rgb8_faces_ragged_f32": [_c_void] * 7 + [_c_int] * 4 + [_c_void],
    "emo_nv12_faces_ragged_f32": [_c_void] * 7 + [_c_int] * 6 + [_c_void],
    "emo_paste_faces_ragged_rgb8": [_c_void] * 8 + [_c_int] * 3 + [_c_float, _c_void],
    "emo_paste_faces_ragged_nv12": [_c_void] * 8 + [_c_int] * 3 + [_c_float, _c_int, _c_int, _c_void],
    "emo_yuv420_crop_f32": [_c_int] + [_c_void] * 3 + [_c_i64] * 3 + [_c_int, _c_int] + [_c_void] * 5 + [_c_int] * 6 + [_c_void],
    "emo_pack_yuv420": [_c_int] + [_c_void] * 4 + [_c_i64] * 3 + [_c_int] * 5 + [_c_void],
    "emo_paste_yuv420": [_c_int] + [_c_void] * 9 + [_c_i64] * 3 + [_c_int] * 5 + [_c_float, _c_int, _c_int, _c_void],
    "emo_yuv420_crop_ragged_f32": [_c_int] + [_c_void] * 7 + [_c_int] * 6 + [_c_void],
    "emo_paste_ragged_yuv420": [_c_int] + [_c_void] * 8 + [_c_int] * 3 + [_c_float, _c_int, _c_int, _c_void],
}
_RESTYPES = {"emo_build_info": ctypes.c_char_p, "emo_groupnorm_workspace_bytes": _c_i64}

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load():
    """dlopen the library (idempotent).  Raises HipLibraryError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `python -m emoportraits_amd.build` (there is no CPU/eager fallback)")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise HipLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}; rebuild the library") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, _c_int)
    from . import _abi_version
    v = lib.emo_abi_version()
    if v != _abi_version.EMO_ABI_VERSION:
        raise HipLibraryError(f"ABI mismatch: library {v}, python {_abi_version.EMO_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


# emo_op_launch_form (ABI 28): the ops, their forms and the plan slots of include/emo_hip.h (tests/test_abi.py pins them to it)
OPS = {"upsample_trilinear": 0, "upsample_trilinear_gn_sums": 1, "avgpool": 2, "groupnorm_affine": 3}
OP_FORMS = {"upsample_trilinear": ("generic", "block"), "upsample_trilinear_gn_sums": ("generic", "block"),
            "avgpool": ("generic", "x4_w1", "x4_w2"), "groupnorm_affine": ("pass",)}
OP_PLAN = ("form", "grid", "items", "cr", "runs", "split", "per", "run_items")


def op_launch_form(op, x, out, dims):
    """What the launcher of `op` would do with these arguments, launching nothing: (rc, plan).  x, out: addresses (ints) or None;
    dims: the launcher's integer shape arguments in its order.  plan: OP_PLAN names -> ints, 'form' as its name; None if rc != 0"""
    lib = load()
    d = (_c_i64 * 9)(*[int(v) for v in dims])              # (the longest argument list; the rest zero)
    p = (_c_i64 * len(OP_PLAN))()
    rc = lib.emo_op_launch_form(OPS[op], ctypes.c_void_p(x) if x else None, ctypes.c_void_p(out) if out else None, d, p)
    if rc != 0:
        return rc, None
    plan = dict(zip(OP_PLAN, (int(v) for v in p)))
    plan["form"] = OP_FORMS[op][plan["form"]]
    return rc, plan


# emo_grid_sample3d_launch_form / emo_volume_repack_launch_form (ABI 29): the enums of include/emo_hip.h (tests/test_abi.py)
GS3D_KINDS = {"grid": 0, "delta": 1, "theta": 2}
GS3D_FORMS = ("planar", "rows", "rows_ncdhw", "brick", "tile_p4", "tile_p4_ncdhw", "tile_planar")
GS3D_PLAN = ("form", "order", "fma", "nt", "bank", "grid_x", "grid_y", "grid_z", "bps", "last_vox", "cpb", "lds", "threads", "vpt",
             "upb", "txs", "tys", "tzs", "stage_slots")
REPACK_DIRECTIONS = ("from_channels_last", "to_channels_last", "to_channels_last_indexed", "to_p4", "from_p4")
REPACK_PLAN = ("direction", "grid_x", "grid_y", "grid_z")
_LAYOUTS = {"ncdhw": LAYOUT_NCDHW, "ndhwc": LAYOUT_NDHWC, "p4": LAYOUT_P4}


def sampler_launch_form(vol, out, N, C, vol_dims, out_dims, padding_mode="zeros", in_layout="ncdhw", out_layout="ncdhw", variant=0,
                        mode="grid", shared=False, banked=False):
    """What grid_sample3d's entry would do with these arguments, launching nothing: (rc, plan).  vol, out: addresses (ints) or
    None; vol_dims (D, H, W), out_dims (Do, Ho, Wo); mode 'grid' / 'delta' / 'theta'; shared: one volume for the N samples
    (stride 0); banked: the indexed entry.  plan: GS3D_PLAN names -> ints, 'form' as its name; None if rc != 0"""
    lib = load()
    D, H, W = (int(v) for v in vol_dims)
    Do, Ho, Wo = (int(v) for v in out_dims)
    p = (_c_i64 * len(GS3D_PLAN))()
    rc = lib.emo_grid_sample3d_launch_form(ctypes.c_void_p(vol) if vol else None, ctypes.c_void_p(out) if out else None, int(bool(banked)),
                                           int(N), int(C), D, H, W, Do, Ho, Wo, 0 if shared else int(C) * D * H * W,
                                           PAD_MODES[padding_mode], _LAYOUTS[in_layout], _LAYOUTS[out_layout], int(variant),
                                           GS3D_KINDS[mode], p)
    if rc != 0:
        return rc, None
    plan = dict(zip(GS3D_PLAN, (int(v) for v in p)))
    plan["form"] = GS3D_FORMS[plan["form"]]
    return rc, plan


def repack_launch_form(inp, out, N, C, DHW, to_channels_last, indexed=False):
    """The same question about emo_volume_repack_f32 / emo_volume_repack_indexed_f32: (rc, plan), plan REPACK_PLAN names -> ints
    with 'direction' as its name; None if rc != 0"""
    lib = load()
    p = (_c_i64 * len(REPACK_PLAN))()
    rc = lib.emo_volume_repack_launch_form(ctypes.c_void_p(inp) if inp else None, ctypes.c_void_p(out) if out else None, int(N), int(C),
                                           int(DHW), int(to_channels_last), int(bool(indexed)), p)
    if rc != 0:
        return rc, None
    plan = dict(zip(REPACK_PLAN, (int(v) for v in p)))
    plan["direction"] = REPACK_DIRECTIONS[plan["direction"]]
    return rc, plan


_ERR = {-1: "EMO_ERR_BAD_ARG", -2: "EMO_ERR_UNSUPPORTED", -3: "EMO_ERR_ALIGN"}


def check(rc, what):
    if rc != 0:
        name = _ERR.get(rc, f"hipError {rc}" if rc > 0 else f"error {rc}")
        raise RuntimeError(f"{what} failed: {name}")


def ptr(t):
    """device pointer of a tensor (or None)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda_f32(*tensors):
    import torch
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("emoportraits_amd ops run on the GPU only (got a %s tensor); there is no CPU path"
                               % t.device.type)
        if t.dtype != torch.float32:
            raise RuntimeError("expected float32, got %s" % t.dtype)
        if not t.is_contiguous():
            raise RuntimeError("expected a contiguous tensor")
