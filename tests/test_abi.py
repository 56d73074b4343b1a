"""CPU test: libemoportraits_hip.so loads and exports every symbol include/emo_hip.h declares (no kernel is launched)."""
import ctypes
import os
import re

from emoportraits_amd import hip, _abi_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(emo_[a-z0-9_]+)\s*\(", src)))


def test_header_python_and_library_agree():
    names = _declared()
    assert names, "no declarations parsed"
    assert sorted(hip.SIGNATURES) == names, "emoportraits_amd/hip.py SIGNATURES out of sync with include/emo_hip.h"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in emo_hip.h but not exported"


def test_abi_version_and_build_info():
    lib = hip.load()
    assert lib.emo_abi_version() == _abi_version.EMO_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert int(re.search(r"#define EMO_ABI_VERSION (\d+)", hdr).group(1)) == _abi_version.EMO_ABI_VERSION
    assert b"gfx950" in lib.emo_build_info()


def test_argument_errors_are_reported_without_touching_the_gpu():
    lib = hip.load()
    # null pointers -> EMO_ERR_BAD_ARG before any launch
    rc = lib.emo_grid_sample3d_f32(None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, None)
    assert rc == -1
    rc = lib.emo_conv_igemm_f32(None, None, None, None, None, None, None, 1, 4, 4, 1, 8, 8, 1, 3, 3, 0, 0, 0, 0, 0, 1, None, None, None)
    assert rc == -1


def test_op_launch_form_tables_and_answers_without_a_device():
    """ABI 28: hip.OPS / OP_FORMS / OP_PLAN are the enums of include/emo_hip.h, and emo_op_launch_form answers from the launchers'
    own host functions -- no launch, no device"""
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    enum = lambda prefix: {n.lower(): int(v) for n, v in re.findall(rf"\b{prefix}([A-Z0-9_]+) = (\d+)", hdr)}
    ops_, plan = enum("EMO_OP_(?!PLAN_)"), enum("EMO_OP_PLAN_")
    assert ops_.pop("count") == len(ops_) and ops_ == hip.OPS
    assert plan.pop("count") == len(plan) and plan == {n: i for i, n in enumerate(hip.OP_PLAN)}
    for op, prefix in (("upsample_trilinear", "UPSAMPLE"), ("avgpool", "AVGPOOL"), ("groupnorm_affine", "GROUPNORM")):
        forms = enum(f"EMO_{prefix}_FORM_")
        assert forms.pop("count") == len(forms) and forms == {n: i for i, n in enumerate(hip.OP_FORMS[op])}
    assert "ABI 28." in hdr and "int emo_op_launch_form(int op, const void* x, const void* out, const int64_t* dims, int64_t* plan);" in hdr
    a = 1 << 20                                                 # an aligned address: read for nullness and alignment only
    assert hip.op_launch_form("avgpool", a, a, (6, 4, 6, 8, 2, 1, 1)) == (0, dict(form="x4_w1", grid=1, items=144, cr=0, runs=0, split=0,
                                                                                   per=0, run_items=0))
    assert hip.op_launch_form("avgpool", a + 4, a, (6, 4, 6, 8, 2, 1, 1))[1]["form"] == "generic"
    assert hip.op_launch_form("avgpool", a, a, (6, 4, 6, 8, 17, 1, 1)) == (-2, None)
    assert hip.op_launch_form("avgpool", None, a, (6, 4, 6, 8, 2, 1, 1)) == (-1, None)
    rc, p = hip.op_launch_form("upsample_trilinear", a, a, (1, 8, 16, 34, 2, 2, 2))
    assert rc == 0 and (p["form"], p["cr"], p["runs"], p["split"], p["per"], p["run_items"], p["grid"]) == ("block", 1, 1, 2, 1301, 2601, 2)
    assert hip.op_launch_form("upsample_trilinear", a, a + 4, (1, 8, 16, 34, 2, 2, 2))[1]["form"] == "generic"
    assert hip.op_launch_form("upsample_trilinear_gn_sums", a, a + 4, (1, 2, 1, 8, 16, 34, 2, 2, 2)) == (-2, None)
    rc, p = hip.op_launch_form("groupnorm_affine", a, None, (1, 2, 1100 * 1000, 1))
    assert rc == 0 and (p["form"], p["split"], p["runs"], p["run_items"], p["grid"]) == ("pass", 64, 1, 2200000, 64)
    assert hip.op_launch_form("groupnorm_affine", a, None, (1, 3, 10, 2)) == (-1, None)


def test_sampler_launch_form_tables_and_answers_without_a_device():
    """ABI 29: hip.GS3D_KINDS / GS3D_FORMS / GS3D_PLAN / REPACK_DIRECTIONS / REPACK_PLAN are the enums of include/emo_hip.h, and the two
    entry points answer from the launchers' own host functions -- no launch, no device"""
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    enum = lambda prefix: {n.lower(): int(v) for n, v in re.findall(rf"\b{prefix}([A-Z0-9_]+) = (\d+)", hdr)}
    for prefix, table in (("EMO_GS3D_KIND_", tuple(hip.GS3D_KINDS)), ("EMO_GS3D_FORM_", hip.GS3D_FORMS), ("EMO_GS3D_PLAN_", hip.GS3D_PLAN),
                          ("EMO_REPACK_(?!PLAN_)", hip.REPACK_DIRECTIONS), ("EMO_REPACK_PLAN_", hip.REPACK_PLAN)):
        e = enum(prefix)
        assert e.pop("count") == len(e) and e == {n: i for i, n in enumerate(table)}, prefix
    assert hip.GS3D_KINDS == {"grid": 0, "delta": 1, "theta": 2}
    assert _abi_version.EMO_ABI_VERSION >= 29 and "ABI 29." in hdr
    assert ("int emo_grid_sample3d_launch_form(const void* vol, const void* out, int banked, int N, int C, int D, int H, int W, int Do, "
            "int Ho, int Wo, int64_t vol_batch_stride, int padding_mode, int in_layout, int out_layout, int variant, int grid_kind, "
            "int64_t* plan);") in hdr
    assert ("int emo_volume_repack_launch_form(const void* in, const void* out, int N, int C, int DHW, int to_channels_last, int indexed, "
            "int64_t* plan);") in hdr
    a = 1 << 20                                                 # an aligned address: read for nullness and alignment only
    zero = dict.fromkeys(hip.GS3D_PLAN, 0)
    q = lambda *args, **kw: hip.sampler_launch_form(a, a, *args, **kw)
    assert q(16, 4, (3, 5, 7), (2, 16, 32), in_layout="ndhwc", out_layout="ndhwc", shared=True, variant=4) == (0, dict(
        zero, form="rows", order=3, fma=1, grid_x=256, grid_y=1, grid_z=1, bps=16, last_vox=64, cpb=4))
    assert q(12, 4, (3, 5, 7), (2, 16, 32), in_layout="ndhwc", out_layout="ndhwc", shared=True)[1]["order"] == 1
    assert q(2, 232, (3, 5, 7), (1, 3, 5), in_layout="ndhwc", out_layout="ncdhw", variant=2) == (0, dict(
        zero, form="rows_ncdhw", order=1, nt=1, grid_x=2, grid_y=1, grid_z=1, bps=1, last_vox=15, cpb=232, lds=65440))
    assert q(2, 236, (3, 5, 7), (1, 3, 5), in_layout="ndhwc", out_layout="ncdhw") == (-2, None)
    assert q(5, 12, (3, 5, 7), (4, 4, 8), in_layout="ndhwc", out_layout="ndhwc", variant=5, banked=True) == (0, dict(
        zero, form="brick", order=1, bank=1, grid_x=10, grid_y=1, grid_z=1, bps=2, last_vox=64, cpb=12))
    assert q(3, 7, (3, 5, 7), (3, 10, 11), variant=4, mode="delta") == (0, dict(
        zero, form="planar", grid_x=2, grid_y=2, grid_z=3, bps=2, last_vox=74, cpb=4))
    assert q(2, 8, (3, 6, 8), (5, 9, 20), in_layout="p4", out_layout="ncdhw", mode="theta") == (0, dict(        # 3 x 2 x 2 tiles of 8 x 8 x 4
        zero, form="tile_p4_ncdhw", grid_x=24, grid_y=1, grid_z=1, bps=12, cpb=8, lds=40960, threads=256, vpt=1, upb=2, txs=3, tys=3, tzs=2,
        stage_slots=2296))
    assert q(2, 8, (3, 6, 7), (4, 8, 8), variant=1 << 30)[1]["form"] == "planar"          # W % 4: the tile flag falls through
    assert q(2, 8, (3, 6, 8), (4, 8, 8), variant=1 << 30)[1]["form"] == "tile_planar"
    assert q(2, 8, (3, 6, 8), (4, 8, 8), in_layout="ndhwc", out_layout="ndhwc", variant=8) == (-1, None)
    assert hip.sampler_launch_form(a + 4, a, 2, 8, (3, 6, 8), (4, 8, 8)) == (-3, None)
    assert hip.sampler_launch_form(None, a, 2, 8, (3, 6, 8), (4, 8, 8)) == (-1, None)
    assert hip.repack_launch_form(a, a, 3, 65, 130, 1) == (0, dict(direction="to_channels_last", grid_x=3, grid_y=2, grid_z=3))
    assert hip.repack_launch_form(a, a, 3, 65, 130, 0) == (0, dict(direction="from_channels_last", grid_x=2, grid_y=3, grid_z=3))
    assert hip.repack_launch_form(a, a, 3, 65, 130, 1, indexed=True)[1]["direction"] == "to_channels_last_indexed"
    assert hip.repack_launch_form(a, a, 3, 8, 65, 4) == (0, dict(direction="to_p4", grid_x=1, grid_y=3, grid_z=1))
    assert hip.repack_launch_form(a, a, 1, 1, 65536 * 64, 0) == (-2, None)             # grid y > 65535
    assert hip.repack_launch_form(a, a, 1, 1, 65535 * 64, 0)[1]["grid_y"] == 65535
    assert hip.repack_launch_form(a, a, 3, 65, 130, 0, indexed=True) == (-1, None)


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from emoportraits_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grid_sample3d(torch.zeros(1, 4, 2, 2, 2), torch.zeros(1, 1, 1, 1, 3))
