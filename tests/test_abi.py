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


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from emoportraits_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grid_sample3d(torch.zeros(1, 4, 2, 2, 2), torch.zeros(1, 1, 1, 1, 3))
