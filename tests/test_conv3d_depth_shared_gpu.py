"""GPU parity of the depth-shared 32-row kernel of 3x3x3 layers (csrc/conv_igemm_f16x2_zs.h): the same config-F f16x2 launches
as tests/test_conv3d_depth_shared_emul.py, through ops.conv_igemm, against torch's CPU convolution and an fp64 one.

The launcher takes this kernel only when runs of at least six slices fill the chip; these volumes are far smaller, so the tests
set its measurement switch EMO_CONV_ZS_RUN (runs of that many output slices whatever the size; read at every launch) and ask the
launcher which kernel each launch took (emo_debug_conv_zs_last_run)."""
import math

import pytest
import torch
import torch.nn.functional as F

from emoportraits_amd import hip, ops, pack
from conv_plans import Expect
from test_kernels_gpu import DEV, rel_err, run_conv

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
RUN = 3      # forced run length: three live accumulator sets, and a seam wherever D > 3


@pytest.fixture(autouse=True)
def forced_runs(monkeypatch):
    monkeypatch.setenv("EMO_CONV_ZS_RUN", str(RUN))


def took(run):
    return hip.load().emo_debug_conv_zs_last_run() == run


def seam_depth(N, Cout, H, W):
    """the depth at which the launcher's run length leaves one slice for a second run"""
    lib = hip.load()
    for D in range(2, 66):
        if lib.emo_debug_conv_zs_run(N, Cout, D, H, W, 0) == D - 1:
            return D
    raise AssertionError("no depth with run length D - 1")


CASES = {
    "64->32 (3,8,64) affine relu res": dict(N=2, Cin=64, Cout=32, dims=(3, 8, 64), affine=True, relu_in=True, res=True),
    "32->32 (1,4,64) kd = 1 only": dict(N=1, Cin=32, Cout=32, dims=(1, 4, 64), affine=True, relu_in=True),
    "32->32 (2,4,64) kd pairs": dict(N=1, Cin=32, Cout=32, dims=(2, 4, 64), affine=True, relu_in=True),
    "16->32 (5,4,64) no bias, one chunk": dict(N=1, Cin=16, Cout=32, dims=(5, 4, 64), bias=False),
    "24->24 (4,8,64) ragged chunk and tile": dict(N=2, Cin=24, Cout=24, dims=(4, 8, 64), affine=True, relu_in=True),
    "32->32 (run+1,8,64) seam": dict(N=3, Cin=32, Cout=32, dims=None, affine=True, relu_in=True, res=True),
    "32->3 (4,4,64) tanh: the warp head": dict(N=2, Cin=32, Cout=3, dims=(4, 4, 64), affine=True, relu_in=True, act="tanh"),
    # (beyond the issue's list: more items than the chip has CUs, so that persistent blocks walk consecutive items)
    "16->32 (4,520,64) 520 items": dict(N=2, Cin=16, Cout=32, dims=(4, 520, 64), affine=True, relu_in=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_depth_shared_kernel_meets_the_split_kernels_bound(name):
    case = dict(CASES[name])
    if case["dims"] is None:
        case["dims"] = (seam_depth(case["N"], case["Cout"], 8, 64), 8, 64)
        assert case["dims"][0] == RUN + 1
    tile = Expect("f16x2", pack.CFG_F)
    e, got, ref = run_conv(seed=41, precision="f16x2", k=3, cfg=3, expect=tile, **case)
    assert took(min(RUN, case["dims"][0])), "the launch did not take the depth-shared kernel"
    print("PARITY conv f16x2 depth-shared:", name, f"{e:.2e}")
    assert e < 2e-5, e
    e2, got2, _ = run_conv(seed=41, precision="f16x2", k=3, cfg=3, expect=tile, **case)
    assert torch.equal(got, got2), "two launches on the same input differ: a race in the pipeline"


def test_statistics_and_range_check():
    """tile statistics (one entry per 4 x 64 tile of one output slice) give the GroupNorm affine of a direct reduction; an input
    pushed past the fp16 range raises the overflow word and the guarded bf16x3 launch rewrites output and statistics:
    bit-identical to a plain bf16x3 launch"""
    g = torch.Generator().manual_seed(43)
    N, Cin, Cout, D, H, W = 2, 64, 32, 3, 8, 64
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(Cin * 27)
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(N, Cin, D, H, W, generator=g)
    sc, sh = torch.rand(N, Cin, generator=g) + 0.5, torch.randn(N, Cin, generator=g) * 0.3
    r = torch.randn(N, Cout, D, H, W, generator=g)
    l2 = pack.PackedConv("zs", w, b, DEV, precision="f16x2")
    ops.clear_overflow_flags(DEV)
    out, st = ops.conv_igemm(x.to(DEV), l2, sc.to(DEV), sh.to(DEV), relu_in=True, res=r.to(DEV), want_stats=True)
    assert took(RUN)
    ref = F.conv3d(F.relu(x * sc.view(N, Cin, 1, 1, 1) + sh.view(N, Cin, 1, 1, 1)), w, b, padding=1) + r
    assert ops.overflow_events(DEV) == {} and rel_err(out, ref) < 2e-5
    s1, h1 = ops.groupnorm_affine(out, stats=st)
    s0, h0 = ops.groupnorm_affine(out)
    assert (s1 - s0).abs().max().item() <= 2e-6 * s0.abs().max().item() and (h1 - h0).abs().max().item() <= 2e-6
    xa = x.clone()
    xa[1, 7, 2, 5, 33] = 5000.0
    got, sg = ops.conv_igemm(xa.to(DEV), l2, relu_in=True, want_stats=True)
    assert list(ops.overflow_events(DEV).values()) == ["zs"]
    want = ops.torch.empty_like(got)             # (ops.torch: the guarded allocator of this module's tests)
    stw = ops.torch.empty_like(sg.stats)
    lib = hip.load()
    rc = lib.emo_conv_igemm_bf16x3(hip.ptr(xa.to(DEV)), hip.ptr(l2.packed(pack.CFG_D, "bf16x3")), hip.ptr(l2.bias), None, None, None,
                                   hip.ptr(want), N, Cin, Cout, D, H, W, 3, 3, 3, 0, 1, 0, 0, pack.CFG_D, 1, None, hip.ptr(stw),
                                   hip.current_stream(), None)
    hip.check(rc, "emo_conv_igemm_bf16x3")
    assert torch.equal(got.cpu(), want.cpu()) and torch.equal(sg.stats.cpu(), stw.cpu())
    ops.clear_overflow_flags(DEV)


def test_as_close_to_fp64_as_the_exact_fp32_kernel(monkeypatch):
    """mean error against an fp64 convolution on the first shape: at most 1.25 x (max: 2.0 x) the exact-fp32 MFMA kernel's on the
    same tensors, the project's bound for the split kernels; the one-slice kernel's figures are printed beside it"""
    g = torch.Generator().manual_seed(45)
    N, Cin, Cout, dims = 2, 64, 32, (3, 8, 64)
    x = torch.relu(torch.randn(N, Cin, *dims, generator=g) * 3 + 0.5)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(Cin * 27)
    ref = F.conv3d(x.double(), w.double(), padding=1)
    scale = ref.abs().mean().item()
    outs = {}
    for tag, prec, run in (("f32", "f32", None), ("one-slice", "f16x2", 0), ("depth-shared", "f16x2", RUN)):
        if run is not None:
            monkeypatch.setenv("EMO_CONV_ZS_RUN", str(run))
        layer = pack.PackedConv(tag, w, None, DEV, cfg=3, precision=prec)
        y = ops.conv_igemm(x.to(DEV), layer)
        assert layer.last_plan[2] == prec, layer.last_plan
        if run is not None:
            assert took(run)
        err = (y.cpu().double() - ref).abs()
        outs[tag] = (err.mean().item() / scale, err.max().item() / scale)
    new, old, f32 = outs["depth-shared"], outs["one-slice"], outs["f32"]
    print("PARITY conv vs fp64 [64->32 @(3,8,64)] (rel mean, rel max): fp32 MFMA %.2e %.2e | one-slice f16x2 %.2e %.2e | depth-shared "
          "f16x2 %.2e %.2e | depth-shared to fp32 MFMA: mean %.3f max %.3f" % (f32 + old + new + (new[0] / f32[0], new[1] / f32[1])))
    assert new[0] <= 1.25 * f32[0] + 1e-8 and new[1] <= 2.0 * f32[1] + 1e-7
