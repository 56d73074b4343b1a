"""The fp64 conv reference and launch checker of tests/conv_reference.py, on the CPU: the reference equals the plain torch
composition of what ops.conv_igemm computes, and the checker fails each of the kernel faults it is there to catch."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_reference as R
from emoportraits_amd.ops import TileStats


def _torch_conv(x, w, b, scale, shift, relu_in, ups, res, res_ups, act):
    """the plain torch composition in fp32 (tests/test_kernels_gpu.py run_conv)"""
    v = x
    if scale is not None:
        bshape = scale.shape + (1,) * (x.dim() - 2)
        v = v * scale.view(bshape) + shift.view(bshape)
    if relu_in:
        v = F.relu(v)
    if ups:
        v = F.interpolate(v, scale_factor=(1, 2, 2) if x.dim() == 5 else 2, mode="nearest")
    conv = F.conv3d if x.dim() == 5 else F.conv2d
    y = conv(v, w, b, padding=tuple(k // 2 for k in w.shape[2:]))
    if res is not None:
        y = y + (F.interpolate(res, scale_factor=(1, 2, 2) if x.dim() == 5 else 2, mode="nearest") if res_ups else res)
    return {"none": y, "tanh": torch.tanh(y), "sigmoid": torch.sigmoid(y), "relu": F.relu(y)}[act]


CASES = [
    dict(dims=(8, 16), k=(3, 3)),
    dict(dims=(8, 16), k=(3, 3), affine=True, relu_in=True),
    dict(dims=(6, 8), k=(3, 3), affine=True, relu_in=True, ups=True),
    dict(dims=(8, 16), k=(3, 3), res=True, act="tanh"),
    dict(dims=(4, 8), k=(3, 3), ups=True, res=True, res_ups=True, act="sigmoid"),
    dict(dims=(8, 8), k=(1, 1), ups=True, act="relu", bias=False),
    dict(dims=(8, 16), k=(1, 1), res=True, res_ups=True),
    dict(dims=(4, 6, 8), k=(3, 3, 3), affine=True, relu_in=True, res=True),
    dict(dims=(4, 6, 8), k=(1, 1, 1), affine=True, relu_in=True, act="tanh"),
    dict(dims=(4, 6, 8), k=(3, 3, 3), ups=True),
    dict(dims=(16, 1, 16), k=(7, 1, 7), cin=3),              # the 7x7 stem on its [N, 3, H, 1, W] view
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_reference_equals_the_torch_composition(case, monkeypatch):
    g = torch.Generator().manual_seed(len(case["dims"]) * 100 + sum(case["dims"]))
    N, cin, cout = 2, case.get("cin", 12), 10
    dims, k = case["dims"], case["k"]
    x = torch.randn(N, cin, *dims, generator=g)
    w = torch.randn(cout, cin, *k, generator=g) / math.sqrt(cin * math.prod(k))
    b = torch.randn(cout, generator=g) if case.get("bias", True) else None
    scale = shift = res = None
    if case.get("affine"):
        scale, shift = torch.rand(N, cin, generator=g) + 0.5, torch.randn(N, cin, generator=g) * 0.3
    osp = list(dims)
    if case.get("ups"):
        osp[-2:] = [2 * osp[-2], 2 * osp[-1]]
    if case.get("res"):
        rsp = list(osp)
        if case.get("res_ups"):
            rsp[-2:] = [rsp[-2] // 2, rsp[-1] // 2]
        res = torch.randn(N, cout, *rsp, generator=g)
    flags = dict(relu_in=case.get("relu_in", False), ups=case.get("ups", False), res_ups=case.get("res_ups", False),
                 act=case.get("act", "none"))
    want = _torch_conv(x, w, b, scale, shift, res=res, **flags)
    got = R.reference(x, w, b, scale, shift, res=res, **flags)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want.double()).abs().max().item() <= 1e-5 * want.abs().max().item()
    # row blocks of the tap sum: one output row per block gives the same values
    monkeypatch.setattr(R, "CHUNK_ELEMS", 1)
    assert torch.allclose(R.reference(x, w, b, scale, shift, res=res, **flags), got, rtol=1e-13, atol=1e-13)


# ---- the checker catches what it is meant to catch --------------------------------------------------------------------------
N, CIN, COUT, H, W = 16, 32, 64, 8, 64          # two 16-channel input stages; a frame = two 4 x 64 position tiles
BP = 256


def _setup():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, CIN, H, W, generator=g)
    w = torch.randn(COUT, CIN, 3, 3, generator=g) / math.sqrt(CIN * 9)
    b = torch.randn(COUT, generator=g) * 0.3
    scale, shift = torch.rand(N, CIN, generator=g) + 0.5, torch.randn(N, CIN, generator=g) * 0.3
    ref = R.reference(x, w, b, scale, shift, relu_in=True)
    return g, (x, w, b, scale, shift), ref


def _fp32_like(ref, g):
    """the reference with the error of an fp32 convolution: accumulation noise of a few ulp of the typical value, then
    rounded to fp32"""
    noise = torch.randn(ref.shape, generator=g, dtype=torch.float64) * 3e-7 * ref.abs().mean()
    return (ref + noise).float()


def _tile_stats(out):
    """TileStats of `out` in the kernels' layout: (mean, centred sum of squares) of BP consecutive positions per channel"""
    v = out.double().reshape(N, COUT, -1, BP)
    m = v.mean(-1)
    m2 = ((v - m[..., None]) ** 2).sum(-1)
    return TileStats(torch.stack((m, m2), -1).permute(0, 2, 1, 3).float().contiguous(), BP)


def _check(out, inputs, yard, stats):
    x, w, b, scale, shift = inputs
    return R.check_launch(out, x, w, b, scale, shift, relu_in=True, precision="f16x2", yardstick=yard, stats=stats, groups=32,
                          affine=R.groupnorm_affine_fp64)


def test_checker_passes_an_fp32_accurate_output():
    g, inputs, ref = _setup()
    out, yard = _fp32_like(ref, g), _fp32_like(ref, g)
    fig = _check(out, inputs, yard, _tile_stats(out))
    assert fig["failures"] == [], fig["failures"]
    assert fig["frames"] == list(range(N)) and max(fig["frame_rel_max"]) < R.FP32_FRAME
    # the fp16-operand bounds and the plain fp32 bound pass it too
    x, w, b, scale, shift = inputs
    for prec in ("f32", "f16w8"):
        assert R.check_launch(out, x, w, b, scale, shift, relu_in=True, precision=prec)["failures"] == []


def _corrupt(kind, out, stats, inputs):
    x, w, b, scale, shift = inputs
    if kind == "tile":                       # one 4 x 64 position tile of frame 11, all 64 channels, scaled by (1 + 1e-4)
        out[11, :, 4:8, :] *= 1 + 1e-4
    elif kind == "stage":                    # frame 5 computed without input channels 16..31 (one 16-channel stage)
        w2 = w.clone()
        w2[:, 16:32] = 0
        out[5] = R.reference(x[5:6], w2, b, scale[5:6], shift[5:6], relu_in=True)[0].float()
    elif kind == "bias":                     # the bias left out on output channel 37, every frame
        out[:, 37] -= b[37]
    elif kind == "stats":                    # the mean of one tile (frame 3, tile 1, channel 9) off by 1 % of the channel's spread
        stats.stats[3, 1, 9, 0] += 0.01 * out[3, 9].std()
    return out, stats


@pytest.mark.parametrize("kind", ["tile", "stage", "bias", "stats"])
def test_checker_fails_a_corrupted_output(kind):
    g, inputs, ref = _setup()
    out, yard = _fp32_like(ref, g), _fp32_like(ref, g)
    stats = _tile_stats(out)
    out, stats = _corrupt(kind, out, stats, inputs)
    fig = _check(out, inputs, yard, stats)
    assert fig["failures"], f"the checker passed a corrupted output ({kind})"
    if kind == "tile":
        assert any(f.startswith("frame 11:") for f in fig["failures"]), fig["failures"]
        assert [n for n, r in zip(fig["frames"], fig["frame_rel_max"]) if r > R.FP32_FRAME] == [11]
    elif kind == "stage":
        assert any(f.startswith("frame 5:") for f in fig["failures"]), fig["failures"]
    elif kind == "stats":
        assert all(f.startswith("tile statistics") for f in fig["failures"]), fig["failures"]


def test_checker_rejects_a_split_launch_without_yardstick_and_an_unknown_plan():
    g, (x, w, b, scale, shift), ref = _setup()
    out = _fp32_like(ref, g)
    assert R.check_launch(out, x, w, b, scale, shift, relu_in=True, precision="f16x2")["failures"]
    assert R.check_launch(out, x, w, b, scale, shift, relu_in=True, precision="f8")["failures"]


def test_reference_is_fp64_even_from_fp32_inputs():
    g, (x, w, b, scale, shift), _ = _setup()
    for _, o in R.reference_frames(x[:2], w, b, scale[:2], shift[:2], relu_in=True):
        assert o.dtype == torch.float64
