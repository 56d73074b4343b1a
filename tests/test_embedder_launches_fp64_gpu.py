"""Every launch the embedders make, against fp64, on every frame.

emoportraits_amd/embedders.py runs IdtEmbed (a ResNet-50) on every enrolled source and HeadPoseRegressor / ExpressionEmbed (two
ResNet-18s) on every driver frame: 54 + 20 + 21 launches of conv2d_generic, and maxpool2d, affine_add_relu, grid_sample2d,
pose_theta, resize2d, the 2-D avgpool, groupnorm_affine on 4-D maps, small_gemm, add and mat4_inverse.  All of them are wrapped
with the OpLaunchChecker of test_op_launches_fp64_gpu.py while each embedder runs eagerly at its released shapes on
random_state_dict checkpoints; each launch is compared at once, sample by sample, with the fp64 reference of
tests/ops_reference.py under the bounds derived there.  A convolution is checked with the K split count the library's
heuristic chose for it (emo_conv2d_generic_splits, asked for the same shape), which no explicit test passes.

One PARITY line per pass: the worst figure per operation, the rms error of the convolutions, the samplers' error ratios to
ATen's fp32 CPU kernels, and the inventory.

The tests at the end run without a GPU: the split counts the heuristic gives the released trunks (a copy of splits_for over
trunk_plan), and the coverage guard over embedders.py, stage2.py and encoder.py.
"""
import os

import pytest
import torch

import ops_reference as R
from emoportraits_amd import embedders as E
from emoportraits_amd import encoder, hip, ops, stage2
from guarded_outputs import guarded_outputs  # noqa: F401  (every output ops allocates: poisoned, between guards; the GPU tests ask for it)
from test_op_launches_fp64_gpu import CONV_CHECKER, EXEMPT, OpLaunchChecker, ops_called, register

DEV = "cuda:0"

EMBEDDER_OPS = ("conv2d_generic", "maxpool2d", "affine_add_relu", "grid_sample2d", "pose_theta", "resize2d", "avgpool",
                "groupnorm_affine", "small_gemm", "add", "mat4_inverse")
register(EMBEDDER_OPS)
# calls of stage2.py / encoder.py, none of which runs under the checker here: the test that holds each one to its reference
HELD_ELSEWHERE = {
    "resize2d": "tests/test_op_launch_forms_gpu.py::test_resize2d (both modes, windows, clamp01, the wrap: check_resize2d)",
    "mul_mask": "tests/test_op_launch_forms_gpu.py::test_mul_mask_and_stage2_compose (check_mul_mask: the fp32 product's bits)",
    "stage2_compose": "tests/test_op_launch_forms_gpu.py::test_mul_mask_and_stage2_compose (check_stage2_compose: the derived bound, exact clamps)",
    "stage2_head": "tests/test_refine_gpu.py::test_stage2_head_kernel_is_the_three_launch_chain_bit_for_bit_at_the_real_shape",
    "pack_rgb8": "tests/test_op_launch_forms_gpu.py::test_pack_and_unpack_rgb8 (check_pack_rgb8: byte equality at every byte's edges)",
    "unpack_rgb8": "tests/test_op_launch_forms_gpu.py::test_pack_and_unpack_rgb8 (check_unpack_rgb8: the fp32 quotient's bits, all 256 bytes)",
}


# ---- the launches the trunks make, on the CPU ------------------------------------------------------------------------------
def splits_for(ncols, cout, K):
    """a copy of the launch heuristic of csrc/conv_generic.hip: >= 2 blocks per CU of 256, >= 4 K chunks per split, <= 32"""
    tiles = -(-ncols // 64) * -(-cout // 64)
    chunks = -(-K // R.GENERIC_KC)
    return max(1, min(-(-512 // tiles), chunks // 4, 32))


def trunk_convs(arch, px, B, head=None):
    """(N, Cin, H, W, Cout, k, stride, pad) of every conv2d_generic launch of ResNetTrunk on B crops of px x px (+ the 1x1 `fc`
    conv to `head` channels), from trunk_plan"""
    kind, exp, plan = E.trunk_plan(arch)
    convs = [(B, 3, px, px, 64, 7, 2, 3)]
    h = ((px + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1                                        # the stem, then the 3/2/1 max-pool
    for _, cin, planes, stride, down in plan:
        ho = (h + 2 - 3) // stride + 1
        if kind == "basic":
            convs += [(B, cin, h, h, planes, 3, stride, 1), (B, planes, ho, ho, planes, 3, 1, 1)]
        else:
            convs += [(B, cin, h, h, planes, 1, 1, 0), (B, planes, h, h, planes, 3, stride, 1), (B, planes, ho, ho, planes * 4, 1, 1, 0)]
        if down:
            convs.append((B, cin, h, h, planes * exp, 1, stride, 0))
        h = ho
    if head is not None:
        convs.append((B, 512 * exp, h, h, head, 1, 1, 0))
    return convs


def _launch_key(N, Cin, H, W, Cout, k, stride, pad):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return (Cin * k * k, N * Ho * Wo, Cout, splits_for(N * Ho * Wo, Cout, Cin * k * k))


def predicted(arch, px, B, head=None):
    """sorted (K, GEMM columns, Cout, split count) of every launch of the trunk"""
    return sorted(_launch_key(*c) for c in trunk_convs(arch, px, B, head))


def test_split_counts_of_the_released_trunks():
    """what the heuristic returns where it is used; none of these launches is made by a test that passes `splits`"""
    sets = lambda arch, px, B: {k[3] for k in predicted(arch, px, B)}
    assert sets("resnet18", 128, 1) == sets("resnet18", 128, 2) == {1, 2, 4, 9, 18, 32}
    assert sets("resnet50", 256, 1) == {1, 2, 4, 8, 9, 16, 18, 32}
    assert sets("resnet50", 256, 16) == {1, 2, 4}
    assert [len(trunk_convs(a, 128, 1, h)) for a, h in (("resnet50", 512), ("resnet18", None), ("resnet18", 128))] == [54, 20, 21]
    # ResNet-18 layer 1 at one frame: K = 576 = 18 chunks in 4 splits of 5, 5, 5 and 3; the stem's K = 147 ends in a 19-row chunk
    assert (576, 1024, 64, 4) in predicted("resnet18", 128, 1) and R.generic_splits_run(576, 4) == 4 and 18 % 5 == 3
    assert (147, 4096, 64, 1) in predicted("resnet18", 128, 1) and 147 % R.GENERIC_KC == 19


# ---- the checker -----------------------------------------------------------------------------------------------------------
class EmbedderLaunchChecker(OpLaunchChecker):
    """OpLaunchChecker over the operations embedders.py launches; keeps one record of integers per convolution"""
    wrapped = EMBEDDER_OPS
    title = "embedder launches"

    def __init__(self, tag):
        super().__init__(tag)
        self.convs = []

    def _check_conv2d_generic(self, a, out):
        x, cout, kh, kw, stride, pad = a["x"], a["cout"], a["kh"], a["kw"], a["stride"], a["pad"]
        N, Cin, H, W = x.shape
        asked = a["splits"]
        if asked is None:                    # what ops.conv2d_generic asked the library for this shape
            asked = hip.load().emo_conv2d_generic_splits(N, Cin, H, W, cout, kh, kw, stride, pad)
            assert asked >= 1, asked
        fig = R.check_conv2d_generic(out, x, a["wt"], cout, kh, kw, stride, pad, a["bias"], a["scale"], a["shift"], a["relu_in"], asked)
        K = Cin * kh * kw
        chunks = -(-K // R.GENERIC_KC)
        run, per = fig["splits_run"], -(-chunks // min(asked, chunks))
        self.convs.append(dict(N=N, K=K, cols=N * out.shape[2] * out.shape[3], cout=cout, splits=asked, run=run,
                               uneven=run > 1 and chunks % per != 0, ragged=K % R.GENERIC_KC != 0,
                               affine=a["scale"] is not None, relu=bool(a["relu_in"]), bias=a["bias"] is not None))
        return f"{kh}x{kw}/{stride} K={K} splits={asked}", tuple(x.shape[1:]), fig

    def _check_maxpool2d(self, a, out):
        form = f"{a['k']}/{a['stride']}/{a['pad']}" + (" scale" if a["scale"] is not None else "") + (" relu" if a["relu"] else "")
        return form, tuple(a["x"].shape[1:]), R.check_maxpool2d(out, a["x"], a["k"], a["stride"], a["pad"], a["scale"], a["shift"], a["relu"])

    def _check_affine_add_relu(self, a, out):
        form = "none" if a["b"] is None else "downsample affine" if a["sb"] is not None else "block input"
        return form, tuple(a["a"].shape[1:]), R.check_affine_add_relu(out, a["a"], a["sa"], a["ta"], a["b"], a["sb"], a["tb"], a["relu"])

    def _check_grid_sample2d(self, a, result):
        out, warp = result if a["want_grid"] else (result, None)
        form = ("theta" if a["theta"] is not None else "grid") + ("+warp" if warp is not None else "")
        return form, tuple(a["img"].shape[1:]), R.check_grid_sample2d(out, a["img"], a["grid"], a["theta"], a["size"], warp)

    def _check_resize2d(self, a, out):
        form = f"{a['mode']} -> {tuple(a['size'])}" + (" window" if a["window"] is not None else "") + (" clamp01" if a["clamp01"] else "")
        return form, tuple(a["x"].shape[1:]), R.check_resize2d(out, a["x"], a["size"], a["mode"], a["window"], a["clamp01"])

    def _check_pose_theta(self, a, out):
        return f"scale [{a['scale'].shape[1]}]", (4, 4), R.check_pose_theta(out, a["scale"], a["rotation"], a["translation"])


def _run(monkeypatch, tag, fn):
    chk = EmbedderLaunchChecker(tag)
    with monkeypatch.context() as mp:
        chk.install(mp)
        result = fn()
    torch.cuda.synchronize()
    inv = chk.report()
    chk.assert_clean()
    return chk, inv, result


def _assert_convs(chk, arch, px, B, head, count):
    """the launches are the trunk's, each with the split count the CPU table predicts for this batch"""
    seen = sorted((c["K"], c["cols"], c["cout"], c["splits"]) for c in chk.convs)
    assert len(seen) == count and seen == predicted(arch, px, B, head), (seen, predicted(arch, px, B, head))
    assert {c["splits"] for c in chk.convs} == {k[3] for k in predicted(arch, px, B, head)}
    assert any(c["ragged"] for c in chk.convs), "no launch with a ragged last K chunk"
    assert any(c["uneven"] for c in chk.convs), "no launch with an uneven last split"


def _crops(B, seed):
    return torch.rand(B, 3, 512, 512, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _thetas(B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda s: (s * torch.randn(B, 3, generator=g)).to(DEV)
    return ops.pose_theta(1 + r(0.1), r(0.3), r(0.1))


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_idt_embed_every_launch_vs_fp64(monkeypatch):
    """the ResNet-50 of an enrolment: released flags (GroupNorm + weight standardisation), 512 px crops, so the resize launches"""
    cfg = E.embedder_config()
    assert cfg["norm_layer_type"] == "gn" and cfg["use_ws"]
    net = E.IdtEmbed(E.random_state_dict(E.idt_schema(cfg), 11), cfg, torch.device(DEV))
    x = _crops(2, 12)
    chk, inv, out = _run(monkeypatch, "IdtEmbed resnet50 gn+ws B=2", lambda: net(x))
    assert tuple(out.shape) == (2, 512, 4, 4)
    _assert_convs(chk, "resnet50", 256, 2, 512, 54)
    assert chk.has("resize2d", "bilinear -> (256, 256)") and chk.has("maxpool2d", "3/2/1 scale relu"), inv
    assert chk.has("affine_add_relu", "downsample affine") and chk.has("affine_add_relu", "block input"), inv
    assert chk.has("groupnorm_affine", "pass", lambda s: len(s) == 3) and chk.has("avgpool", (2, 2)), inv
    assert any(c["bias"] and c["affine"] and c["relu"] for c in chk.convs) and any(not c["affine"] for c in chk.convs)


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_head_pose_regressor_every_launch_vs_fp64(monkeypatch):
    net = E.HeadPoseRegressor(E.random_state_dict(E.head_pose_schema(), 13), torch.device(DEV))
    x = _crops(3, 14)
    chk, inv, _ = _run(monkeypatch, "HeadPoseRegressor resnet18 bn B=3", lambda: net(x))
    _assert_convs(chk, "resnet18", 128, 3, None, 20)
    assert any(c["cols"] < 64 and c["N"] > 1 for c in chk.convs), "no tile that spans several frames"
    assert chk.has("resize2d", "bilinear -> (128, 128)") and chk.has("pose_theta", "scale [3]"), inv
    assert chk.has("avgpool", (4, 4)) and chk.has("small_gemm", "NN=1") and chk.has("add", "period 9"), inv
    assert not chk.has("groupnorm_affine"), inv


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
@pytest.mark.parametrize("released", [True, False])
def test_expression_embed_every_launch_vs_fp64(released, monkeypatch):
    """released: GroupNorm + weight standardisation, 128 expression channels; default: eval BatchNorm, 512 channels"""
    cfg = E.embedder_config(released=released)
    assert cfg["norm_layer_type"] == ("gn" if released else "bn")
    net = E.ExpressionEmbed(E.random_state_dict(E.expression_schema(cfg), 15), cfg, torch.device(DEV))
    x, theta = _crops(3, 16), _thetas(3, 17)
    chk, inv, _ = _run(monkeypatch, f"ExpressionEmbed resnet18 {'gn+ws' if released else 'bn'} B=3", lambda: net(x, theta))
    _assert_convs(chk, "resnet18", 128, 3, cfg["lpe_output_channels_expression"], 21)
    assert any(c["cols"] < 64 and c["N"] > 1 for c in chk.convs), "no tile that spans several frames"
    assert chk.has("grid_sample2d", "theta+warp", lambda s: s == (3, 512, 512)) and chk.has("mat4_inverse"), inv
    assert chk.has("maxpool2d", "3/2/1 scale relu") and chk.has("small_gemm", "NN=1"), inv
    assert chk.has("affine_add_relu", "downsample affine") and chk.has("affine_add_relu", "block input"), inv
    assert bool(chk.has("groupnorm_affine", "pass", lambda s: len(s) == 3)) == released, inv
    assert any(c["bias"] for c in chk.convs) == released


# ---- the guard (no GPU) ----------------------------------------------------------------------------------------------------
def test_every_ops_call_of_the_embedders_and_stage2_is_checked_or_exempt():
    """a launch added to embedders.py, stage2.py or encoder.py later cannot go unchecked without someone deciding so"""
    called = ops_called(E)
    assert {"conv2d_generic", "maxpool2d", "grid_sample2d", "pose_theta"} <= called, called   # (the pattern still finds the calls)
    unchecked = sorted(called - set(EMBEDDER_OPS))
    assert not unchecked, f"ops called by embedders.py that the launch checker does not wrap: {unchecked}"
    assert all(callable(getattr(EmbedderLaunchChecker, "_check_" + name, None)) and callable(getattr(ops, name)) for name in EMBEDDER_OPS)
    called = ops_called(stage2, encoder)
    assert {"conv_igemm", "stage2_head", "mul_mask"} <= called, called
    # (no pass over stage 2 or the encoder runs under EmbedderLaunchChecker: a name it wraps is no cover here)
    unchecked = sorted(called - set(CONV_CHECKER) - set(EXEMPT) - set(HELD_ELSEWHERE))
    assert not unchecked, f"ops called by stage2.py / encoder.py that no test is named for: {unchecked}"
    for reason in HELD_ELSEWHERE.values():                                                # the named tests exist
        path, name = reason.split(" ")[0].split("::")
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)) as f:
            assert f"def {name}(" in f.read(), reason
