"""Every launch form of the pointwise and resampling ops, held to fp64 on the device.

The cases are tests/op_launch_forms.py's, read from the launchers of csrc/resample.hip, groupnorm.hip, smallops.hip and
embed_ops.hip: every kernel a launcher can select, every edge of its plan (runs, slices, a ragged last slice, the caps), and the
second trip of every capped grid-stride launch (`wrap`).  Each case runs the op through emoportraits_amd.ops on poisoned, guarded
outputs, passes the op's checker of tests/ops_reference.py with no failure, prints one PARITY line with its worst figure in
units of the checker's bound, and -- where the library can be asked (emo_op_launch_form, ABI 28) -- is the form and the plan it
is named for.  The last test holds the case lists to the forms of the C enums and to the plan edges.

The run_* functions take the device, so tests/test_op_launch_forms_emul.py runs the same cases on the host-compiled libraries.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import op_launch_forms as L
import ops_reference as R
from emoportraits_amd import hip, ops
from guarded_outputs import guarded_outputs  # noqa: F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, dev, decades=False):
    """normal values drawn on the CPU (the same on every device); decades: the channels' magnitudes run over 1e2 ... 1e-2, so a
    fault in a small channel is not hidden behind the tensor's maximum"""
    x = torch.randn(*shape, generator=_g(seed))
    if decades and len(shape) > 2 and shape[1] > 1:
        x = x * torch.tensor([10.0 ** (2 - (c % 5)) for c in range(shape[1])]).view((1, -1) + (1,) * (len(shape) - 2))
    return x.to(dev)


def parity(op, c, fig, extra=""):
    """the case's PARITY line; a case passes with no failure of its checker"""
    print(f"PARITY launch form {op} [{c['id']}]: worst {fig['worst']:.3g} {fig['unit']}{extra}")
    assert fig["failures"] == [], fig["failures"]
    return fig


def expect_form(op, c, x, out):
    """the library reports the form and the plan the case names, for the launch's own addresses"""
    rc, plan = hip.op_launch_form(op, x.data_ptr(), None if out is None else out.data_ptr(), L.form_dims(op, c))
    assert rc == 0 and plan["form"] == c["form"], (c["id"], rc, plan)
    got = {k: plan[k] for k in c["plan"]}
    assert got == c["plan"], (c["id"], plan)
    assert ("wrap" in L.plan_edges(op, plan)) == c["wrap"], (c["id"], plan)
    return plan


def nan_buffer(n, dev, dtype=torch.float32):
    """n elements of NaN from the allocator ops uses (guarded under the fixture)"""
    return ops.torch.empty(n, dtype=dtype, device=dev).fill_(float("nan"))


def refused(what, code):
    """ops raises with the entry point's name and the code it returned"""
    return pytest.raises(RuntimeError, match=what + " failed: " + {BAD_ARG: "EMO_ERR_BAD_ARG", UNSUPPORTED: "EMO_ERR_UNSUPPORTED"}[code])


# ---- upsample_trilinear --------------------------------------------------------------------------------------------------
def _upsample_into(x, factors, out):
    NC, (D, H, W) = x.shape[0] * x.shape[1], x.shape[2:]
    return hip.load().emo_upsample_trilinear_f32(hip.ptr(x), hip.ptr(out), NC, D, H, W, *factors, hip.current_stream())


def run_upsample(c, dev):
    x = _randn((1, c["nc"]) + tuple(c["dims"]), 101, dev, decades=True)
    factors = c["factors"]
    n_out = x.numel() * factors[0] * factors[1] * factors[2]
    if c.get("out_offset"):                                     # an aligned shape through an output 4 bytes off: the generic kernel
        buf = nan_buffer(n_out + 4, dev)
        out = buf[c["out_offset"]:c["out_offset"] + n_out]
        assert out.data_ptr() % 16 == 4 * c["out_offset"]
        assert _upsample_into(x, factors, out) == 0
        assert bool(torch.isnan(buf[:c["out_offset"]]).all()) and bool(torch.isnan(buf[c["out_offset"] + n_out:]).all()), "a store next to the output"
        out = out.view(1, c["nc"], *(d * f for d, f in zip(c["dims"], factors)))
        assert torch.equal(out, ops.upsample_trilinear(x, factors))                           # the block kernel's bits
    else:
        out = ops.upsample_trilinear(x, factors)
    plan = expect_form("upsample_trilinear", c, x, out)
    if c["form"] == "block":                                    # bit for bit the generic kernel (reached 4 bytes off)
        buf = nan_buffer(n_out + 4, dev)
        assert _upsample_into(x, factors, buf[1:1 + n_out]) == 0
        assert torch.equal(out.flatten(), buf[1:1 + n_out]), "block kernel and generic kernel differ"
        assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + n_out:]).all())
    parity("upsample_trilinear", c, R.check_upsample_trilinear(out, x, factors), f"; {plan}")
    return plan


def run_upsample_gn(c, dev):
    N, C, G = c["N"], c["C"], c["G"]
    x = (_randn((N, C) + tuple(c["dims"]), 102, dev) * 3.0 + 0.7)
    gamma, beta = _randn((C,), 103, dev), _randn((C,), 104, dev)
    plain = ops.upsample_trilinear(x, c["factors"])
    out, sums = ops.upsample_trilinear(x, c["factors"], gn_groups=G)
    plan = expect_form("upsample_trilinear_gn_sums", c, x, out)
    assert sums is not None and sums.split == plan["split"] and torch.equal(out, plain), "the fused call's tensor is not the plain call's"
    scale, shift = ops.groupnorm_affine(out, gamma, beta, groups=G, stats=sums)
    parity("upsample_trilinear gn_groups", c, R.check_upsample_trilinear(out, x, c["factors"]))
    parity("upsample_trilinear gn_groups -> groupnorm_affine", c, R.check_groupnorm_affine(scale, shift, out, gamma, beta, groups=G), f"; {plan}")
    return plan


@pytest.mark.parametrize("c", L.UPSAMPLE, ids=L.ids(L.UPSAMPLE))
def test_upsample_trilinear(c):
    run_upsample(c, DEV)


@pytest.mark.parametrize("c", L.UPSAMPLE_GN, ids=L.ids(L.UPSAMPLE_GN))
def test_upsample_trilinear_with_groupnorm_sums(c):
    run_upsample_gn(c, DEV)


# ---- avgpool -------------------------------------------------------------------------------------------------------------
def run_avgpool(c, dev):
    if "shape4" in c:
        x = _randn(c["shape4"], 111, dev, decades=True)
    elif c["wrap"]:
        x = _randn((c["nc"], 1) + tuple(c["dims"]), 111, dev)                                  # (a sample per volume: small fp64 frames)
    else:
        x = _randn((1, c["nc"]) + tuple(c["dims"]), 111, dev, decades=True)
    xin = x
    if c.get("x_offset"):                                       # a legal view 4 bytes off the allocation: the generic kernel
        buf = nan_buffer(x.numel() + 4, dev)
        xin = buf[c["x_offset"]:c["x_offset"] + x.numel()].view(x.shape)
        xin.copy_(x)
        assert xin.data_ptr() % 16 == 4 * c["x_offset"] and xin.is_contiguous()
    out = ops.avgpool(xin, c["kernel"])
    plan = expect_form("avgpool", c, xin, out)
    if c.get("x_offset"):
        aligned = ops.avgpool(x, c["kernel"])
        assert hip.op_launch_form("avgpool", x.data_ptr(), aligned.data_ptr(), L.form_dims("avgpool", c))[1]["form"] == "x4_w2"
        assert torch.equal(out, aligned), "generic kernel and x4 kernel differ"
    parity("avgpool", c, R.check_avgpool(out, x, c["kernel"]), f"; {plan}")
    return plan


def run_avgpool_refused(c, dev):
    D, H, W = c["dims"]
    kd, kh, kw = c["kernel"]
    x = _randn((1, c["nc"], D, H, W), 112, dev)
    out = nan_buffer(c["nc"] * D * H * W, dev)
    rc = hip.load().emo_avgpool_f32(hip.ptr(x), hip.ptr(out), c["nc"], D, H, W, kd, kh, kw, hip.current_stream())
    assert rc == UNSUPPORTED and bool(torch.isnan(out).all()), (c["id"], rc)
    assert hip.op_launch_form("avgpool", x.data_ptr(), out.data_ptr(), L.form_dims("avgpool", c)) == (UNSUPPORTED, None)
    with refused("emo_avgpool_f32", UNSUPPORTED):
        ops.avgpool(x, c["kernel"])


@pytest.mark.parametrize("c", L.AVGPOOL, ids=L.ids(L.AVGPOOL))
def test_avgpool(c):
    run_avgpool(c, DEV)


@pytest.mark.parametrize("c", L.AVGPOOL_REFUSED, ids=L.ids(L.AVGPOOL_REFUSED))
def test_avgpool_refuses_before_any_launch(c):
    run_avgpool_refused(c, DEV)


# ---- add / add_rows_indexed ----------------------------------------------------------------------------------------------
def run_add(c, dev):
    a, b = _randn(c["a"], 121, dev, decades=True), _randn(c["b"], 122, dev)
    out = ops.add(a, b, c["alpha"])
    assert (a.numel() > L.GRID_CAP) == c["wrap"]
    parity("add", c, R.check_add(out, a, b, c["alpha"]))


def run_add_rows(c, dev):
    B, K, row = len(c["index"]), c["K"], c["row"]
    a, table = _randn((B, row), 123, dev), _randn((K, row), 124, dev)
    index = torch.tensor(c["index"], dtype=torch.int32).to(dev)
    assert (row >= L.ADD_ROWS_STRIDED_FROM) == (c["form"] == "strided")
    out = ops.add_rows_indexed(a, table, index, c["alpha"])
    parity("add_rows_indexed", c, R.check_add_rows_indexed(out, a, table, index, c["alpha"]))
    for b, k in enumerate(c["index"]):
        if not 0 <= k < K:
            assert bool((out[b] == 0).all()), f"row {b} with index {k} is not zero"
    # rows whose indices are all equal: the `period` form with that table row, bit for bit
    for k in range(K):
        same = ops.add_rows_indexed(a, table, torch.full((B,), k, dtype=torch.int32).to(dev), c["alpha"])
        assert torch.equal(same, ops.add(a, table[k].contiguous(), c["alpha"])), f"equal indices {k}: not ops.add's bits"


def run_add_rows_refused(dev):
    a, table = torch.zeros(65536, 1).to(dev), torch.zeros(1, 1).to(dev)
    out = nan_buffer(65536, dev).view(65536, 1)
    with refused("emo_add_rows_indexed_f32", UNSUPPORTED):
        ops.add_rows_indexed(a, table, torch.zeros(65536, dtype=torch.int32).to(dev), out=out)
    assert bool(torch.isnan(out).all())
    ops.add_rows_indexed(a[:65535], table, torch.zeros(65535, dtype=torch.int32).to(dev), out=out[:65535])    # the largest batch runs
    assert bool((out[:65535] == 0).all()) and bool(torch.isnan(out[65535:]).all())


@pytest.mark.parametrize("c", L.ADD, ids=L.ids(L.ADD))
def test_add(c):
    run_add(c, DEV)


@pytest.mark.parametrize("c", L.ADD_ROWS, ids=L.ids(L.ADD_ROWS))
def test_add_rows_indexed(c):
    run_add_rows(c, DEV)


def test_add_rows_indexed_refuses_65536_rows():
    run_add_rows_refused(DEV)


# ---- groupnorm_affine ----------------------------------------------------------------------------------------------------
def run_groupnorm(c, dev):
    C = c["shape"][1]
    x = _randn(c["shape"], 131, dev) * 2.0 + 0.5
    gamma, beta = _randn((C,), 132, dev), _randn((C,), 133, dev)
    scale, shift = ops.groupnorm_affine(x, gamma, beta, groups=c["groups"])
    plan = expect_form("groupnorm_affine", c, x, None)
    parity("groupnorm_affine", c, R.check_groupnorm_affine(scale, shift, x, gamma, beta, groups=c["groups"]), f"; {plan}")
    return plan


@pytest.mark.parametrize("c", L.GROUPNORM, ids=L.ids(L.GROUPNORM))
def test_groupnorm_affine(c):
    run_groupnorm(c, DEV)


# ---- small_gemm / projector_finalize -------------------------------------------------------------------------------------
def run_small_gemm(c, dev):
    A, B = _randn((c["M"], c["K"]), 141, dev), _randn((c["batch"], c["K"], c["NN"]), 142, dev)
    out = ops.small_gemm(A, B, c["NN"])
    parity("small_gemm", c, R.check_small_gemm(out, A, B, c["NN"]))


def run_small_gemm_refused(dev):
    A = _randn((2, 5), 143, dev)
    with refused("emo_small_gemm_f32", UNSUPPORTED):
        ops.small_gemm(A, _randn((1, 5, 3), 144, dev), 3)
    with refused("emo_small_gemm_f32", UNSUPPORTED):
        ops.small_gemm(A[:1, :1].contiguous(), torch.zeros(65536, 1, 1).to(dev), 1)


def run_projector(c, dev):
    B, Rr, E = c["B"], c["R"], c["E"]
    T, V = _randn((B, Rr, E), 145, dev), _randn((3, E, 2), 146, dev)
    nor = torch.randint(0, 3, (Rr,), generator=_g(147), dtype=torch.int32)
    nor[0] = nor[-1] = c["edge"]
    nor = nor.to(dev)
    gamma, beta = _randn((Rr,), 148, dev), _randn((Rr,), 149, dev)
    ag, ab = ops.projector_finalize(T, V, nor, gamma, beta)
    parity("projector_finalize", c, R.check_projector_finalize(ag, ab, T, V, nor, gamma, beta))


@pytest.mark.parametrize("c", L.SMALL_GEMM, ids=L.ids(L.SMALL_GEMM))
def test_small_gemm(c):
    run_small_gemm(c, DEV)


def test_small_gemm_refuses_other_widths_and_65536_batches():
    run_small_gemm_refused(DEV)


@pytest.mark.parametrize("c", L.PROJECTOR, ids=L.ids(L.PROJECTOR))
def test_projector_finalize(c):
    run_projector(c, DEV)


# ---- mul_mask / stage2_compose -------------------------------------------------------------------------------------------
def run_compose(c, dev):
    N, C, H, W = c["shape"]
    img, add = torch.rand(N, C, H, W, generator=_g(151)).to(dev), 2.0 * _randn((N, C, H, W), 152, dev)   # add: both clamps act
    mask = torch.rand(N, 1, H, W, generator=_g(153)).to(dev)
    face = {"zeros": torch.zeros(N, 1, H, W), "ones": torch.ones(N, 1, H, W),
            "random": (torch.rand(N, 1, H, W, generator=_g(154)) > 0.3).float()}[c["face"]].to(dev)
    assert (img.numel() > L.GRID_CAP) == c["wrap"]
    parity("mul_mask", c, R.check_mul_mask(ops.mul_mask(img, mask), img, mask))
    out = ops.stage2_compose(img, add, mask, face)
    if c["face"] != "zeros" and img.numel() > 50:
        assert bool((out == 0).any()) and bool((out == 1).any()), "a clamp that never acts"
    parity("stage2_compose", c, R.check_stage2_compose(out, img, add, mask, face))


@pytest.mark.parametrize("c", L.COMPOSE, ids=L.ids(L.COMPOSE))
def test_mul_mask_and_stage2_compose(c):
    run_compose(c, DEV)


# ---- pack_rgb8 / unpack_rgb8 ---------------------------------------------------------------------------------------------
def run_rgb8(c, dev, unpack=None):
    unpack = unpack or ops.unpack_rgb8
    if c["image"] == "edges":
        img = R.rgb8_edge_image().to(dev)
        b = (torch.arange(4 * 193) % 256).to(torch.uint8)
        frames = torch.stack([b, b.flip(0), b.roll(50)], -1).reshape(1, 4, 193, 3)            # all 256 values in each channel
    else:
        N, _, H, W = c["image"]
        img = (torch.rand(*c["image"], generator=_g(161)) * 1.4 - 0.2).to(dev)
        frames = torch.randint(0, 256, (N, H, W, 3), generator=_g(162), dtype=torch.uint8)
    frames = frames.to(dev)
    assert (img.numel() // 3 > L.GRID_CAP) == c["wrap"] and (c["wrap"] or (img.shape[2] * img.shape[3]) % 256)
    assert frames.numel() == img.numel()
    packed = ops.pack_rgb8(img)
    parity("pack_rgb8", c, R.check_pack_rgb8(packed, img))
    unpacked = unpack(frames)
    parity("unpack_rgb8", c, R.check_unpack_rgb8(unpacked, frames))
    assert torch.equal(ops.pack_rgb8(unpacked), frames), "pack(unpack(b)) != b"


@pytest.mark.parametrize("c", L.RGB8, ids=L.ids(L.RGB8))
def test_pack_and_unpack_rgb8(c):
    run_rgb8(c, DEV)


# ---- resize2d ------------------------------------------------------------------------------------------------------------
def run_resize(c, dev):
    """`bicubic (1, 1) to (5, 3)` found that the cubic weights were less accurate than the yardstick allows: on a 1 x 1 plane
    all sixteen taps are the pixel p, an output is p (sum wx)(sum wy), and its error is that of the fp32 weight sums alone.  With
    the Horner steps of cubic1 / cubic2 rounded as a product and a sum each, the sums came to 1 + 4.8e-07 (t = 2/3) and
    1 + 3.6e-07 (t = 0.8): over 192 planes a mean error of 1.70e-07 against 1.25 x ATen's 9.40e-08 + floor = 1.67e-07 (with six
    planes the maximum missed instead: 7.15e-07 against 6.37e-07).  csrc/resample.hip now takes each step as one FMA:
    0.42 x the allowance."""
    window, clamp01 = c.get("window"), c.get("clamp01", False)
    N, C = c.get("batch", (2, 3))
    H, W = L.RESIZE_FRAME if window is not None else c["src"]
    x = torch.rand(N, C, H, W, generator=_g(171))
    if clamp01:
        x = x * 1.4 - 0.2                                       # values in [-0.2, 1.2]
    x = x.to(dev)
    out = ops.resize2d(x, c["dst"], c["mode"], window=window, clamp01=clamp01)
    assert (out.numel() > L.GRID_CAP) == c["wrap"]
    fig = parity("resize2d", c, R.check_resize2d(out, x, c["dst"], c["mode"], window, clamp01), "")
    if clamp01 and tuple(c["dst"]) != (window[3], window[2]):
        assert bool((out == 0).any()) and bool((out == 1).any()), "a clamp that never acts"
    if (window is None and tuple(c["src"]) == tuple(c["dst"])):
        assert torch.equal(out, x)                              # (the checker holds this too: 'exact_bad')
    return fig


@pytest.mark.parametrize("c", L.RESIZE, ids=L.ids(L.RESIZE))
def test_resize2d(c):
    run_resize(c, DEV)


# ---- maxpool2d / affine_add_relu / grid_sample2d -------------------------------------------------------------------------
def run_maxpool(c, dev):
    x = _randn(c["shape"], 181, dev, decades=True)
    N, C = c["shape"][:2]
    scale, shift = (_randn((N, C), 182, dev), _randn((N, C), 183, dev)) if c["affine"] else (None, None)
    out = ops.maxpool2d(x, c["k"], c["stride"], c["pad"], scale, shift, c["relu"])
    parity("maxpool2d", c, R.check_maxpool2d(out, x, c["k"], c["stride"], c["pad"], scale, shift, c["relu"]))


def run_affine_add(c, dev):
    N, C, S = 2, 3, c["S"]
    a = _randn((N, C, S), 184, dev, decades=True)
    sa, ta = (_randn((N, C), 185, dev), _randn((N, C), 186, dev)) if c["sa"] else (None, None)
    b = _randn((N, C, S), 187, dev, decades=True) if c["b"] else None
    sb, tb = (_randn((N, C), 188, dev), _randn((N, C), 189, dev)) if c["sb"] else (None, None)
    out = ops.affine_add_relu(a, sa, ta, b, sb, tb, c["relu"])
    parity("affine_add_relu", c, R.check_affine_add_relu(out, a, sa, ta, b, sb, tb, c["relu"]))


def run_affine_add_refused(dev):
    a, s = _randn((2, 3, 8), 190, dev), _randn((2, 3), 191, dev)
    with refused("emo_affine_add_relu_f32", BAD_ARG):
        ops.affine_add_relu(a, sb=s, tb=s)                      # the second operand's affine without a second operand


def run_grid_sample2d(c, dev):
    N, C, (H, W), (Ho, Wo) = c["N"], c["C"], c["src"], c["out"]
    img = _randn((N, C, H, W), 192, dev)
    if c["form"] == "grid":
        grid = (torch.rand(N, Ho, Wo, 2, generator=_g(193)) * 2.4 - 1.2).to(dev)              # some samples leave the image
        out, warp = ops.grid_sample2d(img, grid=grid, want_grid=True)
        parity("grid_sample2d", c, R.check_grid_sample2d(out, img, grid=grid, warp=warp))
    else:
        theta = (torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) + 0.2 * torch.randn(N, 2, 3, generator=_g(194))).to(dev)
        out, warp = ops.grid_sample2d(img, theta=theta, size=Ho, want_grid=True)
        parity("grid_sample2d", c, R.check_grid_sample2d(out, img, theta=theta, size=Ho, warp=warp))


def run_grid_sample2d_refused(dev):
    """theta= samples the square lattice of one linspace: Ho != Wo is refused before any launch (the C entry point; ops has no
    way to ask for it)"""
    img, theta, lin = _randn((1, 1, 4, 4), 195, dev), torch.eye(2, 3)[None].contiguous().to(dev), torch.linspace(-1, 1, 4).to(dev)
    out = nan_buffer(12, dev)
    rc = hip.load().emo_grid_sample2d_f32(hip.ptr(img), None, hip.ptr(theta), hip.ptr(lin), hip.ptr(out), None, 1, 1, 4, 4, 4, 3,
                                          hip.current_stream())
    assert rc == BAD_ARG and bool(torch.isnan(out).all())


def run_grid_sample2d_non_finite(dev):
    """a grid row [NaN, +Inf, -Inf (in y), 1e30, 0]: NaN exactly where ATen's CPU kernel gives NaN (the first three), equal
    elsewhere.  Where both are finite each is four exact products (weights 0, 1/4 or 1) and three rounded sums of at most
    max |img|: they differ by at most 6 u max |img|."""
    img = _randn((1, 1, 4, 6), 196, "cpu")
    grid = torch.zeros(1, 1, 5, 2)
    grid[0, 0, 0, 0], grid[0, 0, 1, 0], grid[0, 0, 2, 1], grid[0, 0, 3, 0] = float("nan"), float("inf"), float("-inf"), 1e30
    want = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    assert torch.isnan(want).flatten().tolist() == [True, True, True, False, False] and want[0, 0, 0, 3] == 0
    got = ops.grid_sample2d(img.to(dev), grid=grid.to(dev)).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (got, want)
    assert got[0, 0, 0, 3] == 0 and abs(float(got[0, 0, 0, 4] - want[0, 0, 0, 4])) <= 6 * R.U * float(img.abs().max()), (got, want)


@pytest.mark.parametrize("c", L.MAXPOOL, ids=L.ids(L.MAXPOOL))
def test_maxpool2d(c):
    run_maxpool(c, DEV)


@pytest.mark.parametrize("c", L.AFFINE_ADD, ids=L.ids(L.AFFINE_ADD))
def test_affine_add_relu(c):
    run_affine_add(c, DEV)


def test_affine_add_relu_refuses_an_affine_without_its_operand():
    run_affine_add_refused(DEV)


@pytest.mark.parametrize("c", L.GRID_SAMPLE2D, ids=L.ids(L.GRID_SAMPLE2D))
def test_grid_sample2d(c):
    run_grid_sample2d(c, DEV)


def test_grid_sample2d_refuses_theta_on_a_lattice_that_is_not_square():
    run_grid_sample2d_refused(DEV)


def test_grid_sample2d_non_finite_grid_values_as_aten():
    run_grid_sample2d_non_finite(DEV)


# ---- the lists against the C enums and the plan edges --------------------------------------------------------------------
def header_forms():
    """op -> the form names of include/emo_hip.h's EMO_<OP>_FORM_* enumerators, in the order of their values"""
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    forms = {}
    for op, prefix in (("upsample_trilinear", "UPSAMPLE"), ("avgpool", "AVGPOOL"), ("groupnorm_affine", "GROUPNORM")):
        found = re.findall(rf"EMO_{prefix}_FORM_([A-Z0-9_]+) = (\d+)", hdr)
        names = [n.lower() for n, v in sorted(found, key=lambda nv: int(nv[1])) if n != "COUNT"]
        assert names and dict(found)["COUNT"] == str(len(names)), (op, found)
        forms[op] = tuple(names)
    forms["upsample_trilinear_gn_sums"] = forms["upsample_trilinear"]
    return forms


def coverage(base=4096):
    """per op with a form entry point: every form of the C enum and every required plan edge has a case.  Asked for aligned
    addresses (and the case's own offsets): what decides a form besides the shape"""
    forms = header_forms()
    assert forms == {op: tuple(f) for op, f in hip.OP_FORMS.items()}, "hip.OP_FORMS out of step with include/emo_hip.h"
    seen = {}
    for op in hip.OPS:
        edges = set()
        for c in L.BY_OP[op]:
            x, out = base + 4 * c.get("x_offset", 0), base + 4 * c.get("out_offset", 0)
            rc, plan = hip.op_launch_form(op, x, out, L.form_dims(op, c))
            assert rc == 0 and plan["form"] == c["form"] and {k: plan[k] for k in c["plan"]} == c["plan"], (op, c["id"], rc, plan)
            e = L.plan_edges(op, plan)
            assert ("wrap" in e) == c["wrap"], (op, c["id"], plan)
            edges |= e
        want = L.REQUIRED_EDGES[op] | {"form " + f for f in forms[op] if not (op == "upsample_trilinear_gn_sums" and f == "generic")}
        assert want <= edges, f"{op}: no case for {sorted(want - edges)}"
        seen[op] = sorted(edges)
    # the ops without a form entry point: both grids of add_rows_indexed, every small_gemm instantiation and every pair of its
    # axes, a wrap case for every capped grid-stride launcher
    assert {c["form"] for c in L.ADD_ROWS} == {"blocks", "strided"}
    assert all((c["row"] >= L.ADD_ROWS_STRIDED_FROM) == (c["form"] == "strided") for c in L.ADD_ROWS)
    axes = L.SMALL_GEMM_AXES
    for p in axes:
        for q in axes:
            if p < q:
                pairs = {(c[p], c[q]) for c in L.SMALL_GEMM}
                assert pairs == {(u, v) for u in axes[p] for v in axes[q]}, f"small_gemm: pairs of ({p}, {q}) without a case"
    for op in ("add", "mul_mask", "stage2_compose", "pack_rgb8", "unpack_rgb8", "resize2d"):
        assert any(c["wrap"] for c in L.BY_OP[op]), f"{op}: no wrap case"
    assert {c["mode"] for c in L.RESIZE if c["wrap"]} == {"bilinear", "bicubic"}
    return seen


def test_cases_cover_every_form_and_every_plan_edge(guarded_outputs):
    guarded_outputs.may_serve_nothing("asks emo_op_launch_form about every case; nothing is launched")
    print("PARITY launch form coverage:", coverage())
