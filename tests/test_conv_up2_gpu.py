"""The phase form of the decoder's up-convolutions on the GPU (csrc/conv_inst_f16x2_up2.hip, emo_conv_igemm_f16x2, cfg 7): every case
asserts that the phase kernel actually ran (PackedConv.last_form), and checks it against fp64 conv2d(up2(x)), the fp32 MFMA
kernel's error bounds, the guarded bf16x3 recomputation behind a raised overflow word, and launch / graph-replay determinism."""
import math

import pytest
import torch
import torch.nn.functional as F

from emoportraits_amd import ops, pack
from test_kernels_gpu import DEV

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]


def _case(N, Cin, Cout, H, W, seed, affine=True, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    sc = torch.rand(N, Cin, generator=g) + 0.5 if affine else None
    sh = torch.randn(N, Cin, generator=g) * 0.2 if affine else None
    xin = x if sc is None else x * sc[:, :, None, None] + sh[:, :, None, None]
    ref = F.conv2d(F.interpolate(F.relu(xin).double(), scale_factor=2, mode="nearest"), w.double(),
                   None if b is None else b.double(), padding=1)
    layer = pack.PackedConv("up", w, b, DEV, precision="f16x2")
    dev = lambda t: None if t is None else t.to(DEV)
    return layer, x.to(DEV), dev(sc), dev(sh), ref


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(1, 16, 128, 2, 64), (2, 40, 192, 8, 64), (3, 64, 320, 4, 128), (4, 192, 128, 16, 64)])
def test_up2_against_fp64_and_statistics(N, Cin, Cout, H, W):
    layer, x, sc, sh, ref = _case(N, Cin, Cout, H, W, seed=Cout + Cin)
    out, st = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True, want_stats=True)
    assert layer.last_form == "up2" and layer.last_plan[2] == "f16x2"
    o = out.cpu().double()
    assert (o - ref).abs().max().item() / max(1.0, ref.abs().max().item()) < 2e-5
    s1, h1 = ops.groupnorm_affine(out, stats=st)
    s0, h0 = ops.groupnorm_affine(out)
    assert (s1 - s0).abs().max().item() <= 2e-6 * s0.abs().max().item() and (h1 - h0).abs().max().item() <= 2e-6


def test_up2_32_wide_map_runs_the_direct_kernel():
    layer, x, sc, sh, ref = _case(1, 16, 64, 4, 32, seed=3)
    out = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    assert layer.last_form is None and layer.last_plan[2] == "f16x2"
    assert (out.cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item()) < 2e-5


def test_up2_is_as_close_to_fp64_as_the_fp32_kernel():
    """the bounds of test_conv_bf16x3_is_as_close_to_fp64_as_the_fp32_kernel on its upsampling shape, the phase form running"""
    g = torch.Generator().manual_seed(7)
    N, Cin, Cout = 1, 512, 320
    x = torch.relu(torch.randn(N, Cin, 64, 64, generator=g) * 3 + 0.5)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest").double(), w.double(), padding=1)
    scale = ref.abs().mean().item()
    outs = {}
    for prec in ("f32", "f16x2"):
        layer = pack.PackedConv(prec, w, None, DEV, cfg=3, precision=prec)
        y = ops.conv_igemm(x.to(DEV), layer, ups=True, ksplit=1)      # (one sample: the planner would split K; the phase kernel does not)
        assert layer.last_plan[2] == prec
        if prec == "f16x2":
            assert layer.last_form == "up2"
        err = (y.cpu().double() - ref).abs()
        outs[prec] = (err.mean().item() / scale, err.max().item() / scale)
    print("PARITY up2 vs fp64 (rel mean, rel max): fp32 MFMA %.2e %.2e | f16x2 up2 %.2e %.2e | ratio %.3f"
          % (outs["f32"] + outs["f16x2"] + (outs["f16x2"][0] / outs["f32"][0],)))
    assert outs["f16x2"][0] <= 1.25 * outs["f32"][0] + 1e-8 and outs["f16x2"][1] <= 2.0 * outs["f32"][1] + 1e-7


def test_up2_overflow_recomputes_bit_identically_to_bf16x3():
    layer, x, sc, sh, _ = _case(2, 48, 128, 8, 64, seed=31)
    x[1, 7, 3, 20] = 1.0e5
    pack.clear_overflow_flags(DEV)
    out, st = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True, want_stats=True)
    assert layer.last_form == "up2"
    torch.cuda.synchronize()
    assert pack.overflow_events(DEV)
    ref_layer = pack.PackedConv("ref", layer._weight, layer.bias.cpu(), DEV, precision="bf16x3")
    out3, st3 = ops.conv_igemm(x, ref_layer, sc, sh, relu_in=True, ups=True, want_stats=True, ksplit=1)
    assert torch.equal(out.view(torch.int32), out3.view(torch.int32))
    assert torch.equal(st.stats.view(torch.int32), st3.stats.view(torch.int32))
    pack.clear_overflow_flags(DEV)


def test_up2_launches_and_graph_replay_are_bit_identical():
    layer, x, sc, sh, _ = _case(2, 64, 192, 8, 64, seed=5)
    a = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    b = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    assert layer.last_form == "up2"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        c = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
