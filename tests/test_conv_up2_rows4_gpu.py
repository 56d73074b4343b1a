"""The phase kernel's 4-row item with one accumulator set (csrc/conv_inst_f16x2_up2.hip) on the GPU: a ragged height (6 low-res
rows: the last item's rows 2, 3 lie outside the map), chained items across three samples, and the decoder's longest accumulation
(512 input channels) -- every case asserts that the phase kernel ran, and is held to fp64 frame by frame (conv_reference), its tile
statistics to a direct reduction; the 512-channel case also to the fp32 MFMA kernel's error.  A plain launch and a graph replay
give the same bits."""
import math

import pytest
import torch

import conv_reference as CR
from emoportraits_amd import ops, pack
from test_kernels_gpu import DEV

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]


def _case(N, Cin, Cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1
    sc = torch.rand(N, Cin, generator=g) + 0.5
    sh = torch.randn(N, Cin, generator=g) * 0.2
    layer = pack.PackedConv("up", w, b, DEV, precision="f16x2")
    return layer, w, b, x.to(DEV), sc.to(DEV), sh.to(DEV)


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 16, 128, 6, 64), (3, 40, 320, 8, 128), (1, 512, 64, 4, 64)])
def test_up2_rows4_against_fp64_and_statistics(N, Cin, Cout, H, W):
    layer, w, b, x, sc, sh = _case(N, Cin, Cout, H, W, seed=Cout + Cin + H)
    kw = dict(relu_in=True, ups=True, ksplit=1)
    out, st = ops.conv_igemm(x, layer, sc, sh, want_stats=True, **kw)
    assert layer.last_form == "up2" and layer.last_plan[2] == "f16x2"
    yard = None
    if Cin == 512:
        f32 = pack.PackedConv("f32", w, b, DEV, cfg=3, precision="f32")
        yard = ops.conv_igemm(x, f32, sc, sh, **kw)
        assert f32.last_plan[2] == "f32"
    fig = CR.check_launch(out, x, w, b, sc, sh, relu_in=True, ups=True, precision="f16x2" if yard is not None else "f32", yardstick=yard,
                          stats=st, groups=32)
    if yard is not None:
        print("PARITY up2 rows4 one accumulator set Cin=512 Cout=64 4x64 vs fp64: mean err %.3e = %.3f x fp32 MFMA's %.3e; max err %.3e = "
              "%.3f x fp32 MFMA's %.3e" % (fig["mean_err"], fig["mean_err"] / fig["f32_mean_err"], fig["f32_mean_err"],
                                           fig["max_err"], fig["max_err"] / fig["f32_max_err"], fig["f32_max_err"]))
    assert max(fig["frame_rel_max"]) < 2e-5
    assert fig["failures"] == [], fig["failures"]


def test_up2_rows4_launches_and_graph_replay_are_bit_identical():
    layer, w, b, x, sc, sh = _case(3, 40, 320, 8, 128, seed=5)
    a = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    b2 = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
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
    assert torch.equal(a.view(torch.int32), b2.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
