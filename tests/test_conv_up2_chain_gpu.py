"""Chained items of the phase kernel on the GPU (csrc/conv_inst_f16x2_up2.hip, EMO_UP2_CHAIN).  The launches of
tests/test_conv_up2_gpu.py hold at most 160 items, one per persistent block; every launch here holds at least three items per
compute unit, so every block runs a full prologue and then chained ones (or, with one 16-channel stage, full ones again), and
blocks whose XCD range crosses a sample boundary go chained -> full prologue -> chained.  Every case asserts that the phase kernel
ran (PackedConv.last_form).  fp64 conv2d(up2(relu(affine(x)))) at the 2e-5 * max bound of tests/test_conv_up2_gpu.py, statistics
through ops.groupnorm_affine at its 2e-6 bounds, chained launches bitwise against one-item-per-block launches of the same samples,
the guarded bf16x3 recomputation behind an overflow raised inside a chained launch, launch / stream / graph-replay determinism."""
import math

import pytest
import torch
import torch.nn.functional as F

from emoportraits_amd import ops, pack
from test_kernels_gpu import DEV

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]


def _operands(N, Cin, Cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1
    sc = torch.rand(N, Cin, generator=g) + 0.5
    sh = torch.randn(N, Cin, generator=g) * 0.2
    return x, w, b, sc, sh


def _items(N, Cout, H, W):
    return N * (H // 2) * (W // 64) * (Cout // 64)


# N, Cin, Cout, low-res H, W -- 960 / 768 / 768 items
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(3, 40, 320, 64, 128),     # sample boundaries inside XCD ranges: chained -> full -> chained
                                            (2, 24, 128, 128, 192),    # 2 stages (the shortest chain), ragged stage, 3 tiles per row
                                            (1, 16, 192, 128, 256)])   # 1 stage: never chained, several full prologues per block
def test_up2_multi_item_blocks_against_fp64_and_statistics(N, Cin, Cout, H, W):
    assert _items(N, Cout, H, W) >= 3 * ops.device_cu_count()
    x, w, b, sc, sh = _operands(N, Cin, Cout, H, W, seed=Cout + Cin)
    xin = F.relu(x * sc[:, :, None, None] + sh[:, :, None, None]).double()
    ref = F.conv2d(F.interpolate(xin, scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    layer = pack.PackedConv("up", w, b, DEV, precision="f16x2")
    out, st = ops.conv_igemm(x.to(DEV), layer, sc.to(DEV), sh.to(DEV), relu_in=True, ups=True, want_stats=True, ksplit=1)
    assert layer.last_form == "up2" and layer.last_plan[2] == "f16x2"
    err = (out.cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("up2 chained N=%d %d->%d @%dx%d: max error / max(1, max|ref|) = %.3e" % (N, Cin, Cout, H, W, err))
    assert err < 2e-5
    s1, h1 = ops.groupnorm_affine(out, stats=st)
    s0, h0 = ops.groupnorm_affine(out)
    assert (s1 - s0).abs().max().item() <= 2e-6 * s0.abs().max().item() and (h1 - h0).abs().max().item() <= 2e-6


@pytest.fixture(scope="module")
def four_samples():
    """40 -> 192 @64x128: 192 items per sample.  (layer, operands on the device, the N = 1 launches of every sample: one item per
    block, the full prologue, no chain)"""
    N, Cin, Cout, H, W = 4, 40, 192, 64, 128
    assert _items(1, Cout, H, W) <= ops.device_cu_count() and _items(N, Cout, H, W) >= 3 * ops.device_cu_count()
    x, w, b, sc, sh = _operands(N, Cin, Cout, H, W, seed=17)
    layer = pack.PackedConv("up", w, b, DEV, precision="f16x2")
    x, sc, sh = x.to(DEV), sc.to(DEV), sh.to(DEV)
    singles = []
    for k in range(N):
        o, st = ops.conv_igemm(x[k:k + 1].contiguous(), layer, sc[k:k + 1].contiguous(), sh[k:k + 1].contiguous(), relu_in=True, ups=True, want_stats=True,
                               ksplit=1)      # (one sample: the planner would split K; the phase kernel does not)
        assert layer.last_form == "up2"
        singles.append((o.clone(), st.stats.clone()))
    return layer, x, sc, sh, singles


def test_up2_chained_items_equal_one_item_per_block_bitwise(four_samples):
    layer, x, sc, sh, singles = four_samples
    out, st = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True, want_stats=True)
    assert layer.last_form == "up2"
    for k, (o1, s1) in enumerate(singles):
        assert torch.equal(out[k].view(torch.int32), o1[0].view(torch.int32)), k
        assert torch.equal(st.stats[k].view(torch.int32), s1[0].view(torch.int32)), k


def test_up2_overflow_inside_a_chained_launch_recomputes_bit_identically_to_bf16x3(four_samples):
    layer, x, sc, sh, _ = four_samples
    x = x.clone()
    x[2, 7, 33, 70] = 1.0e5
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


def test_up2_chained_launches_stream_and_graph_replay_are_bit_identical(four_samples):
    layer, x, sc, sh, _ = four_samples
    a = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    b = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    assert layer.last_form == "up2"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        c = ops.conv_igemm(x, layer, sc, sh, relu_in=True, ups=True)
    gr.replay()
    torch.cuda.synchronize()
    for other in (b, c, d):
        assert torch.equal(a.view(torch.int32), other.view(torch.int32))
