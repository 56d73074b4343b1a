"""The decoder's up-convolutions in the phase form (csrc/conv_inst_f16x2_up2.hip, emo_conv_igemm_f16x2 with cfg 7: conv3x3 of a nearest x2
upsample as four 2x2 convolutions of the low-res input) run on the CPU from copies of the product's sources (tests/emul/convlib.py)
against fp64 conv2d(up2(x)): channel-tile counts, a ragged input stage, chained persistent items across samples, GroupNorm affine
+ ReLU in, tile statistics, the overflow word, and the launch forms it leaves to the direct kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_conv_split_emul import Case, _buf, _half_bits, _p, convlib, pack  # noqa: E402

pytestmark = pytest.mark.skipif(not convlib.available(), reason="needs ROCm clang++ and the built product library")
EMO_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def lib():
    return convlib.build()


def _launch(lib, c, stats=False, flag=None):
    out = _buf(np.full(c.ref.shape, np.nan, np.float32))
    st = _buf(np.full((c.N, 4 * c.H * c.W // 256, c.Cout, 2), np.nan, np.float32)) if stats else None
    flat, ws = pack.pack_weight_f16x2_up2(c.w)
    wpk = _buf(_half_bits(flat))
    arr = lambda t: None if t is None else _buf(t)
    xa, ba, sc, sh = _buf(c.x), arr(c.b), arr(c.scale), arr(c.shift)
    rc = lib.emo_conv_igemm_f16x2(_p(xa), _p(wpk), _p(ba), _p(sc), _p(sh), None, _p(out), c.N, c.Cin, c.Cout, 1, c.H, c.W,
                                      1, 3, 3, 1, int(c.relu_in), 0, 0, pack.CFG_F16X2_UP2, 1, None, _p(st), None,
                                      ctypes.c_float(pack.F16X2_IN_SCALE), ctypes.c_float(ws), _p(flag))
    return rc, out, st


def test_phase_kernels_are_the_upsampled_convolution():
    """the packing's phase kernels, unpacked and applied as four 2x2 convolutions in fp64, are conv3x3(up2(x))"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 8, 5, 6, generator=g, dtype=torch.float64)
    w = torch.randn(64, 8, 3, 3, generator=g)
    flat, ws = pack.pack_weight_f16x2_up2(w)
    t = flat.view(1, 1, 2, 2, 2, 2, 2, 2, 64, 8).double()                # [cot][cc][p][q][a][b][plane][half][BM][8]
    ph = (t[0, 0, :, :, :, :, 0] + t[0, 0, :, :, :, :, 1]) / ws              # [p][q][a][b][half][BM][8]
    wpq = ph.permute(5, 4, 6, 0, 1, 2, 3).reshape(64, 16, 2, 2, 2, 2)[:, :8]   # [co][ci = 8 half + k8][p][q][a][b]
    ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), w.double(), padding=1)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    for p in range(2):
        for q in range(2):
            o = torch.nn.functional.conv2d(xp[:, :, p:p + 5 + 1, q:q + 6 + 1], wpq[:, :, p, q])
            assert (o - ref[:, :, p::2, q::2]).abs().max().item() < 1e-5


@pytest.mark.parametrize("cout,cin,N,dims", [(128, 16, 1, (2, 64)), (192, 40, 1, (2, 64)), (320, 16, 1, (2, 64)),
                                             (192, 24, 3, (4, 64)), (64, 16, 2, (2, 128))])
def test_up2_kernel_against_fp64(lib, cout, cin, N, dims):
    """3 and 5 channel tiles (no odd-last-tile launch), a ragged last 16-channel stage (40 / 24 input channels), and 18 items on
    eight persistent blocks: several items per block, crossing sample boundaries"""
    c = Case(N, cin, cout, dims, ups=True, seed=cout + cin)
    flag = _buf(np.zeros(4, np.int32))
    rc, out, _ = _launch(lib, c, flag=flag)
    assert rc == 0
    assert c.err(out) < 2e-5
    assert flag[0] == 0


def test_up2_plain_operands_without_bias(lib):
    c = Case(1, 16, 64, (2, 64), ups=True, affine=False, relu_in=False, bias=False, seed=7)
    rc, out, _ = _launch(lib, c)
    assert rc == 0 and c.err(out) < 2e-5


def test_up2_tile_statistics(lib):
    """(mean, M2) per 4 x 64 output tile and channel (the layout of block config D) against torch on the kernel's own output"""
    c = Case(2, 16, 128, (4, 64), ups=True, seed=11)
    rc, out, st = _launch(lib, c, stats=True)
    assert rc == 0 and c.err(out) < 2e-5
    o = torch.from_numpy(out.copy()).double()                               # [N, C, 8, 128]
    tiles = o.view(2, 128, 2, 4, 2, 64).permute(0, 2, 4, 1, 3, 5).reshape(2, 4, 128, 256)
    s = torch.from_numpy(st.copy()).double()
    assert (s[..., 0] - tiles.mean(-1)).abs().max().item() < 1e-5
    m2 = ((tiles - tiles.mean(-1, keepdim=True)) ** 2).sum(-1)
    assert (s[..., 1] - m2).abs().max().item() < 1e-4 * m2.abs().max().item()


def test_up2_overflow_word(lib):
    """one staged input beyond the fp16 range raises the layer's overflow word"""
    c = Case(1, 16, 64, (2, 64), ups=True, affine=False, relu_in=False, seed=3)
    c.x[0, 5, 1, 17] = 4096.0                                              # * in_scale 32 > 65504
    flag = _buf(np.zeros(4, np.int32))
    rc, _, _ = _launch(lib, c, flag=flag)
    assert rc == 0 and flag[0] == 1


def test_up2_leaves_other_launch_forms_to_the_direct_kernels(lib):
    """a 32-wide low-res map (and the other forms the kernel does not take) is refused by the C launcher and by the planner's question to it,
    pack.up2_launch_fits, so ops.conv_igemm runs the direct kernels there"""
    c = Case(1, 16, 64, (2, 32), ups=True, seed=5)
    rc, _, _ = _launch(lib, c)
    assert rc == EMO_ERR_UNSUPPORTED
    assert not pack.up2_launch_fits(64, 16, 1, 3, 3, 1, 2, 32, True)
    assert pack.up2_launch_fits(64, 16, 1, 3, 3, 1, 2, 64, True)
    assert not pack.up2_launch_fits(64, 16, 1, 3, 3, 1, 2, 64, False)
    assert not pack.up2_launch_fits(96, 16, 1, 3, 3, 1, 2, 64, True)
    assert not pack.up2_launch_fits(64, 16, 1, 3, 3, 1, 2, 64, True, res=True)
    assert not pack.up2_launch_fits(64, 16, 1, 3, 3, 1, 2, 64, True, act="tanh")
