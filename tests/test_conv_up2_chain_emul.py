"""Chained items of the phase kernel (csrc/conv_inst_f16x2_up2.hip, EMO_UP2_CHAIN) on the CPU, from copies of the product's sources
(tests/emul/convlib.py: 8 persistent blocks, one per XCD range, so block b runs the items of its range one after the other).  A
block's next item is the next channel tile of the same position tile, then the next position tile, then the next sample: chained
inside a sample (when the layer has >= 2 stages), a full prologue across a sample boundary.

Every launch is checked against fp64 conv2d(up2(relu(affine(x)))) at the project's 2e-5 * max bound AND bitwise against launches
that run ONE item per block (one sample, one channel tile, at most 8 position tiles: the full prologue, no chain): the chain moves
where an item's first stage is fetched and where the epilogue image lives, never a product or the order of a sum."""
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


@pytest.fixture(scope="module")
def lib():
    return convlib.build()


def _launch(lib, x, wflat, ws, b, sc, sh, cout, dims, relu_in=True, flag=None):
    N, cin = x.shape[:2]
    H, W = dims
    out = _buf(np.full((N, cout, 2 * H, 2 * W), np.nan, np.float32))
    st = _buf(np.full((N, 4 * H * W // 256, cout, 2), np.nan, np.float32))
    xa, wa, ba, sca, sha = _buf(x), _buf(_half_bits(wflat)), _buf(b), _buf(sc), _buf(sh)
    rc = lib.emo_conv_igemm_f16x2(_p(xa), _p(wa), _p(ba), _p(sca), _p(sha), None, _p(out), N, cin, cout, 1, H, W,
                                  1, 3, 3, 1, int(relu_in), 0, 0, pack.CFG_F16X2_UP2, 1, None, _p(st), None,
                                  ctypes.c_float(pack.F16X2_IN_SCALE), ctypes.c_float(ws), _p(flag))
    assert rc == 0
    return out, st


def _both(lib, c, flag=None):
    """(chained launch of the whole case, the same assembled from one-item-per-block launches)"""
    H, W = c.H, c.W
    n_tiles = (H // 2) * (W // 64)
    assert n_tiles <= 8 and n_tiles * (c.Cout // 64) * c.N > 8        # reference: one item per block; the case: several
    flat, ws = pack.pack_weight_f16x2_up2(c.w)
    per_tile = flat.view(c.Cout // 64, -1)                             # [channel tile] is the slowest index of the layout
    out, st = _launch(lib, c.x, flat, ws, c.b, c.scale, c.shift, c.Cout, (H, W), flag=flag)
    out1, st1 = np.empty_like(out), np.empty_like(st)
    for k in range(c.N):
        for t in range(c.Cout // 64):
            o, s = _launch(lib, c.x[k:k + 1], per_tile[t].contiguous(), ws, c.b[64 * t:64 * t + 64], c.scale[k:k + 1], c.shift[k:k + 1], 64, (H, W))
            out1[k, 64 * t:64 * t + 64] = o[0]
            st1[k, :, 64 * t:64 * t + 64] = s[0]
    return out, st, out1, st1


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


# (cout, cin, N, low-res dims): items = N * tiles * cout / 64 on 8 blocks
CASES = [(320, 40, 3, (4, 64)),      # 5 channel tiles, 3 stages (ragged last): 30 items; block 2 runs items 8 .. 11 -- chained,
                                     # full prologue at the sample boundary 9 | 10, chained again
         (192, 32, 2, (4, 128)),     # 3 channel tiles, 2 stages: the shortest chain, 24 items, 3 per block
         (128, 16, 2, (8, 64))]      # 1 stage: never chained, 2 items per block through the full prologue


@pytest.mark.parametrize("cout,cin,N,dims", CASES)
def test_chained_items_against_fp64_and_one_item_per_block(lib, cout, cin, N, dims):
    c = Case(N, cin, cout, dims, ups=True, seed=cout + cin)
    flag = _buf(np.zeros(4, np.int32))
    out, st, out1, st1 = _both(lib, c, flag=flag)
    assert c.err(out) < 2e-5 and c.err(out1) < 2e-5
    assert flag[0] == 0
    assert _same_bits(out, out1)
    assert _same_bits(st, st1)
    # tile statistics of the chained launch: (mean, M2) per 4 x 64 output tile and channel against torch on the kernel's own output
    H, W = dims
    o = torch.from_numpy(out.copy()).double()
    tiles = o.view(N, cout, H // 2, 4, W // 32, 64).permute(0, 2, 4, 1, 3, 5).reshape(N, -1, cout, 256)
    s = torch.from_numpy(st.copy()).double()
    assert (s[..., 0] - tiles.mean(-1)).abs().max().item() < 1e-5
    m2 = ((tiles - tiles.mean(-1, keepdim=True)) ** 2).sum(-1)
    assert (s[..., 1] - m2).abs().max().item() < 1e-4 * m2.abs().max().item()


def test_overflow_word_raised_inside_a_chained_item(lib):
    """One staged input beyond the fp16 range that ONLY chained-in items read.  3 channel tiles x 12 position tiles in one tile row =
    36 items, XCD ranges 0-4, 5-9, ...: block 1 starts with item 5 (tile 1, last channel tile: the full prologue) and runs items 6, 7,
    8 = the three channel tiles of position tile 2 behind it, each staged by its predecessor's look-ahead.  The value lies in low-res
    row 0 (no tile row above reads it), 30 columns inside tile 2 (no neighbour's halo), input channel 21 (stage 1: loaded by the
    predecessor's LAST stage)"""
    c = Case(1, 40, 192, (2, 768), ups=True, seed=3)
    flat, ws = pack.pack_weight_f16x2_up2(c.w)
    flag = _buf(np.zeros(4, np.int32))
    out, _ = _launch(lib, c.x, flat, ws, c.b, c.scale, c.shift, 192, (2, 768), flag=flag)
    assert flag[0] == 0 and c.err(out) < 2e-5
    c.x[0, 21, 0, 2 * 64 + 30] = 1.0e5
    _launch(lib, c.x, flat, ws, c.b, c.scale, c.shift, 192, (2, 768), flag=flag)
    assert flag[0] == 1
