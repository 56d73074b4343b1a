"""The phase kernel's 4-row item with ONE accumulator set (csrc/conv_inst_f16x2_up2.hip: a low-res region of 4 rows x 64 columns per
item, the three products of the fp16 split summed into one accumulator) on the CPU, from copies of the product's sources
(tests/emul/convlib.py, the harness of tests/test_conv_up2_emul.py):

1. the error of the single set on the kernel itself, at the decoder's longest accumulation (512 input channels), against fp64 and
   against the emulated fp32 MFMA kernel on the same inputs, under the project's bounds for the fp16 split (conv_reference.verdict);
2. ragged heights (2 and 6 low-res rows: the last item's rows 2, 3 lie outside the map): output, statistics, and guard bands
   around both buffers;
3. chained items against one item per block, bit for bit;
4. the overflow word from a value in rows 2, 3 of an item.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_reference as CR  # noqa: E402
from test_conv_split_emul import CFG_D, Case, _buf, _half_bits, _p, convlib, pack  # noqa: E402

pytestmark = pytest.mark.skipif(not convlib.available(), reason="needs ROCm clang++ and the built product library")
GUARD = 4096                                         # floats on either side of a guarded buffer
SENTINEL = np.float32(-7.25e30)


@pytest.fixture(scope="module")
def lib():
    return convlib.build()


def _guarded(shape):
    """-> (whole allocation, 16-byte aligned view of `shape` GUARD floats inside it); everything holds SENTINEL"""
    n = int(np.prod(shape))
    raw = np.empty(n + 2 * GUARD + 4, np.float32)
    off = (-(raw.ctypes.data // 4)) % 4
    raw[...] = SENTINEL
    return raw, raw[off + GUARD:off + GUARD + n].reshape(shape)


def _guards_intact(raw, view):
    lo = (view.ctypes.data - raw.ctypes.data) // 4
    return bool((raw[:lo] == SENTINEL).all() and (raw[lo + view.size:] == SENTINEL).all())


def _launch(lib, x, wflat, ws, b, sc, sh, cout, dims, relu_in=True, flag=None):
    """-> (out, statistics, their whole allocations): both buffers between guard bands"""
    N, cin = x.shape[:2]
    H, W = dims
    raw_o, out = _guarded((N, cout, 2 * H, 2 * W))
    raw_s, st = _guarded((N, 4 * H * W // 256, cout, 2))
    arr = lambda t: None if t is None else _buf(t)
    xa, wa, ba, sca, sha = _buf(x), _buf(_half_bits(wflat)), arr(b), arr(sc), arr(sh)
    rc = lib.emo_conv_igemm_f16x2(_p(xa), _p(wa), _p(ba), _p(sca), _p(sha), None, _p(out), N, cin, cout, 1, H, W,
                                  1, 3, 3, 1, int(relu_in), 0, 0, pack.CFG_F16X2_UP2, 1, None, _p(st), None,
                                  ctypes.c_float(pack.F16X2_IN_SCALE), ctypes.c_float(ws), _p(flag))
    assert rc == 0
    return out, st, (raw_o, raw_s)


def _launch_case(lib, c, flag=None):
    flat, ws = pack.pack_weight_f16x2_up2(c.w)
    return _launch(lib, c.x, flat, ws, c.b, c.scale, c.shift, c.Cout, (c.H, c.W), relu_in=c.relu_in, flag=flag)


def _check_stats(out, st, N, cout, dims):
    """(mean, M2) per 4 x 64 output tile and channel (the layout of block config D) against a direct reduction of the output"""
    H, W = dims
    o = torch.from_numpy(out.copy()).double()
    tiles = o.view(N, cout, H // 2, 4, W // 32, 64).permute(0, 2, 4, 1, 3, 5).reshape(N, -1, cout, 256)
    s = torch.from_numpy(st.copy()).double()
    assert torch.isfinite(s).all()
    assert (s[..., 0] - tiles.mean(-1)).abs().max().item() < 1e-5
    m2 = ((tiles - tiles.mean(-1, keepdim=True)) ** 2).sum(-1)
    assert (s[..., 1] - m2).abs().max().item() < 1e-4 * m2.abs().max().item()


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1. the single accumulator set --------------------------------------------------------------------------------------------
def test_single_accumulator_set_is_as_close_to_fp64_as_the_fp32_kernel(lib):
    """512 input channels (the decoder's longest phase accumulation: 2048 products of the leading term and 4096 cross products into
    one fp32 accumulator), one 64-channel tile, one 4 x 64 item.  Bounds: conv_reference.verdict for the fp16 split -- every frame
    max <= 2e-5 max|ref|, mean <= 1.25 x and max <= 2 x the fp32 MFMA kernel's error against fp64 (plus its additive terms)"""
    c = Case(1, 512, 64, (4, 64), ups=True, seed=512)
    flag = _buf(np.zeros(4, np.int32))
    out, _, raws = _launch_case(lib, c, flag=flag)
    assert flag[0] == 0
    # the yardstick: the exact-fp32 MFMA kernel (block config D) on the same operands
    f32 = _buf(np.full(c.ref.shape, np.nan, np.float32))
    xa, wa, ba, sca, sha = _buf(c.x), _buf(pack.pack_weight(c.w, CFG_D)), _buf(c.b), _buf(c.scale), _buf(c.shift)
    rc = lib.emo_conv_igemm_f32(_p(xa), _p(wa), _p(ba), _p(sca), _p(sha), None, _p(f32), 1, 512, 64, 1, 4, 64, 1, 3, 3, 1, 1, 0, 0,
                                CFG_D, 1, None, None, None)
    assert rc == 0
    ref = torch.from_numpy(c.ref)
    assert ref.dtype == torch.float64
    fig = CR.launch_errors(torch.from_numpy(out.copy()), [(0, ref[0])], yardstick=torch.from_numpy(f32.copy()))
    print(f"PARITY up2 rows4 one accumulator set (emulation) Cin=512 Cout=64 4x64: mean err {fig['mean_err']:.3e} = "
          f"{fig['mean_err'] / fig['f32_mean_err']:.3f} x fp32 kernel's {fig['f32_mean_err']:.3e}; max err {fig['max_err']:.3e} = "
          f"{fig['max_err'] / fig['f32_max_err']:.3f} x fp32 kernel's {fig['f32_max_err']:.3e}; frame max / max|ref| "
          f"{fig['frame_rel_max'][0]:.3e}")
    assert CR.verdict(fig, "f16x2") == []
    assert _guards_intact(raws[0], out)


# ---- 2. ragged height ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 64), (6, 64)])
@pytest.mark.parametrize("cin", [16, 40])
def test_ragged_height(lib, dims, cin):
    """a height of 2 or 6 low-res rows: the last (only) item of a column holds two rows of the map and two beyond it, which are
    staged as zeros and neither stored nor counted.  Every output row against fp64, every tile's statistics against a direct
    reduction, nothing written outside the two buffers"""
    c = Case(2, cin, 128, dims, ups=True, seed=cin + dims[0])
    flag = _buf(np.zeros(4, np.int32))
    out, st, (raw_o, raw_s) = _launch_case(lib, c, flag=flag)
    assert flag[0] == 0
    assert np.isfinite(out).all() and not (out == SENTINEL).any()
    ref_max = max(1.0, np.abs(c.ref).max())
    per_row = np.abs(out - c.ref).max(axis=(0, 1, 3)) / ref_max
    assert per_row.shape == (2 * dims[0],) and (per_row < 2e-5).all(), per_row
    assert not (st == SENTINEL).any()
    _check_stats(out, st, 2, 128, dims)
    assert _guards_intact(raw_o, out) and _guards_intact(raw_s, st)


# ---- 3. chained items against one item per block ------------------------------------------------------------------------------
# (cout, cin, N, low-res dims): items = N * tiles * cout / 64 on 8 blocks
CHAIN_CASES = [(320, 40, 3, (8, 64)),      # 5 channel tiles, 3 stages (ragged last), 30 items: chained inside a sample, full prologue across
               (128, 32, 2, (8, 128)),     # 2 stages: the shortest chain, 16 items, 2 per block
               (128, 16, 2, (8, 128))]     # 1 stage: nothing chains, 16 items, 2 per block through the full prologue


@pytest.mark.parametrize("cout,cin,N,dims", CHAIN_CASES)
def test_chained_items_are_one_item_per_block_bit_for_bit(lib, cout, cin, N, dims):
    c = Case(N, cin, cout, dims, ups=True, seed=cout + cin + 1)
    H, W = dims
    n_tiles = ((H + 3) // 4) * (W // 64)
    assert n_tiles <= 8                                                   # the reference launches: one item per block
    flat, ws = pack.pack_weight_f16x2_up2(c.w)
    per_tile = flat.view(cout // 64, -1)                                  # [channel tile] is the slowest index of the layout
    flag = _buf(np.zeros(4, np.int32))
    out, st, raws = _launch(lib, c.x, flat, ws, c.b, c.scale, c.shift, cout, dims, flag=flag)
    out1, st1 = np.empty_like(out), np.empty_like(st)
    for k in range(N):
        for t in range(cout // 64):
            o, s, _ = _launch(lib, c.x[k:k + 1], per_tile[t].contiguous(), ws, c.b[64 * t:64 * t + 64], c.scale[k:k + 1], c.shift[k:k + 1],
                              64, dims)
            out1[k, 64 * t:64 * t + 64] = o[0]
            st1[k, :, 64 * t:64 * t + 64] = s[0]
    assert flag[0] == 0
    assert c.err(out) < 2e-5 and c.err(out1) < 2e-5
    assert _same_bits(out, out1)
    assert _same_bits(st, st1)
    _check_stats(out, st, N, cout, dims)
    assert _guards_intact(raws[0], out) and _guards_intact(raws[1], st)


# ---- 4. range word ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [2, 3])
def test_overflow_word_from_rows_2_and_3_of_an_item(lib, row):
    """one staged input beyond the fp16 range in low-res row 2 resp. 3 of the (only) item raises the layer's overflow word"""
    c = Case(1, 16, 64, (4, 64), ups=True, affine=False, relu_in=False, seed=3)
    flag = _buf(np.zeros(4, np.int32))
    out, _, _ = _launch_case(lib, c, flag=flag)
    assert flag[0] == 0 and c.err(out) < 2e-5
    c.x[0, 5, row, 17] = 4096.0                                            # * in_scale 32 > 65504
    _launch_case(lib, c, flag=flag)
    assert flag[0] == 1
