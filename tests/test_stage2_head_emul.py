"""emo_stage2_head_f32 (csrc/conv_head.hip, ABI 16: the tail of stage 2 as one stream launch) without a GPU: the kernel is compiled
for the host from the product's own source (tests/emul/emulibs.py, the sequential build) and run on host memory.
  * bit for bit, fp32 planes and bytes, against the chain of the three entry points it replaces, from the same library:
    emo_conv_head_f32(act = tanh) -> emo_stage2_compose_f32 -> emo_pack_rgb8;
  * against a float64 evaluation of the formula: the fp32 output within 2e-5 * max(1, largest |pre-activation|) -- the bound
    test_stream_kernels_emul.py::test_conv_head_stream_kernel holds the sum to; tanh (slope <= 1) and a gate in [0, 1] do not
    amplify it -- and every byte within 1;
  * each refusal, and the header, hip.SIGNATURES and the ABI version agree.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "emul"))
import emulibs  # noqa: E402

ACT_TANH = 2
V, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    lib = emulibs.stream(False)
    assert hasattr(lib, "emo_stage2_head_f32"), "csrc/conv_head.hip does not export emo_stage2_head_f32"
    lib.emo_stage2_head_f32.argtypes = [V] * 10 + [I, I, I64, I, V]
    lib.emo_conv_head_f32.argtypes = [V] * 6 + [I, I, I, I64, I, I, V]
    lib.emo_stage2_compose_f32.argtypes = [V] * 5 + [I, I, I64, V]
    lib.emo_pack_rgb8.argtypes = [V, V, I, I, I, V]
    return lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _aligned(n, dtype=np.float32, offset_bytes=0):
    """buffer of n elements that starts offset_bytes behind a 16-byte aligned address"""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset_bytes
    out = raw[start:start + n * item].view(dtype)
    assert out.ctypes.data % 16 == offset_bytes % 16
    return out


def _put(values):
    buf = _aligned(values.size)
    buf[:] = np.asarray(values, np.float32).ravel()
    return buf


def operands(N, cin, S, affine, with_face, seed):
    """x, w, bias, scale, shift, img, mask, face: masks holding exact 0, exact 1 and fractions; img close enough to 0 and 1 (and
    the residual large enough) that img + add * gate leaves [0, 1] on both sides"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, S, generator=g)
    w = torch.randn(3, cin, generator=g) * (2.0 / math.sqrt(cin))
    b = torch.randn(3, generator=g) * 0.3
    scale = shift = None
    if affine:
        scale, shift = torch.rand(N, cin, generator=g) + 0.5, torch.randn(N, cin, generator=g) * 0.3
    img = torch.rand(N, 3, S, generator=g)
    img = torch.where(torch.rand(N, 3, S, generator=g) < 0.3, (img * 0.05).where(img < 0.5, 1 - img * 0.05), img)

    def mask():
        m = torch.rand(N, 1, S, generator=g)
        sel = torch.rand(N, 1, S, generator=g)
        return torch.where(sel < 0.25, torch.zeros(()), torch.where(sel < 0.5, torch.ones(()), m))
    return x, w, b, scale, shift, img, mask(), (mask() if with_face else None)


def run_fused(lib, ops_, N, cin, S, relu_in, want_f32, want_u8):
    x, w, b, scale, shift, img, mask, face = ops_
    out_f = _aligned(N * 3 * S) if want_f32 else None
    out_b = _aligned(N * S * 3, np.uint8) if want_u8 else None
    if out_f is not None:
        out_f[:] = np.nan
    rc = lib.emo_stage2_head_f32(_p(x), _p(w), _p(b), _p(scale), _p(shift), _p(img), _p(mask), _p(face), _p(out_f), _p(out_b), N, cin,
                                 S, int(relu_in), None)
    assert rc == 0
    return out_f, out_b


def run_chain(lib, ops_, N, cin, S, relu_in):
    x, w, b, scale, shift, img, mask, face = ops_
    add, out_f, out_b = _aligned(N * 3 * S), _aligned(N * 3 * S), _aligned(N * S * 3, np.uint8)
    if face is None:
        face = _put(np.ones(N * S, np.float32))
    assert lib.emo_conv_head_f32(_p(x), _p(w), _p(b), _p(scale), _p(shift), _p(add), N, cin, 3, S, int(relu_in), ACT_TANH, None) == 0
    assert lib.emo_stage2_compose_f32(_p(img), _p(add), _p(mask), _p(face), _p(out_f), N, 3, S, None) == 0
    assert lib.emo_pack_rgb8(_p(out_f), _p(out_b), N, 1, S, None) == 0
    return out_f, out_b


S_CASE = 4 * (256 + 37)          # more than one thread block per sample, the last one partly idle


@pytest.mark.parametrize("with_face", [False, True])
@pytest.mark.parametrize("relu_in", [0, 1])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("cin", [32, 20, 128])          # 20: the tail of the channel loop behind two unrolled groups of 8
def test_fused_tail_is_the_three_launch_chain_bit_for_bit_and_the_formula_in_fp64(lib, cin, N, affine, relu_in, with_face):
    S = S_CASE
    t = operands(N, cin, S, affine, with_face, seed=cin * 16 + N * 4 + affine * 2 + relu_in)
    x, w, b, scale, shift, img, mask, face = t
    bufs = tuple(None if v is None else _put(v.numpy()) for v in t)
    want_f, want_b = run_chain(lib, bufs, N, cin, S, relu_in)
    for want_f32, want_u8 in ((True, True), (True, False), (False, True)):      # both / f32 only / u8 only
        got_f, got_b = run_fused(lib, bufs, N, cin, S, relu_in, want_f32, want_u8)
        if want_f32:
            assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32))
        if want_u8:
            assert np.array_equal(got_b, want_b)
    # the formula in float64
    xin = x.double()
    if affine:
        xin = xin * scale.double()[:, :, None] + shift.double()[:, :, None]
    if relu_in:
        xin = xin.clamp(min=0)
    pre = torch.einsum("oc,ncp->nop", w.double(), xin) + b.double().view(1, 3, 1)
    gate = mask.double() * (1.0 if face is None else face.double())
    raw = img.double() + torch.tanh(pre) * gate
    assert (raw < 0).any() and (raw > 1).any(), "the inputs must drive img + add * gate below 0 and above 1"
    assert (gate == 0).any() and (gate == 1).any() and ((gate > 0) & (gate < 1)).any()
    ref = raw.clamp(0, 1)
    got_f, got_b = run_fused(lib, bufs, N, cin, S, relu_in, True, True)
    err = np.abs(got_f.reshape(N, 3, S).astype(np.float64) - ref.numpy()).max()
    bound = 2e-5 * max(1.0, pre.abs().max().item())
    print(f"cin={cin} N={N} affine={affine} relu_in={relu_in} face={with_face}: fp32 error {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    ref_b = (ref * 255.0).floor().permute(0, 2, 1).numpy()
    assert np.abs(got_b.reshape(N, S, 3).astype(np.int64) - ref_b.astype(np.int64)).max() <= 1


def test_nothing_is_written_outside_the_outputs(lib):
    """the byte run of the last thread of a sample ends where the next sample's begins; guard bytes around both outputs stay"""
    N, cin, S = 2, 8, 40
    t = operands(N, cin, S, True, True, seed=3)
    bufs = tuple(_put(v.numpy()) for v in t)
    raw_b = np.full(N * S * 3 + 32, 0xA5, np.uint8)
    start = (-raw_b.ctypes.data) % 4 + 4
    out_b = raw_b[start:start + N * S * 3]
    raw_f = _aligned(N * 3 * S + 8)
    raw_f[:] = 7.0
    out_f = raw_f[4:4 + N * 3 * S]
    rc = lib.emo_stage2_head_f32(*[_p(v) for v in bufs], _p(out_f), _p(out_b), N, cin, S, 1, None)
    assert rc == 0
    assert (raw_b[:start] == 0xA5).all() and (raw_b[start + N * S * 3:] == 0xA5).all()
    assert (raw_f[:4] == 7.0).all() and (raw_f[4 + N * 3 * S:] == 7.0).all()
    want_f, want_b = run_chain(lib, bufs, N, cin, S, 1)
    assert np.array_equal(out_b, want_b) and np.array_equal(out_f.view(np.uint32), want_f.view(np.uint32))


def test_refusals(lib):
    N, cin, S = 1, 16, 8
    x, w, img, mask = _aligned(cin * S + 4), _aligned(3 * cin), _aligned(3 * S + 4), _aligned(S + 4)
    of, ob = _aligned(3 * S + 4), _aligned(3 * S + 4, np.uint8)
    ob[:] = 0

    def call(x_=x, w_=w, sc=None, sh=None, img_=img, mask_=mask, face=None, of_=of, ob_=ob, N_=N, cin_=cin, S_=S):
        return lib.emo_stage2_head_f32(_p(x_), _p(w_), None, _p(sc), _p(sh), _p(img_), _p(mask_), _p(face), _p(of_), _p(ob_), N_, cin_,
                                       S_, 0, None)
    assert call() == 0
    assert call(S_=6) == -2                                       # not whole quads            EMO_ERR_UNSUPPORTED
    assert call(N_=65536) == -2                                   # more samples than grid.y
    assert call(x_=x[1:]) == -3                                   # alignment                  EMO_ERR_ALIGN
    assert call(img_=img[1:]) == -3
    assert call(mask_=mask[2:]) == -3
    assert call(face=mask[1:]) == -3
    assert call(of_=of[3:]) == -3
    assert call(ob_=ob[1:]) == -3 and call(ob_=ob[2:]) == -3
    assert call(ob_=ob[4:]) == 0                                  # bytes need 4-byte alignment only
    assert call(sc=w) == -1 and call(sh=w) == -1                  # scale without shift        EMO_ERR_BAD_ARG
    assert call(of_=None, ob_=None) == -1                         # no output at all
    assert call(x_=None) == -1 and call(w_=None) == -1 and call(img_=None) == -1 and call(mask_=None) == -1
    for bad in (dict(N_=0), dict(cin_=0), dict(S_=0), dict(N_=-1)):
        assert call(**bad) == -1


def test_stage2_head_is_in_the_abi_table():
    from emoportraits_amd import hip, _abi_version
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "int emo_stage2_head_f32(" in hdr and _abi_version.EMO_ABI_VERSION >= 16
    assert len(hip.SIGNATURES["emo_stage2_head_f32"]) == 15
    assert hip.SIGNATURES["emo_conv_head_f32"] == [V] * 6 + [I, I, I, I64, I, I, V]          # (its signature stays)
