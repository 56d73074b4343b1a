"""The depth-shared 32-row kernel of 3x3x3 layers (csrc/conv_igemm_f16x2_zs.h: a work item marches through a run of output
slices, every staged input slice feeds the MFMAs of all three depth taps) on the CPU, from copies of the product's sources
through the C ABI (tests/emul/convlib.py): the same emo_conv_igemm_f16x2(..., cfg = F, KD = 3) calls and packed weights as the
one-slice kernel, against fp64 convolutions.

The launcher sends a launch to this kernel only when runs of at least six slices fill the chip; the volumes here are far smaller,
so the tests set the launcher's measurement switch EMO_CONV_ZS_RUN (runs of that many output slices whatever the size) and ask
the launcher -- emo_debug_conv_zs_last_run -- which kernel every launch took.  The rule itself is checked on its own below."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import convlib  # noqa: E402
from emoportraits_amd import pack  # noqa: E402
from test_conv_split_emul import ACT, CFG_D, CFG_F, Case, _bits, _buf, _p  # noqa: E402

pytestmark = pytest.mark.skipif(not convlib.available(), reason="needs ROCm clang++ and the built product library (weight packing asks it for tile sizes)")
RUN = 3      # forced run length: three live accumulator sets, and a seam wherever D > 3


@pytest.fixture(scope="module")
def lib():
    return convlib.build()


@pytest.fixture(autouse=True)
def forced_runs(monkeypatch):
    monkeypatch.setenv("EMO_CONV_ZS_RUN", str(RUN))


def seam_depth(lib, N, Cout, H, W):
    """the depth at which the launcher's run length leaves one slice for a second run"""
    for D in range(2, 66):
        if lib.emo_debug_conv_zs_run(N, Cout, D, H, W, 0) == D - 1:
            return D
    raise AssertionError("no depth with run length D - 1")


# (N, Cin, Cout, dims, Case keywords, launch keywords)
SHAPES = {
    "64->32 (3,8,64) affine relu res stats": (2, 64, 32, (3, 8, 64), dict(res=True), dict(stats=True)),
    "32->32 (1,4,64) kd = 1 only": (1, 32, 32, (1, 4, 64), dict(), dict()),
    "32->32 (2,4,64) kd pairs": (1, 32, 32, (2, 4, 64), dict(), dict()),
    "16->32 (5,4,64) no bias, one chunk": (1, 16, 32, (5, 4, 64), dict(bias=False), dict()),
    "24->24 (4,8,64) ragged chunk and tile": (2, 24, 24, (4, 8, 64), dict(), dict()),
    "32->32 (run+1,8,64) seam, chained items": (3, 32, 32, None, dict(), dict()),
    "32->3 (4,4,64) tanh: the warp head": (2, 32, 3, (4, 4, 64), dict(), dict(act="tanh")),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_depth_shared_kernel_against_fp64(lib, name):
    N, Cin, Cout, dims, ckw, lkw = SHAPES[name]
    if dims is None:
        dims = (seam_depth(lib, N, Cout, 8, 64), 8, 64)
        assert dims[0] == RUN + 1
    c = Case(N, Cin, Cout, dims, seed=len(name), **ckw)
    flag = _buf(np.zeros(4, np.int32))
    out, st = c.launch(lib, "f16x2", cfg=CFG_F, flag=flag, **lkw)
    assert lib.emo_debug_conv_zs_last_run() == min(RUN, dims[0]), "the launch did not take the depth-shared kernel"
    act = lkw.get("act", "none")
    e = c.err(out, act)
    print("PARITY conv f16x2 depth-shared (emulation):", name, f"{e:.2e}")
    assert e < 2e-5, e
    assert flag[0] == 0
    out2, st2 = c.launch(lib, "f16x2", cfg=CFG_F, **lkw)
    assert np.array_equal(_bits(out), _bits(out2)), "two launches on the same input differ"
    if st is not None:
        # one (mean, M2) entry per 4 x 64 tile of one output slice, recombined over the tiles against a direct reduction
        assert np.array_equal(_bits(st), _bits(st2))
        o = torch.from_numpy(out.copy()).double().view(N, Cout, -1)
        s = torch.from_numpy(st.copy()).double()
        assert s.shape[1] == dims[0] * dims[1] * dims[2] // 256
        tiles = o.view(N, Cout, -1, 256)
        assert (s[..., 0] - tiles.mean(-1).transpose(1, 2)).abs().max().item() < 1e-5
        mean = s[..., 0].mean(1)
        m2 = s[..., 1].sum(1) + 256 * ((s[..., 0] - mean[:, None]) ** 2).sum(1)
        assert (mean - o.mean(-1)).abs().max().item() < 1e-5
        assert (m2 - ((o - o.mean(-1, keepdim=True)) ** 2).sum(-1)).abs().max().item() < 1e-3 * m2.abs().max().item()


def test_the_one_slice_kernel_computes_the_same_layer(lib, monkeypatch):
    """EMO_CONV_ZS_RUN=0 keeps the launch on the one-slice kernel: same tolerances, and the two kernels agree to the order of an
    output's accumulation"""
    c = Case(2, 64, 32, (3, 8, 64), res=True, seed=3)
    new, _ = c.launch(lib, "f16x2", cfg=CFG_F)
    assert lib.emo_debug_conv_zs_last_run() == RUN
    monkeypatch.setenv("EMO_CONV_ZS_RUN", "0")
    old, _ = c.launch(lib, "f16x2", cfg=CFG_F)
    assert lib.emo_debug_conv_zs_last_run() == 0
    assert c.err(old) < 2e-5 and np.abs(new - old).max() < 2e-5 * max(1.0, np.abs(c.ref).max())


def test_range_check_and_guarded_exact_recomputation(lib):
    """an input pushed past the fp16 range raises the overflow word (same word, same meaning); the guarded bf16x3 launch behind it
    leaves the output bit-identical to a plain bf16x3 launch"""
    c = Case(1, 32, 32, (4, 4, 64), res=True, seed=11)
    c.x[0, 7, 2, 1, 33] = 5000.0                     # (the case's fp64 reference no longer applies: outputs are compared in bits)
    flag = _buf(np.zeros(4, np.int32))
    out, _ = c.launch(lib, "f16x2", cfg=CFG_F, flag=flag)
    assert lib.emo_debug_conv_zs_last_run() == RUN
    assert flag[0] == 1
    c.launch(lib, "bf16x3", run_if=flag, out=out)
    plain, _ = c.launch(lib, "bf16x3")
    assert np.array_equal(_bits(out), _bits(plain))
    calm = Case(1, 32, 32, (4, 4, 64), res=True, seed=12)
    flag = _buf(np.zeros(4, np.int32))
    out, _ = calm.launch(lib, "f16x2", cfg=CFG_F, flag=flag)
    assert flag[0] == 0 and calm.err(out) < 2e-5
    before = out.copy()
    calm.launch(lib, "bf16x3", run_if=flag, out=out)
    assert np.array_equal(_bits(out), _bits(before))


def test_as_close_to_fp64_as_the_exact_fp32_kernel(lib):
    """mean error against fp64 on the first shape: at most 1.25 x (max: 2.0 x) the exact-fp32 MFMA kernel's on the same tensors --
    the project's bound for the split kernels"""
    N, Cin, Cout, dims = 2, 64, 32, (3, 8, 64)
    c = Case(N, Cin, Cout, dims, res=True, seed=5)
    new, _ = c.launch(lib, "f16x2", cfg=CFG_F)
    assert lib.emo_debug_conv_zs_last_run() == RUN
    arr = lambda t: None if t is None else _buf(t)
    f32 = _buf(np.full(c.ref.shape, np.nan, np.float32))
    xa, wpk, ba, sc, sh, ra = _buf(c.x), _buf(pack.pack_weight(c.w, CFG_D)), arr(c.b), arr(c.scale), arr(c.shift), arr(c.r)
    rc = lib.emo_conv_igemm_f32(_p(xa), _p(wpk), _p(ba), _p(sc), _p(sh), _p(ra), _p(f32), N, Cin, Cout, dims[0], dims[1], dims[2],
                                3, 3, 3, 0, 1, ACT["none"], 0, CFG_D, 1, None, None, None)
    assert rc == 0, rc
    scale = np.abs(c.ref).mean()
    e_new, e_f32 = np.abs(new - c.ref) / scale, np.abs(f32 - c.ref) / scale
    print("PARITY conv vs fp64 [64->32 @(3,8,64) depth-shared, emulation] (rel mean, rel max): fp32 MFMA %.2e %.2e | f16x2 %.2e %.2e | "
          "ratios mean %.3f max %.3f" % (e_f32.mean(), e_f32.max(), e_new.mean(), e_new.max(), e_new.mean() / e_f32.mean(), e_new.max() / e_f32.max()))
    assert e_new.mean() <= 1.25 * e_f32.mean() + 1e-8 and e_new.max() <= 2.0 * e_f32.max() + 1e-7


def test_run_length_rule(lib, monkeypatch):
    """the launcher's choice from the item count: at 16 frames a whole-depth run is exactly one item per CU; one frame would leave
    most CUs idle with any run worth taking and stays on the one-slice kernel, as do 2-D layers' shapes and short volumes"""
    monkeypatch.delenv("EMO_CONV_ZS_RUN")
    run = lib.emo_debug_conv_zs_run
    assert run(16, 32, 32, 64, 64, 256) == 32 and run(16, 3, 16, 64, 64, 256) == 16
    assert run(1, 32, 32, 64, 64, 256) == 0
    assert run(16, 32, 4, 64, 64, 256) == 0 and run(16, 32, 32, 64, 32, 256) == 0
    assert run(4, 32, 32, 64, 64, 256) in range(6, 9)          # 64 (sample, tile) pairs: runs short enough for four items each
    for n in (2, 3, 5, 16, 40):
        r = run(n, 32, 32, 64, 64, 256)
        assert r == 0 or (6 <= r <= 32 and n * 16 * math.ceil(32 / 6) >= 256)
