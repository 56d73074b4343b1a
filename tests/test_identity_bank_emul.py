"""The identity bank's two indexed kernels without a GPU: emo_grid_sample3d_indexed_f32 (csrc/grid_sample3d.hip) and
emo_add_rows_indexed_f32 (csrc/resample.hip), compiled for the host from the product's own sources (tests/emul/emulibs.py, as in
tests/test_direct_sampler_emul.py), against the existing entries run frame by frame -- bit for bit.

    default            the two entries: every layout, mode, padding and variant bit they serve; out-of-range indices; refusals
    EMO_EMUL_FULL=1    + a 2-identity bank through HotPath.driver_pass at the tiny_hotpath configuration (minutes)
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "emul"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
PAD = {"zeros": 0, "border": 1, "reflection": 2}
NCDHW, NDHWC, P4 = 0, 1, 3
TILE = 1 << 30
FULL = os.environ.get("EMO_EMUL_FULL") == "1"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")


@pytest.fixture(scope="module")
def sampler():
    import emulibs
    return emulibs.sampler()


@pytest.fixture(scope="module")
def stream():
    import emulibs
    return emulibs.stream(False)


def _aligned(n, dtype=np.float32, fill=np.nan):
    """16-byte aligned 1-D array of n elements"""
    raw = np.empty(n + 16, dtype)
    off = (-(raw.ctypes.data // raw.itemsize)) % (16 // raw.itemsize)
    out = raw[off:off + n]
    out[...] = fill
    assert out.ctypes.data % 16 == 0
    return out


def _buf(t):
    a = np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
    out = _aligned(a.size).reshape(a.shape)
    out[...] = a
    return out


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


GUARD = 4096      # NaN floats before and after the bank: a read outside it would show up in the output


def _bank(vols, in_layout):
    """[K,C,D,H,W] -> (guarded buffer, view of the bank inside it) in in_layout"""
    v = vols.permute(0, 2, 3, 4, 1) if in_layout == NDHWC else vols
    a = np.ascontiguousarray(v.numpy(), dtype=np.float32)
    whole = _aligned(2 * GUARD + a.size)
    whole[GUARD:GUARD + a.size] = a.reshape(-1)
    return whole, whole[GUARD:GUARD + a.size].reshape(a.shape)


def _coords(gen, N, D, H, W, mode):
    """(grid, theta, kind, out size) of a sampling mode: 'grid', 'theta' or 'delta'; outputs D x H x W"""
    if mode == "theta":
        a = torch.rand(N, generator=gen) - 0.5
        theta = torch.eye(4)[None].repeat(N, 1, 1)
        theta[:, 0, 0], theta[:, 0, 1], theta[:, 1, 0], theta[:, 1, 1] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a)
        theta[:, :3, 3] = 0.2 * torch.randn(N, 3, generator=gen)
        return None, _buf(theta[:, :3, :4]), 0
    if mode == "delta":
        return _buf(0.3 * torch.tanh(torch.randn(N, 3, D, H, W, generator=gen))), None, 1
    lin = [torch.linspace(-1, 1, n) for n in (D, H, W)]
    zz, yy, xx = torch.meshgrid(*lin, indexing="ij")
    g = torch.stack([xx, yy, zz], -1)[None] + 0.6 * torch.tanh(torch.randn(N, D, H, W, 3, generator=gen))
    return _buf(g), None, 0


def _lattice(D, H, W):
    return tuple(_buf(torch.linspace(-1, 1, n)) for n in (W, H, D))


def _frame(a, n):
    return None if a is None else _buf(a[n:n + 1])


CASES = [(NDHWC, NDHWC, 0), (NDHWC, NDHWC, 1), (NDHWC, NDHWC, 4), (NDHWC, NDHWC, 5),
         (NDHWC, NCDHW, 0), (NDHWC, NCDHW, 2), (NDHWC, NCDHW, 4), (NDHWC, NCDHW, 6),
         (NCDHW, NCDHW, 0), (NCDHW, NCDHW, 3)]


@pytest.mark.parametrize("pad", ["zeros", "border", "reflection"])
@pytest.mark.parametrize("mode", ["grid", "theta", "delta"])
def test_indexed_sampler_equals_the_plain_entry_frame_by_frame(sampler, pad, mode):
    """K = 3 volumes, N = 5 frames with repeated and unordered indices: every channels-last output (rows, 4x4x4 bricks, the FMA
    bit, non-temporal NCDHW stores) and the planar direct gather (channels per block 0 / 3) are bit for bit the plain entry on
    the frame's own volume"""
    gen = torch.Generator().manual_seed(PAD[pad] * 3 + ["grid", "theta", "delta"].index(mode))
    K, N, C, D, H, W = 3, 5, 8, 4, 4, 8
    index = np.array([2, 0, 2, 1, 0], np.int32)
    vols = torch.randn(K, C, D, H, W, generator=gen)
    grid, theta, kind = _coords(gen, N, D, H, W, mode)
    lx, ly, lz = _lattice(D, H, W)
    for il, ol, variant in CASES:
        _, bank = _bank(vols, il)
        shape = (N, D, H, W, C) if ol == NDHWC else (N, C, D, H, W)
        got = _aligned(int(np.prod(shape))).reshape(shape)
        rc = sampler.emo_grid_sample3d_indexed_f32(_p(bank), _p(index), K, _p(grid), _p(theta), _p(lx), _p(ly), _p(lz), _p(got),
                                                   N, C, D, H, W, D, H, W, PAD[pad], il, ol, variant, kind, None)
        assert rc == 0, (il, ol, variant, rc)
        for n in range(N):
            one = _buf(bank[index[n]][None])
            want = _aligned(int(np.prod(shape[1:]))).reshape((1,) + shape[1:])
            g1, t1 = _frame(grid, n), _frame(theta, n)          # (held: ctypes keeps no reference to the buffers)
            rc = sampler.emo_grid_sample3d_f32(_p(one), _p(g1), _p(t1), _p(lx), _p(ly), _p(lz), _p(want),
                                               1, C, D, H, W, D, H, W, ctypes.c_int64(C * D * H * W), PAD[pad], il, ol, variant, kind,
                                               None)
            assert rc == 0
            assert np.array_equal(got[n].view(np.uint32), want[0].view(np.uint32)), (il, ol, variant, n)


@pytest.mark.parametrize("il,ol,variant", CASES)
def test_out_of_range_indices_give_zero_frames_without_reading(sampler, il, ol, variant):
    """indices -1 and K: all-zero frames; the bank sits between NaN guards, so a stray read would leave a NaN in the output"""
    gen = torch.Generator().manual_seed(7)
    K, C, D, H, W = 2, 8, 4, 4, 8
    index = np.array([-1, 1, K, 0], np.int32)
    N = len(index)
    vols = torch.randn(K, C, D, H, W, generator=gen)
    whole, bank = _bank(vols, il)
    grid, theta, kind = _coords(gen, N, D, H, W, "delta")
    lx, ly, lz = _lattice(D, H, W)
    shape = (N, D, H, W, C) if ol == NDHWC else (N, C, D, H, W)
    got = _aligned(int(np.prod(shape))).reshape(shape)
    assert sampler.emo_grid_sample3d_indexed_f32(_p(bank), _p(index), K, _p(grid), None, _p(lx), _p(ly), _p(lz), _p(got), N, C, D,
                                                 H, W, D, H, W, PAD["zeros"], il, ol, variant, kind, None) == 0
    assert np.array_equal(got[0].view(np.uint32), np.zeros_like(got[0]).view(np.uint32))
    assert np.array_equal(got[2].view(np.uint32), np.zeros_like(got[2]).view(np.uint32))
    assert np.isfinite(got).all()
    assert np.isnan(whole[:GUARD]).all() and np.isnan(whole[-GUARD:]).all()


def test_refusals(sampler):
    C, D, H, W = 8, 4, 4, 8
    vol = _aligned(2 * C * D * H * W, fill=0.0)
    grid = _aligned(D * H * W * 3, fill=0.0)
    out = _aligned(C * D * H * W, fill=0.0)
    idx = np.zeros(1, np.int32)
    call = lambda index, k, il, ol, variant: sampler.emo_grid_sample3d_indexed_f32(
        _p(vol), index, k, _p(grid), None, None, None, None, _p(out), 1, C, D, H, W, D, H, W, 0, il, ol, variant, 0, None)
    assert call(_p(idx), 2, P4, NCDHW, 0) == -2                 # the LDS-staged tile kernels take no bank
    assert call(_p(idx), 2, NCDHW, NCDHW, TILE) == -2
    assert call(None, 2, NDHWC, NDHWC, 0) == -1                 # no index
    assert call(_p(idx), 0, NDHWC, NDHWC, 0) == -1              # empty bank
    assert call(_p(idx), -1, NDHWC, NDHWC, 0) == -1
    assert call(_p(idx), 2, NDHWC, NDHWC, 8) == -1              # the plain entry's own checks still apply (variant word)
    assert sampler.emo_grid_sample3d_indexed_f32(_p(vol), _p(idx), 2, None, None, None, None, None, _p(out), 1, C, D, H, W, D, H, W,
                                                 0, NDHWC, NDHWC, 0, 0, None) == -1   # neither grid nor theta
    assert call(_p(idx), 2, NDHWC, NDHWC, 0) == 0


def test_indexed_add_equals_the_period_form_row_by_row(stream):
    """emo_add_rows_indexed_f32 == emo_add_f32 per row with that row's table entry (the same roundings); an index outside
    [0, K) writes a zero row; all-equal indices equal the period form over the whole batch"""
    gen = torch.Generator().manual_seed(3)
    K, B, row = 3, 6, 1000
    table = _buf(torch.randn(K, row, generator=gen))
    a = _buf(torch.randn(B, row, generator=gen) * 7)
    for index, alpha in (([2, 0, 2, 1, 1, 0], 0.5), ([1, -1, 0, 3, 2, 2], 1.0), ([1] * B, 0.5)):
        index = np.array(index, np.int32)
        out = _aligned(B * row).reshape(B, row)
        assert stream.emo_add_rows_indexed_f32(_p(a), _p(table), _p(index), _p(out), B, K, ctypes.c_int64(row),
                                               ctypes.c_float(alpha), None) == 0
        for b in range(B):
            if 0 <= index[b] < K:
                want = _aligned(row)
                assert stream.emo_add_f32(_p(a[b]), _p(table[index[b]]), _p(want), ctypes.c_int64(row), ctypes.c_int64(row),
                                          ctypes.c_float(alpha), None) == 0
                assert np.array_equal(out[b].view(np.uint32), want.view(np.uint32)), b
            else:
                assert np.array_equal(out[b].view(np.uint32), np.zeros(row, np.uint32)), b
        if (index == index[0]).all():
            want = _aligned(B * row)
            assert stream.emo_add_f32(_p(a), _p(table[index[0]]), _p(want), ctypes.c_int64(B * row), ctypes.c_int64(row),
                                      ctypes.c_float(alpha), None) == 0
            assert np.array_equal(out.reshape(-1).view(np.uint32), want.view(np.uint32))
    out = _aligned(B * row)
    idx = np.zeros(B, np.int32)
    assert stream.emo_add_rows_indexed_f32(_p(a), _p(table), None, _p(out), B, K, ctypes.c_int64(row), ctypes.c_float(1), None) == -1
    assert stream.emo_add_rows_indexed_f32(_p(a), _p(table), _p(idx), _p(out), B, 0, ctypes.c_int64(row), ctypes.c_float(1), None) == -1


@pytest.mark.skipif(not FULL, reason="EMO_EMUL_FULL=1: two emulated driver passes (minutes)")
def test_two_identity_bank_through_the_driver_pass(monkeypatch):
    """HotPath.driver_pass at tiny_hotpath, B = 2, identity = [1, 0] over a 2-identity bank: each row bit for bit the row of the
    single-identity pass of its identity (the same launch plans: same B)"""
    import emulibs
    if not emulibs.available():
        pytest.skip("needs the built product library (weight packing asks it for tile sizes)")
    emulibs.install(monkeypatch.setattr)
    from emoportraits_amd import config, nets
    monkeypatch.delenv("EMO_CONV_PRECISION", raising=False)
    tiny = torch.load(os.path.join(HERE, "golden", "tiny_hotpath.pt"), weights_only=False)
    cfg = config.hot_path_config(overrides=tiny["cfg"])
    hp = nets.HotPath(tiny["state_dict"], cfg, "cpu")
    gen = torch.Generator().manual_seed(1)
    canon = [tiny["source"]["canonical"], tiny["source"]["canonical"].flip(-1).contiguous()]
    idt = [tiny["idt_embed"], (tiny["idt_embed"] + 0.1 * torch.randn(tiny["idt_embed"].shape, generator=gen)).contiguous()]
    pose, theta = tiny["target_pose_embed"][:2].contiguous(), tiny["theta_drv"][:2].contiguous()
    single = [hp.driver_pass(hp.prepare_canonical(canon[k]), idt[k], pose, theta) for k in range(2)]
    bank_cl = torch.cat([hp.prepare_canonical(c) for c in canon])
    identity = torch.tensor([1, 0], dtype=torch.int32)
    mixed = hp.driver_pass(bank_cl, torch.cat(idt), pose, theta, identity=identity)
    for b in range(2):
        k = int(identity[b])
        assert torch.equal(mixed[b].view(torch.int32), single[k][b].view(torch.int32)), b
