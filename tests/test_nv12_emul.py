"""The NV12 entry points (csrc/resample.hip, ABI 17: emo_nv12_windows_f32, emo_pack_nv12, emo_paste_windows_nv12) without a GPU:
the kernels are compiled for the host from the product's own source (tests/emul/emulibs.py, the sequential build) and run on host
memory, every surface between guard bytes and, where a case says so, with a row pitch larger than the width.
  * against the definitions restated in torch and evaluated in fp64 (tests/nv12_reference.py): D within 1e-6, C within 1e-5; E and
    P every byte within 1 and at most 2e-3 of the touched bytes different at all, torch's own fp32 evaluation of the restatement
    held to the same caps as the premise;
  * exact cases: the fused crop is the whole-frame conversion followed by emo_resize2d_windows_f32; device and host window tables
    agree; a frame does not depend on its batch; achromatic frames survive pack(D(.)); a paste with side == S, even origin and no
    feather writes emo_pack_nv12's bytes; a zero matte changes nothing and a matte of ones is no matte; no byte outside the
    touched rectangles, in the guards or beside the rows changes;
  * refusals, with nothing written;
  * ops.*, InferenceWrapper.paste_back / animate_frames(frame_format='nv12') on CPU tensors, the package pointed at the
    host-compiled library inside the test only, calls counted.
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
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
from counting_lib import CountingLib as _Lib  # noqa: E402
import emulibs  # noqa: E402
import nv12_reference as R  # noqa: E402
import yuv420_reference as Y  # noqa: E402

FILL = Y.FILL
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def lib():
    from emoportraits_amd import hip
    lib = emulibs.stream(False)
    for name in ("emo_nv12_windows_f32", "emo_pack_nv12", "emo_paste_windows_nv12", "emo_resize2d_windows_f32"):
        assert hasattr(lib, name), f"csrc/resample.hip does not export {name}"
        getattr(lib, name).argtypes = hip.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def small():
    return R.small_inputs()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _np(t):
    return None if t is None else np.ascontiguousarray(t.numpy())


def _w4(wins):
    return np.ascontiguousarray([(w[0], w[1], w[2], w[3] if len(w) > 3 else w[2]) for w in wins], dtype=np.int32)


class Surface(Y.Surface):
    """N NV12 frames [rows, W] in one buffer (yuv420_reference.Surface, layout nv12, host memory): GUARD bytes in front and behind,
    rows `pitch` apart, all padding = FILL"""

    def __init__(self, n, rows, w, pitch=None, frames=None):
        super().__init__(Y.HostMemory(), "nv12", n, rows // 3 * 2, w, pad=(pitch or w) - w, arr=None if frames is None else frames.numpy())

    def args(self):
        y, uv, _, pitch, _, fstride = super().args()
        return y, uv, pitch, fstride

    def frames(self):
        return torch.from_numpy(self.read()[0])

    def padding_intact(self):
        return self.read()[1]


def nv12_windows(lib, nv12, wins, size, mode, host_windows=True, pitch=None):
    """emo_nv12_windows_f32 -> (return code, fp32 [N,3,Ho,Wo]); wins None = whole frames"""
    n, rows, w = nv12.shape
    s = Surface(n, rows, w, pitch, nv12)
    out = np.full((n, 3) + tuple(size), np.float32(-7.0))
    w4 = None if wins is None else _w4(wins)
    y, uv, p, fs = s.args()
    rc = lib.emo_nv12_windows_f32(y, uv, p, fs, s.h, w, _p(w4), _p(w4) if host_windows else None, _p(out), n, size[0], size[1],
                                  R.MATRIX_ID[mode[0]], int(mode[1]), None)
    assert s.padding_intact() and torch.equal(s.frames(), nv12)
    return rc, torch.from_numpy(out)


def pack(lib, img, mode, pitch=None):
    n, _, h, w = img.shape
    s = Surface(n, 3 * h // 2, w, pitch)
    im = _np(img)
    y, uv, p, fs = s.args()
    rc = lib.emo_pack_nv12(_p(im), y, uv, p, fs, n, h, w, R.MATRIX_ID[mode[0]], int(mode[1]), None)
    assert s.padding_intact()
    return rc, s.frames()


def paste(lib, nv12, img, wins, feather=0.0, matte=None, mode=R.MODES[0], host_windows=True, pitch=None):
    """emo_paste_windows_nv12 on a copy -> (return code, uint8 [N, 3Hf/2, Wf])"""
    n, rows, w = nv12.shape
    s = Surface(n, rows, w, pitch, nv12)
    w4 = _w4(wins)
    im, mt = _np(img), _np(matte)
    y, uv, p, fs = s.args()
    rc = lib.emo_paste_windows_nv12(_p(im), _p(mt), _p(w4), _p(w4) if host_windows else None, y, uv, p, fs, n, img.shape[-1], s.h, w,
                                    feather, R.MATRIX_ID[mode[0]], int(mode[1]), None)
    assert s.padding_intact()
    return rc, s.frames()


def untouched_equal(got, nv12, wins):
    keep = ~R.touched_mask(nv12.shape, wins)
    return torch.equal(got[keep], nv12[keep])


# ---- D and C -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_decode_against_the_fp64_restatement(lib, small, kind, mode):
    nv12 = small[kind][0]
    rc, got = nv12_windows(lib, nv12, None, (R.H, R.W), mode, pitch=R.W + 32 if kind == "noise" else None)
    assert rc == 0
    ref = R.decode(nv12, *mode, F64)
    err, err32 = (got.double() - ref).abs().max().item(), (R.decode(nv12, *mode, F32).double() - ref).abs().max().item()
    print(f"PARITY nv12 D {kind} {mode[0]} full_range {mode[1]}: max abs err {err:.2e} (torch fp32 against fp64: {err32:.2e})")
    assert err32 <= R.D_TOL
    assert err <= R.D_TOL
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_crop_against_the_fp64_restatement(lib, small, kind, which):
    nv12 = small[kind][0]
    wins = (R.WINDOWS, R.WINDOWS_ODD)[which]
    for mode in R.MODES[which::2]:
        rc, got = nv12_windows(lib, nv12, wins, (R.S, R.S), mode)
        assert rc == 0
        ref = R.crop(nv12, wins, R.S, *mode, F64)
        err, err32 = (got.double() - ref).abs().max().item(), (R.crop(nv12, wins, R.S, *mode, F32).double() - ref).abs().max().item()
        print(f"PARITY nv12 C {kind} windows {which} {mode[0]} full_range {mode[1]}: max abs err {err:.2e} "
              f"(torch fp32 against fp64: {err32:.2e})")
        assert err32 <= R.C_TOL
        assert err <= R.C_TOL


@pytest.mark.parametrize("which", [0, 1])
def test_the_fused_crop_is_conversion_then_resize_windows_bit_for_bit(lib, small, which):
    nv12 = small["noise"][0]
    wins = (R.WINDOWS, R.WINDOWS_ODD)[which]
    mode = R.MODES[which + 1]
    rc, rgb = nv12_windows(lib, nv12, None, (R.H, R.W), mode)
    assert rc == 0
    x, w4 = _np(rgb), _w4(wins)
    want = np.zeros((R.N, 3, R.S, R.S), np.float32)
    assert lib.emo_resize2d_windows_f32(_p(x), R.H * R.W, R.W, _p(w4), _p(want), R.N, 3, R.S, R.S, 1, 1, None) == 0
    want = torch.from_numpy(want)
    rc, got = nv12_windows(lib, nv12, wins, (R.S, R.S), mode)
    assert rc == 0 and torch.equal(got, want)
    # the window table read on the device only; a padded surface; every frame on its own
    rc, dev = nv12_windows(lib, nv12, wins, (R.S, R.S), mode, host_windows=False, pitch=R.W + 2)
    assert rc == 0 and torch.equal(dev, want)
    for n in range(R.N):
        rc, one = nv12_windows(lib, nv12[n:n + 1], wins[n:n + 1], (R.S, R.S), mode)
        assert rc == 0 and torch.equal(one[0], want[n]), n
    # a non-square output and window, and the whole frame resized (null table)
    rect = [(x0, y0, s, max(2, s // 2)) for x0, y0, s in wins]
    want = np.zeros((R.N, 3, 40, 72), np.float32)
    w4 = _w4(rect)
    assert lib.emo_resize2d_windows_f32(_p(x), R.H * R.W, R.W, _p(w4), _p(want), R.N, 3, 40, 72, 1, 1, None) == 0
    rc, got = nv12_windows(lib, nv12, rect, (40, 72), mode)
    assert rc == 0 and torch.equal(got, torch.from_numpy(want))
    w4 = _w4([(0, 0, R.W, R.H)] * R.N)
    assert lib.emo_resize2d_windows_f32(_p(x), R.H * R.W, R.W, _p(w4), _p(want), R.N, 3, 40, 72, 1, 1, None) == 0
    rc, got = nv12_windows(lib, nv12, None, (40, 72), mode)
    assert rc == 0 and torch.equal(got, torch.from_numpy(want))


def test_a_bad_device_side_window_gives_zeros_for_its_frame(lib, small):
    nv12 = small["noise"][0]
    rc, want = nv12_windows(lib, nv12, R.WINDOWS, (R.S, R.S), R.MODES[0])
    bad = [(10, 5, 70), (411, 5, 70), (0, 0, 271), (300, 100, 0), (-1, 1, 180), (352, 143, 128)]
    rc, got = nv12_windows(lib, nv12, bad, (R.S, R.S), R.MODES[0], host_windows=False)
    assert rc == 0 and torch.equal(got[0], want[0]) and not got[1:].any()
    for n in range(1, R.N):
        rc, got = nv12_windows(lib, nv12[n:n + 1], bad[n:n + 1], (R.S, R.S), R.MODES[0])
        assert rc == -1 and bool((got == -7.0).all()), n


# ---- E -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_pack_against_the_fp64_restatement(lib, small, kind, mode):
    img = small[kind][1]
    for im, pitch in ((img, None), (img[:2, :, :6, :10].contiguous(), 13), (img[:, :, 1:127, :126].contiguous(), 200)):
        rc, got = pack(lib, im, mode, pitch)
        assert rc == 0
        worst, share, share32 = R.compare_bytes(got, R.encode(im.double(), *mode, F64), R.encode(im, *mode, F32), got.numel())
        print(f"PARITY nv12 E {kind} {tuple(im.shape[-2:])} {mode[0]} full_range {mode[1]}: max byte diff {worst}, share of bytes "
              f"that differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
        assert share32 <= R.MAX_SHARE
        assert worst <= R.MAX_BYTE_DIFF
        assert share <= R.MAX_SHARE


@pytest.mark.parametrize("mode", R.MODES)
def test_achromatic_frames_survive_decode_and_pack(lib, mode):
    nv12 = R.achromatic(mode[1])
    h, w = nv12.shape[1] // 3 * 2, nv12.shape[2]
    rc, rgb = nv12_windows(lib, nv12, None, (h, w), mode)
    assert rc == 0 and torch.equal(rgb[:, 0], rgb[:, 1]) and torch.equal(rgb[:, 0], rgb[:, 2])
    rc, back = pack(lib, rgb, mode)
    assert rc == 0 and torch.equal(back, nv12)
    assert torch.equal(R.encode(R.decode(nv12, *mode, F32), *mode, F32), nv12)          # (the restatement in fp32 holds it too)


# ---- P -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("case", range(len(R.CASES)))
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_paste_against_the_fp64_restatement(lib, small, kind, case, which):
    nv12, img, matte = small[kind]
    feather, use_matte = R.CASES[case]
    wins = (R.WINDOWS, R.WINDOWS_ODD)[which]
    mode = R.MODES[(case + which) % 4]
    m = matte if use_matte else None
    rc, got = paste(lib, nv12, img, wins, feather, m, mode)
    assert rc == 0
    worst, share, share32 = R.compare_paste(got, nv12, img, wins, feather, m, *mode)
    print(f"PARITY nv12 P {kind} windows {which} feather {feather} matte {use_matte} {mode[0]} full_range {mode[1]}: max byte diff "
          f"{worst}, share of touched bytes that differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
    assert share32 <= R.MAX_SHARE
    assert worst <= R.MAX_BYTE_DIFF
    assert share <= R.MAX_SHARE
    assert untouched_equal(got, nv12, wins)


@pytest.mark.parametrize("host_windows", [True, False])
@pytest.mark.parametrize("mode", R.MODES)
def test_side_equal_to_the_image_on_an_even_origin_without_feather_is_pack_nv12(lib, small, mode, host_windows):
    nv12, img, _ = small["noise"]
    wins = [(0, 0, R.S), (2, 142, R.S), (352, 0, R.S), (350, 142, R.S), (100, 70, R.S), (352, 142, R.S)]
    rc, got = paste(lib, nv12, img, wins, 0.0, None, mode, host_windows, pitch=R.W + 6)
    assert rc == 0
    rc, want = pack(lib, img, mode)
    assert rc == 0
    for n, (x0, y0, s) in enumerate(wins):
        assert torch.equal(got[n, y0:y0 + s, x0:x0 + s], want[n, :s]), n
        assert torch.equal(got[n, R.H + y0 // 2:R.H + (y0 + s) // 2, x0:x0 + s], want[n, s:]), n
    assert untouched_equal(got, nv12, wins)


@pytest.mark.parametrize("feather,use_matte", R.CASES)
def test_no_byte_outside_the_touched_rectangles_changes(lib, small, feather, use_matte):
    nv12, img, matte = small["noise"]
    edge = [(0, 0, 33), (R.W - 34, 0, 34), (0, R.H - 35, 35), (R.W - 36, R.H - 36, 36), (1, 1, 129), (2, 3, 131)]
    for i, wins in enumerate((R.WINDOWS, R.WINDOWS_ODD, edge)):
        rc, got = paste(lib, nv12, img, wins, feather, matte if use_matte else None, R.MODES[i], pitch=R.W + 10 * i)
        assert rc == 0
        assert untouched_equal(got, nv12, wins)
        touched = R.touched_mask(nv12.shape, wins)
        assert int((got != nv12)[touched].sum()) > 0.5 * int(touched.sum()) * (0.2 if use_matte else 1.0)     # (and they were written)


def test_a_zero_matte_changes_nothing_and_a_matte_of_ones_is_no_matte(lib, small):
    nv12, img, _ = small["noise"]
    for wins, mode in ((R.WINDOWS, R.MODES[1]), (R.WINDOWS_ODD, R.MODES[3])):
        for feather in (0.0, 0.0625):
            rc, got = paste(lib, nv12, img, wins, feather, torch.zeros(R.N, 1, R.S, R.S), mode)
            assert rc == 0 and torch.equal(got, nv12)
            rc1, ones = paste(lib, nv12, img, wins, feather, torch.ones(R.N, 1, R.S, R.S), mode)
            rc2, none = paste(lib, nv12, img, wins, feather, None, mode)
            assert rc1 == 0 and rc2 == 0 and torch.equal(ones, none) and not torch.equal(none, nv12)


def test_a_pasted_frame_does_not_depend_on_its_batch(lib, small):
    nv12, img, matte = small["smooth"]
    for wins in (R.WINDOWS, R.WINDOWS_ODD):
        rc, whole = paste(lib, nv12, img, wins, 0.0625, matte, R.MODES[2])
        assert rc == 0
        for n in range(R.N):
            rc, one = paste(lib, nv12[n:n + 1], img[n:n + 1], wins[n:n + 1], 0.0625, matte[n:n + 1], R.MODES[2])
            assert rc == 0 and torch.equal(one[0], whole[n]), n
        rc, dev = paste(lib, nv12, img, wins, 0.0625, matte, R.MODES[2], host_windows=False)
        assert rc == 0 and torch.equal(dev, whole)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_paste_refusals_write_nothing(lib, small):
    nv12, img, _ = small["noise"]
    f1, i1 = nv12[:1], img[:1]
    for wins, code in (([(10, 5, 70, 71)], -2), ([(10, 5, 31)], -2),
                       ([(411, 5, 70)], -1), ([(10, 201, 70)], -1), ([(-1, 5, 70)], -1), ([(10, -1, 70)], -1),
                       ([(10, 5, 0)], -1), ([(10, 5, -4)], -1), ([(0, 0, 271)], -1)):
        rc, got = paste(lib, f1, i1, wins)
        assert rc == code and torch.equal(got, f1), (wins, rc)
        rc, got = paste(lib, f1, i1, wins, host_windows=False)               # only the device sees them: the kernel skips the frame
        assert rc == 0 and torch.equal(got, f1), (wins, rc)
    rc, got = paste(lib, f1, i1, [(10, 5, 32)])
    assert rc == 0 and not torch.equal(got, f1)
    for feather in (-0.01, 0.51, float("nan")):
        rc, got = paste(lib, f1, i1, [(10, 5, 70)], feather)
        assert rc == -1 and torch.equal(got, f1)
    fr, im, w4 = np.zeros((1, 12, 8), np.uint8), np.zeros((1, 3, 4, 4), np.float32), np.array([[0, 0, 4, 4]], np.int32)
    y, uv = _p(fr), ctypes.c_void_p(fr.ctypes.data + 64)
    call = lib.emo_paste_windows_nv12
    ok = (_p(im), None, _p(w4), _p(w4), y, uv, 8, 96, 1, 4, 8, 8, 0.0, 0, 0, None)
    bad = {0: None, 2: None, 4: None, 5: None, 6: 7, 7: -1, 8: 0, 9: 0, 10: 7, 10.5: 0, 11: 7, 11.5: 0, 13: 2, 13.5: -1}
    for k, v in bad.items():
        a = list(ok)
        a[int(k)] = v
        assert call(*a) == -1, (k, v)
    assert not fr.any()


def test_crop_and_pack_refusals_write_nothing(lib):
    fr, im = np.full((1, 12, 8), 9, np.uint8), np.full((1, 3, 8, 8), 0.5, np.float32)
    out, w4 = np.full((1, 3, 4, 4), np.float32(-7)), np.array([[0, 0, 4, 4]], np.int32)
    y, uv = _p(fr), ctypes.c_void_p(fr.ctypes.data + 64)
    ok = (y, uv, 8, 96, 8, 8, _p(w4), _p(w4), _p(out), 1, 4, 4, 0, 0, None)
    for k, v in {0: None, 1: None, 2: 7, 3: -1, 4: 7, 4.5: 0, 5: 7, 5.5: 0, 6: None, 8: None, 9: 0, 10: 0, 11: -1, 12: 2, 12.5: -1}.items():
        a = list(ok)
        a[int(k)] = v
        assert lib.emo_nv12_windows_f32(*a) == -1, (k, v)
    for win in ((5, 0, 4, 4), (0, 5, 4, 4), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 9, 4)):
        w = np.array([win], np.int32)
        assert lib.emo_nv12_windows_f32(y, uv, 8, 96, 8, 8, _p(w), _p(w), _p(out), 1, 4, 4, 0, 0, None) == -1
    assert bool((out == -7).all())
    ok = (_p(im), y, uv, 8, 96, 1, 8, 8, 0, 0, None)
    for k, v in {0: None, 1: None, 2: None, 3: 7, 4: -1, 5: 0, 6: 7, 6.5: 0, 7: 7, 7.5: 0, 8: 2, 8.5: -1}.items():
        a = list(ok)
        a[int(k)] = v
        assert lib.emo_pack_nv12(*a) == -1, (k, v)
    assert bool((fr == 9).all())
    assert lib.emo_pack_nv12(*ok) == 0 and not bool((fr == 9).all())


def test_the_nv12_entry_points_are_in_the_abi_table():
    from emoportraits_amd import hip, _abi_version
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert _abi_version.EMO_ABI_VERSION >= 17
    for name, n in (("emo_nv12_windows_f32", 15), ("emo_pack_nv12", 11), ("emo_paste_windows_nv12", 16)):
        assert f"int {name}(" in hdr and len(hip.SIGNATURES[name]) == n


# ---- host logic on CPU tensors ---------------------------------------------------------------------------------------------
def _image(k, b):
    """what the stubbed driver pass returns for its k-th call"""
    return torch.rand(b, 3, R.S, R.S, generator=torch.Generator().manual_seed(40 + k)) * 1.2 - 0.1


@pytest.fixture()
def wrapper(monkeypatch, lib):
    """an InferenceWrapper on CPU tensors: the library the host-compiled one, the networks stand-ins (the driver pass a seeded
    image per call), the upload a plain copy"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import hip
    from emoportraits_amd.infer import InferenceWrapper
    facade = _Lib(lib)
    monkeypatch.setattr(hip, "load", lambda: facade)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    monkeypatch.setattr(frames_mod, "uploaded", lambda chunk, spans, device, stream: ((a, b, chunk[a:b].clone()) for a, b in spans))
    w = object.__new__(InferenceWrapper)
    w.device, w.rank, w.world = torch.device("cpu"), 0, 1
    w.cfg = dict(image_size=R.S)
    w._init_state(use_graphs=False)
    w.embedders = {}
    w._canonical_cl = torch.zeros(1)
    w.lib = facade
    w.crops, w.driven = [], []

    def head_pose(crops):
        w.crops.append(crops.clone())
        return (torch.eye(4).expand(crops.shape[0], 4, 4).contiguous(),)

    def drive(pose, theta):
        w.driven.append(_image(len(w.driven), pose.shape[0]))
        return w.driven[-1].clone()
    w._head_pose = head_pose
    w._expression = lambda crops, theta, what: (torch.zeros(crops.shape[0], 4), None)
    w._drive = drive
    return w


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


def test_ops_on_cpu_tensors_take_a_padded_view(wrapper, lib, small):
    from emoportraits_amd import ops
    nv12, img, matte = small["smooth"]
    mode = ("bt601", True)
    padded = torch.full((R.N, nv12.shape[1], R.W + 32), FILL, dtype=torch.uint8)
    padded[:, :, :R.W] = nv12
    view = padded[:, :, :R.W]
    rc, want = nv12_windows(lib, nv12, R.WINDOWS_ODD, (R.S, R.S), mode)
    assert torch.equal(ops.nv12_windows(view, (R.S, R.S), _sq(R.WINDOWS_ODD), *mode), want)
    rc, want = nv12_windows(lib, nv12, None, (R.H, R.W), mode)
    assert torch.equal(ops.nv12_windows(view, colorspace=mode[0], full_range=mode[1]), want)
    rc, want = paste(lib, nv12, img, R.WINDOWS_ODD, 0.0625, matte, mode)
    assert ops.paste_windows_nv12(view, img, _sq(R.WINDOWS_ODD), 0.0625, matte, *mode) is view
    assert torch.equal(view, want) and bool((padded[:, :, R.W:] == FILL).all())
    rc, want = pack(lib, img, mode)
    assert torch.equal(ops.pack_nv12(img, *mode), want)
    dst = torch.full((R.N, 3 * R.S // 2, R.S + 8), FILL, dtype=torch.uint8)
    assert torch.equal(ops.pack_nv12(img, *mode, out=dst[:, :, :R.S]), want) and bool((dst[:, :, R.S:] == FILL).all())
    wrapper.lib.calls.clear()
    work = nv12.clone()
    sq = _sq(R.WINDOWS)
    for bad, msg in ((sq[:5], "windows for"), (sq[:5] + [(352, 142, 128, 127)], "square"), (sq[:5] + [(353, 142, 128, 128)], "inside"),
                     (sq[:5] + [(352, 142, 31, 31)], "quarter")):
        with pytest.raises(ValueError, match=msg):
            ops.paste_windows_nv12(work, img, bad)
    with pytest.raises(ValueError, match="inside"):
        ops.nv12_windows(work, (R.S, R.S), sq[:5] + [(353, 142, 128, 128)])
    with pytest.raises(ValueError, match="colorspace"):
        ops.nv12_windows(work, (R.S, R.S), sq, colorspace="bt2020")
    with pytest.raises(ValueError, match="even"):
        ops.pack_nv12(img[:, :, :127])
    with pytest.raises(ValueError, match="even"):
        ops.nv12_windows(work[:, :, :479], (R.S, R.S), sq)
    with pytest.raises(ValueError, match="3H/2"):
        ops.nv12_windows(work[:, :404], (R.S, R.S), sq)
    with pytest.raises(ValueError, match="pitch"):
        ops.nv12_windows(work[:, :, ::2], (R.S, R.S), sq)
    assert wrapper.lib.calls == {} and torch.equal(work, nv12)


def test_wrapper_paste_back_on_nv12_frames(wrapper, lib, small):
    nv12, img, matte = small["smooth"]
    mode = ("bt709", True)
    rc, want = paste(lib, nv12, img, R.WINDOWS, 0.0625, matte, mode)
    before = nv12.clone()
    got = wrapper.paste_back(nv12, img, R.WINDOWS, matte=matte, frame_format="nv12", colorspace=mode[0], full_range=mode[1])
    assert torch.equal(got, want) and torch.equal(nv12, before) and got.data_ptr() != nv12.data_ptr()
    assert wrapper.lib.calls == {"emo_paste_yuv420": 1} and wrapper.lib.forms == {"emo_paste_yuv420": ["windows"]}
    with pytest.raises(ValueError, match="NV12"):
        wrapper.paste_back(nv12[:, :404], img, R.WINDOWS, frame_format="nv12")
    with pytest.raises(ValueError, match="frame_format"):
        wrapper.paste_back(nv12, img, R.WINDOWS, frame_format="yuv")


@pytest.mark.parametrize("out_format", [None, "rgb8"])
def test_animate_frames_nv12_runs_one_crop_launch_per_batch(wrapper, lib, small, out_format):
    """frames in NV12: per batch ONE emo_yuv420_crop_f32 in its one-window-per-frame form and none of the rgb8 ends; the crops the
    networks see are ops.nv12_windows' and what is yielded is emo_pack_yuv420 (or, out_format='rgb8', emo_pack_rgb8) of the driver
    pass' images"""
    from emoportraits_amd import ops
    nv12 = small["noise"][0]
    w, mode = wrapper, ("bt601", False)
    kw = dict(frame_format="nv12", colorspace=mode[0], full_range=mode[1])
    got = list(w.animate_frames(nv12, batch_size=4, windows=R.WINDOWS_ODD, to_host=False, out_format=out_format, **kw))
    assert [b0 for b0, _ in got] == [0, 4] and [t.shape[0] for _, t in got] == [4, 2]
    pack_name = "emo_pack_yuv420" if out_format is None else "emo_pack_rgb8"
    assert w.lib.calls == {"emo_yuv420_crop_f32": 2, pack_name: 2} and w.lib.forms == {"emo_yuv420_crop_f32": ["windows"] * 2}
    rc, crops = nv12_windows(lib, nv12, R.WINDOWS_ODD, (R.S, R.S), mode)
    assert torch.equal(torch.cat(w.crops), crops)
    images = torch.cat(w.driven)
    want = ops.pack_nv12(images, *mode) if out_format is None else ops.pack_rgb8(images)
    assert torch.equal(torch.cat([t for _, t in got]), want)
    assert tuple(want.shape[1:]) == ((3 * R.S // 2, R.S) if out_format is None else (R.S, R.S, 3))


def test_animate_frames_nv12_paste_back_is_paste_back_of_the_rendered_images(wrapper, lib, small):
    from emoportraits_amd import ops
    nv12, _, matte = small["smooth"]
    w, mode = wrapper, ("bt709", False)
    before = nv12.clone()
    got = list(w.animate_frames(nv12, batch_size=4, windows=R.WINDOWS, to_host=False, paste_back=True, feather=0.25,
                                paste_matte=lambda img: matte[:img.shape[0]], frame_format="nv12"))
    assert w.lib.calls == {"emo_yuv420_crop_f32": 2, "emo_paste_yuv420": 2}
    assert w.lib.forms == {"emo_yuv420_crop_f32": ["windows"] * 2, "emo_paste_yuv420": ["windows"] * 2}
    images = torch.cat(w.driven)
    want = torch.cat([w.paste_back(nv12[a:b], images[a:b], R.WINDOWS[a:b], 0.25, matte[:b - a], frame_format="nv12") for a, b in ((0, 4), (4, 6))])
    assert torch.equal(torch.cat([t for _, t in got]), want) and torch.equal(nv12, before)
    assert untouched_equal(want, nv12, R.WINDOWS) and not torch.equal(want, nv12)


def test_animate_frames_checks_its_nv12_arguments_before_any_launch(wrapper, small):
    nv12 = small["smooth"][0]
    w = wrapper
    rgb = torch.zeros(R.N, R.H, R.W, 3, dtype=torch.uint8)
    nv = dict(frame_format="nv12", windows=R.WINDOWS)
    for match, frames, kw in (("3H/2", nv12[:, :404], nv), ("3H/2", nv12[:, :, :479], nv), ("3H/2", rgb, nv),
                              (r"\[N,H,W,3\]", nv12, dict(windows=R.WINDOWS)),
                              ("paste_back", nv12, dict(nv, paste_back=True, out_format="rgb8")),
                              ("paste_back", rgb, dict(windows=R.WINDOWS, paste_back=True, out_format="nv12")),
                              ("out_format", nv12, dict(nv, to_host=False, as_uint8=False, out_format="nv12")),
                              ("out_format", rgb, dict(windows=R.WINDOWS, to_host=False, as_uint8=False, out_format="rgb8")),
                              ("frame_format", nv12, dict(windows=R.WINDOWS, frame_format="i420")),
                              ("out_format", nv12, dict(nv, out_format="yuv")),
                              ("colorspace", nv12, dict(nv, colorspace="bt2020"))):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(frames, **kw))
    w.cfg["image_size"] = R.S - 1
    with pytest.raises(ValueError, match="even image_size"):
        next(w.animate_frames(nv12, **nv))
    with pytest.raises(ValueError, match="even image_size"):
        next(w.animate_frames(rgb, windows=R.WINDOWS, out_format="nv12"))
    with pytest.raises(ValueError, match="even image_size"):
        next(w.animate(torch.zeros(2, 4), [torch.zeros(2, 3)] * 3, out_format="nv12"))
    w.cfg["image_size"] = R.S
    with pytest.raises(ValueError, match="out_format"):
        next(w.animate(torch.zeros(2, 4), [torch.zeros(2, 3)] * 3, out_format="nv12", as_uint8=False))
    with pytest.raises(ValueError, match="out_format"):
        next(w.animate(torch.zeros(2, 4), [torch.zeros(2, 3)] * 3, out_format="yuv"))
    assert w.lib.calls == {} and w.driven == []


def test_the_video_tool_reads_raw_nv12_files_in_chunks(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("animate_video", os.path.join(ROOT, "tools", "animate_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    clip = torch.randint(0, 256, (5, 12, 16), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    path = str(tmp_path / "clip.nv12")
    clip.numpy().tofile(path)
    chunks = list(tool.load_nv12(path, 16, 8, 2))
    assert [c.shape[0] for c in chunks] == [2, 2, 1] and torch.equal(torch.cat(chunks), clip)
    with open(path, "ab") as f:
        f.write(b"\0" * 7)
    with pytest.raises(SystemExit, match="whole number"):
        next(tool.load_nv12(path, 16, 8, 2))
