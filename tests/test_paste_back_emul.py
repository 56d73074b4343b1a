"""emo_paste_windows_rgb8 (csrc/resample.hip, ABI 15: the rendered crops go back into the full driver frames) without a GPU: the
kernel is compiled for the host from the product's own source (tests/emul/emulibs.py, the sequential build) and run on host memory.
  * exact cases: side == S without feather is emo_pack_rgb8's bytes; no byte outside a window changes, whatever the window's
    position (all four frame borders, x0 % 4 = 0 .. 3: the head and the tail of the three-dword runs); a matte of zeros leaves the
    frame as it was, a matte of ones is no matte; a frame's result does not depend on the batch it is in;
  * against the definition restated in torch and evaluated in fp64 (tests/paste_back_reference.py): every byte within 1, and at
    most 2e-3 of the window bytes different at all -- torch's own fp32 evaluation differs from its fp64 one on 1.3e-5 ... 3.4e-4
    of them on these inputs, which the test recomputes and holds against the same cap;
  * refusals, with nothing written;
  * ops.paste_windows, InferenceWrapper.paste_back and the argument checks of animate_frames(paste_back=True) on CPU tensors,
    the package pointed at the host-compiled library inside the test only.
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
import paste_back_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    lib = emulibs.stream(False)
    assert hasattr(lib, "emo_paste_windows_rgb8"), "csrc/resample.hip does not export emo_paste_windows_rgb8"
    lib.emo_paste_windows_rgb8.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def small():
    return R.small_inputs()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _np(t):
    return None if t is None else np.ascontiguousarray(t.numpy())


def paste(lib, frames, img, wins, feather=0.0, matte=None, host_windows=True, offset=0):
    """emo_paste_windows_rgb8 on copies -> (return code, uint8 tensor [N,Hf,Wf,3]); wins (x0, y0, s) or (x0, y0, w, h) per frame;
    offset: the frames start that many bytes behind a 4-byte aligned address"""
    N, Hf, Wf, _ = frames.shape
    S = img.shape[-1]
    raw = np.zeros(frames.numel() + 8, np.uint8)
    start = (-raw.ctypes.data) % 4 + offset
    buf = raw[start:start + frames.numel()]
    buf[...] = frames.numpy().reshape(-1)
    w4 = np.ascontiguousarray([(w[0], w[1], w[2], w[3] if len(w) > 3 else w[2]) for w in wins], dtype=np.int32)
    im, mt = _np(img), _np(matte)
    rc = lib.emo_paste_windows_rgb8(_p(im), _p(mt), _p(w4), _p(w4) if host_windows else None, _p(buf), N, S, Hf, Wf, feather, None)
    assert raw[:start].sum() == 0 and raw[start + frames.numel():].sum() == 0          # nothing in front of or behind the frames
    return rc, torch.from_numpy(buf.reshape(N, Hf, Wf, 3).copy())


def pack_rgb8(lib, img):
    N, _, H, W = img.shape
    out = np.zeros((N, H, W, 3), np.uint8)
    im = _np(img)
    assert lib.emo_pack_rgb8(_p(im), _p(out), N, H, W, None) == 0
    return torch.from_numpy(out)


def outside_equal(got, frames, wins):
    mask = torch.ones(frames.shape[:3], dtype=torch.bool)
    for n, w in enumerate(wins):
        mask[n, w[1]:w[1] + w[2], w[0]:w[0] + w[2]] = False
    return torch.equal(got[mask], frames[mask])


# ---- exact cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_windows", [True, False])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_side_equal_to_the_image_without_feather_is_pack_rgb8(lib, small, host_windows, offset):
    frames, img, _ = small["noise"]
    S = img.shape[-1]
    wins = [(0, 0, S), (1, 142, S), (2, 7, S), (3, 100, S), (352, 0, S), (351, 142, S)]      # x0 % 4 = 0 .. 3, all four borders
    rc, got = paste(lib, frames, img, wins, 0.0, None, host_windows, offset)
    assert rc == 0
    want = pack_rgb8(lib, img)
    for n, (x0, y0, s) in enumerate(wins):
        assert np.array_equal(got[n, y0:y0 + s, x0:x0 + s].numpy(), want[n].numpy()), n
    assert outside_equal(got, frames, wins)


@pytest.mark.parametrize("feather,use_matte", R.CASES)
def test_no_byte_outside_a_window_changes(lib, small, feather, use_matte):
    frames, img, matte = small["noise"]
    Hf, Wf = frames.shape[1:3]
    # up- and downscaling windows on every border and corner, x0 % 4 and side % 4 of every residue
    for wins in ([(0, 0, 33), (Wf - 34, 0, 34), (0, Hf - 35, 35), (Wf - 36, Hf - 36, 36), (1, 1, 129), (2, 3, 131)],
                 [(3, 0, 270), (209, 0, 270), (210, 0, 270), (0, 1, 269), (5, 17, 32), (6, 18, 201)]):
        rc, got = paste(lib, frames, img, wins, feather, matte if use_matte else None)
        assert rc == 0
        assert outside_equal(got, frames, wins)
        changed = sum(int((got[n] != frames[n]).sum()) for n in range(len(wins)))
        assert changed > 0.5 * R.window_bytes(wins) * (0.2 if use_matte else 1.0)           # (and the windows were written)


def test_a_zero_matte_changes_nothing_and_a_matte_of_ones_is_no_matte(lib, small):
    frames, img, _ = small["noise"]
    for feather in (0.0, 0.0625):
        rc, got = paste(lib, frames, img, R.WINDOWS, feather, torch.zeros(6, 1, 128, 128))
        assert rc == 0 and torch.equal(got, frames)
        rc1, ones = paste(lib, frames, img, R.WINDOWS, feather, torch.ones(6, 1, 128, 128))
        rc2, none = paste(lib, frames, img, R.WINDOWS, feather, None)
        assert rc1 == 0 and rc2 == 0 and torch.equal(ones, none) and not torch.equal(none, frames)


def test_a_frame_does_not_depend_on_its_batch(lib, small):
    frames, img, matte = small["smooth"]
    rc, whole = paste(lib, frames, img, R.WINDOWS, 0.0625, matte)
    assert rc == 0
    for n in range(6):
        rc, one = paste(lib, frames[n:n + 1], img[n:n + 1], R.WINDOWS[n:n + 1], 0.0625, matte[n:n + 1])
        assert rc == 0 and torch.equal(one[0], whole[n]), n
    # and the windows read on the device only (the grid then covers min(Hf, Wf) rows) give the same bytes
    rc, dev = paste(lib, frames, img, R.WINDOWS, 0.0625, matte, host_windows=False)
    assert rc == 0 and torch.equal(dev, whole)


# ---- against the fp64 restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather,use_matte", R.CASES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_against_the_fp64_restatement(lib, small, kind, feather, use_matte):
    frames, img, matte = small[kind]
    m = matte if use_matte else None
    rc, got = paste(lib, frames, img, R.WINDOWS, feather, m)
    assert rc == 0
    worst, share, share32 = R.compare(got, frames, img, R.WINDOWS, feather, m)
    print(f"PARITY paste {kind} feather {feather} matte {use_matte}: max byte diff {worst}, share of window bytes that differ "
          f"{share:.2e} (torch fp32 against fp64: {share32:.2e})")
    assert share32 <= R.MAX_SHARE                     # the premise: torch's own fp32 noise stays under the cap
    assert worst <= R.MAX_BYTE_DIFF
    assert share <= R.MAX_SHARE
    assert outside_equal(got, frames, R.WINDOWS)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(lib, small):
    frames, img, matte = small["noise"]
    f1, i1 = frames[:1], img[:1]
    for wins, code in (([(10, 5, 70, 71)], -2),            # not square
                       ([(10, 5, 31)], -2),                 # 4 * 31 < 128: downscaling by more than 4
                       ([(411, 5, 70)], -1), ([(10, 201, 70)], -1), ([(-1, 5, 70)], -1), ([(10, -1, 70)], -1),
                       ([(10, 5, 0)], -1), ([(10, 5, -4)], -1), ([(0, 0, 271)], -1)):
        rc, got = paste(lib, f1, i1, wins)
        assert rc == code and torch.equal(got, f1), (wins, rc)
        # the same windows where only the device sees them: the launch succeeds and the kernel skips the frame
        rc, got = paste(lib, f1, i1, wins, host_windows=False)
        assert rc == 0 and torch.equal(got, f1), (wins, rc)
    rc, got = paste(lib, f1, i1, [(10, 5, 32)])            # 4 * 32 == 128 is the last supported side
    assert rc == 0 and not torch.equal(got, f1)
    for feather in (-0.01, 0.51, float("nan")):
        rc, got = paste(lib, f1, i1, [(10, 5, 70)], feather)
        assert rc == -1 and torch.equal(got, f1)
    fr, im, w4 = np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 3, 4, 4), np.float32), np.array([[0, 0, 4, 4]], np.int32)
    call = lib.emo_paste_windows_rgb8
    assert call(None, None, _p(w4), _p(w4), _p(fr), 1, 4, 8, 8, 0.0, None) == -1
    assert call(_p(im), None, None, _p(w4), _p(fr), 1, 4, 8, 8, 0.0, None) == -1
    assert call(_p(im), None, _p(w4), _p(w4), None, 1, 4, 8, 8, 0.0, None) == -1
    for N, S, Hf, Wf in ((0, 4, 8, 8), (-1, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, -2)):
        assert call(_p(im), None, _p(w4), _p(w4), _p(fr), N, S, Hf, Wf, 0.0, None) == -1
    assert not fr.any()


def test_paste_windows_is_in_the_abi_table():
    from emoportraits_amd import hip, _abi_version
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "int emo_paste_windows_rgb8(" in hdr and _abi_version.EMO_ABI_VERSION >= 15
    assert len(hip.SIGNATURES["emo_paste_windows_rgb8"]) == 11


# ---- host logic on CPU tensors ---------------------------------------------------------------------------------------------
@pytest.fixture()
def wrapper(monkeypatch, lib):
    from emoportraits_amd import hip
    from emoportraits_amd.infer import InferenceWrapper
    facade = _Lib(lib)
    monkeypatch.setattr(hip, "load", lambda: facade)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    w = object.__new__(InferenceWrapper)
    w.device, w.rank, w.world = torch.device("cpu"), 0, 1
    w.cfg = dict(image_size=128)
    w._init_state(use_graphs=False)
    w.embedders = {}
    w._canonical_cl = torch.zeros(1)
    w.lib = facade
    return w


def test_ops_and_wrapper_paste_back_on_cpu_tensors(wrapper, lib, small):
    from emoportraits_amd import ops
    frames, img, matte = small["smooth"]
    rc, want = paste(lib, frames, img, R.WINDOWS, 0.0625, matte)
    assert rc == 0
    before = frames.clone()
    got = wrapper.paste_back(frames, img, R.WINDOWS, matte=matte)                      # (x_lo, y_lo, side); feather 1/16
    assert torch.equal(got, want) and torch.equal(frames, before) and got.data_ptr() != frames.data_ptr()
    assert wrapper.lib.calls == {"emo_paste_windows_rgb8": 1}
    assert torch.equal(wrapper.paste_back(frames, img, R.WINDOWS, matte=lambda x: matte), want)
    work = frames.clone()
    assert ops.paste_windows(work, img, [(x, y, s, s) for x, y, s in R.WINDOWS], 0.0625, matte) is work and torch.equal(work, want)
    with pytest.raises(RuntimeError, match="matting"):
        wrapper.paste_back(frames, img, R.WINDOWS, matte=True)
    wrapper.lib.calls.clear()
    work = frames.clone()
    sq = [(x, y, s, s) for x, y, s in R.WINDOWS]
    for bad, msg in ((sq[:5], "windows for"), (sq[:5] + [(352, 142, 128, 127)], "square"), (sq[:5] + [(353, 142, 128, 128)], "inside"),
                     (sq[:5] + [(352, 142, 31, 31)], "quarter")):
        with pytest.raises(ValueError, match=msg):
            ops.paste_windows(work, img, bad)
    with pytest.raises(ValueError, match="feather"):
        ops.paste_windows(work, img, sq, feather=0.6)
    with pytest.raises(ValueError, match="matte"):
        ops.paste_windows(work, img, sq, matte=matte[:, :, :64])
    with pytest.raises(ValueError, match="side"):
        wrapper.paste_back(frames, img, [(0, 0, 128, 64)] * 6)
    assert wrapper.lib.calls == {} and torch.equal(work, frames)


def test_animate_frames_checks_its_paste_arguments_before_any_launch(wrapper, small):
    frames = small["smooth"][0]
    w = wrapper
    with pytest.raises(ValueError, match="windows"):
        next(w.animate_frames(frames, paste_back=True))
    with pytest.raises(ValueError, match="feather"):
        next(w.animate_frames(frames, windows=R.WINDOWS, paste_back=True, feather=0.75))
    with pytest.raises(RuntimeError, match="matting"):
        next(w.animate_frames(frames, windows=R.WINDOWS, paste_back=True, paste_matte=True))
    with pytest.raises(ValueError, match="paste_matte"):
        next(w.animate_frames(frames, windows=R.WINDOWS, paste_back=True, paste_matte=3))
    with pytest.raises(ValueError, match="quarter"):
        next(w.animate_frames(frames, windows=[(0, 0, 31)] * 6, paste_back=True))
    with pytest.raises(ValueError, match="as_uint8"):
        next(w.animate_frames(frames, windows=R.WINDOWS, as_uint8=False))
    with pytest.raises(ValueError, match="as_uint8"):
        next(w.animate_frames(frames, windows=R.WINDOWS, to_host=False, as_uint8=False, paste_back=True))
    assert w.lib.calls == {}
