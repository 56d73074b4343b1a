"""Several faces per frame (ABI 18: emo_resize2d_faces_f32, emo_nv12_faces_f32, emo_paste_faces_rgb8, emo_paste_faces_nv12)
without a GPU: the kernels are compiled for the host from the product's own source (tests/emul/emulibs.py, the sequential build)
and run on host memory.  Nothing here has a tolerance: the crops are held bit for bit to the single-window entry points on
frames[frame_of], the pastes to the faces pasted one after another with the single-window entry points (N = 1 each, list order),
which the existing tests hold to the fp64 restatement; -ffp-contract=off makes the equality exact.
  * the shared small case (tests/faces_reference.py): overlaps of two and of three faces, a frame without a face, odd origins,
    the frame's corner; reversing two overlapping faces changes bytes inside their intersection only; nothing outside the union
    of the windows changes; frame_of = arange(N) is the batched entry point; device-only windows with an invalid one among them;
  * refusals, with nothing written; M == 0;
  * the ABI table, frames.flatten_faces / face_spans, parallel.gather_rows at world 1 and at world 2 on gloo;
  * ops.*, InferenceWrapper.paste_back(faces=) / animate_frames(faces=) on CPU tensors, calls counted; animate_frames(windows=)
    against faces= with one face per frame: one loop, the same tensors, the entry points' names apart.
frames.face_spans: the issue that asked for it states the rule in words (whole frames, greedily, while faces <= batch_size and
frames <= batch_size) and gives counts [2,0,3,1], batch_size 4 -> [(0,2),(2,3),(3,4)] as an example.  The example contradicts the
rule (frames 2 and 3 hold 3 + 1 = 4 faces) and the requirement that a clip of 6 frames x 2 faces at batch_size 4 has the
batches of its flattened windows= form (4 faces each); the test holds the function to the rule: [(0,2),(2,4)]."""
import ctypes
import multiprocessing as mp
import os
import socket
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
import faces_reference as R  # noqa: E402
import nv12_reference as NV  # noqa: E402
import paste_back_reference as PB  # noqa: E402

NEW = ("emo_resize2d_faces_f32", "emo_nv12_faces_f32", "emo_paste_faces_rgb8", "emo_paste_faces_nv12")
OLD = ("emo_resize2d_windows_f32", "emo_nv12_windows_f32", "emo_paste_windows_rgb8", "emo_paste_windows_nv12")
# what the Python layer launches: rgb8 the entry points above, NV12 the ABI 22 crop and paste, which serve both forms under one name
# -- the facade records the form of every call (counting_lib: frame_of null or not)
RUN_NEW = {"rgb8": (NEW[0], NEW[2]), "nv12": ("emo_yuv420_crop_f32", "emo_paste_yuv420")}
RUN_OLD = {"rgb8": (OLD[0], OLD[2]), "nv12": RUN_NEW["nv12"]}
MODE = ("bt601", True)                                   # (colorspace, full_range) of the NV12 cases
MATRIX = (NV.MATRIX_ID[MODE[0]], int(MODE[1]))


@pytest.fixture(scope="module")
def lib():
    from emoportraits_amd import hip
    lib = emulibs.stream(False)
    for name in NEW + OLD:
        assert hasattr(lib, name), f"csrc/resample.hip does not export {name}"
        getattr(lib, name).argtypes = hip.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def rgb():
    R.check_case()
    return R.small_rgb()


@pytest.fixture(scope="module")
def nv12():
    return R.small_nv12()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _np(t):
    return None if t is None else np.ascontiguousarray(t.numpy())


def _w4(wins):
    return np.ascontiguousarray([(w[0], w[1], w[2], w[3] if len(w) > 3 else w[2]) for w in wins], dtype=np.int32).reshape(-1, 4)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _planes(buf, hf):
    """(Y pointer, UV pointer, pitch, frame stride) of contiguous NV12 frames [F, 3Hf/2, Wf] in a numpy array"""
    return ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data + hf * buf.shape[2]), buf.shape[2], buf.shape[1] * buf.shape[2]


# ---- the four entry points and their single-window counterparts on host memory ------------------------------------------------
def crop_rgb(lib, x, wins, frame_of=None):
    xs, w4 = _np(x), _w4(wins)
    F, C, H, W = xs.shape
    out = np.full((len(wins), C, R.S, R.S), np.float32(-7.0))
    if frame_of is None:
        rc = lib.emo_resize2d_windows_f32(_p(xs), H * W, W, _p(w4), _p(out), F, C, R.S, R.S, 1, 1, None)
    else:
        fo = _i32(frame_of)
        rc = lib.emo_resize2d_faces_f32(_p(xs), H * W, W, _p(w4), _p(fo), _p(out), len(wins), F, C, R.S, R.S, 1, 1, None)
    return rc, torch.from_numpy(out)


def crop_nv12(lib, frames, wins, frame_of=None, host=True):
    buf, w4 = _np(frames).copy(), _w4(wins)
    y, uv, pitch, fs = _planes(buf, R.HF)
    out = np.full((len(wins), 3, R.S, R.S), np.float32(-7.0))
    if frame_of is None:
        rc = lib.emo_nv12_windows_f32(y, uv, pitch, fs, R.HF, R.WF, _p(w4), _p(w4) if host else None, _p(out), len(wins), R.S, R.S, *MATRIX, None)
    else:
        fo = _i32(frame_of)
        rc = lib.emo_nv12_faces_f32(y, uv, pitch, fs, R.HF, R.WF, _p(w4), _p(w4) if host else None, _p(fo), _p(fo) if host else None,
                                    _p(out), len(wins), buf.shape[0], R.S, R.S, *MATRIX, None)
    assert np.array_equal(buf, frames.numpy())
    return rc, torch.from_numpy(out)


def paste_rgb(lib, frames, img, matte, wins, feather=0.0, frame_of=None, host_windows=True, host_frame_of=True, dev_frame_of=None):
    """emo_paste_faces_rgb8 (frame_of given) or emo_paste_windows_rgb8 on a copy -> (return code, the frames)"""
    buf, w4, im, mt = _np(frames).copy(), _w4(wins), _np(img), _np(matte)
    F, Hf, Wf, _ = buf.shape
    hw = _p(w4) if host_windows else None
    if frame_of is None:
        rc = lib.emo_paste_windows_rgb8(_p(im), _p(mt), _p(w4), hw, _p(buf), F, img.shape[-1], Hf, Wf, feather, None)
    else:
        fo = _i32(frame_of)
        fd = fo if dev_frame_of is None else _i32(dev_frame_of)
        rc = lib.emo_paste_faces_rgb8(_p(im), _p(mt), _p(w4), hw, _p(fd), _p(fo) if host_frame_of else None, _p(buf), len(wins), F,
                                      img.shape[-1], Hf, Wf, feather, None)
    return rc, torch.from_numpy(buf)


def paste_nv12(lib, frames, img, matte, wins, feather=0.0, frame_of=None, host_windows=True, host_frame_of=True):
    buf, w4, im, mt = _np(frames).copy(), _w4(wins), _np(img), _np(matte)
    y, uv, pitch, fs = _planes(buf, R.HF)
    hw = _p(w4) if host_windows else None
    if frame_of is None:
        rc = lib.emo_paste_windows_nv12(_p(im), _p(mt), _p(w4), hw, y, uv, pitch, fs, buf.shape[0], img.shape[-1], R.HF, R.WF, feather,
                                        *MATRIX, None)
    else:
        fo = _i32(frame_of)
        rc = lib.emo_paste_faces_nv12(_p(im), _p(mt), _p(w4), hw, _p(fo), _p(fo) if host_frame_of else None, y, uv, pitch, fs, len(wins),
                                      buf.shape[0], img.shape[-1], R.HF, R.WF, feather, *MATRIX, None)
    return rc, torch.from_numpy(buf)


PASTE = {"rgb8": paste_rgb, "nv12": paste_nv12}
MASK = {"rgb8": R.rgb_mask, "nv12": R.nv12_mask}


def _one(lib, fmt, feather):
    def paste_one(frame, img, matte, w):
        rc, out = PASTE[fmt](lib, frame, img, matte, [w], feather)
        assert rc == 0
        return out
    return paste_one


def _inputs(rgb, nv12, fmt, kind):
    return (rgb if fmt == "rgb8" else nv12)[kind]


def _bytes(mask, t):
    """the bytes of t under a pixel mask [F,H,W] (rgb8 frames [F,H,W,3]) or a byte mask (NV12)"""
    return t[mask]


# ---- crops ---------------------------------------------------------------------------------------------------------------------
def test_crops_are_the_window_crops_of_the_faces_frames(lib, rgb, nv12):
    frames = rgb["noise"][0]
    x = (frames.permute(0, 3, 1, 2).float() / 255).contiguous()
    rc, got = crop_rgb(lib, x, R.WINDOWS, R.FRAME_OF)
    rc0, want = crop_rgb(lib, x[R.FRAME_OF].contiguous(), R.WINDOWS)
    assert rc == 0 and rc0 == 0 and torch.equal(got, want)
    for host in (True, False):
        rc, got = crop_nv12(lib, nv12["noise"][0], R.WINDOWS, R.FRAME_OF, host)
        rc0, want = crop_nv12(lib, nv12["noise"][0][R.FRAME_OF].contiguous(), R.WINDOWS)
        assert rc == 0 and rc0 == 0 and torch.equal(got, want)


def test_a_face_of_no_frame_and_a_device_window_outside_the_frame_get_zeros(lib, rgb, nv12):
    x = (rgb["smooth"][0].permute(0, 3, 1, 2).float() / 255).contiguous()
    rc, got = crop_rgb(lib, x, R.WINDOWS, [0, 0, 2, 2, 2, 4])                   # (no host copy in this entry point: the device's word)
    rc0, want = crop_rgb(lib, x, R.WINDOWS, R.FRAME_OF)
    assert rc == 0 and torch.equal(got[:5], want[:5]) and not got[5].any()
    wins = R.WINDOWS[:4] + [(400, 1, 180)] + R.WINDOWS[5:]
    rc, got = crop_nv12(lib, nv12["smooth"][0], wins, R.FRAME_OF, host=False)
    rc0, want = crop_nv12(lib, nv12["smooth"][0], R.WINDOWS, R.FRAME_OF)
    assert rc == 0 and not got[4].any() and torch.equal(got[:4], want[:4]) and torch.equal(got[5], want[5])


# ---- paste ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather,use_matte", PB.CASES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_paste_is_the_faces_pasted_one_after_another(lib, rgb, nv12, fmt, kind, feather, use_matte):
    frames, img, matte = _inputs(rgb, nv12, fmt, kind)
    m = matte if use_matte else None
    want = R.sequential(_one(lib, fmt, feather), frames, img, m, R.WINDOWS, R.FRAME_OF)
    rc, got = PASTE[fmt](lib, frames, img, m, R.WINDOWS, feather, R.FRAME_OF)
    assert rc == 0 and torch.equal(got, want)
    # the frame without a face and every byte outside the union of the windows are the input's
    touched = MASK[fmt](len(R.FACES), R.WINDOWS, R.FRAME_OF)
    assert torch.equal(got[1], frames[1]) and torch.equal(_bytes(~touched, got), _bytes(~touched, frames))
    assert not torch.equal(got, frames)
    # the windows read on the device only (the grid then covers min(Hf, Wf)) give the same bytes
    rc, dev = PASTE[fmt](lib, frames, img, m, R.WINDOWS, feather, R.FRAME_OF, host_windows=False)
    assert rc == 0 and torch.equal(dev, want)


@pytest.mark.parametrize("feather,use_matte", PB.CASES)
@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_the_order_of_two_overlapping_faces_matters_inside_their_intersection_only(lib, rgb, nv12, fmt, feather, use_matte):
    frames, img, matte = _inputs(rgb, nv12, fmt, "noise")
    m = matte if use_matte else None
    rc, got = PASTE[fmt](lib, frames, img, m, R.WINDOWS, feather, R.FRAME_OF)
    order = [1, 0, 2, 3, 4, 5]                                                   # the two faces of frame 0, the other way round
    wins = [R.WINDOWS[i] for i in order]
    rc2, swapped = PASTE[fmt](lib, frames, img[order], None if m is None else m[order], wins, feather, R.FRAME_OF)
    assert rc == 0 and rc2 == 0
    assert torch.equal(swapped, R.sequential(_one(lib, fmt, feather), frames, img[order], None if m is None else m[order], wins, R.FRAME_OF))
    both = MASK[fmt](len(R.FACES), R.WINDOWS[:1], [0]) & MASK[fmt](len(R.FACES), R.WINDOWS[1:2], [0])
    assert not torch.equal(_bytes(both, got), _bytes(both, swapped))
    assert torch.equal(_bytes(~both, got), _bytes(~both, swapped))


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_one_face_per_frame_is_the_batched_entry_point(lib, fmt):
    frames, img, matte = (PB.small_inputs() if fmt == "rgb8" else NV.small_inputs())["smooth"]
    rc, want = PASTE[fmt](lib, frames, img, matte, PB.WINDOWS, 0.0625)
    rc2, got = PASTE[fmt](lib, frames, img, matte, PB.WINDOWS, 0.0625, list(range(6)))
    assert rc == 0 and rc2 == 0 and torch.equal(got, want)


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_an_invalid_device_only_window_is_absent(lib, rgb, nv12, fmt):
    """windows that exist on the device only: the middle face of frame 2 not square, outside the frame, or too small -- the
    result is the paste of the others, and the bytes only that face would have touched stay"""
    frames, img, matte = _inputs(rgb, nv12, fmt, "smooth")
    want = R.sequential(_one(lib, fmt, 0.0625), frames, img, matte, R.WINDOWS, R.FRAME_OF, skip=(3,))
    for bad in ((300, 100, 96, 95), (400, 100, 96), (300, 100, 31), (-2, 100, 96), (300, 100, 0)):
        wins = R.WINDOWS[:3] + [bad] + R.WINDOWS[4:]
        rc, got = PASTE[fmt](lib, frames, img, matte, wins, 0.0625, R.FRAME_OF, host_windows=False)
        assert rc == 0 and torch.equal(got, want), bad


def test_a_device_frame_of_outside_the_frames_is_absent(lib, rgb):
    frames, img, matte = rgb["smooth"]
    want = R.sequential(_one(lib, "rgb8", 0.0), frames, img, matte, R.WINDOWS, R.FRAME_OF, skip=(5,))
    rc, got = paste_rgb(lib, frames, img, matte, R.WINDOWS, 0.0, R.FRAME_OF, dev_frame_of=[0, 0, 2, 2, 2, 4])
    assert rc == 0 and torch.equal(got, want)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_refusals_write_nothing(lib, rgb, nv12, fmt):
    frames, img, matte = _inputs(rgb, nv12, fmt, "noise")
    W = R.WINDOWS

    def refused(code, wins=W, frame_of=R.FRAME_OF, **kw):
        rc, got = PASTE[fmt](lib, frames, img, matte, wins, kw.pop("feather", 0.0625), frame_of, **kw)
        assert rc == code and torch.equal(got, frames), (wins, frame_of, kw, rc)
    refused(-1, frame_of=[0, 0, 2, 2, 1, 3])                                    # decreases
    refused(-1, frame_of=[0, 0, 2, 2, 2, 4])                                    # leaves [0, F)
    refused(-1, frame_of=[-1, 0, 2, 2, 2, 3])
    refused(-1, host_frame_of=False)                                            # the paste needs the host copy
    refused(-1, wins=W[:5] + [(353, 142, 128)])                                 # leaves the frame
    refused(-1, wins=W[:5] + [(352, 143, 128)])
    refused(-1, wins=[(-1, 5, 70)] + W[1:])
    refused(-1, wins=[(10, 5, 0)] + W[1:])
    refused(-2, wins=[(10, 5, 70, 71)] + W[1:])                                 # not square
    refused(-2, wins=[(10, 5, 31)] + W[1:])                                     # 4 * 31 < 128
    for feather in (-0.01, 0.51, float("nan")):
        refused(-1, feather=feather)


def test_refusals_of_the_crops_and_of_bad_sizes(lib, rgb, nv12):
    frames = nv12["noise"][0]
    for fo in ([0, 0, 2, 2, 1, 3], [0, 0, 2, 2, 2, 4]):
        rc, out = crop_nv12(lib, frames, R.WINDOWS, fo)
        assert rc == -1 and bool((out == -7.0).all())
    rc, out = crop_nv12(lib, frames, R.WINDOWS[:5] + [(353, 142, 128)], R.FRAME_OF)
    assert rc == -1 and bool((out == -7.0).all())
    fr, im = np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 3, 4, 4), np.float32)
    nv, w4, fo, out = np.zeros((1, 12, 8), np.uint8), np.array([[0, 0, 4, 4]], np.int32), np.zeros(1, np.int32), np.zeros((1, 3, 4, 4), np.float32)
    y, uv, pitch, fs = _planes(nv, 8)
    rgb8, n12, crop, ncrop = lib.emo_paste_faces_rgb8, lib.emo_paste_faces_nv12, lib.emo_resize2d_faces_f32, lib.emo_nv12_faces_f32
    assert rgb8(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), _p(fr), 1, 1, 4, 8, 8, 0.0, None) == 0
    assert n12(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), y, uv, pitch, fs, 1, 1, 4, 8, 8, 0.0, 0, 0, None) == 0
    fr[...], nv[...] = 0, 0
    for M, F in ((-1, 1), (1, 0), (1, -3)):
        assert rgb8(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), _p(fr), M, F, 4, 8, 8, 0.0, None) == -1
        assert n12(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), y, uv, pitch, fs, M, F, 4, 8, 8, 0.0, 0, 0, None) == -1
        assert crop(_p(im), 16, 4, _p(w4), _p(fo), _p(out), M, F, 3, 4, 4, 1, 1, None) == -1
        assert ncrop(y, uv, pitch, fs, 8, 8, _p(w4), _p(w4), _p(fo), _p(fo), _p(out), M, F, 4, 4, 0, 0, None) == -1
    assert rgb8(None, None, _p(w4), _p(w4), _p(fo), _p(fo), _p(fr), 1, 1, 4, 8, 8, 0.0, None) == -1
    assert rgb8(_p(im), None, None, _p(w4), _p(fo), _p(fo), _p(fr), 1, 1, 4, 8, 8, 0.0, None) == -1
    assert rgb8(_p(im), None, _p(w4), _p(w4), None, _p(fo), _p(fr), 1, 1, 4, 8, 8, 0.0, None) == -1
    assert rgb8(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), None, 1, 1, 4, 8, 8, 0.0, None) == -1
    assert n12(_p(im), None, _p(w4), _p(w4), None, _p(fo), y, uv, pitch, fs, 1, 1, 4, 8, 8, 0.0, 0, 0, None) == -1
    assert n12(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), y, uv, pitch, fs, 1, 1, 4, 8, 8, 0.0, 2, 0, None) == -1
    assert crop(_p(im), 16, 4, _p(w4), None, _p(out), 1, 1, 3, 4, 4, 1, 1, None) == -1
    assert ncrop(y, uv, pitch, fs, 8, 8, _p(w4), _p(w4), None, None, _p(out), 1, 1, 4, 4, 0, 0, None) == -1
    # M == 0 is fine and launches nothing
    assert rgb8(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), _p(fr), 0, 1, 4, 8, 8, 0.0, None) == 0
    assert n12(_p(im), None, _p(w4), _p(w4), _p(fo), _p(fo), y, uv, pitch, fs, 0, 1, 4, 8, 8, 0.0, 0, 0, None) == 0
    assert crop(_p(im), 16, 4, _p(w4), _p(fo), _p(out), 0, 1, 3, 4, 4, 1, 1, None) == 0
    assert ncrop(y, uv, pitch, fs, 8, 8, _p(w4), _p(w4), _p(fo), _p(fo), _p(out), 0, 1, 4, 4, 0, 0, None) == 0
    assert not fr.any() and not nv.any() and not out.any()


def test_the_faces_entry_points_are_in_the_abi_table():
    from emoportraits_amd import hip, _abi_version
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert _abi_version.EMO_ABI_VERSION >= 18
    for name, n_args in zip(NEW, (14, 18, 14, 19)):
        assert f"int {name}(" in hdr and len(hip.SIGNATURES[name]) == n_args


# ---- host helpers --------------------------------------------------------------------------------------------------------------
def test_flatten_faces_and_face_spans():
    from emoportraits_amd import frames as F
    flat, counts = F.flatten_faces(R.FACES)
    assert flat == [(x, y, s, s) for x, y, s in R.WINDOWS] and counts == [2, 0, 3, 1]
    assert F.flatten_faces([]) == ([], []) and F.flatten_faces([[], []]) == ([], [0, 0])
    with pytest.raises(ValueError, match="side"):
        F.flatten_faces([[(0, 0, 8, 9)]])
    assert F.face_spans([2, 0, 3, 1], 0, 4, 4) == [(0, 2), (2, 4)]               # (the module docstring: the rule, not the example)
    assert F.face_spans([2, 0, 3, 1], 0, 4, 3) == [(0, 2), (2, 3), (3, 4)]
    assert F.face_spans([2, 0, 3, 1], 1, 3, 4) == [(1, 3)] and F.face_spans([2, 0, 3, 1], 2, 2, 4) == []
    assert F.face_spans([2] * 6, 0, 6, 4) == [(0, 2), (2, 4), (4, 6)]             # a regular clip: batches of one shape
    with pytest.raises(ValueError, match="faces"):
        F.face_spans([1, 5, 1], 0, 3, 4)
    spans = F.face_spans([0] * 10, 0, 10, 4)
    assert spans == [(0, 4), (4, 8), (8, 10)]
    assert F.face_spans([4, 4, 0, 1], 0, 4, 4) == [(0, 1), (1, 3), (3, 4)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), EMO_PIN_CORES="0")
    sys.path.insert(0, ROOT)
    from emoportraits_amd import parallel
    torch.distributed.init_process_group(backend="gloo", init_method="env://")
    rows = torch.arange(7 * 16, dtype=torch.float32).view(7, 4, 4)
    ok = True
    for counts in ([5, 2], [0, 7], [7, 0]):
        lo = sum(counts[:rank])
        ok = ok and torch.equal(parallel.gather_rows(rows[lo:lo + counts[rank]].clone(), counts, rank, world), rows)
    q.put((rank, ok))
    torch.distributed.destroy_process_group()


def test_gather_rows():
    from emoportraits_amd import parallel
    assert torch.equal(parallel.gather_rows(torch.ones(5, 2), [5], 0, 1), torch.ones(5, 2))
    assert parallel.gather_rows(torch.ones(0, 4, 4), [0], 0, 1).shape == (0, 4, 4)
    with pytest.raises(ValueError, match="its count"):
        parallel.gather_rows(torch.ones(4, 2), [5], 0, 1)
    with pytest.raises(ValueError, match="ranks"):
        parallel.gather_rows(torch.ones(4, 2), [4, 1], 0, 1)
    with pytest.raises(RuntimeError, match="process group"):
        parallel.gather_rows(torch.ones(3, 2), [3, 2], 0, 2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, True), (1, True)]


# ---- host logic on CPU tensors ---------------------------------------------------------------------------------------------
@pytest.fixture()
def wrapper(monkeypatch, lib):
    """an InferenceWrapper on CPU tensors: the library the host-compiled one, the networks stand-ins (the driver pass a seeded
    image per call), the upload a plain copy, the byte -> fp32 unpacking (an op that insists on device memory) torch's"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import hip, ops
    from emoportraits_amd.infer import InferenceWrapper
    facade = _Lib(lib)
    monkeypatch.setattr(hip, "load", lambda: facade)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    monkeypatch.setattr(ops, "unpack_rgb8", lambda u8: (u8.permute(0, 3, 1, 2).float() / 255).contiguous())
    w = object.__new__(InferenceWrapper)
    w.uploads = []

    def uploaded(chunk, spans, device, stream):
        for a, b in spans:
            w.uploads.append((a, b))
            yield a, b, chunk[a:b].clone()
    monkeypatch.setattr(frames_mod, "uploaded", uploaded)
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
        g = torch.Generator().manual_seed(40 + len(w.driven))
        w.driven.append(torch.rand(pose.shape[0], 3, R.S, R.S, generator=g) * 1.2 - 0.1)
        return w.driven[-1].clone()
    w._head_pose = head_pose
    w._expression = lambda crops, theta, what: (torch.zeros(crops.shape[0], 4), None)
    w._drive = drive
    return w


def test_ops_take_frame_of_on_cpu_tensors(wrapper, lib, rgb, nv12):
    from emoportraits_amd import ops
    sq = [(x, y, s, s) for x, y, s in R.WINDOWS]
    frames, img, matte = rgb["smooth"]
    rc, want = paste_rgb(lib, frames, img, matte, R.WINDOWS, 0.0625, R.FRAME_OF)
    work = frames.clone()
    assert ops.paste_windows(work, img, sq, 0.0625, matte, frame_of=R.FRAME_OF) is work and torch.equal(work, want)
    x = ops.unpack_rgb8(frames)
    assert torch.equal(ops.resize2d_windows(x, (R.S, R.S), sq, "bicubic", True, frame_of=R.FRAME_OF),
                       ops.resize2d_windows(x[R.FRAME_OF].contiguous(), (R.S, R.S), sq, "bicubic", True))
    nv, img, matte = nv12["smooth"]
    rc, want = paste_nv12(lib, nv, img, matte, R.WINDOWS, 0.0625, R.FRAME_OF)
    work = nv.clone()
    assert ops.paste_windows_nv12(work, img, sq, 0.0625, matte, *MODE, frame_of=R.FRAME_OF) is work and torch.equal(work, want)
    assert torch.equal(ops.nv12_windows(nv, (R.S, R.S), sq, *MODE, frame_of=R.FRAME_OF),
                       ops.nv12_windows(nv[R.FRAME_OF].contiguous(), (R.S, R.S), sq, *MODE))
    assert wrapper.lib.calls == {"emo_paste_faces_rgb8": 1, "emo_resize2d_faces_f32": 1, "emo_resize2d_windows_f32": 1,
                                 "emo_paste_yuv420": 1, "emo_yuv420_crop_f32": 2}
    assert wrapper.lib.forms == {"emo_paste_yuv420": ["faces"], "emo_yuv420_crop_f32": ["faces", "windows"]}
    # no face at all: nothing to launch
    assert ops.paste_windows(work[:0].reshape(0, 1, 1, 3), img[:0], [], frame_of=[]).shape[0] == 0
    assert ops.nv12_windows(nv, (R.S, R.S), [], frame_of=[]).shape == (0, 3, R.S, R.S)
    wrapper.lib.calls.clear()
    work = frames.clone()
    for fo, msg in (([0, 0, 2, 2, 1, 3], "non-decreasing"), ([0, 0, 2, 2, 2, 4], "outside"), ([-1, 0, 2, 2, 2, 3], "outside"),
                    ([0, 0, 2, 2, 2], "windows for")):
        for call in (lambda: ops.paste_windows(work, img[:len(fo)], sq, frame_of=fo), lambda: ops.resize2d_windows(x, (R.S, R.S), sq, frame_of=fo),
                     lambda: ops.paste_windows_nv12(nv.clone(), img[:len(fo)], sq, frame_of=fo), lambda: ops.nv12_windows(nv, (R.S, R.S), sq, frame_of=fo)):
            with pytest.raises(ValueError, match=msg):
                call()
    assert wrapper.lib.calls == {} and torch.equal(work, frames)


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_wrapper_paste_back_takes_faces(wrapper, lib, rgb, nv12, fmt):
    frames, img, matte = _inputs(rgb, nv12, fmt, "smooth")
    kw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    rc, want = PASTE[fmt](lib, frames, img, matte, R.WINDOWS, 0.0625, R.FRAME_OF)
    before = frames.clone()
    got = wrapper.paste_back(frames, img, faces=R.FACES, matte=matte, **kw)
    assert torch.equal(got, want) and torch.equal(frames, before) and got.data_ptr() != frames.data_ptr()
    assert wrapper.lib.calls == {RUN_NEW[fmt][1]: 1} and wrapper.lib.forms == ({} if fmt == "rgb8" else {RUN_NEW[fmt][1]: ["faces"]})
    for bad in (dict(windows=R.WINDOWS[:4], faces=R.FACES), dict(), dict(faces=R.FACES[:3])):
        with pytest.raises(ValueError, match="faces"):
            wrapper.paste_back(frames, img, **bad, **kw)


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_animate_frames_with_faces_is_paste_back_of_its_own_renders(wrapper, lib, rgb, nv12, fmt):
    """12 frames: the shared four, six without a face, one with a face, one without: batch_size 4 gives the spans (0,2) (2,6) (6,10)
    (10,12) -- one crop launch and one paste launch for each of the three that have a face, none for (6,10), whose frames come
    back as they were"""
    frames, _, matte = _inputs(rgb, nv12, fmt, "noise")
    frames = torch.cat([frames, frames, frames])
    faces = R.FACES + [[]] * 6 + [[(33, 17, 40)], []]
    kw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    w, before = wrapper, frames.clone()
    got = list(w.animate_frames(frames, batch_size=4, faces=faces, to_host=False, paste_back=True, feather=0.25,
                                paste_matte=lambda img: matte[:img.shape[0]], **kw))
    assert [b0 for b0, _ in got] == [0, 2, 6, 10] and [t.shape[0] for _, t in got] == [2, 4, 4, 2]
    crop, paste = RUN_NEW[fmt]
    assert w.lib.calls == {crop: 3, paste: 3} and w.lib.forms == ({} if fmt == "rgb8" else {crop: ["faces"] * 3, paste: ["faces"] * 3})
    assert w.uploads == [(0, 2), (2, 6), (6, 10), (10, 12)] and [c.shape[0] for c in w.crops] == [2, 4, 1]
    renders, spans = list(w.driven), [(0, 2), (2, 6), (10, 12)]
    want = frames.clone()
    for (a, b), img in zip(spans, renders):
        want[a:b] = w.paste_back(frames[a:b], img, faces=faces[a:b], feather=0.25, matte=matte[:img.shape[0]], **kw)
    out = torch.cat([t for _, t in got])
    assert torch.equal(out, want) and torch.equal(frames, before) and torch.equal(out[6:10], frames[6:10]) and not torch.equal(out, frames)
    # without paste_back: the crops of the faces, indexed by face; frames without a face yield nothing and are not uploaded
    w.lib.calls.clear()
    w.uploads.clear()
    w.driven.clear()
    got = list(w.animate_frames(frames, batch_size=4, faces=faces, to_host=False, **kw))
    assert [m0 for m0, _ in got] == [0, 2, 6] and [t.shape[0] for _, t in got] == [2, 4, 1]
    assert w.uploads == spans and w.lib.calls[crop] == 3 and paste not in w.lib.calls
    assert w.lib.forms == ({} if fmt == "rgb8" else {crop: ["faces"] * 3})


def test_animate_frames_checks_its_faces_arguments_before_any_launch(wrapper, rgb):
    frames = rgb["smooth"][0]
    w = wrapper
    w.identity_capacity = 2
    many = [[(0, 0, 40)] * 5, [], [], []]
    for match, kw in (("mutually exclusive", dict(faces=R.FACES, windows=R.WINDOWS[:4])),
                      ("entries for 4 frames", dict(faces=R.FACES[:3])),
                      ("identities has 4 entries for 6 faces", dict(faces=R.FACES, identities=[0, 1, 0, 1])),
                      ("smooth_per_identity", dict(faces=R.FACES, smooth_pose=True)),
                      ("smooth_per_identity", dict(faces=R.FACES, smooth_pose=True, identities=[0, 1] * 3)),
                      ("more than batch_size", dict(faces=many, batch_size=4)),
                      ("quarter", dict(faces=[[(0, 0, 31)], [], [], []], paste_back=True)),
                      ("side", dict(faces=[[(0, 0, 40, 41)], [], [], []]))):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(frames, **kw))
    with pytest.raises(ValueError, match="run past"):
        list(w.animate_frames(iter([frames, frames]), faces=R.FACES, batch_size=4, to_host=False))
    assert w.uploads == [(0, 2), (2, 4)] and w.lib.calls.get("emo_resize2d_faces_f32") == 2     # (the first chunk ran, the second did not)
    w.lib.calls.clear()
    with pytest.raises(ValueError, match="inside"):
        next(w.animate_frames(frames, faces=[[(400, 0, 128)], [], [], []], to_host=False))
    assert w.lib.calls == {}


def _renamed(calls):
    """the call counts of a faces= run under the names of the per-frame entry points"""
    return {dict(zip(NEW, OLD)).get(name, name): n for name, n in calls.items()}


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("paste", [True, False])
@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_windows_is_faces_with_one_face_per_frame(wrapper, rgb, nv12, fmt, paste, bank):
    """animate_frames(windows=W) and animate_frames(faces=[[w] for w in W]) are one loop: equal indices, equal tensors, and the
    same launches but for the entry points' names -- the per-frame ones for windows=, the *_faces_* ones for faces= -- or, NV12, but
    for the form of the ABI 22 entry points' calls: frame_of null for windows=, given for faces=.  5 frames at
    batch_size 2: three spans, the last a tail.  With a bank: identities, mix and the per-identity smooth_pose on the way, and the
    thetas and slots the driver pass receives are equal too."""
    frames, _, matte = _inputs(rgb, nv12, fmt, "noise")
    frames, W, w = torch.cat([frames, frames[:1]]), R.WINDOWS[:5], wrapper
    kw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    kw.update(dict(paste_back=True, feather=0.25, paste_matte=lambda img: matte[:img.shape[0]]) if paste else dict(as_uint8=False))
    seen = []
    if bank:
        w.cfg.update(latent_volume_channels=4, latent_volume_depth=2, latent_volume_size=2, gen_embed_size=1, gen_max_channels=4)
        w._init_identity_bank(2)
        g = torch.Generator().manual_seed(7)
        for k in range(2):
            w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4) + 0.05 * torch.randn(4, 4, generator=g))
        w._head_pose = lambda crops: (torch.eye(4) + 0.1 * crops.mean(dim=(1, 2, 3)).reshape(-1, 1, 1) * torch.ones(4, 4),)
        w._drive_bank = lambda pose, theta, ident: (seen.append((theta.clone(), ident.clone())), w._drive(pose, theta))[1]
        kw.update(identities=[0, 1, 1, 0, 1], mix=True, smooth_pose=True, smooth_per_identity=True)
    runs = []
    for how in (dict(windows=W), dict(faces=[[x] for x in W])):
        w.lib.calls.clear()
        w.uploads.clear()
        w.driven.clear()
        w.reset_pose_state()
        seen.clear()
        got = [(i, t.clone()) for i, t in w.animate_frames(frames, batch_size=2, to_host=False, **how, **kw)]
        runs.append((got, dict(w.lib.calls), list(w.uploads), list(seen), {k: list(v) for k, v in w.lib.forms.items()}))
    (got_w, calls_w, up_w, seen_w, forms_w), (got_f, calls_f, up_f, seen_f, forms_f) = runs
    assert [i for i, _ in got_w] == [i for i, _ in got_f] == [0, 2, 4] and [t.shape[0] for _, t in got_w] == [2, 2, 1]
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(got_w, got_f))
    crop, pasted = RUN_OLD[fmt]
    assert calls_w[crop] == 3 and calls_w.get(pasted, 0) == (3 if paste else 0)
    assert not set(calls_w) & set(NEW) and not set(calls_f) & set(OLD) and _renamed(calls_f) == calls_w
    n_of = {crop: 3, pasted: 3} if paste else {crop: 3}                          # NV12: the form of every one of those calls
    assert forms_w == ({} if fmt == "rgb8" else {k: ["windows"] * n for k, n in n_of.items()})
    assert forms_f == ({} if fmt == "rgb8" else {k: ["faces"] * n for k, n in n_of.items()})
    # smooth_pose: the crops of the head-pose pass stay resident, and only a paste needs the frames a second time
    assert up_w == up_f == [(0, 2), (2, 4), (4, 5)] * (2 if bank and paste else 1)
    assert len(seen_w) == len(seen_f) == (3 if bank else 0)
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(seen_w, seen_f))


def test_whole_frames_at_image_size_need_no_crop_launch(wrapper):
    """windows=None and frames of image_size: the crop step is the byte -> fp32 unpacking alone"""
    w = wrapper
    clip = torch.randint(0, 256, (5, R.S, R.S, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    got = list(w.animate_frames(clip, batch_size=2, to_host=False))
    assert [i for i, _ in got] == [0, 2, 4] and w.lib.calls == {"emo_pack_rgb8": 3}
    assert torch.equal(torch.cat(w.crops), (clip.permute(0, 3, 1, 2).float() / 255))
