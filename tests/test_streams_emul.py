"""Frames of different sizes in one batch (ABI 19: emo_rgb8_faces_ragged_f32, emo_nv12_faces_ragged_f32,
emo_paste_faces_ragged_rgb8, emo_paste_faces_ragged_nv12) without a GPU: the kernels are compiled for the host from the product's
own source (tests/emul/emulibs.py, the sequential build) and run on host memory.  Nothing here has a tolerance: every comparison
is bit for bit against the ABI 18 entry points on the canvas batch of tests/streams_reference.py, whose premise is asserted on
those entry points first; -ffp-contract=off makes the equality exact.
  * the shared small case: four frames of different (rgb8: odd) sizes, six faces -- crops and pastes, rgb8 and NV12, the feather
    and matte cases of paste_back_reference.CASES, host and device-only windows, packed frames and row-pitch views at odd
    addresses (the padding stays untouched);
  * a device-only window that fits the canvas but not ITS OWN frame is absent; a device-side frame_of outside [0, F) too;
  * M == 0; refusals with nothing written; the ABI table;
  * ops.frame_table / crop_faces_mixed / paste_faces_mixed: the checks that stand between a caller and a raw address;
  * frames.interleave and the batching rule on unequal stream lengths; the arena upload (one batch ahead) and the byte ring with
    stand-in streams; InferenceWrapper.animate_streams on CPU tensors against
    animate_frames(canvas clip, faces=), the launches counted: one crop and at most one paste per batch, no emo_unpack_rgb8."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
from counting_lib import CountingLib as _Lib  # noqa: E402
import emulibs  # noqa: E402
import nv12_reference as NV  # noqa: E402
import paste_back_reference as PB  # noqa: E402
import streams_reference as R  # noqa: E402

NEW = ("emo_rgb8_faces_ragged_f32", "emo_nv12_faces_ragged_f32", "emo_paste_faces_ragged_rgb8", "emo_paste_faces_ragged_nv12")
OLD = ("emo_unpack_rgb8", "emo_resize2d_faces_f32", "emo_nv12_faces_f32", "emo_paste_faces_rgb8", "emo_paste_faces_nv12")
# what the Python layer launches for a mixed batch: rgb8 the ABI 19 entry points above, NV12 the ABI 22 ones with layout 0
RUN = {"rgb8": (NEW[0], NEW[2]), "nv12": ("emo_yuv420_crop_ragged_f32", "emo_paste_ragged_yuv420")}
MODE = ("bt601", True)                                   # (colorspace, full_range) of the NV12 cases
MATRIX = (NV.MATRIX_ID[MODE[0]], int(MODE[1]))
FMTS = ["rgb8", "nv12"]


@pytest.fixture(scope="module")
def raw():
    lib = emulibs.stream(False)
    for name in NEW + OLD + RUN["nv12"]:
        assert hasattr(lib, name), f"the host build of csrc does not export {name}"
    return lib


@pytest.fixture()
def lib(monkeypatch, raw):
    """emoportraits_amd.ops on CPU tensors, served by the host-compiled library"""
    from emoportraits_amd import hip
    facade = _Lib(raw)
    monkeypatch.setattr(hip, "load", lambda: facade)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    return facade


@pytest.fixture(scope="module")
def inputs():
    """{fmt: (frames, img, matte by kind)}: random frame bytes, the images and mattes of paste_back_reference (six rows)"""
    out = {}
    for fmt in FMTS:
        R.check_case(fmt)
        out[fmt] = (R.random_frames(R.SIZES[fmt], fmt, 7), {k: v[1:] for k, v in PB.small_inputs().items()})
    return out


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sq(wins):
    return [(w[0], w[1], w[2], w[3] if len(w) > 3 else w[2]) for w in wins]


def _w4(wins):
    return torch.tensor(_sq(wins), dtype=torch.int32).reshape(-1, 4)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32)


def _table(frames, fmt):
    rows = []
    for f in frames:
        h, w = R.frame_size(f, fmt)
        rows.append((f.data_ptr(), f.stride(0), h, w))
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)


def pitched(frames, fmt, pad=5):
    """the same frames as row-pitch views (pitch = row bytes + pad) that start 1, 2, 3, ... bytes into their buffers
    -> (views, buffers, bool masks of the buffers' bytes that belong to no frame)"""
    views, bufs, outside = [], [], []
    for i, f in enumerate(frames):
        rows, row_bytes = f.shape[0], f[0].numel()
        pitch, off = row_bytes + pad, 1 + i % 3
        buf = torch.randint(0, 256, (off + rows * pitch,), generator=torch.Generator().manual_seed(50 + i), dtype=torch.uint8)
        size, stride = (tuple(f.shape), (pitch, 3, 1)) if fmt == "rgb8" else (tuple(f.shape), (pitch, 1))
        v = torch.as_strided(buf, size, stride, off)
        v.copy_(f)
        mask = torch.ones_like(buf, dtype=torch.bool)
        torch.as_strided(mask, size, stride, off)[...] = False
        views.append(v)
        bufs.append(buf)
        outside.append(mask)
    return views, bufs, outside


# ---- the mixed entry points and the parent's, on host memory -------------------------------------------------------------------
def mixed_crop(lib, fmt, frames, wins, frame_of, host=True, dev_frame_of=None, F=None):
    tab, w4, fo = _table(frames, fmt), _w4(wins), _i32(frame_of)
    fd = fo if dev_frame_of is None else _i32(dev_frame_of)
    out = torch.full((len(wins), 3, R.S, R.S), -7.0)
    args = (_p(tab), _p(tab), _p(w4), _p(w4) if host else None, _p(fd), _p(fo), _p(out), len(wins), F or len(frames), R.S, R.S)
    if fmt == "rgb8":
        rc = lib.emo_rgb8_faces_ragged_f32(*args, None)
    else:
        rc = lib.emo_nv12_faces_ragged_f32(*args, *MATRIX, None)
    return rc, out


def mixed_paste(lib, fmt, frames, img, matte, wins, frame_of, feather=0.0, host=True, dev_frame_of=None):
    """on the frames themselves, in place -> return code"""
    tab, w4, fo = _table(frames, fmt), _w4(wins), _i32(frame_of)
    fd = fo if dev_frame_of is None else _i32(dev_frame_of)
    args = (_p(img), _p(matte), _p(tab), _p(tab), _p(w4), _p(w4) if host else None, _p(fd), _p(fo), len(wins), len(frames),
            img.shape[-1], feather)
    if fmt == "rgb8":
        return lib.emo_paste_faces_ragged_rgb8(*args, None)
    return lib.emo_paste_faces_ragged_nv12(*args, *MATRIX, None)


def canvas_crop(lib, fmt, canvas, wins, frame_of):
    """the parent: emo_unpack_rgb8 + emo_resize2d_faces_f32(bicubic, clamp01), or emo_nv12_faces_f32"""
    w4, fo = _w4(wins), _i32(frame_of)
    out = torch.full((len(wins), 3, R.S, R.S), -7.0)
    if fmt == "rgb8":
        F, H, W, _ = canvas.shape
        x = torch.empty((F, 3, H, W))
        assert lib.emo_unpack_rgb8(_p(canvas), _p(x), F, H, W, None) == 0
        rc = lib.emo_resize2d_faces_f32(_p(x), H * W, W, _p(w4), _p(fo), _p(out), len(wins), F, 3, R.S, R.S, 1, 1, None)
    else:
        F, rows, W = canvas.shape
        H = rows // 3 * 2
        y, uv = ctypes.c_void_p(canvas.data_ptr()), ctypes.c_void_p(canvas.data_ptr() + H * W)
        rc = lib.emo_nv12_faces_f32(y, uv, W, rows * W, H, W, _p(w4), _p(w4), _p(fo), _p(fo), _p(out), len(wins), F, R.S, R.S, *MATRIX, None)
    assert rc == 0
    return out


def canvas_paste(lib, fmt, canvas, img, matte, wins, frame_of, feather=0.0):
    buf, w4, fo = canvas.clone(), _w4(wins), _i32(frame_of)
    if fmt == "rgb8":
        F, H, W, _ = buf.shape
        rc = lib.emo_paste_faces_rgb8(_p(img), _p(matte), _p(w4), _p(w4), _p(fo), _p(fo), _p(buf), len(wins), F, img.shape[-1], H, W, feather, None)
    else:
        F, rows, W = buf.shape
        H = rows // 3 * 2
        y, uv = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + H * W)
        rc = lib.emo_paste_faces_nv12(_p(img), _p(matte), _p(w4), _p(w4), _p(fo), _p(fo), y, uv, W, rows * W, len(wins), F, img.shape[-1],
                                      H, W, feather, *MATRIX, None)
    assert rc == 0
    return buf


def _equal_lists(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the premise, crops, pastes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_the_canvas_bytes_outside_the_regions_do_not_change_the_parents_result(lib, inputs, fmt):
    frames, by_kind = inputs[fmt]
    img, matte = by_kind["noise"]
    wins = R.windows(fmt)
    R.check_premise(frames, fmt, lambda c: canvas_crop(lib, fmt, c, wins, R.FRAME_OF),
                    lambda c: canvas_paste(lib, fmt, c, img, matte, wins, R.FRAME_OF, 0.0625))


@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_crops_are_the_canvas_crops(lib, inputs, fmt):
    frames, _ = inputs[fmt]
    wins = R.windows(fmt)
    want = canvas_crop(lib, fmt, R.canvas(frames, fmt, 1), wins, R.FRAME_OF)
    assert bool(want.any()) and ("emo_unpack_rgb8" in lib.calls) == (fmt == "rgb8")
    lib.calls.clear()
    before = [f.clone() for f in frames]
    for host in (True, False):
        rc, got = mixed_crop(lib, fmt, frames, wins, R.FRAME_OF, host)
        assert rc == 0 and torch.equal(got, want)
    views, bufs, _ = pitched(frames, fmt)
    kept = [b.clone() for b in bufs]
    rc, got = mixed_crop(lib, fmt, views, wins, R.FRAME_OF)
    assert rc == 0 and torch.equal(got, want)
    assert _equal_lists(frames, before) and _equal_lists(bufs, kept) and "emo_unpack_rgb8" not in lib.calls


@pytest.mark.parametrize("feather,use_matte", PB.CASES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_paste_is_the_canvas_paste(lib, inputs, fmt, kind, feather, use_matte):
    frames, by_kind = inputs[fmt]
    img, matte = by_kind[kind]
    m = matte if use_matte else None
    wins, sizes = R.windows(fmt), R.SIZES[fmt]
    want = R.regions(canvas_paste(lib, fmt, R.canvas(frames, fmt, 2), img, m, wins, R.FRAME_OF, feather), sizes, fmt)
    for host in (True, False):                                                   # (device-only windows: the grid covers any side)
        work = [f.clone() for f in frames]
        assert mixed_paste(lib, fmt, work, img, m, wins, R.FRAME_OF, feather, host) == 0
        assert _equal_lists(work, want)
    assert torch.equal(want[1], frames[1]) and not torch.equal(want[0], frames[0]) and not torch.equal(want[3], frames[3])
    # row-pitch views at odd addresses: the same frames, and not a byte of the padding around them
    views, bufs, outside = pitched(frames, fmt)
    kept = [b.clone() for b in bufs]
    assert mixed_paste(lib, fmt, views, img, m, wins, R.FRAME_OF, feather) == 0
    assert _equal_lists(views, want) and all(torch.equal(b[o], k[o]) for b, k, o in zip(bufs, kept, outside))


@pytest.mark.parametrize("fmt", FMTS)
def test_a_device_only_window_outside_its_own_frame_is_absent(lib, inputs, fmt):
    """the second face of frame 0 (70 x 66) replaced by a window that fits the canvas (and the other frames) but not frame 0;
    windows on the device only: the paste is that of the other five, the crop of that face zeros"""
    frames, by_kind = inputs[fmt]
    img, matte = by_kind["smooth"]
    wins, sizes = R.windows(fmt), R.SIZES[fmt]
    bad = wins[:1] + [R.OUTSIDE_ITS_FRAME] + wins[2:]
    keep = [0, 2, 3, 4, 5]
    canvas = R.canvas(frames, fmt, 3)
    want = R.regions(canvas_paste(lib, fmt, canvas, img[keep], matte[keep], [wins[i] for i in keep], [R.FRAME_OF[i] for i in keep], 0.0625),
                     sizes, fmt)
    work = [f.clone() for f in frames]
    assert mixed_paste(lib, fmt, work, img, matte, bad, R.FRAME_OF, 0.0625, host=False) == 0 and _equal_lists(work, want)
    for other in ((21, 17, 45, 44), (21, 17, 31), (-1, 17, 45), (21, 17, 0)):    # not square, too small, negative, empty
        work = [f.clone() for f in frames]
        assert mixed_paste(lib, fmt, work, img, matte, wins[:1] + [other] + wins[2:], R.FRAME_OF, 0.0625, host=False) == 0
        assert _equal_lists(work, want), other
    crops = canvas_crop(lib, fmt, canvas, wins, R.FRAME_OF)
    rc, got = mixed_crop(lib, fmt, frames, bad, R.FRAME_OF, host=False)
    assert rc == 0 and not got[1].any() and torch.equal(got[keep], crops[keep])
    # a device-side frame_of outside [0, F): that face is absent / zeros
    keep = [0, 1, 2, 3, 4]
    want = R.regions(canvas_paste(lib, fmt, canvas, img[keep], matte[keep], wins[:5], R.FRAME_OF[:5], 0.0625), sizes, fmt)
    work = [f.clone() for f in frames]
    assert mixed_paste(lib, fmt, work, img, matte, wins, R.FRAME_OF, 0.0625, dev_frame_of=[0, 0, 2, 3, 3, 4]) == 0
    assert _equal_lists(work, want)
    rc, got = mixed_crop(lib, fmt, frames, wins, R.FRAME_OF, dev_frame_of=[0, 0, 2, 3, 3, 4])
    assert rc == 0 and not got[5].any() and torch.equal(got[:5], crops[:5])


# ---- refusals, M == 0, the ABI table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_refusals_write_nothing_and_no_face_is_no_launch(lib, inputs, fmt):
    frames, by_kind = inputs[fmt]
    img, matte = by_kind["noise"]
    W = R.windows(fmt)

    def refused(code, wins=W, frame_of=R.FRAME_OF, feather=0.0625, frames=frames):
        work = [f.clone() for f in frames]
        rc = mixed_paste(lib, fmt, work, img[:len(wins)], matte[:len(wins)], wins, frame_of, feather)
        assert rc == code and _equal_lists(work, frames), (wins, frame_of, feather, rc)
        rc, out = mixed_crop(lib, fmt, work, wins, frame_of)
        crop_code = 0 if code == -2 or feather != 0.0625 else code              # (what only a paste refuses)
        assert rc == crop_code and (crop_code == 0 or bool((out == -7.0).all())), (wins, frame_of, rc)
    refused(-1, frame_of=[0, 0, 2, 3, 1, 3])                                    # decreases
    refused(-1, frame_of=[0, 0, 2, 3, 3, 4])                                    # leaves [0, F)
    refused(-1, frame_of=[-1, 0, 2, 3, 3, 3])
    refused(-1, wins=W[:1] + [R.OUTSIDE_ITS_FRAME] + W[2:])                      # inside the canvas, outside ITS frame
    refused(-1, wins=W[:2] + [(1, 0, 64)] + W[3:])
    refused(-1, wins=[(-1, 3, 40)] + W[1:])
    refused(-1, wins=[(1, 3, 0)] + W[1:])
    refused(-2, wins=[(1, 3, 40, 41)] + W[1:])                                  # not square
    refused(-2, wins=[(1, 3, 31)] + W[1:])                                      # 4 * 31 < 128
    for feather in (-0.01, 0.51, float("nan")):
        refused(-1, feather=feather)
    # the table: a pitch shorter than a row, a null address, an empty or (NV12) odd frame
    tab, w4, fo, out = _table(frames, fmt), _w4(W), _i32(R.FRAME_OF), torch.full((6, 3, R.S, R.S), -7.0)
    work = [f.clone() for f in frames]

    def call(table, M=6, F=4, dev=True, fo_host=True):
        t = table.clone()
        tail = () if fmt == "rgb8" else MATRIX
        crop = lib.emo_rgb8_faces_ragged_f32 if fmt == "rgb8" else lib.emo_nv12_faces_ragged_f32
        paste = lib.emo_paste_faces_ragged_rgb8 if fmt == "rgb8" else lib.emo_paste_faces_ragged_nv12
        a = crop(_p(t) if dev else None, _p(t), _p(w4), _p(w4), _p(fo), _p(fo) if fo_host else None, _p(out), M, F, R.S, R.S, *tail, None)
        b = paste(_p(img), _p(matte), _p(t) if dev else None, _p(t), _p(w4), _p(w4), _p(fo), _p(fo) if fo_host else None, M, F, R.S,
                  0.0625, *tail, None)
        return a, b
    tab = _table(work, fmt)
    for col, value in ((1, tab[3, 1] - 1), (0, 0), (2, 0), (3, -2)) + (((2, tab[3, 2] + 1), (3, tab[3, 3] - 1)) if fmt == "nv12" else ()):
        bad = tab.clone()
        bad[3, col] = value
        assert call(bad) == (-1, -1), (col, value)
    assert call(tab, M=-1) == (-1, -1) and call(tab, F=0) == (-1, -1) and call(tab, F=-2) == (-1, -1)
    assert call(tab, dev=False) == (-1, -1) and call(tab, fo_host=False) == (-1, -1)
    assert call(tab, M=0) == (0, 0)                                             # fine, and launches nothing
    assert _equal_lists(work, frames) and bool((out == -7.0).all())
    assert call(tab) == (0, 0) and not _equal_lists(work, frames) and not bool((out == -7.0).any())


def test_the_ragged_entry_points_are_in_the_abi_table():
    from emoportraits_amd import hip, _abi_version
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert _abi_version.EMO_ABI_VERSION >= 19 and "#define EMO_ABI_VERSION %d" % _abi_version.EMO_ABI_VERSION in hdr
    for name, n_args in zip(NEW, (12, 14, 13, 15)):
        assert f"int {name}(" in hdr and len(hip.SIGNATURES[name]) == n_args


# ---- ops -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_ops_build_the_table_from_checked_tensors_only(lib, inputs, fmt):
    from emoportraits_amd import ops
    frames, by_kind = inputs[fmt]
    img, matte = by_kind["smooth"]
    wins, sizes = _sq(R.windows(fmt)), R.SIZES[fmt]
    mode = MODE if fmt == "nv12" else ()
    dev, host = ops.frame_table(frames, fmt)
    assert torch.equal(dev, host) and torch.equal(host, _table(frames, fmt)) and host.dtype == torch.int64
    canvas = R.canvas(frames, fmt, 4)
    got = ops.crop_faces_mixed(frames, R.S, wins, R.FRAME_OF, fmt, *mode)
    assert torch.equal(got, canvas_crop(lib, fmt, canvas, wins, R.FRAME_OF))
    work = [f.clone() for f in frames]
    assert ops.paste_faces_mixed(work, img, wins, R.FRAME_OF, 0.0625, matte, fmt, *mode) is work
    assert _equal_lists(work, R.regions(canvas_paste(lib, fmt, canvas, img, matte, wins, R.FRAME_OF, 0.0625), sizes, fmt))
    views, _, _ = pitched(frames, fmt)
    assert torch.equal(ops.crop_faces_mixed(views, (R.S, R.S), wins, R.FRAME_OF, fmt, *mode), got)
    assert ops.crop_faces_mixed(frames, R.S, [], [], fmt, *mode).shape == (0, 3, R.S, R.S)
    assert ops.paste_faces_mixed(work, img[:0], [], [], 0.0, None, fmt, *mode) is work
    lib.calls.clear()
    work = [f.clone() for f in frames]
    crop = lambda fr=work, w=wins, fo=R.FRAME_OF: ops.crop_faces_mixed(fr, R.S, w, fo, fmt, *mode)
    paste = lambda fr=work, w=wins, fo=R.FRAME_OF, im=img, **kw: ops.paste_faces_mixed(fr, im, w, fo, kw.get("feather", 0.0), None, fmt, *mode)
    bad_win = wins[:1] + [_sq([R.OUTSIDE_ITS_FRAME])[0]] + wins[2:]
    geometry = RuntimeError if fmt == "rgb8" else ValueError                     # a YUV 4:2:0 frame's dtype, stride or pitch: ValueError
    for call in (crop, paste):
        for kw, err, msg in ((dict(w=bad_win), ValueError, "its own frame"), (dict(fo=[0, 0, 2, 3, 1, 3]), ValueError, "non-decreasing"),
                             (dict(fo=[0, 0, 2, 3, 3, 4]), ValueError, "outside"), (dict(w=wins[:5]), ValueError, "windows for"),
                             (dict(fr=[]), ValueError, "non-empty list"), (dict(fr=torch.zeros(4, 8, 8, 3, dtype=torch.uint8)), ValueError, "list"),
                             (dict(fr=work[:3] + [work[3].float()]), geometry, "uint8"),
                             (dict(fr=work[:3] + [work[3][None]]), ValueError, "expected"),
                             (dict(fr=work[:3] + [work[3][:, ::2]]), (RuntimeError, ValueError), "stride|expected"),
                             (dict(fr=work[:3] + [torch.as_strided(work[3], work[3].shape, (1,) + work[3].stride()[1:])]), geometry, "pitch")):
            with pytest.raises(err, match=msg):
                call(**kw)
    for kw, msg in ((dict(w=[(1, 3, 40, 41)] + wins[1:]), "square"), (dict(w=[(1, 3, 31, 31)] + wins[1:]), "quarter"),
                    (dict(feather=0.6), "feather"), (dict(im=img[:5]), "frame_of")):
        with pytest.raises(ValueError, match=msg):
            paste(**kw)
    if fmt == "nv12":
        with pytest.raises(ValueError, match="even"):
            crop(fr=work[:3] + [work[3][:, :149]])
    assert lib.calls == {} and _equal_lists(work, frames)
    assert not hasattr(ops, "crop_faces_table") and "table" not in ops.crop_faces_mixed.__code__.co_varnames[:7]


# ---- the order of the frames and the batches -----------------------------------------------------------------------------------
def test_interleave_and_the_batches_of_unequal_streams():
    from emoportraits_amd import frames as F
    assert F.interleave([3, 1, 2]) == [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2)]
    assert F.interleave([]) == [] and F.interleave([0, 2]) == [(1, 0), (1, 1)]
    # three streams of 3, 1 and 2 frames with 1, 2 and (0, 3) faces per frame: the counts in tick order, then face_spans' rule
    per_stream = [[1, 1, 1], [2], [0, 3]]
    counts = [per_stream[s][t] for s, t in F.interleave([3, 1, 2])]
    assert counts == [1, 2, 0, 1, 3, 1]
    assert F.face_spans(counts, 0, 6, 4) == [(0, 4), (4, 6)] and F.face_spans(counts, 0, 6, 3) == [(0, 3), (3, 4), (4, 5), (5, 6)]
    assert F.face_spans(counts, 0, 6, 16) == [(0, 6)] and F.face_spans([1] * 6, 0, 6, 4) == [(0, 4), (4, 6)]
    with pytest.raises(ValueError, match="faces"):
        F.face_spans(counts, 0, 6, 2)
    offsets, total = F.arena_layout([(70, 66, 3), (3, 5), (64, 64, 3)])
    assert offsets == [0, 14080, 14336] and total == 14336 + 64 * 64 * 3         # (13860 and 15 bytes, each rounded up to 256)
    assert all(o % F.ARENA_ALIGN == 0 for o in offsets) and total >= offsets[2] + 64 * 64 * 3
    buf = torch.arange(total, dtype=torch.int64).to(torch.uint8)
    views = F.arena_views(buf, [(70, 66, 3), (3, 5), (64, 64, 3)], offsets)
    assert [tuple(v.shape) for v in views] == [(70, 66, 3), (3, 5), (64, 64, 3)] and all(v.data_ptr() == buf.data_ptr() + o for v, o in zip(views, offsets))


def test_the_arena_upload_runs_one_batch_ahead_and_the_byte_ring_grows(monkeypatch):
    """frames.uploaded_mixed and frames.ArenaRing themselves, the streams, events and pinned memory replaced by stand-ins: batch
    i + 1 is taken (its copies enqueued) before batch i is handed out, every frame sits at its aligned offset of one buffer, and
    a batch that needs more bytes than the ring's slots hold drains the ring and re-makes it"""
    import contextlib
    from emoportraits_amd import frames as F

    class Event:
        def record(self, stream=None):
            pass

        def synchronize(self):
            pass

    class Stream:
        def wait_event(self, event):
            pass

        def wait_stream(self, stream):
            pass
    empty = torch.empty
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: Stream())
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: Stream())
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: empty(*a, **{x: y for x, y in k.items() if x != "pin_memory"}))
    g = torch.Generator().manual_seed(0)
    batches = [[torch.randint(0, 256, (5, 7, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (6, 4), generator=g, dtype=torch.uint8)],
               [torch.randint(0, 256, (9, 2, 3), generator=g, dtype=torch.uint8)]]
    taken = []

    def source():
        for b in batches:
            taken.append(len(taken))
            yield b
    got = [(len(taken), frames, arena) for frames, arena in F.uploaded_mixed(source(), "cpu", None, True)]
    assert [n for n, _, _ in got] == [2, 2] and [a.numel() for _, _, a in got] == [512, 256]
    for (_, frames, arena), batch in zip(got, batches):
        assert _equal_lists(frames, batch)
        assert [f.data_ptr() - arena.data_ptr() for f in frames] == F.arena_layout([f.shape for f in batch])[0]
    ring, out = F.ArenaRing("cpu", 2), []
    for k, n in enumerate((300, 200, 700, 100, 50)):
        out += [(tag, buf.numel(), int(buf[0]), int(buf[-1])) for tag, buf in ring.push(k, torch.full((n,), k, dtype=torch.uint8))]
    out += [(tag, buf.numel(), int(buf[0]), int(buf[-1])) for tag, buf in ring.drain()]
    assert out == [(k, n, k, k) for k, n in enumerate((300, 200, 700, 100, 50))] and [s.numel() for s in ring.slots] == [700, 700]


# ---- the wrapper on CPU tensors ------------------------------------------------------------------------------------------------
@pytest.fixture()
def wrapper(monkeypatch, lib):
    """an InferenceWrapper on CPU tensors: the library the host-compiled one, the networks stand-ins (the driver pass a seeded
    image per call), the uploads plain copies (into an arena for the mixed path), the uniform path's byte -> fp32 unpacking torch's"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import ops
    from emoportraits_amd.infer import InferenceWrapper
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    monkeypatch.setattr(ops, "unpack_rgb8", lambda u8: (u8.permute(0, 3, 1, 2).float() / 255).contiguous())
    w = object.__new__(InferenceWrapper)
    w.uploads = []

    def uploaded(chunk, spans, device, stream):
        for a, b in spans:
            yield a, b, chunk[a:b].clone()

    def uploaded_mixed(batches, device, stream, copy_all):
        for batch in batches:
            shapes = [tuple(f.shape) for f in batch]
            offsets, total = frames_mod.arena_layout(shapes)
            arena = torch.zeros(total, dtype=torch.uint8)
            views = frames_mod.arena_views(arena, shapes, offsets)
            for v, f in zip(views, batch):
                v.copy_(f)
            w.uploads.append(shapes)
            yield views, arena
    monkeypatch.setattr(frames_mod, "uploaded", uploaded)
    monkeypatch.setattr(frames_mod, "uploaded_mixed", uploaded_mixed)
    w.device, w.rank, w.world = torch.device("cpu"), 0, 1
    w.cfg = dict(image_size=R.S)
    w._init_state(use_graphs=False)
    w.embedders = {}
    w._canonical_cl = torch.zeros(1)
    w.lib = lib
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


def _streams(fmt, seed=60):
    """three streams of 3, 1 and 2 frames in three sizes; 'windows' for the first, 'faces' (0 ... 2 per frame) for the others"""
    sizes = R.SIZES[fmt]
    g = torch.Generator().manual_seed(seed)
    clip = lambda n, hw: torch.randint(0, 256, (n,) + R.frame_shape(hw, fmt), generator=g, dtype=torch.uint8)
    return [dict(frames=clip(3, sizes[0]), windows=[(1, 3, 40), (21, 17, 45), (0, 0, 64)]),
            dict(frames=clip(1, sizes[3]), faces=[[(7, 11, 32), (60, 100, 63)]]),
            dict(frames=iter([clip(1, sizes[1]), clip(1, sizes[1])]), faces=[[], [(33, 5, 64), (2, 2, 33)]])]


def _canvas_clip(streams, fmt, frames_of):
    """the same frames in tick order on a canvas, with faces= per frame"""
    from emoportraits_amd import frames as F
    order = F.interleave([len(st.get("windows", st.get("faces"))) for st in streams])
    faces = [[st["windows"][t]] if "windows" in st else st["faces"][t] for st, t in ((streams[s], t) for s, t in order)]
    return order, R.canvas([frames_of[s][t] for s, t in order], fmt, 5), faces


@pytest.mark.parametrize("fmt", FMTS)
def test_animate_streams_is_animate_frames_of_the_canvas_clip(wrapper, fmt):
    w = wrapper
    kw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    streams = _streams(fmt)
    frames_of = [st["frames"] if isinstance(st["frames"], torch.Tensor) else torch.cat(list(_streams(fmt)[k]["frames"])) for k, st in enumerate(streams)]
    before = [f.clone() for f in frames_of]
    order, canvas, faces = _canvas_clip(streams, fmt, frames_of)
    assert order == [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2)] and [len(f) for f in faces] == [1, 2, 0, 1, 2, 1]
    matte = lambda img: img.mean(dim=1, keepdim=True).clamp(0, 1)
    paste = dict(batch_size=4, to_host=False, paste_back=True, feather=0.25, paste_matte=matte, **kw)
    want = torch.cat([t for _, t in w.animate_frames(canvas, faces=faces, **paste)])
    parent_calls, n_driven = dict(w.lib.calls), len(w.driven)
    assert all(form == "faces" for forms in w.lib.forms.values() for form in forms) and (len(w.lib.forms) == 2) == (fmt == "nv12")
    w.lib.calls.clear()
    w.driven.clear()
    w.crops.clear()
    got = list(w.animate_streams(streams, **paste))
    assert [[(s, t) for s, t, _ in batch] for batch in got] == [order[:4], order[4:]] and len(w.driven) == n_driven == 2
    flat = [item for batch in got for item in batch]
    for i, (s, t, out) in enumerate(flat):
        hw = R.frame_size(frames_of[s][t], fmt)
        assert tuple(out.shape) == tuple(frames_of[s][t].shape) and torch.equal(out, R.region(want[i], hw, fmt)), (s, t)
    assert torch.equal(flat[2][2], frames_of[2][0]) and not torch.equal(flat[0][2], frames_of[0][0])   # (no face: as it went in)
    crop, pst = RUN[fmt]
    assert w.lib.calls == {crop: 2, pst: 2} and sum(parent_calls.values()) == 4
    assert _equal_lists(frames_of, before) and len(w.uploads) == 2
    # crops out: frames without a face are left out; the rows are the parent's crops of the canvas clip, split by frame
    w.lib.calls.clear()
    w.driven.clear()
    crops_kw = dict(batch_size=4, to_host=False, as_uint8=False, **kw)
    want = torch.cat([t for _, t in w.animate_frames(canvas, faces=faces, **crops_kw)])
    w.lib.calls.clear()
    w.driven.clear()
    got = [item for batch in w.animate_streams(_streams(fmt), **crops_kw) for item in batch]
    assert [(s, t, o.shape[0]) for s, t, o in got] == [(0, 0, 1), (1, 0, 2), (0, 1, 1), (2, 1, 2), (0, 2, 1)]
    assert torch.equal(torch.cat([o for _, _, o in got]), want) and w.lib.calls == {crop: 2}


def test_animate_streams_checks_its_arguments_before_any_launch(wrapper):
    w = wrapper
    w.identity_capacity = 2
    ok = lambda: _streams("rgb8")
    s = ok()
    for match, streams, kw in (("either", [dict(frames=s[0]["frames"])], {}),
                               ("either", [dict(s[0], faces=[[]] * 3)], {}),
                               ("for 3 frames", [dict(s[0], windows=s[0]["windows"][:2])], {}),
                               ("one slot, or one per face", [dict(s[0], identities=[0, 1])], {}),
                               ("every stream or in none", [dict(s[0], identities=0), s[1]], {}),
                               ("identities", ok(), dict(smooth_pose=True)),
                               ("more than batch_size", ok(), dict(batch_size=1)),
                               ("quarter", [dict(s[0], windows=[(1, 3, 31)] * 3)], dict(paste_back=True)),
                               ("side", [dict(s[0], windows=[(1, 3, 40, 41)] * 3)], {}),
                               ("out_format", ok(), dict(paste_back=True, out_format="nv12")),
                               ("as_uint8", ok(), dict(as_uint8=False)),
                               ("uint8", [dict(s[0], frames=s[0]["frames"].float())], {})):
        with pytest.raises(ValueError, match=match):
            next(w.animate_streams(streams, **kw))
    with pytest.raises(ValueError, match="its own frame"):
        next(w.animate_streams([dict(s[0], windows=[(30, 10, 50)] * 3)], to_host=False))
    assert w.lib.calls == {} and w.driven == []
    short = ok()
    short[2]["frames"] = iter([short[0]["frames"][:0].reshape((0,) + tuple(R.frame_shape(R.SIZES["rgb8"][1], "rgb8")))])
    with pytest.raises(ValueError, match="stream 2 has"):
        list(w.animate_streams(short, to_host=False))
