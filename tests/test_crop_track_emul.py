"""Crop tracking on the device without a GPU: emo_crop_track_f64 (csrc/smallops.hip), compiled for the host from the product's own
source (tests/emul/emulibs.stream, the sequential and the threaded build), against the windows the reference's crop_image recorded
(tests/golden/hostglue.pt) and, bit for bit, against the host code it restates (hostglue.crop_track), which is itself held to the
already pinned hostglue.crop_window + CropTracker; then ops.crop_track and InferenceWrapper.animate_frames / animate_streams(boxes=)
on the recorder rigs of tests/test_head_pose_controls_emul.py.  Everything compared is an integer or a bit pattern: no tolerances.
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
import crop_track_cases as C  # noqa: E402
from test_head_pose_controls_emul import _bare_wrapper, _drivers, _Lib  # noqa: E402,F401

NAME = "emo_crop_track_f64"
V, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = [V] * 3 + [I, I] + [V] * 3 + [I, I, D, D, I, I, D, I, I, I] + [V] * 4


@pytest.fixture(scope="module", params=[False, True], ids=["loop", "threads"])
def stream(request):
    import emulibs
    return emulibs.stream(request.param)


@pytest.fixture(scope="module")
def glue():
    return torch.load(os.path.join(HERE, "golden", "hostglue.pt"), weights_only=False)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def raw(lib, boxes, so, sizes, Wf, Hf, state, has, last, M, K, m, om, smooth, fixed, scale, box_format, hold, min_side, crop, paste, fs):
    fn = lib.emo_crop_track_f64
    fn.argtypes, fn.restype = ARGTYPES, ctypes.c_int
    return fn(_p(boxes), _p(so), _p(sizes), Wf, Hf, _p(state), _p(has), _p(last), M, K, m, om, int(smooth), int(fixed), scale, box_format,
              int(hold), min_side, _p(crop), _p(paste), _p(fs), None)


def kernel(lib, boxes, so, size, st, K, momentum=0.01, smooth=False, fixed=False, scale=1.0, box_format="xyxy", missing="skip", min_side=2):
    """one call of the entry point on numpy arrays, the outputs pre-filled with a pattern the kernel must overwrite"""
    boxes = np.ascontiguousarray(boxes, np.float64)
    M = boxes.shape[0]
    size = np.asarray(size)
    sizes, (Wf, Hf) = (None, (int(size[0]), int(size[1]))) if size.ndim == 1 else (np.ascontiguousarray(size, np.int32), (0, 0))
    crop, paste, fs = np.full((M, 4), -7, np.int32), np.full((M, 4), -7, np.int32), np.full(M, np.nan)
    m = float(momentum)
    state, has, last = st
    rc = raw(lib, boxes, so, sizes, Wf, Hf, state if smooth else None, has if smooth else None, last, M, K, m, 1.0 - m, smooth, fixed,
             float(scale), {"xyxy": 0, "relative": 1}[box_format], missing == "hold", min_side, crop, paste, fs)
    assert rc == 0
    return crop, paste, fs


def _same_out(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


def _same_states(a, b):
    """flags and last windows equal; the state rows of the streams that have begun equal bit for bit (the others were never written)"""
    on = a[1] != 0
    return np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[0][on].view(np.uint64), b[0][on].view(np.uint64))


def _case_kernel(lib, c, st, rows=slice(None)):
    so = None if c.so is None else np.ascontiguousarray(c.so[rows])
    return kernel(lib, c.boxes[rows], so, c.size_arg(rows), st, c.K, **c.kw)


def _windows_ok(crop, paste, sizes, paste_S):
    """the safety property: every crop window passes ops.windows_host for its own frame, every paste window with a side passes it
    as a paste into a paste_S image"""
    from emoportraits_amd import ops
    own = torch.as_tensor(np.broadcast_to(np.asarray(sizes), (len(crop), 2)).copy())
    ops.windows_host(crop.tolist(), len(crop), own, "crop")
    on = paste[:, 2] != 0
    assert (paste[~on] == 0).all()
    if on.any():
        ops.windows_host(paste[on].tolist(), int(on.sum()), own[torch.as_tensor(on)], "paste", paste_S=paste_S)


# ---- 1. the reference's recorded windows ---------------------------------------------------------------------------------------------
def test_kernel_gives_the_windows_crop_image_recorded(stream, glue):
    """every case of the golden: one call per case, frames in order, then the same rows one call each with the state carried; the 34
    recorded windows exactly, the recorded missing rows absent with the state untouched, face_scale the recorded value"""
    n = 0
    for case in glue["crop_cases"]:
        kw = case["kwargs"]
        M = len(case["faces"])
        boxes = np.array([[np.nan] * 4 if f is None else [float(v) for v in f] for f in case["faces"]])
        sizes = np.array([(w, h) for h, w in case["sizes"]], np.int32)
        args = dict(momentum=case["momentum"] if kw.get("use_smoothed_crop") else 0.01, smooth=bool(kw.get("use_smoothed_crop")),
                    fixed=bool(case["fixed"]), scale=kw.get("scale", 1))
        st = np.full((1, 3), np.nan), np.zeros(1, np.int32), np.zeros((1, 4), np.int32)
        crop, paste, fs = kernel(stream, boxes, None, sizes, st, 1, **args)
        one = np.full((1, 3), np.nan), np.zeros(1, np.int32), np.zeros((1, 4), np.int32)
        for i, (want, scale_ref, ok) in enumerate(zip(case["windows"], case["face_scale"], case["face_check"])):
            before = [a.copy() for a in one]
            row = kernel(stream, boxes[i:i + 1], None, sizes[i:i + 1], one, 1, **args)
            assert _same_out(row, (crop[i:i + 1], paste[i:i + 1], fs[i:i + 1])), (case["name"], i)
            if want is None:
                assert not ok and scale_ref == 0 and not paste[i].any() and fs[i] == 0.0
                assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, one)), (case["name"], i)
                continue
            assert tuple(paste[i]) == tuple(int(v) for v in want) == tuple(crop[i]), (case["name"], i, paste[i], want)
            assert fs[i] == scale_ref
            n += 1
        assert _same_states(st, one)
        _windows_ok(crop, paste, sizes, 8)
    assert n == 34


# ---- 2. the contract against the functions it restates -------------------------------------------------------------------------------
def test_the_restatement_is_crop_window_with_a_tracker_per_stream():
    """hostglue.crop_track against a loop of hostglue.crop_window + CropTracker (pinned to the reference by tests/test_host_logic.py)
    on every row where that loop yields a window inside its frame: the same window, the same face_scale; elsewhere the row is
    missing or absent"""
    from emoportraits_amd import hostglue as H
    seen = 0
    for M, K in ((37, 3), (130, 65)):
        for c in C.sweep(M, K):
            if c.kw["box_format"] != "xyxy":
                continue
            crop, paste, fs = c.restated(c.states())
            trackers = [H.CropTracker(c.kw["momentum"], c.kw["fixed"]) if c.kw["smooth"] else None for _ in range(K)]
            for i in range(M):
                k = 0 if c.so is None else int(c.so[i])
                box = c.boxes[i]
                if not 0 <= k < K or not (np.isfinite(box).all() and (np.abs(box) < C.BIG).all()):
                    assert fs[i] == 0.0 and (c.kw["missing"] == "hold" or not paste[i].any())
                    continue
                W, H_ = (int(v) for v in c.sizes[i])
                try:
                    x_lo, y_lo, side, scale = H.crop_window(box, W, H_, trackers[k], c.kw["scale"])
                except ZeroDivisionError:                                       # (a size of zero: the loop yields no window;
                    x_lo = y_lo = side = 0                                       # its tracker has taken the row by then)
                if H.window_inside(x_lo, y_lo, side, W, H_, c.kw["min_side"]):
                    assert tuple(paste[i]) == (x_lo, y_lo, side, side) == tuple(crop[i]) and fs[i] == scale, (M, K, i)
                    seen += 1
                elif c.kw["missing"] == "skip":
                    assert not paste[i].any() and fs[i] == 0.0
    assert seen > 500


def test_the_relative_format_is_detection_to_face(glue):
    from emoportraits_amd import hostglue as H
    for d in glue["detections"]:
        W, H_ = d["size"]
        assert np.array_equal(H.detection_to_face(*d["rel"], W, H_), d["face"])
        rel = H.crop_track(np.array([d["rel"]]), None, (W, H_), None, None, None, box_format="relative")
        pix = H.crop_track(np.array([d["face"]]), None, (W, H_), None, None, None)
        assert _same_out(rel, pix) and rel[1][0, 2] > 0


# ---- 3. and 4. the kernel against the contract, and the safety property --------------------------------------------------------------
ABSENT = {"stream", "box", "size", "side", "min_side"}


@pytest.mark.parametrize("M,K", [(37, 3), (130, 65)])
def test_kernel_is_the_restatement(stream, M, K):
    """M = 37 over K = 3 interleaved streams and M = 130 over K = 65 (past one block of stream threads), stream indices -1 and K,
    every frame size, every kind of box and every flag of crop_track_cases: outputs and all three state arrays, as one call and
    split in two at every row with the state carried.  First, on the restatement alone: at least half the rows of each case are
    present, and every cause of absence occurs"""
    causes = set()
    for c in C.sweep(M, K):
        why = []
        host = c.states()
        want = c.restated(host, why=why)
        assert sum(w == "present" for w in why) * 2 >= M, (c.kw, why)
        causes |= set(why)
        _windows_ok(want[0], want[1], c.sizes, 4 * c.kw["min_side"])
        dev = c.states()
        got = _case_kernel(stream, c, dev)
        assert _same_out(got, want) and _same_states(dev, host), c.kw
        # (every row; the threaded build, which starts 128 OS threads a launch for K = 65, at every ninth)
        for cut in range(1, M, 9 if K > 64 and "threads" in stream._name else 1):
            two = c.states()
            parts = [_case_kernel(stream, c, two, rows) for rows in (slice(0, cut), slice(cut, M))]
            assert _same_out(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), want), (c.kw, cut)
            assert _same_states(two, host)
            if cut % 13 == 1:                                                     # (the restatement carries its state the same way)
                two_host = c.states()
                parts = [c.restated(two_host, rows) for rows in (slice(0, cut), slice(cut, M))]
                assert _same_out(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), want) and _same_states(two_host, host)
    assert causes >= ABSENT | {"present"}, causes


def test_one_row_and_one_stream(stream):
    for seed, kw in enumerate((dict(), dict(missing="hold"), dict(smooth=False), dict(box_format="relative"))):
        c = C.Case(1, 1, 40 + seed, null_streams=True, **kw)
        host, dev = c.states(), c.states()
        assert _same_out(_case_kernel(stream, c, dev), c.restated(host)) and _same_states(dev, host)
    c = C.Case(9, 1, 50, null_streams=True, missing="hold")
    host, dev = c.states(), c.states()
    assert _same_out(_case_kernel(stream, c, dev), c.restated(host)) and _same_states(dev, host)


def test_hold_pastes_at_the_last_window_and_skip_does_not(stream):
    boxes = np.array([[20, 10, 60, 50], [np.nan] * 4, [30, 12, 62, 48], [5, 5, 5, 5.0]])
    for missing in ("skip", "hold"):
        st = np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((1, 4), np.int32)
        crop, paste, fs = kernel(stream, boxes, None, (96, 64), st, 1, missing=missing)
        assert paste[0, 2] > 0 and paste[2, 2] > 0 and fs[1] == 0.0 and fs[3] == 0.0
        if missing == "hold":
            assert np.array_equal(paste[1], paste[0]) and np.array_equal(crop[1], paste[0]) and np.array_equal(paste[3], paste[2])
        else:
            assert not paste[1].any() and not paste[3].any() and tuple(crop[1]) == (16, 0, 64, 64) == tuple(crop[3])
        assert np.array_equal(st[2][0], paste[2])
    # a held window that does not fit the row's (smaller) frame is not held
    st = np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((1, 4), np.int32)
    crop, paste, _ = kernel(stream, boxes[:2], None, np.array([(96, 64), (40, 30)], np.int32), st, 1, missing="hold")
    assert not paste[1].any() and tuple(crop[1]) == (5, 0, 30, 30)


def test_refusals_return_bad_arg_and_write_nothing(stream):
    M, K = 4, 2
    boxes, so = np.tile(np.array([[10, 10, 40, 40.0]]), (M, 1)), np.zeros(M, np.int32)
    state, has, last = np.full((K, 3), np.nan), np.zeros(K, np.int32), np.zeros((K, 4), np.int32)
    crop, paste, fs = np.full((M, 4), -7, np.int32), np.full((M, 4), -7, np.int32), np.full(M, np.nan)
    ok = dict(boxes=boxes, so=so, sizes=None, Wf=64, Hf=48, state=state, has=has, last=last, M=M, K=K, m=0.5, om=0.5, smooth=1, fixed=0,
              scale=1.0, box_format=0, hold=1, min_side=2, crop=crop, paste=paste, fs=fs)
    bad = [dict(boxes=None), dict(crop=None), dict(paste=None), dict(M=0), dict(K=0), dict(M=-1), dict(state=None), dict(has=None),
           dict(last=None), dict(m=0.0), dict(m=1.5), dict(m=float("nan")), dict(om=1.0), dict(om=-0.1), dict(Wf=0), dict(Hf=0),
           dict(scale=float("inf")), dict(scale=float("nan")), dict(box_format=2), dict(min_side=0)]
    for change in bad:
        assert raw(stream, **{**ok, **change}) == -1, change
        assert (crop == -7).all() and (paste == -7).all() and np.isnan(fs).all() and np.isnan(state).all() and not has.any() and not last.any()
    assert raw(stream, **{**ok, "fs": None}) == 0 and (crop >= 0).all() and np.isnan(fs).all()
    assert raw(stream, **{**ok, "smooth": 0, "hold": 0, "state": None, "has": None, "last": None, "so": None}) == 0
    assert raw(stream, **{**ok, "m": 1.0, "om": 0.0}) == 0


def test_the_entry_point_is_in_the_abi_table():
    from emoportraits_amd import _abi_version, hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "int emo_crop_track_f64(" in hdr and "ABI 23." in hdr and _abi_version.EMO_ABI_VERSION >= 23
    assert "#define EMO_ABI_VERSION %d" % _abi_version.EMO_ABI_VERSION in hdr
    assert [t for t in hip.SIGNATURES[NAME]] == ARGTYPES


# ---- 5. ops and the wrapper on the recorder rig of tests/test_head_pose_controls_emul.py ---------------------------------------------
def test_ops_crop_track_is_the_restatement_and_checks_its_arguments(monkeypatch):
    import emulibs
    from emoportraits_amd import ops
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(True)), 0)
    c = C.Case(37, 3, 9, momentum=0.5, missing="hold")
    host = c.states()
    want = c.restated(host)
    st = [torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)]
    for dtype, sizes in ((torch.float64, torch.from_numpy(c.sizes)), (torch.float64, c.sizes.tolist())):
        for t in st:
            t.zero_()
        got = ops.crop_track(torch.from_numpy(c.boxes).to(dtype), torch.from_numpy(c.so), sizes, *st, **c.kw)
        assert _same_out([g.numpy() for g in got], want) and _same_states([t.numpy() for t in st], host)
    assert w.lib.calls[NAME] == 2
    # float32 boxes are widened exactly: the windows of the float64 boxes that hold the same values
    b32 = torch.from_numpy(c.boxes).float()
    got = ops.crop_track(b32, None, (1920, 1080), K=1)
    want32 = C.hostglue_crop_track(b32.double().numpy(), (1920, 1080))
    assert _same_out([g.numpy() for g in got], want32)
    w.lib.calls.clear()
    ok = torch.zeros(4, 4, dtype=torch.float64)
    for args, kw, match in (((ok.int(),), {}, "float32 or float64"), ((ok[:, :3],), {}, r"\[M,4\]"), ((ok[:0],), {}, r"\[M,4\]"),
                            ((ok,), dict(box_format="cxcywh"), "box_format"), ((ok,), dict(missing="drop"), "missing"),
                            ((ok,), dict(momentum=0.0), "momentum"), ((ok,), dict(momentum=1.5), "momentum"),
                            ((ok,), dict(scale=float("inf")), "scale"), ((ok,), dict(min_side=0), "min_side"),
                            ((ok,), dict(smooth=True), "state"), ((ok,), dict(missing="hold"), "last"),
                            ((ok,), dict(size=(0, 5)), "size"), ((ok,), dict(size=[(5, 5)] * 3), "size"),
                            ((ok,), dict(stream_of=torch.zeros(3, dtype=torch.int32)), "stream_of"),
                            ((ok,), dict(state=torch.zeros(2, 3), has_state=torch.zeros(2, dtype=torch.int32)), "float64")):
        kw = {**dict(size=(64, 48)), **kw}
        with pytest.raises(ValueError, match=match):
            ops.crop_track(*args, **kw)
    assert NAME not in w.lib.calls


@pytest.fixture()
def video(monkeypatch):
    """the recorder rig of tests/test_head_pose_controls_emul.py's `video`: a wrapper on CPU tensors, the crops and the pastes
    through the host-compiled kernels, toy embedders, the driver pass a recorder that returns a grey image; every window the crop
    and the paste ops are handed is recorded"""
    import emulibs
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import ops
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    monkeypatch.setattr(ops, "unpack_rgb8", lambda u8: (u8.permute(0, 3, 1, 2).float() / 255).contiguous())

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
            yield views, arena
    monkeypatch.setattr(frames_mod, "uploaded", uploaded)
    monkeypatch.setattr(frames_mod, "uploaded_mixed", uploaded_mixed)
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(False)), 3)
    for k in range(3):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4), torch.zeros(5), torch.ones(9))
    w._canonical_cl = torch.zeros(1, 2, 2, 2, 4)
    w.cropped, w.pasted = [], []

    def listed(windows):
        return windows.tensor.tolist() if isinstance(windows, ops.DeviceWindows) else [list(v) for v in windows]

    def spy(name, log, at):
        real = getattr(ops, name)

        def call(*args, **kw):
            log.append(listed(args[at]))
            return real(*args, **kw)
        monkeypatch.setattr(ops, name, call)
    spy("resize2d_windows", w.cropped, 2), spy("crop_faces_mixed", w.cropped, 2)
    spy("paste_windows", w.pasted, 2), spy("paste_faces_mixed", w.pasted, 2)

    def head_pose(crops):
        f = crops.flatten(1)[:, 3::17][:, :9] - 0.5
        srt = (1 + 0.2 * f[:, 0:3]).contiguous(), (4.0 * f[:, 3:6]).contiguous(), (0.2 * f[:, 6:9]).contiguous()
        return (ops.pose_theta(*srt),) + srt
    w._head_pose = head_pose
    w._expression = lambda crops, theta, what: ((crops.flatten(1)[:, 5::31][:, :6] * 4 - 2).contiguous(), None)
    real_drive = w._drive_bank
    grey = lambda pose, theta, ident=None: real_drive(pose, theta, ident) + 0.5
    w._drive_bank, w._drive = grey, lambda pose, theta: grey(pose, theta)
    return w


def _clip(n, hw, seed):
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _walk(N, W, H, seed, lo=0.2, hi=0.5):
    """N boxes of a face that wanders about the middle of a W x H frame: every window fits"""
    rng = np.random.default_rng(seed)
    cx, cy = W * (0.5 + 0.08 * rng.standard_normal(N)).clip(0.4, 0.6), H * (0.5 + 0.08 * rng.standard_normal(N)).clip(0.4, 0.6)
    h = rng.uniform(lo, hi, (2, N)) * min(W, H) / 2
    return np.stack([cx - h[0], cy - h[1], cx + h[0], cy + h[1]], 1)


def _run(w, frames, **kw):
    """-> (frames or crops out, in order; the recorded driver calls; the windows cropped; the windows pasted)"""
    w.recorded.clear(), w.cropped.clear(), w.pasted.clear()
    out = [o.clone() for _, o in w.animate_frames(frames, to_host=False, **kw)]
    rec = [torch.cat([r[i] for r in w.recorded]) for i in (0, 1)] if w.recorded else []
    return torch.cat(out), rec, sum(w.cropped, []), sum(w.pasted, [])


def _restated(boxes, size, min_side=2, st=None, so=None, K=1, **kw):
    from emoportraits_amd import hostglue
    st = st or (np.zeros((K, 3)), np.zeros(K, np.int32), np.zeros((K, 4), np.int32))
    kw.setdefault("momentum", 0.01)
    return hostglue.crop_track(boxes, so, size, *st, min_side=min_side, **kw)


TRACK = dict(smooth=True, momentum=0.5, scale=1.3)


def test_animate_frames_crops_and_pastes_at_the_restated_windows(video):
    """13 frames of 40 x 56: the crop and the paste ops receive exactly the restatement's windows, the driver pass the same rows and
    the caller the same frames as windows= fed with those windows; whatever the batch size, the chunking, a call split in two and
    the number of ranks"""
    w, N, (H, W) = video, 13, (40, 56)
    clip, boxes = _clip(N, (H, W), 1), _walk(N, W, H, 2)
    crop, paste, _ = _restated(boxes, (W, H), smooth=True, momentum=0.5, scale=1.3)
    assert (paste[:, 2] >= 2).all() and np.array_equal(crop, paste)             # all rows present
    tb = torch.from_numpy(boxes)
    for paste_back in (False, True):
        kw = dict(paste_back=paste_back, feather=0.1) if paste_back else dict(as_uint8=False)
        w.lib.calls.clear()
        want_out, want_rec, want_c, want_p = _run(w, clip, batch_size=4, windows=[tuple(r[:3]) for r in crop.tolist()], **kw)
        assert NAME not in w.lib.calls and want_c == crop.tolist() and want_p == (paste.tolist() if paste_back else [])
        assert not paste_back or not torch.equal(want_out, clip)
        runs = [dict(frames=clip, boxes=tb, batch_size=4), dict(frames=clip, boxes=tb.float().double(), batch_size=1),
                dict(frames=clip, boxes=tb, batch_size=16), dict(frames=iter([clip[:5], clip[5:6], clip[6:]]), boxes=tb, batch_size=4),
                dict(frames=iter([clip[:5], clip[5:6], clip[6:]]), boxes=iter([tb[:5], tb[5:6], tb[6:]]), batch_size=3)]
        for k, run in enumerate(runs):
            w.reset_crop_state()
            w.lib.calls.clear()
            out, rec, c, p = _run(w, run.pop("frames"), tracking=TRACK, **run, **kw)
            assert c == want_c and p == want_p, k
            assert torch.equal(out, want_out) and all(torch.equal(a, b) for a, b in zip(rec, want_rec)), k
            assert w.lib.calls[NAME] == (1 if k < 3 else 3)                         # one launch per chunk
            assert w.tracked_windows[0].tolist() == paste[w.tracked_windows[1]:].tolist()
        # a call split in two carries the state on the wrapper
        w.reset_crop_state()
        parts = [_run(w, clip[a:b], boxes=tb[a:b], tracking=TRACK, batch_size=4, **kw) for a, b in ((0, 6), (6, N))]
        assert parts[0][2] + parts[1][2] == want_c and torch.equal(torch.cat([parts[0][0], parts[1][0]]), want_out)
        # two ranks: each tracks the whole chunk and serves its shard
        halves = []
        for rank in (0, 1):
            w.reset_crop_state()
            w.rank, w.world = rank, 2
            halves.append(_run(w, clip, boxes=tb, tracking=TRACK, batch_size=4, **kw))
            assert np.array_equal(w._crop_streams.last.numpy()[0], paste[-1])
        w.rank, w.world = 0, 1
        assert halves[0][2] + halves[1][2] == want_c and halves[0][3] + halves[1][3] == want_p
        assert torch.equal(torch.cat([halves[0][0], halves[1][0]]), want_out)


def test_boxes_alone_is_the_per_frame_window_and_float32_boxes_are_widened(video):
    w, N, (H, W) = video, 7, (40, 56)
    clip, boxes = _clip(N, (H, W), 3), torch.from_numpy(_walk(N, W, H, 4)).float()
    crop, paste, _ = _restated(boxes.double().numpy(), (W, H))
    _, _, c, p = _run(w, clip, boxes=boxes, batch_size=4, as_uint8=False)
    assert c == crop.tolist() and p == [] and not w._crop_streams.has.any()
    rel = torch.stack([boxes[:, 0] / W, boxes[:, 1] / H, (boxes[:, 2] - boxes[:, 0]) / W, (boxes[:, 3] - boxes[:, 1]) / H], 1).double()
    crop, paste, _ = _restated(rel.numpy(), (W, H), box_format="relative", min_side=2)
    _, _, c, p = _run(w, clip, boxes=rel, tracking=dict(box_format="relative"), batch_size=4, paste_back=True)
    assert c == crop.tolist() and p == paste.tolist()


def test_an_absent_row_is_not_pasted_and_hold_pastes_at_the_last_window(video):
    w, N, (H, W) = video, 6, (40, 56)
    clip, boxes = _clip(N, (H, W), 5), _walk(N, W, H, 6)
    boxes[2] = np.nan
    boxes[4] = [10, 10, 11, 10.4]                                                 # a size below two pixels
    for missing in ("skip", "hold"):
        crop, paste, _ = _restated(boxes, (W, H), missing=missing, smooth=True, momentum=1.0)
        w.reset_crop_state()
        out, rec, c, p = _run(w, clip, boxes=torch.from_numpy(boxes), tracking=dict(smooth=True, momentum=1.0, missing=missing),
                              batch_size=4, paste_back=True)
        assert c == crop.tolist() and p == paste.tolist() and rec[0].shape[0] == N  # every row is rendered
        for i in range(N):
            assert torch.equal(out[i], clip[i]) == (paste[i, 2] == 0), (missing, i)
        if missing == "skip":
            assert not paste[2].any() and not paste[4].any() and tuple(crop[2]) == (8, 0, 40, 40)
        else:
            assert np.array_equal(paste[2], paste[1]) and np.array_equal(paste[4], paste[3])
            x, y, s, _ = paste[2]
            assert not torch.equal(out[2, y:y + s, x:x + s], clip[2, y:y + s, x:x + s])


def test_two_tracks_per_frame_are_the_faces_path(video):
    """boxes [N,2,4] with one identity per row against faces= lists of the two tracks' restated windows"""
    w, N, (H, W) = video, 7, (48, 64)
    clip = _clip(N, (H, W), 7)
    a, b = _walk(N, W, H, 8, 0.2, 0.3), _walk(N, W, H, 9, 0.3, 0.5)
    a[:, [0, 2]] -= 12
    b[:, [0, 2]] += 10
    both = np.stack([a, b], 1)                                                   # [N,2,4], rows frame-major
    so = np.tile(np.int32([0, 1]), N)
    crop, paste, _ = _restated(both.reshape(-1, 4), (W, H), so=so, K=2, smooth=True, momentum=0.5)
    assert (paste[:, 2] >= 2).all()
    ids = [0, 2] * N
    faces = [[tuple(crop[2 * i][:3]), tuple(crop[2 * i + 1][:3])] for i in range(N)]
    for kw in (dict(as_uint8=False), dict(paste_back=True)):
        want = _run(w, clip, faces=faces, identities=ids, batch_size=4, **kw)
        for bs in (2, 4, 16):
            w.reset_crop_state()
            got = _run(w, clip, boxes=torch.from_numpy(both), tracking=dict(smooth=True, momentum=0.5), identities=ids, batch_size=bs, **kw)
            assert got[2] == crop.tolist() and got[3] == want[3] and torch.equal(got[0], want[0])
            assert all(torch.equal(x, y) for x, y in zip(got[1], want[1]))
    assert w._crop_streams.K == 2
    _run(w, clip, boxes=torch.from_numpy(a), batch_size=4, as_uint8=False)         # another number of tracks: a new store
    assert w._crop_streams.K == 1
    with pytest.raises(ValueError, match="batch_size"):
        next(w.animate_frames(clip, boxes=torch.zeros(N, 5, 4), batch_size=4))
    with pytest.raises(ValueError, match="one slot per track"):
        next(w.animate_frames(clip, boxes=torch.from_numpy(both), identities=[0] * N))
    with pytest.raises(ValueError, match="smooth_per_identity"):
        next(w.animate_frames(clip, boxes=torch.from_numpy(both), smooth_pose=True))


def test_animate_streams_boxes_are_its_windows_form(video):
    w = video
    sizes = [(32, 48), (40, 56)]                                                 # (H, W) of the two streams
    clips = [_clip(4, sizes[0], 10), _clip(3, sizes[1], 11)]
    boxes = [_walk(4, 48, 32, 12), _walk(3, 56, 40, 13)]
    order = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (0, 3)]             # tick order
    rows = np.stack([boxes[s][t] for s, t in order])
    crop, paste, _ = _restated(rows, [sizes[s][::-1] for s, _ in order], so=np.int32([s for s, _ in order]), K=2, smooth=True, momentum=0.5)
    assert (paste[:, 2] >= 2).all()
    at = {st: crop[i] for i, st in enumerate(order)}

    def run(streams, **kw):
        w.recorded.clear(), w.cropped.clear(), w.pasted.clear()
        out = [(s, t, o.clone()) for batch in w.animate_streams(streams, to_host=False, **kw) for s, t, o in batch]
        return out, sum(w.cropped, []), sum(w.pasted, []), [torch.cat([r[i] for r in w.recorded]) for i in (0, 1)]
    for kw in (dict(as_uint8=False), dict(paste_back=True)):
        w.lib.calls.clear()
        want = run([dict(frames=clips[s], windows=[tuple(at[(s, t)][:3]) for t in range(len(clips[s]))]) for s in (0, 1)], batch_size=4, **kw)
        assert NAME not in w.lib.calls
        forms = [[dict(frames=clips[s], boxes=torch.from_numpy(boxes[s])) for s in (0, 1)],
                 [dict(frames=iter([clips[0][:1], clips[0][1:]]), boxes=torch.from_numpy(boxes[0])),
                  dict(frames=clips[1], boxes=iter([torch.from_numpy(boxes[1][:2]), torch.from_numpy(boxes[1][2:])]))]]
        for k, (streams, bs) in enumerate(zip(forms, (4, 3))):
            w.lib.calls.clear()
            got = run(streams, tracking=dict(smooth=True, momentum=0.5), batch_size=bs, **kw)
            assert got[1] == crop.tolist() and got[2] == (paste.tolist() if "paste_back" in kw else [])
            assert w.lib.calls[NAME] == (2 if bs == 4 else 3)                      # one launch per batch
            assert len(got[0]) == len(want[0]) and all(a[:2] == b[:2] and torch.equal(a[2], b[2]) for a, b in zip(got[0], want[0]))
            assert all(torch.equal(x, y) for x, y in zip(got[3], want[3]))
    assert w._crop_streams is None                                               # the streams' trackers are the call's own
    ok = dict(frames=clips[0], boxes=torch.from_numpy(boxes[0]))
    w.lib.calls.clear()
    for streams, kw, match in (([dict(ok, windows=[(0, 0, 8)] * 4)], {}, "mutually exclusive"), ([dict(ok, faces=[[]] * 4)], {}, "mutually exclusive"),
                               ([ok, dict(frames=clips[1], windows=[(0, 0, 8)] * 3)], {}, "every stream or in none"),
                               ([dict(ok, boxes=torch.zeros(4, 2, 4))], {}, "tracks per stream"),
                               ([dict(ok, boxes=torch.zeros(3, 4))], {}, "rows for 4 frames"),
                               ([dict(frames=iter([clips[0]]), boxes=iter([torch.zeros(4, 4)]))], {}, "length must be known"),
                               ([dict(frames=clips[0], windows=[(0, 0, 8)] * 4)], dict(tracking=dict(smooth=True)), "no stream has any"),
                               ([ok], dict(tracking=dict(missing="drop")), "missing")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_streams(streams, **kw))
    assert not w.lib.calls
    with pytest.raises(ValueError, match="ended before its frames"):
        list(w.animate_streams([dict(frames=clips[0], boxes=iter([torch.from_numpy(boxes[0][:2])]))], to_host=False))


def test_resets_restart_the_tracker_and_bank_events_leave_it_alone(video):
    w, N, (H, W) = video, 6, (40, 56)
    clip, boxes = _clip(N, (H, W), 14), _walk(N, W, H, 15)
    tb, kw = torch.from_numpy(boxes), dict(tracking=dict(smooth=True, momentum=0.5, missing="hold"), batch_size=4, as_uint8=False)
    fresh = _restated(boxes, (W, H), smooth=True, momentum=0.5, missing="hold")[0].tolist()
    st = (np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((1, 4), np.int32))
    _restated(boxes, (W, H), st=st, smooth=True, momentum=0.5, missing="hold")
    carried = _restated(boxes, (W, H), st=st, smooth=True, momentum=0.5, missing="hold")[0].tolist()
    assert carried != fresh
    assert _run(w, clip, boxes=tb, **kw)[2] == fresh
    # the bank's events are the identities' business: the tracker carries on
    w._bank_write(1, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4))
    w.drop_identity(2)
    w.reset_pose_state(), w.reset_expression_state()
    assert w._crop_streams.has.tolist() == [1] and _run(w, clip, boxes=tb, **kw)[2] == carried
    w.reset_crop_state()
    assert w._crop_streams.has.tolist() == [0] and not w._crop_streams.last.any() and _run(w, clip, boxes=tb, **kw)[2] == fresh
    w.reset_crop_state([0])
    assert _run(w, clip, boxes=tb, **kw)[2] == fresh
    with pytest.raises(ValueError, match="track"):
        w.reset_crop_state([1])
    assert w.forward(reset_tracking=True) is None                                # (no driver: the reset alone)
    assert w._crop_streams.has.tolist() == [0] and _run(w, clip, boxes=tb, **kw)[2] == fresh
    fresh_wrapper_reset = type(w).reset_crop_state
    bare = object.__new__(type(w))
    bare._crop_streams = None
    fresh_wrapper_reset(bare)                                                    # (before the first use: nothing to restart)


def test_errors_come_before_any_launch_and_no_boxes_launch_nothing(video):
    w, N, (H, W) = video, 5, (40, 56)
    clip, tb = _clip(N, (H, W), 16), torch.from_numpy(_walk(N, W, H, 17))
    wins = [(8, 4, 16)] * N
    w.lib.calls.clear()
    w.recorded.clear()
    for kw, match in ((dict(boxes=tb, windows=wins), "mutually exclusive"), (dict(boxes=tb, faces=[[w_] for w_ in wins]), "mutually exclusive"),
                      (dict(boxes=tb.int()), "float32 or float64"), (dict(boxes=tb.half()), "float32 or float64"),
                      (dict(boxes=[[0, 0, 5, 5]] * N), "float32 or float64"), (dict(boxes=7), "iterable"),
                      (dict(boxes=tb[:, :3]), r"\[N,4\] or \[N,P,4\]"), (dict(boxes=tb.reshape(N, 2, 2)), r"\[N,4\] or \[N,P,4\]"),
                      (dict(boxes=tb[None, None]), r"\[N,4\] or \[N,P,4\]"), (dict(boxes=tb[:4]), "rows for 5 frames"),
                      (dict(boxes=tb[:, None].expand(N, 5, 4), batch_size=4), "batch_size"),
                      (dict(boxes=tb, tracking=dict(box_format="cxcywh")), "box_format"), (dict(boxes=tb, tracking=dict(missing="drop")), "missing"),
                      (dict(boxes=tb, tracking=dict(momentum=0.0)), "momentum"), (dict(boxes=tb, tracking=dict(momentum=1.01)), "momentum"),
                      (dict(boxes=tb, tracking=dict(momentun=0.5)), "no field"), (dict(boxes=tb, tracking=3), "mapping"),
                      (dict(tracking=dict(smooth=True)), "boxes= is missing"), (dict(windows=wins, tracking={}), "boxes= is missing"),
                      (dict(boxes=iter([])), "ended before the frames")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(clip, **kw))
    # an iterable that ends before the frames do: nothing of the chunk it misses is launched
    with pytest.raises(ValueError, match="ended before the frames"):
        list(w.animate_frames(iter([clip[:2], clip[2:]]), boxes=iter([tb[:2]]), to_host=False, as_uint8=False, batch_size=4))
    assert w.lib.calls.get(NAME, 0) == 1 and sum(r[0].shape[0] for r in w.recorded) == 2
    with pytest.raises(ValueError, match="rows for a chunk of 3 frames"):
        list(w.animate_frames(iter([clip[:2], clip[2:]]), boxes=iter([tb[:2], tb[2:4]]), to_host=False, as_uint8=False, batch_size=4))
    # the keyword absent (or None): no launch, the same frames
    from emoportraits_amd import CropTracking
    assert CropTracking.of(dict(smooth=True)) == CropTracking(smooth=True) and CropTracking.of(None) is None
    w.lib.calls.clear()
    a = _run(w, clip, windows=wins, batch_size=4, paste_back=True)
    b = _run(w, clip, windows=wins, batch_size=4, paste_back=True, boxes=None, tracking=None)
    assert NAME not in w.lib.calls and torch.equal(a[0], b[0]) and a[2:] == b[2:]
