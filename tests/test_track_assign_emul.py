"""Detections to tracks without a GPU: emo_track_assign_f64 and emo_crop_track_restarts_f64 (csrc/smallops.hip), compiled for the
host from the product's own source (tests/emul/emulibs.stream(True): the threaded build, whose shuffles are exchanges between the
lanes of a wave; the loop build's are stubs), against hostglue.track_assign / hostglue.crop_track(restart=) bit for bit, and
hostglue.track_assign against the plain-loop reference of tests/track_assign_cases.py, which is written from the header alone.
Then ops.track_assign, crop_plan's checks and InferenceWrapper.animate_frames(detections=) on the recorder rig of
tests/test_crop_track_emul.py.  Everything compared is an integer or a bit pattern: no tolerances."""
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
import crop_track_cases as CC  # noqa: E402
import track_assign_cases as C  # noqa: E402
from test_crop_track_emul import ARGTYPES as CROP_ARGTYPES  # noqa: E402
from test_crop_track_emul import _clip, _run, _same_out, _same_states, video  # noqa: E402,F401
from test_crop_track_emul import kernel as crop_kernel  # noqa: E402
from test_crop_track_gpu import _walk  # noqa: E402
from test_head_pose_controls_emul import _bare_wrapper, _Lib  # noqa: E402

NAME, RESTARTS = "emo_track_assign_f64", "emo_crop_track_restarts_f64"
V, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = [V, V, I, I, I, I, V, V, D, I, I, V, V, V, V]
RESTARTS_ARGTYPES = CROP_ARGTYPES[:18] + [V] + CROP_ARGTYPES[18:]
CASES = C.cases()


@pytest.fixture(scope="module")
def stream():
    import emulibs
    return emulibs.stream(True)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def raw(lib, dets, so, F, D_, P, K, ref, age, min_iou, max_missed, box_format, boxes, restart, track_of):
    fn = lib.emo_track_assign_f64
    fn.argtypes, fn.restype = ARGTYPES, ctypes.c_int
    return fn(_p(dets), _p(so), F, D_, P, K, _p(ref), _p(age), min_iou, max_missed, box_format, _p(boxes), _p(restart), _p(track_of), None)


def kernel(lib, dets, so, st, min_iou, max_missed, box_format):
    """one call of the entry point on numpy arrays, the outputs pre-filled with a pattern the kernel must overwrite"""
    dets = np.ascontiguousarray(dets, np.float64)
    F, D_ = dets.shape[:2]
    K, P = st[1].shape
    boxes, restart, track_of = np.full((F, P, 4), -7.0), np.full((F, P), -7, np.int32), np.full((F, D_), -7, np.int32)
    assert raw(lib, dets, so, F, D_, P, K, st[0], st[1], min_iou, max_missed, box_format, boxes, restart, track_of) == 0
    return boxes, restart, track_of


def _same(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _same_tracks(a, b):
    """ages equal; the ref rows of the live tracks equal bit for bit (a free slot's ref means nothing)"""
    on = a[1] >= 0
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0][on].view(np.uint64), b[0][on].view(np.uint64))


def _cat(parts):
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def _chunks(F):
    return [r for r in (slice(0, 1), slice(1, 6), slice(6, F)) if r.start < F]


# ---- 1. the contract against the plain loops, and what the cases are there to show ------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_the_restatement_is_the_plain_loop_reference(c):
    a, b = c.states(), c.states()
    want, got = c.reference(a), c.restated(b)
    assert _same(got, want) and _same_tracks(b, a)
    assert (np.isnan(want[0]).all(-1) | ~np.isnan(want[0]).any(-1)).all()
    parts = c.states()
    assert _same(_cat([c.restated(parts, r) for r in _chunks(c.F)]), want) and _same_tracks(parts, a)


def test_the_cases_show_what_they_are_there_for():
    by = {c.name: c for c in CASES}
    run = lambda name: by[name].reference(by[name].states())
    boxes, restart, track_of = run("swap")
    assert track_of.tolist() == [[0, -1, 1] if t % 2 == 0 else [1, 0, -1] for t in range(8)] and restart.sum() == 2
    assert (np.diff(boxes[:, 0, 0]) == 1).all() and (np.diff(boxes[:, 1, 0]) == -1).all()
    boxes, restart, _ = run("gap_max_missed")
    assert restart[1:].sum() == 0 and np.isnan(boxes[2:4, 0]).all() and boxes[4, 0, 0] == 24.0
    boxes, restart, track_of = run("gap_one_more")
    assert restart[:, 0].tolist() == [1, 0, 0, 0, 1, 1, 0, 0] and np.isnan(boxes[2:5, 0]).all() and track_of[5].tolist() == [0, 1]
    boxes, restart, track_of = run("death_and_birth_in_one_frame")
    assert restart[:, 0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0] and np.isnan(boxes[2, 0]).all() and boxes[3, 0, 0] == 142.0
    assert track_of[3].tolist() == [-1, 1, 0] and restart[:, 1].tolist() == [1] + [0] * 7
    _, restart, track_of = run("more_faces_than_slots")
    assert (np.sort(track_of, 1)[:, :2] == -1).all() and (np.sort(track_of, 1)[:, 2:] == [0, 1]).all()
    _, _, track_of = run("tie_on_d")
    assert track_of[1].tolist() == [0, 2, 1] and track_of[2].tolist() == [0, 1, 2]
    _, _, track_of = run("tie_on_p")
    assert track_of.tolist() == [[0, -1], [0, 1], [-1, 0]]
    assert run("iou_at_min_iou")[1].sum() == 1 and run("iou_one_ulp_below")[1][:, 1].tolist() == [0, 1, 0]
    assert run("iou_at_a_rounded_third")[1].sum() == 1 and run("min_iou_1")[1].tolist() == [[1, 0], [0, 0], [0, 1]]
    _, _, track_of = run("unusable")
    assert track_of.tolist() == [[0, -1, -1, -1], [0, -1, -1, -1], [0, -1, -1, 1], [0, -1, -1, 1]]
    assert run("relative")[2].tolist() == [[0, -1, 1] if t % 2 == 0 else [1, 0, -1] for t in range(6)]
    boxes, restart, track_of = run("streams")
    assert (track_of[[4, 7]] == -1).all() and np.isnan(boxes[[4, 7]]).all() and restart.sum() == 4
    st = by["streams"].states()
    by["streams"].reference(st)
    assert st[1].tolist() == [[0, 0], [-1, -1], [0, 0]]
    boxes, restart, track_of = run("full_16_by_32")
    assert restart[0].all() and not restart[1:].any() and not np.isnan(boxes).any() and (np.sort(track_of, 1)[:, 16:] == np.arange(16)).all()
    _, restart, track_of = run("crowd_12_by_32")
    assert restart[1:].sum() > 4 and (track_of.max(1) == 11).any()


# ---- 2. the kernel against the contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_kernel_is_the_restatement(stream, c):
    """outputs and the live tracks, in one call and split into chunks of 1, 5 and the rest with the state carried"""
    host, dev = c.states(), c.states()
    want = c.restated(host)
    got = kernel(stream, c.dets, c.so, dev, **c.kw)
    assert _same(got, want) and _same_tracks(dev, host), c.name
    parts = c.states()
    got = _cat([kernel(stream, *c.rows(r), parts, **c.kw) for r in _chunks(c.F)])
    assert _same(got, want) and _same_tracks(parts, host), c.name


def test_refusals_return_bad_arg_and_write_nothing(stream):
    F, D_, P, K = 3, 4, 2, 2
    dets, so = np.tile(np.array([10, 10, 40, 40.0]), (F, D_, 1)), np.zeros(F, np.int32)
    ref, age = np.full((K, P, 4), np.nan), np.full((K, P), -1, np.int32)
    boxes, restart, track_of = np.full((F, P, 4), -7.0), np.full((F, P), -7, np.int32), np.full((F, D_), -7, np.int32)
    ok = dict(dets=dets, so=so, F=F, D_=D_, P=P, K=K, ref=ref, age=age, min_iou=0.3, max_missed=2, box_format=0, boxes=boxes,
              restart=restart, track_of=track_of)
    bad = [dict(dets=None), dict(ref=None), dict(age=None), dict(boxes=None), dict(restart=None), dict(track_of=None), dict(F=0),
           dict(F=-1), dict(D_=0), dict(P=0), dict(K=0), dict(P=17), dict(D_=33), dict(min_iou=0.0), dict(min_iou=-0.1),
           dict(min_iou=1.0000001), dict(min_iou=float("nan")), dict(max_missed=-1), dict(box_format=2), dict(box_format=-1)]
    for change in bad:
        assert raw(stream, **{**ok, **change}) == -1, change
        assert (boxes == -7).all() and (restart == -7).all() and (track_of == -7).all() and (age == -1).all() and np.isnan(ref).all()
    assert raw(stream, **{**ok, "so": None, "min_iou": 1.0, "max_missed": 0}) == 0 and (track_of >= -1).all()


# ---- 3. the tracker with restarts ------------------------------------------------------------------------------------------------
def restarts_kernel(lib, c, st, restart, rows=slice(None)):
    boxes = np.ascontiguousarray(c.boxes[rows], np.float64)
    M = boxes.shape[0]
    so = None if c.so is None else np.ascontiguousarray(c.so[rows])
    size = np.asarray(c.size_arg(rows))
    sizes, (Wf, Hf) = (None, (int(size[0]), int(size[1]))) if size.ndim == 1 else (np.ascontiguousarray(size, np.int32), (0, 0))
    crop, paste, fs = np.full((M, 4), -7, np.int32), np.full((M, 4), -7, np.int32), np.full(M, np.nan)
    kw, (state, has, last) = c.kw, st
    fn = lib.emo_crop_track_restarts_f64
    fn.argtypes, fn.restype = RESTARTS_ARGTYPES, ctypes.c_int
    m = float(kw["momentum"])
    rc = fn(_p(boxes), _p(so), _p(sizes), Wf, Hf, _p(state if kw["smooth"] else None), _p(has if kw["smooth"] else None), _p(last), M, c.K,
            m, 1.0 - m, int(kw["smooth"]), int(kw["fixed"]), float(kw["scale"]), {"xyxy": 0, "relative": 1}[kw["box_format"]],
            int(kw["missing"] == "hold"), kw["min_side"], _p(None if restart is None else np.ascontiguousarray(restart[rows])), _p(crop),
            _p(paste), _p(fs), None)
    assert rc == 0
    return crop, paste, fs


@pytest.mark.parametrize("M,K", [(37, 3), (130, 65)])
def test_crop_track_with_restarts_is_the_restatement(stream, M, K):
    """the crop_track_cases sweep with a random restart mask (a quarter of the rows): outputs and the three state arrays, in one
    call and in two; with restart = NULL the entry point is emo_crop_track_f64 bit for bit; and the mask changes something"""
    from emoportraits_amd import hostglue
    rng = np.random.default_rng(M)
    changed = 0
    for c in CC.sweep(M, K):
        restart = (rng.random(M) < 0.25).astype(np.int32)
        host, dev, two = c.states(), c.states(), c.states()
        want = hostglue.crop_track(c.boxes, c.so, c.size_arg(), *host, K=K, restart=restart, **c.kw)
        assert _same_out(restarts_kernel(stream, c, dev, restart), want) and _same_states(dev, host), c.kw
        cut = M // 3
        parts = [restarts_kernel(stream, c, two, restart, r) for r in (slice(0, cut), slice(cut, M))]
        assert _same_out(_cat(parts), want) and _same_states(two, host), c.kw
        plain_host, plain, null = c.states(), c.states(), c.states()
        plain_want = c.restated(plain_host)
        assert _same_out(restarts_kernel(stream, c, null, None), plain_want) and _same_states(null, plain_host)
        so = None if c.so is None else c.so
        assert _same_out(crop_kernel(stream, c.boxes, so, c.size_arg(), plain, c.K, **c.kw), plain_want) and _same_states(plain, null)
        changed += not _same_out(want, plain_want)
    assert changed >= 4


def test_a_dead_track_is_not_held_and_a_rebirth_starts_at_its_own_box(stream):
    """one slot, missing='hold', smooth: a face, a gap of max_missed + 1 frames, another face elsewhere -- track_assign, then the
    tracker with its restart flags against the tracker without them"""
    from emoportraits_amd import hostglue
    a, b, nan = [20.0, 10, 60, 50], [70.0, 40, 110, 80], [np.nan] * 4
    dets = np.array([[a], [a], [nan], [nan], [nan], [b], [b]])
    ref, age = np.zeros((1, 1, 4)), np.full((1, 1), -1, np.int32)
    boxes, restart, track_of = hostglue.track_assign(dets, None, ref, age, 0.3, 2, "xyxy")
    assert restart[:, 0].tolist() == [1, 0, 0, 0, 1, 1, 0] and track_of[:, 0].tolist() == [0, 0, -1, -1, -1, 0, 0]
    kw = dict(momentum=0.5, smooth=True, missing="hold")
    st = lambda: (np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((1, 4), np.int32))
    s_host, s_dev = st(), st()
    c = CC.Case(7, 1, 0, null_streams=True, one_size=(128, 96), **kw)
    c.boxes = np.ascontiguousarray(boxes[:, 0])
    crop, paste, _ = want = hostglue.crop_track(boxes[:, 0], None, (128, 96), *s_host, restart=restart[:, 0], **kw)
    assert _same_out(restarts_kernel(stream, c, s_dev, restart[:, 0]), want) and _same_states(s_dev, s_host)
    own = hostglue.crop_track(np.array([b]), None, (128, 96), *st(), **kw)[1][0]
    assert (paste[:, 2] > 0).tolist() == [True] * 4 + [False] + [True] * 2        # held while it lives, not pasted once it is dead
    assert np.array_equal(paste[2], paste[1]) and np.array_equal(paste[5], own) and tuple(crop[4]) == (16, 0, 96, 96)
    without = hostglue.crop_track(boxes[:, 0], None, (128, 96), *st(), **kw)[1]
    assert without[4, 2] > 0 and not np.array_equal(without[5], own)          # (held for ever, and an EMA with the face before)


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_in_the_abi_table():
    from emoportraits_amd import _abi_version, hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "ABI 25." in hdr and "int emo_track_assign_f64(" in hdr and "int emo_crop_track_restarts_f64(" in hdr
    assert _abi_version.EMO_ABI_VERSION >= 25 and "#define EMO_ABI_VERSION %d" % _abi_version.EMO_ABI_VERSION in hdr
    assert list(hip.SIGNATURES[NAME]) == ARGTYPES and list(hip.SIGNATURES[RESTARTS]) == RESTARTS_ARGTYPES


# ---- 5. ops, the plan's checks and the wrapper on the recorder rig ----------------------------------------------------------------
def test_ops_track_assign_is_the_restatement_and_checks_its_arguments(monkeypatch):
    import emulibs
    from emoportraits_amd import hostglue, ops
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(True)), 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    for c in CASES[:4] + [c for c in CASES if c.name in ("relative", "streams")]:
        host = c.states()
        want = c.restated(host)
        dev = [t(a) for a in c.states()]
        kw = dict(c.kw, box_format=("xyxy", "relative")[c.kw["box_format"]])
        got = ops.track_assign(t(c.dets), t(c.so), *dev, **kw)
        assert _same([g.numpy() for g in got], want) and _same_tracks([a.numpy() for a in dev], host), c.name
    # float32 detections are widened exactly, and restart= reaches the tracker
    c = CASES[0]
    d32 = t(c.dets).float()
    st = [t(a) for a in c.states()]
    boxes, restart, _ = ops.track_assign(d32, None, *st, **dict(c.kw, box_format="xyxy"))
    want = hostglue.track_assign(d32.double().numpy(), None, *c.states(), min_iou=c.kw["min_iou"], max_missed=c.kw["max_missed"])
    assert np.array_equal(boxes.numpy().view(np.uint64), want[0].view(np.uint64)) and np.array_equal(restart.numpy(), want[1])
    so = torch.arange(2, dtype=torch.int32).repeat(c.F)
    crop_st = [torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)]
    got = ops.crop_track(boxes.reshape(-1, 4), so, (128, 96), *crop_st, momentum=0.5, smooth=True, restart=restart.reshape(-1))
    host_st = np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros((2, 4), np.int32)
    want = hostglue.crop_track(want[0].reshape(-1, 4), so.numpy(), (128, 96), *host_st, momentum=0.5, smooth=True, restart=want[1].reshape(-1))
    assert _same_out([g.numpy() for g in got], want) and w.lib.calls[RESTARTS] == 1 and "emo_crop_track_f64" not in w.lib.calls
    w.lib.calls.clear()
    ok, (ref, age) = torch.zeros(3, 4, 4, dtype=torch.float64), (torch.zeros(1, 2, 4, dtype=torch.float64), torch.full((1, 2), -1, dtype=torch.int32))
    for args, kw, match in (((ok.int(), None, ref, age), {}, "float32 or float64"), ((ok[0], None, ref, age), {}, r"\[F,D,4\]"),
                            ((ok[:, :, :3], None, ref, age), {}, r"\[F,D,4\]"), ((ok[:0], None, ref, age), {}, r"\[F,D,4\]"),
                            ((torch.zeros(3, 33, 4), None, ref, age), {}, "at most 32"), ((ok, None, ref, age), dict(box_format="cxcywh"), "box_format"),
                            ((ok, None, ref, age), dict(min_iou=0.0), "min_iou"), ((ok, None, ref, age), dict(min_iou=1.5), "min_iou"),
                            ((ok, None, ref, age), dict(max_missed=-1), "max_missed"), ((ok, None, ref, age), dict(max_missed=1.5), "max_missed"),
                            ((ok, None, None, None), {}, "state is missing"), ((ok, None, ref.float(), age), {}, "float64"),
                            ((ok, None, ref, age.long()), {}, "int32"), ((ok, None, torch.zeros(1, 3, 4, dtype=torch.float64), age), {}, "ref must be"),
                            ((ok, None, torch.zeros(1, 17, 4, dtype=torch.float64), torch.zeros(1, 17, dtype=torch.int32)), {}, "P <= 16"),
                            ((ok, torch.zeros(2, dtype=torch.int32), ref, age), {}, "stream_of")):
        with pytest.raises(ValueError, match=match):
            ops.track_assign(*args, **kw)
    with pytest.raises(ValueError, match="restart"):
        ops.crop_track(ok[0], None, (64, 48), restart=torch.zeros(3, dtype=torch.int32))
    assert not w.lib.calls


class _BothBuilds:
    """the association from the threaded build (its argmax is a wave exchange), every other entry point from the loop build, which
    runs the crops and the pastes of whole frames in reasonable time"""

    def __init__(self, loop, threads):
        self._loop, self._threads = loop, threads

    def __getattr__(self, name):
        return getattr(self._threads if name == NAME else self._loop, name)


@pytest.fixture()
def both_builds(monkeypatch):
    import emulibs
    lib = _BothBuilds(emulibs.stream(False), emulibs.stream(True))
    monkeypatch.setattr(emulibs, "stream", lambda threaded: lib)


@pytest.fixture()
def rig(both_builds, video):
    """the recorder rig of tests/test_crop_track_emul.py (`video`) in front of both builds"""
    return video


def test_the_plans_checks_come_before_any_launch(rig):
    w, N, (H, W) = rig, 5, (40, 56)
    clip = _clip(N, (H, W), 16)
    dets = torch.zeros(N, 4, 4, dtype=torch.float64)
    tr = dict(tracks=2)
    w.lib.calls.clear()
    w.recorded.clear()
    for kw, match in ((dict(detections=dets, boxes=dets[:, 0], tracking=tr), "mutually exclusive"),
                      (dict(detections=dets, windows=[(8, 4, 16)] * N, tracking=tr), "mutually exclusive"),
                      (dict(detections=dets, faces=[[(8, 4, 16)]] * N, tracking=tr), "mutually exclusive"),
                      (dict(detections=dets), "tracks=P"), (dict(detections=dets, tracking=dict(smooth=True)), "tracks=P"),
                      (dict(detections=dets, tracking=dict(tracks=5), batch_size=4), "batch_size"),
                      (dict(detections=dets, tracking=dict(tracks=17), batch_size=32), "1 ... 16"),
                      (dict(detections=dets, tracking=dict(tracks=0)), "1 ... 16"), (dict(detections=dets, tracking=dict(tracks=2.0)), "1 ... 16"),
                      (dict(detections=torch.zeros(N, 33, 4), tracking=tr), "at most 32"),
                      (dict(detections=iter([torch.zeros(N, 33, 4)]), tracking=tr), "at most 32"),
                      (dict(detections=dets[:, 0], tracking=tr), r"\[N,D,4\]"), (dict(detections=dets[:4], tracking=tr), "rows for 5 frames"),
                      (dict(detections=dets.int(), tracking=tr), "float32 or float64"),
                      (dict(detections=dets, tracking=dict(tracks=2, min_iou=0.0)), "min_iou"),
                      (dict(detections=dets, tracking=dict(tracks=2, min_iou=1.1)), "min_iou"),
                      (dict(detections=dets, tracking=dict(tracks=2, max_missed=-1)), "max_missed"),
                      (dict(boxes=dets[:, :2], tracking=tr), "detections= is missing"),
                      (dict(detections=dets, tracking=tr, identities=[0] * N), "one slot per track"),
                      (dict(detections=dets, tracking=tr, smooth_pose=True), "smooth_per_identity")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(clip, **kw))
    assert not w.lib.calls and not w.recorded


def _two_faces(N=12, W=128, H=96):
    """the two walks of tests/test_crop_track_gpu.py's two-track test, as ordered boxes [N,2,4] and as detections [N,4,4] (C.permuted)"""
    both = np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)
    return (both,) + C.permuted(both)


def test_detections_are_the_ordered_boxes_on_the_rig(rig):
    """animate_frames(detections=) against animate_frames(boxes=[N,2,4]): the same windows cropped and pasted, the same rows driven,
    the same frames out, for batch sizes 3 and 8, one chunk and chunks of 5, one rank and two"""
    w, N, (H, W) = rig, 12, (96, 128)
    both, dets, at = _two_faces(N, W, H)
    min_iou = 0.2
    same = min(C._iou(both[t, p], both[t + 1, p]) for t in range(N - 1) for p in (0, 1))
    cross = max(C._iou(both[t, p], both[u, 1 - p]) for t in range(N) for u in range(N) for p in (0, 1))
    print(f"same-face consecutive IoU >= {same:.4f}, cross-face IoU <= {cross:.4f}")
    assert same > min_iou > cross                                               # (0.5386 and, over all pairs of frames, 0.0794)
    ref, age = np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32)
    boxes, restart, track_of = C.reference(dets, None, ref, age, min_iou, 15, 0)
    assert np.array_equal(boxes.view(np.uint64), both.view(np.uint64)) and restart.tolist() == [[1, 1]] + [[0, 0]] * (N - 1)
    assert all(track_of[t, at[t]].tolist() == [0, 1] for t in range(N))
    clip = _clip(N, (H, W), 21)
    ids = [0, 2] * N
    tracking = dict(smooth=True, momentum=0.5)
    td, tb = torch.from_numpy(dets), torch.from_numpy(both)
    for kw in (dict(as_uint8=False), dict(paste_back=True, feather=0.1)):
        for bs in (3, 8):
            w.reset_crop_state()
            w.lib.calls.clear()
            want = _run(w, clip, boxes=tb, tracking=tracking, identities=ids, batch_size=bs, **kw)
            assert NAME not in w.lib.calls and RESTARTS not in w.lib.calls and len(want[2]) == 2 * N
            assert "paste_back" not in kw or not torch.equal(want[0], clip)
            runs = [dict(frames=clip, detections=td), dict(frames=clip, detections=td.float().double()),
                    dict(frames=iter([clip[:5], clip[5:10], clip[10:]]), detections=td),
                    dict(frames=iter([clip[:5], clip[5:10], clip[10:]]), detections=iter([td[:5], td[5:10], td[10:]]))]
            for k, run in enumerate(runs):
                w.reset_crop_state()
                w.lib.calls.clear()
                got = _run(w, run.pop("frames"), tracking=dict(tracking, tracks=2, min_iou=min_iou), identities=ids, batch_size=bs, **run, **kw)
                assert got[2] == want[2] and got[3] == want[3], (bs, k)
                assert torch.equal(got[0], want[0]) and all(torch.equal(x, y) for x, y in zip(got[1], want[1])), (bs, k)
                chunks = 1 if k < 2 else 3
                assert w.lib.calls[NAME] == chunks == w.lib.calls[RESTARTS] and "emo_crop_track_f64" not in w.lib.calls
                lo = 0 if k < 2 else 10
                assert w.tracked_assignment[0].tolist() == track_of[lo:].tolist() and w.tracked_assignment[1].tolist() == restart[lo:].tolist()
            halves = []
            for rank in (0, 1):
                w.reset_crop_state()
                w.rank, w.world = rank, 2
                halves.append(_run(w, clip, detections=td, tracking=dict(tracking, tracks=2, min_iou=min_iou), identities=ids, batch_size=bs, **kw))
                assert w._track_states.age.tolist() == [[0, 0]]
            w.rank, w.world = 0, 1
            assert halves[0][2] + halves[1][2] == want[2] and halves[0][3] + halves[1][3] == want[3]
            assert torch.equal(torch.cat([halves[0][0], halves[1][0]]), want[0])
    # the resets free the tracks; without the keyword nothing of this is launched
    w.reset_crop_state()
    assert w._track_states.age.tolist() == [[-1, -1]]
    _run(w, clip[:2], detections=td[:2], tracking=dict(tracks=2), identities=ids[:4], batch_size=4, as_uint8=False)
    assert w._track_states.age.tolist() == [[0, 0]]
    w.reset_crop_state([1])
    assert w._track_states.age.tolist() == [[0, -1]]
    assert w.forward(reset_tracking=True) is None and w._track_states.age.tolist() == [[-1, -1]]
    w.lib.calls.clear()
    _run(w, clip, boxes=tb, identities=ids, batch_size=4, as_uint8=False, detections=None)
    assert NAME not in w.lib.calls and RESTARTS not in w.lib.calls
