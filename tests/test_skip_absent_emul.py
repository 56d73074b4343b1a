"""Skipping the rows without a face, without a GPU: emo_present_rows_i32 (csrc/smallops.hip), compiled for the host from the product's
own source (tests/emul/emulibs.stream(True): OS threads, a real barrier), on the cases of tests/present_rows_cases.py against
hostglue.present_rows bit for bit, and that restatement against a plain loop written from the header; the refusals; the header.
Then the plan's checks and InferenceWrapper.animate_frames(tracking=dict(skip_absent=True)) on the recorder rigs of
tests/test_crop_track_emul.py / tests/test_track_assign_emul.py (the windows cropped and pasted) and of
tests/test_track_controls_emul.py (the rows the controls and the driver pass are handed).  Integers and bits: no tolerances."""
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
import present_rows_cases as C  # noqa: E402
import test_track_assign_emul as TA  # noqa: E402
import test_track_controls_emul as TC  # noqa: E402
from test_crop_track_emul import _clip, _restated, _run, video  # noqa: E402,F401
from test_crop_track_gpu import _walk  # noqa: E402
from test_track_assign_emul import both_builds  # noqa: E402,F401
from test_track_controls_emul import rig as controls_rig  # noqa: E402,F401

NAME = "emo_present_rows_i32"
V, I = ctypes.c_void_p, ctypes.c_int
ARGTYPES = [V, V, I, I] + [V] * 6
CASES = C.cases()
BAD_ARG = -1


@pytest.fixture(scope="module")
def stream():
    import emulibs
    return emulibs.stream(True)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def raw(lib, crop, paste, F, P, outs):
    fn = getattr(lib, NAME)
    fn.argtypes, fn.restype = ARGTYPES, ctypes.c_int
    return fn(_p(crop), _p(paste), F, P, *[_p(o) for o in outs], None)


def _same(a, b):
    return all(x.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 5


# ---- 1. the restatement against the plain loop, the kernel against the restatement -----------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_restatement_is_the_plain_loop_reference(name):
    from emoportraits_amd import hostglue
    crop, paste, F, P = CASES[name]
    assert _same(hostglue.present_rows(crop, paste, F, P), C.reference(crop, paste, F, P))


def test_the_cases_show_what_they_are_there_for():
    T = {name: int((c[1][:, 2] > 0).sum()) for name, c in CASES.items()}
    assert T["one_present"] == 1 and T["one_absent"] == 0 and T["all_absent"] == 0 and T["all_present"] == 12
    count = C.reference(*CASES["mixed_5x3"])[0].tolist()
    assert count == [2, 0, 2, 0, 3]
    assert CASES["sixteen_tracks"][3] == 16 and 0 < T["sixteen_tracks"] < 7 * 16
    assert sorted(c[2] * c[3] for name, c in CASES.items() if name.startswith("rows_")) == [255, 256, 257, 1120]
    assert T["odd_absent"] == 5                                                  # a negative side and a side of 0 beside x / y: absent
    assert all(0 < T[f"rows_{M}"] < M for M in (255, 256, 257, 1120))


@pytest.mark.parametrize("name", CASES)
def test_kernel_is_the_restatement(stream, name):
    from emoportraits_amd import hostglue
    crop, paste, F, P = CASES[name]
    before = crop.copy(), paste.copy()
    outs = C.prefilled(F, P)
    assert raw(stream, crop, paste, F, P, outs) == 0
    assert _same(outs, hostglue.present_rows(crop, paste, F, P)), name
    assert not any((o == np.int32(C.FILL)).any() for o in outs)                  # every element of every output is written
    assert np.array_equal(crop, before[0]) and np.array_equal(paste, before[1])


def test_refusals_return_bad_arg_and_write_nothing(stream):
    crop, paste, F, P = CASES["mixed_5x3"]
    for bad in range(7):                                                         # a NULL pointer, each in turn
        outs = C.prefilled(F, P)
        args = [crop, paste] + outs
        args[bad] = None
        fn = getattr(stream, NAME)
        fn.argtypes, fn.restype = ARGTYPES, ctypes.c_int
        assert fn(_p(args[0]), _p(args[1]), F, P, *[_p(a) for a in args[2:]], None) == BAD_ARG
        assert all((o == np.int32(C.FILL)).all() for o in outs)
    for F_, P_ in ((0, 3), (-1, 3), (5, 0), (5, 17), (1 << 21, 16), ((1 << 24) + 1, 1)):
        outs = C.prefilled(F, P)
        assert raw(stream, crop, paste, F_, P_, outs) == BAD_ARG and all((o == np.int32(C.FILL)).all() for o in outs)
    # an output that is, or overlaps, an input
    outs = C.prefilled(F, P)
    keep = crop.copy(), paste.copy()
    for at, alias in ((3, crop), (4, paste), (3, paste), (2, crop.reshape(-1)[:F * P]), (0, paste.reshape(-1)[4:4 + F]),
                      (1, crop.reshape(-1)[8:9 + F]), (4, crop[1:])):
        args = list(outs)
        args[at] = alias
        assert raw(stream, crop, paste, F, P, args) == BAD_ARG
    assert np.array_equal(crop, keep[0]) and np.array_equal(paste, keep[1]) and all((o == np.int32(C.FILL)).all() for o in outs)
    assert raw(stream, crop, paste, F, P, outs) == 0                             # (the arguments were good but for the one)


def test_the_entry_point_is_in_the_header_and_the_abi_table():
    from emoportraits_amd import _abi_version, hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "ABI 27." in hdr and "int emo_present_rows_i32(const int32_t* crop, const int32_t* paste, int F, int P," in hdr
    assert _abi_version.EMO_ABI_VERSION >= 27 and "#define EMO_ABI_VERSION %d" % _abi_version.EMO_ABI_VERSION in hdr
    assert list(hip.SIGNATURES[NAME]) == ARGTYPES


# ---- 2. ops, the plan's checks and the wrapper on the recorder rigs ----------------------------------------------------------------------
class _Builds:
    """the association and the compaction from the threaded build (a wave exchange, a barrier), every other entry point from the
    loop build, which runs the crops and the pastes of whole frames in reasonable time"""

    def __init__(self, loop, threads):
        self._loop, self._threads = loop, threads

    def __getattr__(self, name):
        return getattr(self._threads if name in (TA.NAME, NAME) else self._loop, name)


@pytest.fixture()
def windows_rig(monkeypatch, request):
    """the recorder rig of tests/test_crop_track_emul.py (`video`) behind tests/test_track_assign_emul.py's two builds"""
    monkeypatch.setattr(TA, "_BothBuilds", _Builds)
    request.getfixturevalue("both_builds")
    return request.getfixturevalue("video")


@pytest.fixture()
def rig(monkeypatch, request):
    """the recorder rig of tests/test_track_controls_emul.py, the compaction from the threaded build"""
    monkeypatch.setattr(TC, "_BothBuilds", _Builds)
    return request.getfixturevalue("controls_rig")


def test_ops_present_rows_is_the_restatement_and_checks_its_arguments(rig):
    from emoportraits_amd import hostglue, ops
    w = rig
    w.lib.calls.clear()
    for name in ("mixed_5x3", "rows_257", "all_absent"):
        crop, paste, F, P = CASES[name]
        got = ops.present_rows(torch.from_numpy(crop), torch.from_numpy(paste), F, P)
        assert _same([g.numpy() for g in got], hostglue.present_rows(crop, paste, F, P)), name
    assert w.lib.calls[NAME] == 3
    w.lib.calls.clear()
    ok = torch.zeros(6, 4, dtype=torch.int32)
    for args, match in (((ok.long(), ok, 3, 2), "int32"), ((ok, ok[:5], 3, 2), r"\[6,4\]"), ((ok, ok, 2, 2), r"\[4,4\]"),
                        ((ok, ok.t().contiguous().t(), 3, 2), "contiguous"), ((ok, ok, 0, 2), "F >= 1"), ((ok, ok, 3, 17), "P <= 16"),
                        ((ok.tolist(), ok, 3, 2), "int32")):
        with pytest.raises(ValueError, match=match):
            ops.present_rows(*args)
    assert not w.lib.calls


def _dropouts(N=10, W=128, H=96):
    """boxes [N,2,4] of two faces that keep apart, column 1 missing in frames 0-2 and 6-7, column 0 in frame 4 -> (boxes, the
    restated crop and paste windows of all rows, present [2N])"""
    both = np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)
    both[[0, 1, 2, 6, 7], 1] = np.nan
    both[4, 0] = np.nan
    crop, paste, _ = _restated(both.reshape(-1, 4), (W, H), so=np.tile(np.int32([0, 1]), N), K=2, smooth=True, momentum=0.5)
    return both, crop, paste, paste[:, 2] > 0


def test_the_plans_checks_come_before_any_launch(windows_rig):
    w, N, (H, W) = windows_rig, 10, (96, 128)
    clip = _clip(N, (H, W), 40)
    boxes = torch.from_numpy(_dropouts(N)[0])
    skip = dict(skip_absent=True)
    ids = [0, 2] * N
    w.lib.calls.clear()
    w.recorded.clear()
    w.tracked_windows = w.tracked_rows = "untouched"
    for kw, match in ((dict(tracking=skip), "boxes= is missing.*skip_absent"),
                      (dict(boxes=boxes[:, 0], tracking=skip), r"\[N,1,4\]"),
                      (dict(boxes=boxes, tracking=skip, as_uint8=False, to_host=False), "as_uint8=False"),
                      (dict(boxes=boxes, tracking=skip, identities=ids, smooth_pose=True, smooth_per_identity=True), "follow_tracks"),
                      (dict(boxes=boxes, tracking=skip, identities=ids, expression=dict(relative=True)), "follow_tracks"),
                      (dict(boxes=boxes, tracking=skip, identities=ids, expression=dict(smooth=True)), "follow_tracks"),
                      (dict(boxes=boxes, tracking=skip, identities=ids, head_pose=dict(relative=True)), "follow_tracks"),
                      (dict(boxes=boxes, tracking=dict(skip_absent=True, follow_tracks=False), identities=ids, smooth_pose=True,
                            smooth_per_identity=True), "cannot be left out"),
                      (dict(boxes=boxes, tracking=dict(skip_absents=True)), "no field")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(clip, **kw))
    with pytest.raises(ValueError, match="skip_absent"):
        next(w.animate_streams([dict(frames=clip, boxes=boxes[:, 0])], tracking=skip))
    assert not w.lib.calls and not w.recorded and w.tracked_windows == w.tracked_rows == "untouched"


def test_skipped_rows_are_neither_cropped_nor_driven_nor_pasted(windows_rig):
    """boxes [N,2,4] with dropouts: the crop op, the driver pass and the paste op are handed the present rows' windows and nothing
    else -- what faces= of those windows hands them -- whatever the batch size, the chunking and the number of ranks; tracked_rows
    says which rows they are"""
    w, N, (H, W) = windows_rig, 10, (96, 128)
    both, crop, paste, present = _dropouts(N, W, H)
    assert present.reshape(N, 2).sum(1).tolist() == [1, 1, 1, 2, 1, 2, 1, 1, 2, 2] and np.array_equal(crop[present], paste[present])
    clip, tb = _clip(N, (H, W), 41), torch.from_numpy(both)
    ids = [0, 2] * N
    faces = [[tuple(crop[2 * i + p][:3]) for p in (0, 1) if present[2 * i + p]] for i in range(N)]
    kept_ids = [ids[i] for i in range(2 * N) if present[i]]
    tracking = dict(smooth=True, momentum=0.5, skip_absent=True)
    kept, first = np.nonzero(present)[0], np.concatenate([[0], np.cumsum(present.reshape(N, 2).sum(1))])
    for kw in (dict(), dict(paste_back=True, feather=0.1)):
        for bs in (2, 4, 16):
            want = _run(w, clip, faces=faces, identities=kept_ids, batch_size=bs, **kw)
            assert want[2] == crop[present].tolist() and len(want[1][0]) == present.sum()
            runs = [dict(frames=clip, boxes=tb), dict(frames=iter([clip[:3], clip[3:4], clip[4:]]), boxes=tb),
                    dict(frames=iter([clip[:7], clip[7:]]), boxes=iter([tb[:7], tb[7:]]))]
            for k, run in enumerate(runs):
                w.reset_crop_state()
                assert w.tracked_rows is None
                w.lib.calls.clear()
                got = _run(w, run.pop("frames"), tracking=tracking, identities=ids, batch_size=bs, **run, **kw)
                assert got[2] == crop[present].tolist() and got[3] == (paste[present].tolist() if kw else []), (bs, k)
                assert torch.equal(got[0], want[0]), (bs, k)
                assert all(torch.equal(x, y) for x, y in zip(got[1], want[1])), (bs, k)
                chunks = (1, 3, 2)[k]
                assert w.lib.calls[NAME] == chunks == w.lib.calls["emo_crop_track_f64"]
                lo = (0, 4, 7)[k]                                                # the last chunk's first frame
                rows, offs, row0 = w.tracked_rows
                assert rows.dtype == torch.int32 and rows.tolist() == (kept[kept >= 2 * lo] - 2 * lo).tolist()
                assert offs == (first[lo:] - first[lo]).tolist() and row0 == 2 * lo
                assert w.tracked_windows[1] == 2 * lo and w.tracked_windows[0].tolist() == paste[2 * lo:].tolist()
        # two ranks: each compacts the whole chunk and serves the kept rows of its frames
        halves = []
        for rank in (0, 1):
            w.reset_crop_state()
            w.rank, w.world = rank, 2
            try:
                halves.append(_run(w, clip, boxes=tb, tracking=tracking, identities=ids, batch_size=4, **kw))
            finally:
                w.rank, w.world = 0, 1
        want = _run(w, clip, faces=faces, identities=kept_ids, batch_size=4, **kw)
        assert halves[0][2] + halves[1][2] == want[2] and halves[0][3] + halves[1][3] == want[3]
        assert torch.equal(torch.cat([halves[0][0], halves[1][0]]), want[0])
    # what is yielded: the index of the batch's first kept row, or with paste_back of its first frame
    w.reset_crop_state()
    at = [i for i, _ in w.animate_frames(clip, boxes=tb, tracking=tracking, identities=ids, batch_size=4, to_host=False)]
    spans = [(0, 3), (3, 5), (5, 8), (8, 10)]                                    # at most 4 kept rows: counts 1 1 1 | 2 1 | 2 1 1 | 2 2
    from emoportraits_amd import frames as frames_mod
    assert frames_mod.face_spans(present.reshape(N, 2).sum(1).tolist(), 0, N, 4) == spans
    assert at == [int(first[a]) for a, _ in spans]
    w.reset_crop_state()
    at = [i for i, _ in w.animate_frames(clip, boxes=tb, tracking=tracking, identities=ids, batch_size=4, to_host=False, paste_back=True)]
    assert at == [a for a, _ in spans]
    # without the field every row is rendered and nothing is compacted
    w.reset_crop_state()
    w.lib.calls.clear()
    got = _run(w, clip, boxes=tb, tracking=dict(smooth=True, momentum=0.5), identities=ids, batch_size=4)
    assert NAME not in w.lib.calls and len(got[2]) == 2 * N and w.tracked_rows is None


def _states(w):
    s = w._bank_streams
    return [t.clone() for t in (s.theta, s.theta_has, s.pose_anchor, s.pose_anchor_has, s.expr_anchor, s.expr_anchor_has, s.expr_ema, s.expr_ema_has)]


def _same_states(a, b):
    """the flags, and the state under a set flag, bit for bit"""
    return all(torch.equal(a[i], b[i]) and torch.equal(a[i - 1][a[i] != 0].view(torch.int32), b[i - 1][b[i] != 0].view(torch.int32))
               for i in (1, 3, 5, 7))


def _drive(w, frames, dets, **kw):
    """TC._drive for a call that yields bytes: -> the rows the driver pass was handed, (pose, theta [rows,16]) as numpy"""
    w.recorded.clear(), w.regressed.clear(), w.embedded.clear()
    for v in w.seen.values():
        v.clear()
    w.lib.calls.clear()
    for _ in w.animate_frames(frames, detections=dets, to_host=False, **kw):
        pass
    if not w.recorded:                                                           # (a rank whose frames nobody is in)
        return np.zeros((0, TC.E5), np.float32), np.zeros((0, 16), np.float32)
    return torch.cat([r[0] for r in w.recorded]).numpy(), torch.cat([r[1] for r in w.recorded]).numpy().reshape(-1, 16)


def empty_frames_clip(N=12):
    """face A in frames 0 ... 3, a second face B in frames 0 and 1, nobody in frames 4 ... 7, face C from frame 8: with max_missed =
    2 B's track dies in frame 4 and A's in frame 6, both in frames nobody is in, and B's slot is never taken again -> dets [N,4,4]"""
    dets = np.full((N, 4, 4), np.nan)
    for t in range(N):
        if t < 4:
            dets[t, 1] = TC._box(40 + t, 44 - t, 14)
        if t < 2:
            dets[t, 3] = TC._box(96 - t, 40 + t, 12)
        if t >= 8:
            dets[t, 2] = TC._box(44 - t, 50 + t % 3, 16)
    return dets


@pytest.mark.parametrize("dets", [TC.birth_clip(), empty_frames_clip()], ids=["birth_clip", "empty_frames"])
def test_the_controls_walk_the_full_rows_and_the_kept_rows_are_those_of_the_call_that_skips_nothing(rig, monkeypatch, dets):
    """the birth clip of tests/test_track_controls_emul.py (a birth, a death, a dropout; somebody in every frame) and a clip whose
    tracks die in frames nobody is in, with the three controls that carry state: the rows driven are the kept rows of the call
    without the field, bit for bit; the control ops are handed the full rows of their frames, zeros where a row is absent, and the
    tracker's masks -- also for the batches that hold no face; the streams end as they do there; whatever the batch size and the
    chunking, on one rank, two and three"""
    from emoportraits_amd import parallel
    w, N, (H, W) = rig, 12, (96, 128)
    clip = TC._clip(N, (H, W), 31)
    restart, present = TC._tracker(dets, W, H)
    keep = present.astype(bool)
    assert 0 < keep.sum() < 2 * N and restart[~keep].any()                       # (a restart in a row that is left out)
    if not np.isfinite(dets[4:8]).any():
        assert not present[8:16].any() and restart[8:16].reshape(4, 2).tolist() == [[0, 1], [0, 0], [1, 0], [0, 0]]
    ids, td = [0, 2] * N, torch.from_numpy(dets)
    follow = dict(TC.TRACKING, follow_tracks=True)
    TC._reset(w)
    from emoportraits_amd import ops
    edits, controls = [], ops.head_pose_controls

    def head_pose_controls(*args, **kwargs):
        out = controls(*args, **kwargs)
        edits.append(out[0].clone())
        return out
    monkeypatch.setattr(ops, "head_pose_controls", head_pose_controls)
    pose, theta = _drive(w, clip, td, tracking=follow, identities=ids, batch_size=4, **TC.CONTROLS)
    assert pose.shape[0] == 2 * N
    edited = torch.cat(edits)[torch.from_numpy(keep)]                            # the edited (scale, rotation, translation) of the kept rows
    states = _states(w)
    full_in = {kind: torch.cat([s[0] for s in w.seen[kind]]) for kind in w.seen}
    assert NAME not in w.lib.calls
    skip = dict(follow, skip_absent=True)
    for kw in (dict(frames=clip, detections=td, batch_size=4), dict(frames=clip, detections=td, batch_size=2),
               dict(frames=clip, detections=td, batch_size=16), dict(frames=iter([clip[:5], clip[5:7], clip[7:]]), detections=td, batch_size=4),
               dict(frames=iter([clip[:7], clip[7:]]), detections=iter([td[:7], td[7:]]), batch_size=6)):
        TC._reset(w)
        got = _drive(w, kw.pop("frames"), kw.pop("detections"), tracking=skip, identities=ids, **kw, **TC.CONTROLS)
        assert TC.C.same_bits(got[0], pose[keep]) and TC.C.same_bits(got[1], theta[keep]), kw
        assert _same_states(_states(w), states), kw
        # pred_target_srt is the last batch's edit of the rows it rendered: its kept rows, not the full rows of its frames
        left = torch.cat(w.pred_target_srt, 1)
        assert 1 <= left.shape[0] <= kw["batch_size"] and torch.equal(left.view(torch.int32), edited[-left.shape[0]:].view(torch.int32)), kw
        assert sum(r.shape[0] for r in w.regressed) == keep.sum() == sum(e.shape[0] for e in w.embedded)
        for kind in ("scan", "expr", "pose"):
            rows, r, p = (torch.cat([s[i] for s in w.seen[kind]]) for i in (0, 1, 2))
            assert r.tolist() == restart.tolist() and p.tolist() == present.tolist(), kind
            assert not rows[~torch.from_numpy(keep)].any(), kind
            if kind != "scan":                                                   # (the scan's input is the edited theta: see got[1])
                assert torch.equal(rows[torch.from_numpy(keep)].view(torch.int32), full_in[kind][torch.from_numpy(keep)].view(torch.int32))
    assert w.tracked_present[0].tolist() == present[14:].tolist() and w.tracked_rows[2] == 14
    # several ranks: the kept rows are gathered, sized from `first`, and scattered into the chunk's full rows on every rank
    TC._reset(w)
    _drive(w, clip, td, tracking=skip, identities=ids, batch_size=4, **TC.CONTROLS)
    kept_in = {(9,): torch.cat([s[0] for s in w.seen["pose"]])[keep], (4, 4): w.seen["scan"][0][0][keep].clone(),
               (TC.E5,): torch.cat([s[0] for s in w.seen["expr"]])[keep]}
    gathers = []

    def gather_rows(local, counts, rank, world):
        whole = kept_in[tuple(local.shape[1:])]
        lo = sum(counts[:rank])
        assert whole.shape[0] == sum(counts) and torch.equal(local.view(torch.int32), whole[lo:lo + counts[rank]].view(torch.int32))
        gathers.append(tuple(local.shape[1:]))
        return whole.clone()
    monkeypatch.setattr(parallel, "gather_rows", gather_rows)
    for world in (2, 3):
        parts = []
        for rank in range(world):
            TC._reset(w)
            gathers.clear()
            w.rank, w.world = rank, world
            try:
                parts.append(_drive(w, clip, td, tracking=skip, identities=ids, batch_size=4, **TC.CONTROLS))
            finally:
                w.rank, w.world = 0, 1
            assert sorted(gathers) == [(4, 4), (TC.E5,), (9,)]
            assert w.lib.calls[NAME] == 1 and all(w.lib.calls[TC.NEW[k]] == 1 for k in TC.NEW)
            for kind in ("scan", "expr", "pose"):
                assert w.seen[kind][0][0].shape[0] == 2 * N == w.seen[kind][0][2].shape[0]
            assert _same_states(_states(w), states), (world, rank)
            # (the pass over the gathered rows edits the chunk's full rows, and pred_target_srt is left as that edit)
            left = torch.cat(w.pred_target_srt, 1)
            assert left.shape[0] == 2 * N and torch.equal(left[torch.from_numpy(keep)].view(torch.int32), edited.view(torch.int32)), (world, rank)
        assert TC.C.same_bits(np.concatenate([p[0] for p in parts]), pose[keep]), world
        assert TC.C.same_bits(np.concatenate([p[1] for p in parts]), theta[keep]), world
