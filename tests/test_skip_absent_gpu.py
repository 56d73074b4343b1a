"""Skipping the rows without a face, on the GPU: ops.present_rows against hostglue.present_rows on the cases of
tests/present_rows_cases.py; then animate_frames(tracking=dict(skip_absent=True)) against calls whose answer needs no arithmetic:
it is the faces= call on the present rows' windows, byte for byte, crops and pasted frames, rgb8 and NV12; with the controls that
carry state it is that faces= call with the same controls, and it leaves the streams as the call that skips nothing leaves them;
a face born after everybody had left is rendered as in a fresh call on the clip from its birth on; and the refusals come before
any launch.  Tiny fixture, toy embedders, every output ops allocates poisoned and between guards.  No tolerances."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import present_rows_cases as C  # noqa: E402
from test_crop_track_gpu import _clip, _walk  # noqa: E402
from test_head_pose_controls_gpu import make_wrapper, project, tiny  # noqa: E402,F401

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"
TRACK = dict(smooth=True, momentum=0.5)
CONTROLS = dict(smooth_pose=True, smooth_per_identity=True, expression=dict(relative=True, smooth=True, momentum=0.4),
                head_pose=dict(relative=True))


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------
def test_ops_present_rows_is_the_restatement():
    """every case; the outputs come poisoned from the guarded allocator, so an element the kernel leaves out fails the comparison"""
    from emoportraits_amd import hostglue, ops
    for name, (crop, paste, F, P) in C.cases().items():
        got = ops.present_rows(torch.from_numpy(crop).to(DEV), torch.from_numpy(paste).to(DEV), F, P)
        want = hostglue.present_rows(crop, paste, F, P)
        assert len(got) == 5 and all(g.dtype == torch.int32 and g.device.type == "cuda" for g in got)
        for g, h, what in zip(got, want, ("count", "first", "row_of", "crop_out", "paste_out")):
            assert g.shape == h.shape and np.array_equal(g.cpu().numpy(), h), (name, what)
    ok = torch.zeros(6, 4, dtype=torch.int32, device=DEV)
    for args, match in (((ok.long(), ok, 3, 2), "int32"), ((ok, ok[:5], 3, 2), r"\[6,4\]"), ((ok, ok, 3, 17), "P <= 16"),
                        ((ok, ok.cpu(), 3, 2), "different devices")):
        with pytest.raises(ValueError, match=match):
            ops.present_rows(*args)


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapper(project, tiny):
    return make_wrapper(project, tiny, K=2)


def _run(w, clip, **kw):
    """a call from reset state -> (its outputs in order, on the host; the index yielded with each batch; the rows of each batch)"""
    w.reset_crop_state(), w.reset_pose_state(), w.reset_expression_state()
    out = [(i, o.clone()) for i, o in w.animate_frames(clip, to_host=False, **kw)]
    torch.cuda.synchronize()
    assert [i for i, _ in out] == sorted(i for i, _ in out)
    return torch.cat([o for _, o in out]).cpu(), [i for i, _ in out], [o.shape[0] for _, o in out]


def _faces_of(w, N, P, ids):
    """from tracked_windows of the call just made (one chunk): faces= of the present rows' windows, their slots, the counts"""
    paste, row0 = w.tracked_windows
    assert row0 == 0 and paste.shape == (N * P, 4)
    paste = paste.cpu().reshape(N, P, 4)
    faces = [[tuple(paste[i, p, :3].tolist()) for p in range(P) if paste[i, p, 2] > 0] for i in range(N)]
    slots = [ids[i * P + p] for i in range(N) for p in range(P) if paste[i, p, 2] > 0]
    return faces, slots, [len(f) for f in faces]


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_skipping_is_the_faces_call_on_the_present_windows_byte_for_byte(wrapper, tiny, fmt):
    """10 frames of 96 x 128, boxes [N,2,4], column 1 missing in frames 0 - 2 and 6 - 7, column 0 in frame 4, batches of at most 4
    rows: both calls form their batches with frames.face_spans on the same counts"""
    from emoportraits_amd import frames as frames_mod
    w, N, H, W = wrapper, 10, 96, 128
    clip = _clip(N, H, W, fmt, 101)
    both = np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)
    both[[0, 1, 2, 6, 7], 1] = np.nan
    both[4, 0] = np.nan
    tb, ids = torch.from_numpy(both).to(DEV), [0, 1] * N
    for paste_back in (True, False):
        kw = dict(frame_format=fmt, paste_back=paste_back, batch_size=4)
        every_row, _, _ = _run(w, clip, boxes=tb, tracking=TRACK, identities=ids, **kw)
        assert w.tracked_rows is None
        faces, slots, count = _faces_of(w, N, 2, ids)
        assert count == [1, 1, 1, 2, 1, 2, 1, 1, 2, 2]
        A, at_a, rows_a = _run(w, clip, boxes=tb, tracking=dict(TRACK, skip_absent=True), identities=ids, **kw)
        row_of, first, full0 = w.tracked_rows
        assert first == frames_mod.face_offsets(count) and full0 == 0 and row_of.dtype == torch.int32
        assert row_of.cpu().tolist() == [2 * i + p for i in range(N) for p in (0, 1) if not np.isnan(both[i, p, 0])]
        B, at_b, rows_b = _run(w, clip, faces=faces, identities=slots, **kw)
        assert A.shape == B.shape and torch.equal(A, B), (fmt, paste_back)
        assert at_a == at_b and rows_a == rows_b
        spans = frames_mod.face_spans(count, 0, N, 4)
        if paste_back:
            assert A.shape[0] == N and at_a == [b0 for b0, _ in spans]
            assert all(not torch.equal(A[t], clip[t]) for t in range(N))         # (somebody in every frame)
        else:
            assert A.shape[0] == sum(count) < every_row.shape[0] == 2 * N and at_a == [first[b0] for b0, _ in spans]


def _dropout_detections(N, W, H):
    """two faces as detections [N,3,4] in changing rows: face a from frame 0, dropped in frame 4; face b from frame 3, dropped in
    frames 6 and 7 -- dropouts only: with max_missed = 15 no track dies, a is track 0 and b track 1"""
    both = np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)
    both[[0, 1, 2, 6, 7], 1] = np.nan
    both[4, 0] = np.nan
    dets = np.full((N, 3, 4), np.nan)
    for t in range(N):
        dets[t, t % 3], dets[t, (t + 1) % 3] = both[t, 1], both[t, 0]
    return dets


def _streams(w):
    s = w._bank_streams
    return [t.cpu().clone() for t in (s.theta, s.theta_has, s.pose_anchor, s.pose_anchor_has, s.expr_anchor, s.expr_anchor_has, s.expr_ema,
                                      s.expr_ema_has)]


def test_skipping_with_the_controls_that_carry_state(wrapper, tiny):
    """detections=, two slots, dropouts only; follow_tracks with smooth_pose, a smoothed relative expression and a relative head
    pose.  The skipped call is the faces= call with the same controls and identities, byte for byte: both walk the same rows of the
    same identity streams from a fresh state.  The streams' flags, and the state under a set flag, are those the call that skips
    nothing leaves"""
    from emoportraits_amd import hostglue
    w, N, H, W = wrapper, 10, 96, 128
    clip, dets = _clip(N, H, W, "rgb8", 111), _dropout_detections(N, W, H)
    assoc = dict(min_iou=0.2, max_missed=15)
    _, restart, _ = hostglue.track_assign(dets, None, np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32), **assoc)
    assert restart[:, 0].tolist() == [1] + [0] * 9 and restart[:, 1].tolist() == [0, 0, 0, 1] + [0] * 6      # two births, no death
    td, ids = torch.from_numpy(dets).to(DEV), [0, 1] * N
    follow = dict(TRACK, tracks=2, follow_tracks=True, **assoc)
    for paste_back in (False, True):
        kw = dict(batch_size=4, paste_back=paste_back, **CONTROLS)
        every_row, _, _ = _run(w, clip, detections=td, tracking=follow, identities=ids, **kw)
        want_streams = _streams(w)
        faces, slots, count = _faces_of(w, N, 2, ids)
        assert count == [1, 1, 1, 2, 1, 2, 1, 1, 2, 2]
        A, at_a, rows_a = _run(w, clip, detections=td, tracking=dict(follow, skip_absent=True), identities=ids, **kw)
        got_streams = _streams(w)
        for j in (1, 3, 5, 7):
            on = want_streams[j] != 0
            assert torch.equal(got_streams[j], want_streams[j]) and want_streams[j].tolist() == [1, 1], j
            assert torch.equal(got_streams[j - 1][on].view(torch.int32), want_streams[j - 1][on].view(torch.int32)), j
        B, at_b, rows_b = _run(w, clip, faces=faces, identities=slots, **kw)
        assert A.shape == B.shape and torch.equal(A, B) and at_a == at_b and rows_a == rows_b, paste_back
        assert A.shape[0] == (N if paste_back else sum(count)) and every_row.shape[0] == (N if paste_back else 2 * N)


def test_a_birth_after_everybody_left(wrapper, tiny):
    """12 frames, batches of at most 2 rows and 2 frames, max_missed = 2: face A in frames 0 ... 3, nobody in frames 4 ... 7 (A's track
    dies in frame 6, in a batch without a face), face C from frame 8, born into A's slot, face E from frame 10 in the other.  The
    batches of the whole clip from frame 8 on are those of clip[8:], so every frame from 8 on is, byte for byte, that frame of the
    skipped call on clip[8:]; frames 4 ... 7 are the input"""
    from emoportraits_amd import frames as frames_mod
    w, N, H, W = wrapper, 12, 96, 128
    clip = _clip(N, H, W, "rgb8", 51)
    A, Cf, E = _walk(N, W, H, 52, 0.4, 0.5, -0.2), _walk(N, W, H, 53, 0.4, 0.5, 0.2), _walk(N, W, H, 60, 0.35, 0.45, -0.15)
    dets = np.full((N, 3, 4), np.nan)
    dets[:4, 1], dets[8:, 2], dets[10:, 0] = A[:4], Cf[8:], E[10:]
    count = [1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 2, 2]
    assert frames_mod.face_spans(count, 0, N, 2) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 11), (11, 12)]
    assert frames_mod.face_spans(count[8:], 0, 4, 2) == [(0, 2), (2, 3), (3, 4)]
    td = torch.from_numpy(dets).to(DEV)
    tracking = dict(TRACK, tracks=2, min_iou=0.2, max_missed=2, follow_tracks=True, skip_absent=True)
    kw = dict(smooth_pose=True, smooth_per_identity=True, expression=dict(relative=True), head_pose=dict(relative=True), paste_back=True,
              batch_size=2)
    got, at, _ = _run(w, clip, detections=td, tracking=tracking, identities=[0, 1] * N, **kw)
    assert w.tracked_rows[1] == frames_mod.face_offsets(count) and w.tracked_rows[0].cpu().tolist() == [0, 2, 4, 6, 16, 18, 20, 21, 22, 23]
    assert at == [0, 2, 4, 6, 8, 10, 11] and got.shape[0] == N
    assert w.tracked_assignment[1].cpu()[:, 0].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0]
    fresh, _, _ = _run(w, clip[8:], detections=td[8:], tracking=tracking, identities=[0, 1] * (N - 8), **kw)
    assert torch.equal(got[4:8], clip[4:8]) and all(not torch.equal(got[t], clip[t]) for t in (0, 1, 2, 3, 8, 9, 10, 11))
    assert torch.equal(got[8:], fresh)


def test_the_refusals_come_before_any_launch(wrapper, tiny, guarded_outputs):  # noqa: F811
    guarded_outputs.may_serve_nothing("only the checks of the keywords are provoked: nothing is launched")
    w, N, H, W = wrapper, 4, 96, 128
    clip = _clip(N, H, W, "rgb8", 121)
    both = torch.from_numpy(np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)).to(DEV)
    skip, ids = dict(skip_absent=True), [0, 1] * N
    w.reset_crop_state()
    w.tracked_windows = "untouched"
    for kw, match in ((dict(tracking=skip), "boxes= is missing"),
                      (dict(boxes=both[:, 0], tracking=skip), r"\[N,1,4\]"),
                      (dict(boxes=both, tracking=skip, identities=ids, as_uint8=False, to_host=False), "as_uint8=False"),
                      (dict(boxes=both, tracking=skip, identities=ids, smooth_pose=True, smooth_per_identity=True), "follow_tracks"),
                      (dict(boxes=both, tracking=skip, identities=ids, expression=dict(relative=True)), "follow_tracks"),
                      (dict(boxes=both, tracking=skip, identities=ids, expression=dict(smooth=True)), "follow_tracks"),
                      (dict(boxes=both, tracking=skip, identities=ids, head_pose=dict(relative=True)), "follow_tracks")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(clip, **kw))
    with pytest.raises(ValueError, match="skip_absent"):
        next(w.animate_streams([dict(frames=clip, boxes=both[:, 0])], tracking=skip))
    assert w.tracked_windows == "untouched" and w.tracked_rows is None
    w.tracked_windows = None
