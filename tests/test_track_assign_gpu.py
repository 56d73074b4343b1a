"""Detections to tracks on the GPU: ops.track_assign against hostglue.track_assign bit for bit on the cases of
tests/track_assign_cases.py, ops.crop_track(restart=) against hostglue.crop_track(restart=); animate_frames(detections=) against
animate_frames(boxes=[N,2,4]) holding the same tracks, byte for byte -- crops out and paste_back, rgb8 and NV12, host and device
detections; a face that leaves for max_missed + 1 frames and others that appear, against the input frames and against faces= fed
with the restatement's windows.  Tiny fixture, toy embedders.  (Several ranks: every rank associates the whole chunk from inputs
every rank has, which tests/test_track_assign_emul.py checks on the recorder rig; there is no collective to test here.)"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import crop_track_cases as CC  # noqa: E402
import track_assign_cases as C  # noqa: E402
from test_crop_track_gpu import _clip, _run, _walk  # noqa: E402
from test_head_pose_controls_gpu import make_wrapper, project, tiny  # noqa: E402,F401

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"
TRACK = dict(smooth=True, momentum=0.5)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def test_ops_track_assign_is_the_restatement_bit_for_bit():
    """every case in two calls that carry the tracks: the bits of the boxes, restart, track_of, the ages and the live refs"""
    from emoportraits_amd import ops
    for c in C.cases():
        host = c.states()
        ref, age = (_dev(a) for a in c.states())
        kw = dict(c.kw, box_format=("xyxy", "relative")[c.kw["box_format"]])
        cut = max(1, c.F // 2)
        for rows in (slice(0, cut), slice(cut, c.F)):
            if rows.start >= c.F:
                continue
            want = c.restated(host, rows)
            dets, so = c.rows(rows)
            got = [g.cpu().numpy() for g in ops.track_assign(_dev(dets), _dev(so), ref, age, **kw)]
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), c.name
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), c.name
        live = host[1] >= 0
        assert np.array_equal(age.cpu().numpy(), host[1]), c.name
        assert np.array_equal(ref.cpu().numpy()[live].view(np.uint64), host[0][live].view(np.uint64)), c.name


def test_ops_crop_track_with_restarts_is_the_restatement_bit_for_bit():
    """the crop_track_cases sweep of 37 rows over 3 streams with a random restart mask, in two calls that carry the state"""
    from emoportraits_amd import hostglue, ops
    M, K = 37, 3
    rng = np.random.default_rng(M)
    for c in CC.sweep(M, K):
        restart = (rng.random(M) < 0.25).astype(np.int32)
        host = c.states()
        host[0][:] = 0.0
        state = [_dev(a) for a in host]
        for rows in (slice(0, M // 2 + 1), slice(M // 2 + 1, M)):
            so = None if c.so is None else c.so[rows]
            want = hostglue.crop_track(c.boxes[rows], so, c.size_arg(rows), *host, K=K, restart=restart[rows], **c.kw)
            size = c.one_size if c.one_size else _dev(c.sizes[rows])
            got = [g.cpu().numpy() for g in ops.crop_track(_dev(c.boxes[rows]), _dev(so), size, *state, restart=_dev(restart[rows]), **c.kw)]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), c.kw
            assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64)), c.kw
        on = host[1] != 0
        assert state[1].cpu().tolist() == host[1].tolist() and np.array_equal(state[2].cpu().numpy(), host[2]), c.kw
        assert np.array_equal(state[0].cpu().numpy()[on].view(np.uint64), host[0][on].view(np.uint64)), c.kw


# ---- the wrapper -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapper(project, tiny):
    return make_wrapper(project, tiny, K=2)


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
@pytest.mark.parametrize("paste_back", [False, True], ids=["crops", "paste_back"])
def test_detections_are_the_ordered_boxes_byte_for_byte(wrapper, tiny, fmt, paste_back):
    """12 frames of 96 x 128, two faces at a random two of four detection rows, in batches of 4 and of 8: detections= against
    boxes= [N,2,4] holding the same tracks; track_of is the inverse of the permutation"""
    w, N, H, W = wrapper, 12, 96, 128
    clip = _clip(N, H, W, fmt, 50)
    both = np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)
    dets, at = C.permuted(both)
    inverse = np.full((N, 4), -1)
    for t in range(N):
        inverse[t, at[t]] = [0, 1]
    kw = dict(frame_format=fmt, paste_back=paste_back, identities=[0, 1] * N)
    for bs in (4, 8):
        want = _run(w, clip, boxes=torch.from_numpy(both), tracking=TRACK, batch_size=bs, **kw)
        for td in (torch.from_numpy(dets), torch.from_numpy(dets).to(DEV)):
            got = _run(w, clip, detections=td, tracking=dict(TRACK, tracks=2, min_iou=0.2), batch_size=bs, **kw)
            assert got.shape == want.shape and torch.equal(got, want), (fmt, paste_back, bs)
            assert w.tracked_assignment[0].cpu().tolist() == inverse.tolist()
            assert w.tracked_assignment[1].cpu().tolist() == [[1, 1]] + [[0, 0]] * (N - 1)
    if paste_back:
        assert not torch.equal(want, clip)


def test_a_face_leaves_and_others_appear(wrapper, tiny):
    """max_missed = 2, two slots, paste_back.  Face A in frames 0 ... 3, nobody in frames 4 ... 6 (A's track dies in frame 6), face
    C from frame 7 (born into A's slot) and face E from frame 9 (born into the other).  Frames 4 ... 6 come back byte for byte as
    they went in, although their rows were rendered; every frame from 7 on is the frame of faces= fed with the restatement's windows
    (batches of two rows in both forms), C's first window that of its own box"""
    from emoportraits_amd import hostglue
    w, N, H, W = wrapper, 12, 96, 128
    S = tiny["cfg"]["image_size"]
    clip = _clip(N, H, W, "rgb8", 51)
    A, Cf, E = _walk(N, W, H, 52, 0.4, 0.5, -0.2), _walk(N, W, H, 53, 0.4, 0.5, 0.2), _walk(N, W, H, 60, 0.35, 0.45, -0.15)
    dets = np.full((N, 3, 4), np.nan)
    dets[:4, 1] = A[:4]
    dets[7:, 2] = Cf[7:]
    dets[9:, 0] = E[9:]
    kw = dict(min_iou=0.2, max_missed=2)
    ref, age = np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32)
    boxes, restart, track_of = hostglue.track_assign(dets, None, ref, age, **kw)
    assert restart[:, 0].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0] and restart[:, 1].tolist() == [0] * 9 + [1, 0, 0]
    assert track_of[:, 2].tolist() == [-1] * 7 + [0] * 5 and track_of[9:, 0].tolist() == [1, 1, 1]
    st = np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros((2, 4), np.int32)
    crop, paste, _ = hostglue.crop_track(boxes.reshape(-1, 4), np.tile(np.int32([0, 1]), N), (W, H), *st, min_side=-(-S // 4),
                                         restart=restart.reshape(-1), missing="hold", **TRACK)
    paste = paste.reshape(N, 2, 4)
    present = paste[:, :, 2] > 0
    # (held for the two frames it may be missed, gone when it is dead; the other slot empty until E)
    assert present[:, 0].tolist() == [True] * 6 + [False] + [True] * 5 and present[:, 1].tolist() == [False] * 9 + [True] * 3
    own = hostglue.crop_track(Cf[7:8], None, (W, H), None, None, None, min_side=-(-S // 4))[1][0]
    assert np.array_equal(paste[7, 0], own)
    got = _run(w, clip, detections=torch.from_numpy(dets).to(DEV), tracking=dict(TRACK, tracks=2, missing="hold", **kw),
               identities=[0, 1] * N, batch_size=2, paste_back=True)
    assert w.tracked_windows[0].cpu().tolist() == paste.reshape(-1, 4).tolist()
    assert torch.equal(got[6], clip[6]) and not torch.equal(got[5], clip[5]) and not torch.equal(got[3], clip[3])
    # the same without 'hold': the three frames of the gap are the frames that went in
    skip = hostglue.crop_track(boxes.reshape(-1, 4), np.tile(np.int32([0, 1]), N), (W, H), np.zeros((2, 3)), np.zeros(2, np.int32), None,
                               min_side=-(-S // 4), restart=restart.reshape(-1), **TRACK)[1].reshape(N, 2, 4)
    got = _run(w, clip, detections=torch.from_numpy(dets), tracking=dict(TRACK, tracks=2, **kw), identities=[0, 1] * N, batch_size=2,
               paste_back=True)
    assert torch.equal(got[4:7], clip[4:7]) and not torch.equal(got[3], clip[3]) and not torch.equal(got[7], clip[7])
    faces = [[tuple(skip[t, p, :3].tolist()) for p in (0, 1) if skip[t, p, 2] > 0] for t in range(N)]
    assert [len(f) for f in faces] == [1] * 4 + [0] * 3 + [1] * 2 + [2] * 3
    ids = [p for t in range(N) for p in (0, 1) if skip[t, p, 2] > 0]
    want = _run(w, clip, faces=faces, identities=ids, batch_size=2, paste_back=True)
    assert torch.equal(got[7:], want[7:])
