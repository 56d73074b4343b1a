"""Crop tracking on the GPU: ops.crop_track against hostglue.crop_track bit for bit on the cases of tests/crop_track_cases.py;
animate_frames(boxes=, tracking=) against animate_frames(windows=) fed with the restatement's windows, byte for byte -- crops out
and paste_back, rgb8 and NV12; a NaN box under 'skip' and 'hold'; two tracks per frame against faces=; animate_streams with two
frame sizes.  Tiny fixture, toy embedders.  (Several ranks: every rank tracks the whole chunk from inputs every rank has, which
tests/test_crop_track_emul.py checks on the recorder rig; there is no collective to test here.)"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import crop_track_cases as C  # noqa: E402
from test_head_pose_controls_gpu import make_wrapper, project, tiny  # noqa: E402,F401

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"
TRACK = dict(smooth=True, momentum=0.5)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(37, 3), (130, 65)])
def test_ops_crop_track_is_the_restatement_bit_for_bit(M, K):
    """every case of crop_track_cases.sweep in two calls that carry the state: crop, paste, the bits of face_scale, and the three
    state arrays"""
    from emoportraits_amd import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for c in C.sweep(M, K):
        host = c.states()
        host[0][:] = 0.0
        state = [dev(a) for a in host]
        for lo, hi in ((0, M // 2 + 1), (M // 2 + 1, M)):
            rows = slice(lo, hi)
            want = c.restated(host, rows)
            size = c.one_size if c.one_size else dev(c.sizes[rows])
            got = ops.crop_track(dev(c.boxes[rows]), None if c.so is None else dev(c.so[rows]), size, *state, **c.kw)
            got = [g.cpu().numpy() for g in got]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), c.kw
            assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64)), c.kw
        on = host[1] != 0
        assert state[1].cpu().tolist() == host[1].tolist() and np.array_equal(state[2].cpu().numpy(), host[2]), c.kw
        assert np.array_equal(state[0].cpu().numpy()[on].view(np.uint64), host[0][on].view(np.uint64)), c.kw


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapper(project, tiny):
    return make_wrapper(project, tiny, K=2)


def _walk(N, W, H, seed, lo=0.35, hi=0.6, dx=0.0):
    """N boxes of a face that wanders about the middle of a W x H frame, wide enough for a paste into the 64-pixel image"""
    rng = np.random.default_rng(seed)
    cx, cy = W * ((0.5 + dx) + 0.05 * rng.standard_normal(N)).clip(0.3, 0.7), H * (0.5 + 0.05 * rng.standard_normal(N)).clip(0.4, 0.6)
    h = rng.uniform(lo, hi, (2, N)) * min(W, H) / 2
    return np.stack([cx - h[0], cy - h[1], cx + h[0], cy + h[1]], 1)


def _clip(N, H, W, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (N, H, W, 3) if fmt == "rgb8" else (N, H * 3 // 2, W)
    return torch.randint(16, 236, shape, generator=g, dtype=torch.uint8)


def _restated(boxes, size, min_side, so=None, K=1, **kw):
    from emoportraits_amd import hostglue
    st = np.zeros((K, 3)), np.zeros(K, np.int32), np.zeros((K, 4), np.int32)
    return hostglue.crop_track(boxes, so, size, *st, min_side=min_side, **kw)


def _run(w, clip, **kw):
    w.reset_crop_state()
    out = [(i, o.clone()) for i, o in w.animate_frames(clip, to_host=False, **kw)]
    torch.cuda.synchronize()
    assert [i for i, _ in out] == sorted(i for i, _ in out)
    return torch.cat([o for _, o in out]).cpu()


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
@pytest.mark.parametrize("paste_back", [False, True], ids=["crops", "paste_back"])
def test_animate_frames_boxes_are_the_windows_form_byte_for_byte(wrapper, tiny, fmt, paste_back):
    """8 frames of 96 x 128 in batches of 3 and of 8: boxes= with smoothing against windows= holding the restatement's windows"""
    w, N, H, W = wrapper, 8, 96, 128
    S = tiny["cfg"]["image_size"]
    clip, boxes = _clip(N, H, W, fmt, 30), _walk(N, W, H, 31)
    crop, paste, _ = _restated(boxes, (W, H), -(-S // 4) if paste_back else 2, **TRACK)
    assert (paste[:, 2] > 0).all() and np.array_equal(crop, paste)               # every row is present
    wins = [tuple(r[:3]) for r in crop.tolist()]
    kw = dict(frame_format=fmt, paste_back=paste_back, identities=[0, 1] * (N // 2))
    for bs in (3, 8):
        want = _run(w, clip, windows=wins, batch_size=bs, **kw)
        for tb in (torch.from_numpy(boxes), torch.from_numpy(boxes).to(DEV)):
            got = _run(w, clip, boxes=tb, tracking=TRACK, batch_size=bs, **kw)
            assert got.shape == want.shape and torch.equal(got, want), (fmt, paste_back, bs)
        assert w.tracked_windows[0].cpu().tolist() == paste.tolist() and w.tracked_windows[1] == 0
    if paste_back:
        assert not torch.equal(want, clip)


@pytest.mark.parametrize("missing", ["skip", "hold"])
def test_a_nan_box_is_skipped_or_held(wrapper, tiny, missing):
    """a NaN box in frame 2 with paste_back: 'skip' returns that frame byte for byte as uploaded and the others as the windows form
    pastes them; 'hold' pastes it at the previous window"""
    w, N, H, W = wrapper, 8, 96, 128
    S = tiny["cfg"]["image_size"]
    clip, boxes = _clip(N, H, W, "rgb8", 32), _walk(N, W, H, 33)
    boxes[2] = np.nan
    crop, paste, _ = _restated(boxes, (W, H), -(-S // 4), missing=missing, **TRACK)
    present = paste[:, 2] > 0
    assert present.tolist() == [True, True, missing == "hold"] + [True] * 5
    want = _run(w, clip, windows=[tuple(r[:3]) for r in crop.tolist()], batch_size=3, paste_back=True)
    got = _run(w, clip, boxes=torch.from_numpy(boxes), tracking=dict(TRACK, missing=missing), batch_size=3, paste_back=True)
    others = [i for i in range(N) if i != 2]
    assert torch.equal(got[others], want[others])
    if missing == "skip":
        assert torch.equal(got[2], clip[2]) and tuple(crop[2]) == (16, 0, 96, 96) and not torch.equal(want[2], clip[2])
    else:
        assert np.array_equal(paste[2], paste[1]) and torch.equal(got[2], want[2]) and not torch.equal(got[2], clip[2])


def test_two_tracks_per_frame_with_two_identities_are_the_faces_path(wrapper, tiny):
    w, N, H, W = wrapper, 6, 96, 128
    S = tiny["cfg"]["image_size"]
    clip = _clip(N, H, W, "rgb8", 34)
    both = np.stack([_walk(N, W, H, 35, 0.35, 0.45, -0.2), _walk(N, W, H, 36, 0.4, 0.5, 0.2)], 1)     # [N,2,4]
    crop, paste, _ = _restated(both.reshape(-1, 4), (W, H), -(-S // 4), so=np.tile(np.int32([0, 1]), N), K=2, **TRACK)
    assert (paste[:, 2] > 0).all()
    faces = [[tuple(crop[2 * i][:3]), tuple(crop[2 * i + 1][:3])] for i in range(N)]
    ids = [0, 1] * N
    for kw in (dict(paste_back=True), dict()):
        want = _run(w, clip, faces=faces, identities=ids, batch_size=4, **kw)
        got = _run(w, clip, boxes=torch.from_numpy(both).float().double(), tracking=TRACK, identities=ids, batch_size=4, **kw)
        assert torch.equal(got, want)
    assert w._crop_streams.K == 2


def test_animate_streams_boxes_are_its_windows_form(wrapper, tiny):
    """a 64 x 96 and a 96 x 128 stream in one batch: 'boxes' against 'windows', crops and pasted frames"""
    w = wrapper
    S = tiny["cfg"]["image_size"]
    hw = [(64, 96), (96, 128)]
    clips = [_clip(4, *hw[0], "rgb8", 37), _clip(3, *hw[1], "rgb8", 38)]
    boxes = [_walk(4, hw[0][1], hw[0][0], 39, 0.5, 0.7), _walk(3, hw[1][1], hw[1][0], 40)]
    order = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (0, 3)]             # tick order
    for paste_back in (False, True):
        crop, paste, _ = _restated(np.stack([boxes[s][t] for s, t in order]), [hw[s][::-1] for s, _ in order], -(-S // 4) if paste_back else 2,
                                   so=np.int32([s for s, _ in order]), K=2, **TRACK)
        assert (paste[:, 2] > 0).all()
        at = {st: crop[i] for i, st in enumerate(order)}

        def run(streams, **kw):
            out = [(s, t, o.clone().cpu()) for batch in w.animate_streams(streams, to_host=False, batch_size=4, paste_back=paste_back, **kw)
                   for s, t, o in batch]
            torch.cuda.synchronize()
            return out
        want = run([dict(frames=clips[s], windows=[tuple(at[(s, t)][:3]) for t in range(len(clips[s]))], identities=s) for s in (0, 1)])
        got = run([dict(frames=clips[s], boxes=torch.from_numpy(boxes[s]), identities=s) for s in (0, 1)], tracking=TRACK)
        assert [a[:2] for a in got] == [b[:2] for b in want] == order
        assert all(torch.equal(a[2], b[2]) for a, b in zip(got, want))
        assert w.tracked_windows[0].cpu().tolist() == paste[4:].tolist() and w.tracked_windows[1] == 4
