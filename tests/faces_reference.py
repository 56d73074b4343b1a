"""TEST INFRASTRUCTURE ONLY -- the small case the CPU and the GPU tests of the several-faces-per-frame entry points (ABI 18) share,
and the reference they are held to: the faces pasted one after another, in list order, each with the single-window entry point
on its own frame.  Inputs come from tests/paste_back_reference.py and tests/nv12_reference.py."""
import torch

import nv12_reference as NV
import paste_back_reference as PB

S, HF, WF = 128, 270, 480
# (x_lo, y_lo, side) per frame, in paste order: a two-way overlap in frame 0, no face in frame 1, a three-way overlap around pixel
# (310, 110) of frame 2, a window in the bottom-right corner of frame 3; odd origins, sides below, above and equal to S
FACES = [[(10, 5, 70), (50, 30, 96)], [], [(100, 20, 250), (300, 100, 96), (211, 1, 180)], [(352, 142, 128)]]
WINDOWS = [w for of_frame in FACES for w in of_frame]
FRAME_OF = [i for i, of_frame in enumerate(FACES) for _ in of_frame]
OVERLAPS = [(0, 1), (2, 3), (2, 4), (3, 4)]          # pairs of faces (indices into WINDOWS) of one frame that intersect


def covers(w, x, y):
    return w[0] <= x < w[0] + w[2] and w[1] <= y < w[1] + w[2]


def check_case():
    """what the shared case is said to contain, asserted"""
    assert len(WINDOWS) == 6 and FRAME_OF == [0, 0, 2, 2, 2, 3]
    assert all(x >= 0 and y >= 0 and x + s <= WF and y + s <= HF and 4 * s >= S for x, y, s in WINDOWS)
    assert all(covers(WINDOWS[m], 310, 110) for m in (2, 3, 4))
    for a, b in OVERLAPS:
        assert FRAME_OF[a] == FRAME_OF[b] and bool(rect_mask(WINDOWS[a]).logical_and(rect_mask(WINDOWS[b])).any())
    assert WINDOWS[5][0] + WINDOWS[5][2] == WF and WINDOWS[5][1] + WINDOWS[5][2] == HF
    assert any(x & 1 for x, _, _ in WINDOWS) and any(y & 1 for _, y, _ in WINDOWS)
    sides = [s for _, _, s in WINDOWS]
    assert min(sides) < S and max(sides) > S and S in sides


def small_rgb():
    """{'smooth' | 'noise': (frames uint8 [4,270,480,3], img fp32 [6,3,128,128], matte fp32 [6,1,128,128])}"""
    return {k: (f[:len(FACES)].contiguous(), img, matte) for k, (f, img, matte) in PB.small_inputs().items()}


def small_nv12():
    """{'smooth' | 'noise': (nv12 uint8 [4,405,480], img fp32 [6,3,128,128], matte fp32 [6,1,128,128])}"""
    return {k: (f[:len(FACES)].contiguous(), img, matte) for k, (f, img, matte) in NV.small_inputs().items()}


def sequential(paste_one, frames, img, matte, wins, frame_of, skip=()):
    """the reference: paste_one(frame [1,...], img [1,3,S,S], matte [1,1,S,S] | None, (x0, y0, s)) -> the frame, face after face"""
    out = frames.clone()
    for m, f in enumerate(frame_of):
        if m not in skip:
            out[f:f + 1] = paste_one(out[f:f + 1].contiguous(), img[m:m + 1], None if matte is None else matte[m:m + 1], wins[m])
    return out


def rect_mask(w):
    """bool [HF, WF]: the pixels of window w"""
    mask = torch.zeros(HF, WF, dtype=torch.bool)
    mask[w[1]:w[1] + w[2], w[0]:w[0] + w[2]] = True
    return mask


def rgb_mask(n_frames, wins, frame_of):
    """bool [F,HF,WF]: the union of the windows of every frame"""
    mask = torch.zeros(n_frames, HF, WF, dtype=torch.bool)
    for w, f in zip(wins, frame_of):
        mask[f] |= rect_mask(w)
    return mask


def nv12_mask(n_frames, wins, frame_of):
    """bool [F, 3HF/2, WF]: the union of the luma rectangles and the covering chroma rectangles of every frame's windows"""
    mask = torch.zeros(n_frames, 3 * HF // 2, WF, dtype=torch.bool)
    for w, f in zip(wins, frame_of):
        mask[f] |= NV.touched_mask((1, 3 * HF // 2, WF), [w])[0]
    return mask
