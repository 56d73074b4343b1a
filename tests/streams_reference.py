"""TEST INFRASTRUCTURE ONLY -- the small case the CPU and the GPU tests of the mixed-size entry points (ABI 19) share, and the
reference they are held to, bit for bit: the "canvas".  Every frame of a mixed batch is embedded at the top-left corner of a
canvas of the batch's largest H x W (NV12: the Y rows at the top of the canvas's Y plane, the UV rows at the top of its UV plane),
the rest filled with other random bytes, and the ABI 18 entry points run on that uniform batch with the same windows.  They clamp
a crop's taps inside its window and read and write only the bytes under the windows (NV12: and the 2 x 2 chroma blocks the
windows touch, which stay inside an even-sized region), so the mixed crops are the canvas crops and every pasted mixed frame is
the top-left H_i x W_i region of the pasted canvas frame.  check_premise asserts exactly that premise on the parent's own entry
points: the bytes outside the regions do not change their result."""
import torch

S = 128
# (H, W) per frame; the rgb8 sizes are odd in places, the NV12 ones even
SIZES = {"rgb8": [(70, 66), (133, 97), (64, 64), (201, 150)], "nv12": [(70, 66), (132, 98), (64, 64), (200, 150)]}
# (x_lo, y_lo, side) per frame, in paste order: two overlapping faces in frame 0, none in frame 1, the whole of frame 2 (the
# smallest frame: the largest side), three in frame 3 with the last one in its bottom-right corner; odd origins; sides S / 4 ... 64
_CORNER = {"rgb8": (99, 150, 51), "nv12": (99, 149, 51)}


def faces(fmt):
    return [[(1, 3, 40), (21, 17, 45)], [], [(0, 0, 64)], [(7, 11, 32), (60, 100, 63), _CORNER[fmt]]]


def windows(fmt):
    return [w for of_frame in faces(fmt) for w in of_frame]


FRAME_OF = [0, 0, 2, 3, 3, 3]
# a window that fits the canvas but not its own frame (frame 0 is 70 x 66): in place of face 1 it must be left out
OUTSIDE_ITS_FRAME = (30, 10, 50)


def check_case(fmt):
    """what the shared case is said to contain, asserted"""
    wins, sizes = windows(fmt), SIZES[fmt]
    assert FRAME_OF == [i for i, of_frame in enumerate(faces(fmt)) for _ in of_frame] and len(wins) == 6
    for (x, y, s), f in zip(wins, FRAME_OF):
        assert x >= 0 and y >= 0 and x + s <= sizes[f][1] and y + s <= sizes[f][0] and 4 * s >= S
    sides = [s for _, _, s in wins]
    assert min(sides) == S // 4 and max(sides) == min(min(hw) for hw in sizes)
    a, b = wins[0], wins[1]
    assert a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[2] and b[1] < a[1] + a[2]
    x, y, s = wins[5]
    assert (y + s, x + s) == sizes[3] and any(w[0] & 1 for w in wins) and any(w[1] & 1 for w in wins)
    x, y, s = OUTSIDE_ITS_FRAME
    Hc, Wc = canvas_size(sizes)
    assert x + s > sizes[0][1] and x + s <= Wc and y + s <= Hc and 4 * s >= S
    if fmt == "nv12":
        assert all(not (h & 1) and not (w & 1) for h, w in sizes)
    else:
        assert any(h & 1 for h, _ in sizes) and any(w & 1 for _, w in sizes)


def frame_shape(hw, fmt):
    return (hw[0], hw[1], 3) if fmt == "rgb8" else (3 * hw[0] // 2, hw[1])


def random_frames(sizes, fmt, seed):
    """one tensor of random bytes per frame"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, frame_shape(hw, fmt), generator=g, dtype=torch.uint8) for hw in sizes]


def canvas_size(sizes):
    return max(h for h, _ in sizes), max(w for _, w in sizes)


def canvas(frames, fmt, seed):
    """the frames (a list of uint8 tensors) at the top-left corners of a uniform batch of the largest H x W, the rest random bytes"""
    sizes = [frame_size(f, fmt) for f in frames]
    Hc, Wc = canvas_size(sizes)
    g = torch.Generator().manual_seed(seed)
    out = torch.randint(0, 256, (len(frames),) + frame_shape((Hc, Wc), fmt), generator=g, dtype=torch.uint8)
    for i, (f, (h, w)) in enumerate(zip(frames, sizes)):
        if fmt == "rgb8":
            out[i, :h, :w] = f.cpu()
        else:
            out[i, :h, :w] = f[:h].cpu()
            out[i, Hc:Hc + h // 2, :w] = f[h:].cpu()
    return out


def frame_size(frame, fmt):
    return (frame.shape[0], frame.shape[1]) if fmt == "rgb8" else (frame.shape[0] // 3 * 2, frame.shape[1])


def region(canvas_frame, hw, fmt):
    """the top-left H x W frame of one canvas frame"""
    h, w = hw
    if fmt == "rgb8":
        return canvas_frame[:h, :w]
    Hc = canvas_frame.shape[0] // 3 * 2
    return torch.cat([canvas_frame[:h, :w], canvas_frame[Hc:Hc + h // 2, :w]])


def regions(canvas_frames, sizes, fmt):
    return [region(c, hw, fmt) for c, hw in zip(canvas_frames, sizes)]


def check_premise(frames, fmt, crop, paste):
    """crop(canvas) -> crops and paste(canvas) -> pasted canvas are the PARENT's entry points (ABI 18) with the case's windows:
    two canvases that differ everywhere outside the regions give the same crops and the same regions, and leave the rest alone"""
    sizes = [frame_size(f, fmt) for f in frames]
    a, b = canvas(frames, fmt, 101), canvas(frames, fmt, 202)
    assert not torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(regions(a, sizes, fmt), regions(b, sizes, fmt)))
    assert torch.equal(crop(a), crop(b))
    pa, pb = paste(a), paste(b)
    assert all(torch.equal(x, y) for x, y in zip(regions(pa, sizes, fmt), regions(pb, sizes, fmt)))
    assert not torch.equal(pa, a)
    inside = region_mask(a, sizes, fmt)
    assert not bool(((pa != a) & ~inside).any()) and not bool(((pb != b) & ~inside).any())


def region_mask(canvas_frames, sizes, fmt):
    """bool, the canvas's shape: the bytes of the regions"""
    inside = torch.zeros(canvas_frames.shape, dtype=torch.bool)
    Hc = canvas_frames.shape[1] if fmt == "rgb8" else canvas_frames.shape[1] // 3 * 2
    for i, (h, w) in enumerate(sizes):
        inside[i, :h, :w] = True
        if fmt == "nv12":
            inside[i, Hc:Hc + h // 2, :w] = True
    return inside
