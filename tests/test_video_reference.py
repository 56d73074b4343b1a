"""The video path's launch checks (tests/video_reference.py) held to themselves, without a GPU, as test_ops_reference.py holds
ops_reference.py: every check_<op> is fed the fp32 (or byte) evaluation of its own reference as the "result" and must find nothing;
then one deliberate error each -- a byte off by 2, a window shifted by a pixel, two faces pasted in the wrong order, a byte changed
outside the touched mask, a stale state row, a row_of entry swapped, an absent row that is not zero, and more -- and the check must
name it.  A checker that checks nothing passes none of the second kind."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_reference as R
import paste_back_reference as PB
import video_reference as V
import yuv420_reference as Y
from emoportraits_amd import hostglue

F64, F32 = torch.float64, torch.float32
S, HF, WF = 32, 48, 64
# faces of three frames (frame 1 has none): an overlap in frame 0, odd origins and sides, a side of S / 4, the bottom-right corner
FACES = [(1, 3, 17), (6, 5, 32), (8, 1, 47), (56, 40, 8)]
FRAME_OF = [0, 0, 2, 2]
SQ = [(x, y, s, s) for x, y, s in FACES]


def clean(fig, rows=None):
    assert fig["failures"] == [], fig["failures"]
    assert rows is None or fig["frames"] == list(range(rows)), fig["frames"]
    return fig


def names(fig, *words):
    """the check failed, and a failure says every one of `words`"""
    assert fig["failures"], "the error went unnoticed"
    assert any(all(w in f for w in words) for f in fig["failures"]), (words, fig["failures"])
    return fig


@pytest.fixture(scope="module")
def pictures():
    g = torch.Generator().manual_seed(5)
    rgb = (PB.smooth(g, (3, 3, HF, WF), 2).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    img = PB.smooth(g, (4, 3, S, S), 2).float()
    matte = PB.smooth(g, (4, 1, S, S), 3).clamp(0, 1).float()
    codes = {8: Y.encode(PB.smooth(g, (3, 3, HF, WF), 2).clamp(0, 1), "bt709", False, 8, F64),
             10: Y.encode(PB.smooth(g, (3, 3, HF, WF), 2).clamp(0, 1), "bt601", True, 10, F64)}
    return dict(rgb=rgb, img=img, matte=matte, codes=codes)


# ---- what is taken from ops_reference is ops_reference's ----------------------------------------------------------------------------
def test_the_plain_operations_are_ops_reference_checks_themselves():
    """their own tests are tests/test_ops_reference.py's"""
    for mine, theirs in (("unpack_rgb8", "unpack_rgb8"), ("pack_rgb8", "pack_rgb8"), ("mul_mask", "mul_mask"), ("resize2d", "resize2d"),
                         ("pose_theta", "pose_theta"), ("mat4_inverse", "mat4_inverse"), ("grid_sample3d", "grid_sample3d"), ("add", "add"),
                         ("volume_to_channels_last", "channels_last")):
        assert getattr(V, "check_" + mine) is getattr(R, "check_" + theirs)
    assert (V.C_TOL, V.D_TOL, V.MAX_BYTE_DIFF, V.MAX_SHARE) == (Y.C_TOL, Y.D_TOL, PB.MAX_BYTE_DIFF, PB.MAX_SHARE)


# ---- crops ---------------------------------------------------------------------------------------------------------------------------
def _rgb_rows(x, wins, fof, size=(S, S)):
    return torch.cat([R.resize2d_fp64(x[f:f + 1], size, "bicubic", w, True).float() for w, f in zip(wins, fof)])


def test_resize2d_windows_rows_each_against_its_own_frame_and_window(pictures):
    x = pictures["rgb"].permute(0, 3, 1, 2).float() / 255
    out = _rgb_rows(x, SQ, FRAME_OF)
    clean(V.check_resize2d_windows(out, x, (S, S), SQ, "bicubic", True, FRAME_OF), 4)
    clean(V.check_resize2d_windows(_rgb_rows(x, SQ[:3], [0, 1, 2]), x, (S, S), torch.tensor(SQ[:3], dtype=torch.int32), "bicubic", True), 3)
    # one window shifted by a pixel: the row was cut one pixel to the right of where its window says
    shifted = [SQ[0], (SQ[1][0] + 1,) + SQ[1][1:], SQ[2], SQ[3]]
    names(V.check_resize2d_windows(_rgb_rows(x, shifted, FRAME_OF), x, (S, S), SQ, "bicubic", True, FRAME_OF), "row 1", "window (6, 5, 32, 32)")
    # a row cut out of the wrong frame
    names(V.check_resize2d_windows(_rgb_rows(x, SQ, [0, 1, 2, 2]), x, (S, S), SQ, "bicubic", True, FRAME_OF), "row 1 (frame 0")
    # an absent row (no side; a frame outside the batch) is zeros, exactly
    absent, fof = SQ[:3] + [(0, 0, 0, 0)], [0, 0, 2, 3]
    out = torch.cat([_rgb_rows(x, SQ[:3], fof[:3]), torch.zeros(1, 3, S, S)])
    clean(V.check_resize2d_windows(out, x, (S, S), absent, "bicubic", True, fof), 4)
    out[3, 1, 2, 3] = 1e-30
    names(V.check_resize2d_windows(out, x, (S, S), absent, "bicubic", True, fof), "row 3", "must be zeros")
    out[3] = 0
    out[2] = 0
    names(V.check_resize2d_windows(out, x, (S, S), absent, "bicubic", True, fof), "row 2")        # (and a present row that is zeros)
    names(V.check_resize2d_windows(out, x, (S, S), SQ[:3] + [(60, 0, 8, 8)], "bicubic", True, [0, 0, 2, 2]), "leaves its")


@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_yuv_crops_rows_and_whole_frames(pictures, fmt):
    bits = Y.BITS[fmt]
    codes = pictures["codes"][bits]
    mode = ("bt601", True)
    frames = Y.tensor_of(codes, fmt, Y.junk_like(codes, fmt))
    # the adapter's (w, h) crop is yuv420_reference.crop on squares
    for dt in (F64, F32):
        rows = torch.stack([V.yuv_crop(codes, f, w, (S, S), *mode, bits, dt) for w, f in zip(SQ, FRAME_OF)])
        assert torch.equal(rows, Y.crop(codes[FRAME_OF], FACES, S, *mode, bits, dt))
    clean(V.check_yuv420_windows(rows, frames, fmt, (S, S), SQ, *mode, FRAME_OF), 4)
    names(V.check_yuv420_windows(rows, frames, fmt, (S, S), [SQ[0], SQ[1], (9, 1, 47, 47), SQ[3]], *mode, FRAME_OF), "row 2")   # a shifted window
    names(V.check_yuv420_windows(rows, frames, fmt, (S, S), SQ, "bt709", True, FRAME_OF), "row")                               # the other matrix
    zero = rows.clone()
    zero[3] = 0
    clean(V.check_yuv420_windows(zero, frames, fmt, (S, S), SQ[:3] + [(60, 44, 8, 8)], *mode, FRAME_OF), 4)                       # leaves the frame: zeros
    names(V.check_yuv420_windows(rows, frames, fmt, (S, S), SQ[:3] + [(60, 44, 8, 8)], *mode, FRAME_OF), "row 3", "must be zeros")
    # whole frames: the plain conversion under D_TOL at the frame's size, the resized whole frame under C_TOL
    whole = Y.decode(codes, *mode, bits, F32)
    clean(V.check_yuv420_windows(whole, frames, fmt, None, None, *mode), 3)
    off = whole.clone()
    off[1, 2, 5, 7] += 4 * V.D_TOL if off[1, 2, 5, 7] < 0.5 else -4 * V.D_TOL                    # inside C_TOL, outside D_TOL
    names(V.check_yuv420_windows(off, frames, fmt, None, None, *mode), "row 1")
    small = torch.stack([V.yuv_crop(codes, f, (0, 0, WF, HF), (S, S), *mode, bits, F32) for f in range(3)])
    clean(V.check_yuv420_windows(small, frames, fmt, (S, S), None, *mode), 3)
    # the same faces out of a list of frames (one of another size)
    other = Y.tensor_of(codes[:1, :, :WF - 8][:, [*range(HF - 16), *range(HF, HF + (HF - 16) // 2)]].contiguous(), fmt)[0]
    mixed = [frames[0], other, frames[2]]
    clean(V.check_crop_faces_mixed(rows, mixed, S, SQ, FRAME_OF, fmt, *mode), 4)
    names(V.check_crop_faces_mixed(rows, [frames[2], other, frames[0]], S, SQ, FRAME_OF, fmt, *mode), "face")


def test_crop_faces_mixed_rgb8_each_face_against_its_own_frame(pictures):
    rgb = pictures["rgb"]
    frames = [rgb[0], rgb[1][:20, :24].contiguous(), rgb[2]]
    x = rgb.permute(0, 3, 1, 2).double() / 255
    out = _rgb_rows(x, SQ, FRAME_OF)
    clean(V.check_crop_faces_mixed(out, frames, S, SQ, FRAME_OF), 4)
    names(V.check_crop_faces_mixed(out, frames, S, [SQ[0], SQ[1], SQ[2], (55, 40, 8, 8)], FRAME_OF), "face 3")
    zero = out.clone()
    zero[2] = 0
    clean(V.check_crop_faces_mixed(zero, frames, S, SQ, [0, 0, 1, 2]), 4)          # face 2 now lies in the small frame: outside it, zeros
    names(V.check_crop_faces_mixed(out, frames, S, SQ, [0, 0, 1, 2]), "face 2", "must be zeros")


# ---- packing -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_pack_yuv420(pictures, fmt):
    img = pictures["img"]
    codes = Y.encode(img, "bt709", False, Y.BITS[fmt], F32)
    clean(V.check_pack_yuv420(Y.tensor_of(codes, fmt), img, fmt, "bt709", False), 4)
    off = codes.clone()
    off[2, 3, 4] += 2
    names(V.check_pack_yuv420(Y.tensor_of(off, fmt), img, fmt, "bt709", False), "frame 2", "a code 2 from")
    names(V.check_pack_yuv420(Y.tensor_of(codes, fmt), img, fmt, "bt709", True), "frame")           # the other range
    if fmt in Y.IGNORED:
        junk = torch.zeros_like(codes)
        junk[1, 0, 0] = Y.IGNORED[fmt] & -Y.IGNORED[fmt]                         # (its lowest ignored bit)
        names(V.check_pack_yuv420(Y.tensor_of(codes, fmt, junk), img, fmt, "bt709", False), "frame 1", "outside their code")


# ---- pastes --------------------------------------------------------------------------------------------------------------------------
def _pasted(frames, img, matte, wins, fof, feather, paste_one, order=None):
    """the restatement evaluated in fp32, face after face (order: another sequence of the faces)"""
    out = frames.clone()
    for m in (range(len(wins)) if order is None else order):
        f = fof[m]
        out[f:f + 1] = paste_one(out[f:f + 1].contiguous(), img[m:m + 1], None if matte is None else matte[m:m + 1], wins[m])
    return out


@pytest.mark.parametrize("feather,use_matte", [(0.0, False), (0.125, True)])
def test_paste_windows_rgb8(pictures, feather, use_matte):
    rgb, img, matte = pictures["rgb"], pictures["img"], pictures["matte"] if use_matte else None
    one = lambda fr, im, ma, w: PB.paste(fr, im, [w], feather, ma, F32)
    got = _pasted(rgb, img, matte, FACES, FRAME_OF, feather, one)
    assert torch.equal(got[1], rgb[1]) and not torch.equal(got[0], rgb[0])
    fig = clean(V.check_paste_windows(got, rgb, img, SQ, feather, matte, FRAME_OF), 4)
    touched = 17 * 17 + 32 * 32 - 12 * 15 + 47 * 47 + 8 * 8                       # (the two faces of frame 0 share 12 x 15 pixels)
    assert fig["batch"] == 4 and fig["extra"][2] == 3 * touched and fig["extra"][0] == fig["extra"][1] <= V.MAX_SHARE * 3 * touched
    # the per-frame form, and a list of frames
    clean(V.check_paste_windows(_pasted(rgb, img[:3], None if matte is None else matte[:3], FACES[:3], [0, 1, 2], feather, one), rgb, img[:3],
                                SQ[:3], feather, None if matte is None else matte[:3]), 3)
    clean(V.check_paste_faces_mixed(list(got), list(rgb), img, SQ, FRAME_OF, feather, matte), 4)
    # a byte off by 2 inside a window
    off = got.clone()
    off[2, 10, 30, 1] += 2 if off[2, 10, 30, 1] < 128 else -2
    names(V.check_paste_windows(off, rgb, img, SQ, feather, matte, FRAME_OF), "face 2", "> 1")
    # a byte changed outside the touched mask
    off = got.clone()
    off[1, 0, 0, 0] ^= 1
    names(V.check_paste_windows(off, rgb, img, SQ, feather, matte, FRAME_OF), "frame 1", "outside the touched mask")
    # the two faces of frame 0 pasted in the wrong order: it shows only inside their intersection
    swapped = _pasted(rgb, img, matte, FACES, FRAME_OF, feather, one, order=[1, 0, 2, 3])
    inter = torch.zeros(HF, WF, dtype=torch.bool)
    inter[5:20, 6:18] = True
    assert torch.equal(swapped[0][~inter], got[0][~inter]) and not torch.equal(swapped[0][inter], got[0][inter])
    names(V.check_paste_windows(swapped, rgb, img, SQ, feather, matte, FRAME_OF), "face", "> 1")
    # a window the paste must leave out (smaller than S / 4; not square): pasting it anyway is found, leaving it out is right
    small = SQ[:3] + [(56, 40, 7, 7)]
    names(V.check_paste_windows(got, rgb, img, small, feather, matte, FRAME_OF), "outside the touched mask")
    left_out = _pasted(rgb, img, matte, FACES, FRAME_OF, feather, one, order=[0, 1, 2])
    clean(V.check_paste_windows(left_out, rgb, img, small, feather, matte, FRAME_OF), 4)
    clean(V.check_paste_windows(left_out, rgb, img, SQ[:3] + [(0, 0, 0, 0)], feather, matte, FRAME_OF), 4)
    # no rows at all
    assert clean(V.check_paste_windows(rgb.clone(), rgb, img[:0], [], feather, None, []), 0)["batch"] == 0


@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_paste_windows_yuv420(pictures, fmt):
    bits, img, matte, feather = Y.BITS[fmt], pictures["img"], pictures["matte"], 0.0625
    codes = pictures["codes"][bits]
    mode = ("bt709", False)
    junk = Y.junk_like(codes, fmt)
    before = Y.tensor_of(codes, fmt, junk)
    one = lambda fr, im, ma, w: Y.paste(fr, im, [w], feather, ma, *mode, bits, F32)
    got = _pasted(codes, img, matte, FACES, FRAME_OF, feather, one)
    touched = Y.touched_mask(tuple(codes.shape), FACES, FRAME_OF)
    after = Y.tensor_of(got, fmt, junk * ~touched)                                # (a touched sample comes out clean, the others keep their bits)
    fig = clean(V.check_paste_windows_yuv420(after, before, fmt, img, SQ, feather, matte, *mode, FRAME_OF), 4)
    assert fig["extra"][2] == int(touched.sum()) and fig["extra"][0] == fig["extra"][1]
    clean(V.check_paste_faces_mixed(list(after), list(before), img, SQ, FRAME_OF, feather, matte, fmt, *mode), 4)
    off = got.clone()
    off[0, HF + 3, 8] += 2                                                        # a chroma code under face 0 and face 1
    names(V.check_paste_windows_yuv420(Y.tensor_of(off, fmt, junk * ~touched), before, fmt, img, SQ, feather, matte, *mode, FRAME_OF), "face", "> 1")
    off = got.clone()
    off[1, 7, 7] += 1
    names(V.check_paste_windows_yuv420(Y.tensor_of(off, fmt, junk * ~touched), before, fmt, img, SQ, feather, matte, *mode, FRAME_OF),
          "frame 1", "outside the touched mask")
    swapped = _pasted(codes, img, matte, FACES, FRAME_OF, feather, one, order=[1, 0, 2, 3])
    names(V.check_paste_windows_yuv420(Y.tensor_of(swapped, fmt, junk * ~touched), before, fmt, img, SQ, feather, matte, *mode, FRAME_OF), "face", "> 1")
    if fmt in Y.IGNORED:
        names(V.check_paste_windows_yuv420(Y.tensor_of(got, fmt, junk), before, fmt, img, SQ, feather, matte, *mode, FRAME_OF), "outside their code")
        names(V.check_paste_windows_yuv420(Y.tensor_of(got, fmt), before, fmt, img, SQ, feather, matte, *mode, FRAME_OF), "ignored bits")


# ---- controls ------------------------------------------------------------------------------------------------------------------------
def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _thetas(n, seed):
    g = torch.Generator().manual_seed(seed)
    return R.pose_theta_fp64(1 + 0.1 * torch.randn(n, 3, generator=g), 0.4 * torch.randn(n, 3, generator=g), 0.1 * torch.randn(n, 3, generator=g)).float()


def test_mixing_theta():
    target, bank = _thetas(5, 1), _thetas(3, 2)
    index = torch.tensor([2, 0, 3, -1, 1], dtype=torch.int32)
    out = target.clone()
    for n, k in enumerate(index.tolist()):
        if 0 <= k < 3:
            out[n, :3] = _t(hostglue.mixing_theta(bank[k][None].numpy(), target[n][None].numpy(), True)[0]).float()
            out[n, 3] = torch.tensor([0.0, 0, 0, 1])
    clean(V.check_mixing_theta(out, target, bank, index, True), 5)
    one = out.clone()
    one[1, 0, 0] = torch.nextafter(one[1, 0, 0], torch.tensor(9.0))
    clean(V.check_mixing_theta(one, target, bank, index, True), 5)               # one ulp: inside the bound
    two = one.clone()
    two[1, 0, 0] = torch.nextafter(two[1, 0, 0], torch.tensor(9.0))
    names(V.check_mixing_theta(two, target, bank, index, True), "row 1 (source 0)", "2 ulp")
    names(V.check_mixing_theta(out, target, bank, index, False), "row")          # the other mixing
    moved = out.clone()
    moved[2] = out[0]
    names(V.check_mixing_theta(moved, target, bank, index, True), "row 2", "index 3", "pass through")
    names(V.check_mixing_theta(out, target, bank[[1, 0, 2]], index, True), "row 1 (source 0)")      # a bank row swapped


def _ema_case(masks):
    rng = np.random.default_rng(3)
    n, K = 9, 3
    values = rng.standard_normal((n, 4, 4)).astype(np.float32)
    so = np.array([0, 2, 2, 5, 1, 0, 2, 0, 1], np.int32)
    state, has = rng.standard_normal((K, 4, 4)).astype(np.float32), np.array([1, 0, 0], np.int32)
    restart = np.array([0, 0, 0, 0, 0, 1, 0, 0, 0], np.int32) if masks else None
    present = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], np.int32) if masks else None
    return values, so, state, has, restart, present


@pytest.mark.parametrize("masks", [False, True])
def test_theta_ema_scan_rows_and_the_state_left_behind(masks):
    values, so, state, has, restart, present = _ema_case(masks)
    st, hs = state.copy(), has.copy()
    want = hostglue.ema_scan_tracks(values, so, st, hs, 0.3, restart, present)
    args = (_t(values), _t(so), _t(state), _t(has), 0.3, _t(restart), _t(present))
    clean(V.check_theta_ema_scan(_t(want), *args, after=dict(state=_t(st), has_state=_t(hs))), 9)
    # a stale state row: the launch left stream 2's state as it was
    stale = st.copy()
    stale[2] = state[2]
    names(V.check_theta_ema_scan(_t(want), *args, after=dict(state=_t(stale), has_state=_t(hs))), "state state")
    names(V.check_theta_ema_scan(_t(want), *args, after=dict(state=_t(st), has_state=_t(has))), "state has_state")
    off = want.copy()
    off[6, 1, 1] = np.nextafter(off[6, 1, 1], np.float32(9))
    names(V.check_theta_ema_scan(_t(off), *args, after=dict(state=_t(st), has_state=_t(hs))), "row 6", "1 elements")
    written = want.copy()
    written[3] = 0                                                               # row 3's stream lies outside the bank: it stays unwritten
    names(V.check_theta_ema_scan(_t(written), *args, after=dict(state=_t(st), has_state=_t(hs))), "row 3", "outside the bank")
    names(V.check_theta_ema_scan(_t(want), _t(values), _t(so), _t(state), _t(has), 0.31, _t(restart), _t(present),
                                 after=dict(state=_t(st), has_state=_t(hs))), "row")            # another momentum
    if masks:                                                                    # the masks matter: without them the rows differ
        names(V.check_theta_ema_scan(_t(want), _t(values), _t(so), _t(state), _t(has), 0.3, None, None, after=dict(state=_t(st), has_state=_t(hs))), "row")


@pytest.mark.parametrize("relative,momentum,masks", [(True, 0.4, True), (True, None, False), (False, 0.5, False), (False, None, False)])
def test_expression_controls_rows_and_the_state_left_behind(relative, momentum, masks):
    rng = np.random.default_rng(4)
    n, K, E = 8, 2, 5
    f32 = lambda a: a.astype(np.float32)
    values, neutral, offset = f32(rng.standard_normal((n, E))), f32(rng.standard_normal((K, E))), f32(rng.standard_normal(E))
    so = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
    state = [f32(rng.standard_normal((K, E))), np.array([0, 1], np.int32), f32(rng.standard_normal((K, E))), np.array([1, 0], np.int32)]
    restart = np.array([0, 0, 0, 1, 0, 0, 0, 0], np.int32) if masks else None
    present = np.array([1, 0, 1, 1, 1, 0, 1, 1], np.int32) if masks else None
    left = [a.copy() for a in state]
    want = hostglue.expression_controls(values, so, neutral, np.full(n, 0.8, np.float32), np.tile(offset, (n, 1)), *left, relative, momentum,
                                        restart, present)
    after = dict(zip(("anchor", "has_anchor", "ema", "has_ema"), map(_t, left)))
    args = (_t(values), _t(so), _t(neutral), 0.8, _t(offset), *map(_t, state), relative, momentum, _t(restart), _t(present))
    clean(V.check_expression_controls(_t(want), *args, after=after), n)
    off = want.copy()
    off[5, 2] = np.nextafter(off[5, 2], np.float32(9))
    names(V.check_expression_controls(_t(off), *args, after=after), "row 5")
    names(V.check_expression_controls(_t(want), _t(values), _t(so), _t(neutral), 0.81, *args[4:], after=after), "row")
    if relative:
        stale = dict(after, anchor=_t(state[0]))                                 # stream 0's anchor was not kept
        names(V.check_expression_controls(_t(want), *args, after=stale), "state anchor")
    else:
        touched = dict(after, has_anchor=_t(1 - state[1]))                       # relative is off: the anchors are not the launch's to write
        names(V.check_expression_controls(_t(want), *args, after=touched), "has_anchor", "is off")
    if momentum is not None:
        names(V.check_expression_controls(_t(want), *args, after=dict(after, has_ema=_t(state[3]))), "state has_ema")


@pytest.mark.parametrize("relative,masks", [(True, True), (True, False), (False, False)])
def test_head_pose_controls_rows_theta_and_the_anchor_left_behind(relative, masks):
    rng = np.random.default_rng(6)
    n, K = 7, 2
    f32 = lambda a: a.astype(np.float32)
    scale, rot, trans = f32(1 + 0.1 * rng.standard_normal((n, 3))), f32(0.5 * rng.standard_normal((n, 3))), f32(0.1 * rng.standard_normal((n, 3)))
    source = f32(np.concatenate([1 + 0.1 * rng.standard_normal((K, 3)), 0.3 * rng.standard_normal((K, 3)), 0.1 * rng.standard_normal((K, 3))], 1))
    so = np.array([0, 1, 1, 0, 1, 0, 0], np.int32)
    anchor, has = f32(rng.standard_normal((K, 9))), np.array([0, 1], np.int32)
    anchor[1, 0:3] = 1.1
    restart = np.array([0, 0, 1, 0, 0, 0, 0], np.int32) if masks else None
    present = np.array([0, 1, 1, 1, 0, 1, 1], np.int32) if masks else None
    an, hs = anchor.copy(), has.copy()
    rows, _ = hostglue.head_pose_controls(scale, rot, trans, so, source, np.full(n, 0.7, np.float32), None, np.tile(f32(np.array([0.01, 0, -0.02])), (n, 1)),
                                          np.full(n, 1.1, np.float32), an if relative else None, hs if relative else None, relative, False, None,
                                          restart, present)
    theta = R.pose_theta_fp64(_t(rows[:, 0:3]), _t(rows[:, 3:6]), _t(rows[:, 6:9])).float()
    after = dict(anchor=_t(an), has_anchor=_t(hs))
    args = (_t(scale), _t(rot), _t(trans), _t(so), _t(source), 0.7, None, torch.tensor([0.01, 0, -0.02]), 1.1, _t(anchor), _t(has), relative, False,
            _t(restart), _t(present))
    fig = clean(V.check_head_pose_controls((_t(rows), theta), *args, after=after), n)
    assert fig["yardstick"] == "torch fp32" and fig["max_ratio"] <= R.SAMPLER_MAX
    off = rows.copy()
    off[4, 7] = np.nextafter(off[4, 7], np.float32(9))
    names(V.check_head_pose_controls((_t(off), theta), *args, after=after), "row 4")
    bad = theta.clone()
    bad[2, 1, 2] += 1e-4
    names(V.check_head_pose_controls((_t(rows), bad), *args, after=after), "pose_theta")
    if relative:
        stale = dict(after, anchor=_t(anchor), has_anchor=_t(hs))                # stream 0 has its flag but not its row
        names(V.check_head_pose_controls((_t(rows), theta), *args, after=stale), "state anchor")
        names(V.check_head_pose_controls((_t(rows), theta), *args, after=dict(after, has_anchor=_t(has))), "state has_anchor")
    else:
        names(V.check_head_pose_controls((_t(rows), theta), *args, after=dict(after, has_anchor=_t(1 - has))), "relative is off")


# ---- trackers ------------------------------------------------------------------------------------------------------------------------
def test_crop_track_windows_and_state():
    rng = np.random.default_rng(8)
    M, K = 8, 2
    c = np.stack([40 + rng.integers(-8, 9, M), 24 + rng.integers(-4, 5, M)], 1).astype(np.float64)
    boxes = np.concatenate([c - 9.5, c + 9], 1)
    boxes[3] = np.nan
    so = np.array([0, 1] * 4, np.int32)
    sizes = np.array([[WF, HF]] * 6 + [[20, 20]] * 2, np.int32)
    restart = np.array([0, 0, 0, 0, 1, 0, 0, 0], np.int32)
    state = [np.zeros((K, 3)), np.zeros(K, np.int32), np.zeros((K, 4), np.int32)]
    kw = dict(momentum=0.5, smooth=True, missing="hold", min_side=8)
    left = [a.copy() for a in state]
    want = hostglue.crop_track(boxes, so, sizes, *left, restart=restart, **kw)
    assert (want[1][:, 2] > 0).tolist() == [True] * 6 + [False] * 2              # (a held window, and two rows whose window leaves a small frame)
    after = dict(zip(("state", "has_state", "last"), map(_t, left)))
    call = lambda result, after=after, **more: V.check_crop_track(tuple(map(_t, result)), _t(boxes), _t(so), _t(sizes), *map(_t, state), restart=_t(restart),
                                                                  after=after, **dict(kw, **more))
    clean(call(want), M)
    moved = [w.copy() for w in want]
    moved[1][2, 0] += 1
    names(call(moved), "row 2", "paste")
    names(call(want, after=dict(after, state=_t(state[0]))), "state state")       # a stale state row
    names(call(want, after=dict(after, last=_t(state[2]))), "state last")
    names(call(want, momentum=0.25), "row")
    names(call(want, min_side=40), "row")


def test_track_assign_rows_and_tracks():
    import track_assign_cases as TC
    dets = np.full((5, 3, 4), np.nan)
    box = lambda x, y: np.array([x, y, x + 10.0, y + 12.0])
    dets[0, 2], dets[1, 0], dets[1, 1], dets[3, 1], dets[4, 0] = box(5, 5), box(6, 5), box(30, 20), box(31, 21), box(7, 6)
    ref, age = np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32)
    r, a = ref.copy(), age.copy()
    want = hostglue.track_assign(dets, None, r, a, 0.3, 1)
    assert want[1].sum() >= 3 and np.array_equal(want[0].view(np.uint64), TC.reference(dets, None, ref.copy(), age.copy(), 0.3, 1, "xyxy")[0].view(np.uint64))
    call = lambda result, rr=r, aa=a, mm=1: V.check_track_assign(tuple(map(_t, result)), _t(dets), None, _t(ref), _t(age), 0.3, mm, "xyxy",
                                                                after=dict(ref=_t(rr), age=_t(aa)))
    clean(call(want), 5)
    swapped = [w.copy() for w in want]
    swapped[2][1] = swapped[2][1][[1, 0, 2]]
    names(call(swapped), "frame 1", "track_of")
    names(call(want, aa=age), "state age")
    names(call(want, mm=3), "frame")
    live = a[0] >= 0
    stale = r.copy()
    stale[0, np.nonzero(live)[0][0]] += 1
    names(call(want, rr=stale), "state ref")


def test_present_rows():
    import present_rows_cases as C
    for name, (crop, paste, F_, P) in C.cases().items():
        want = hostglue.present_rows(crop, paste, F_, P)
        clean(V.check_present_rows(tuple(map(_t, want)), _t(crop), _t(paste), F_, P), F_)
    crop, paste = C.windows([1, 0, 1, 1, 0, 1], seed=2)
    want = [w.copy() for w in hostglue.present_rows(crop, paste, 3, 2)]
    assert want[2].tolist() == [0, 2, 3, 5, -1, -1]
    swapped = [w.copy() for w in want]
    swapped[2][[1, 2]] = swapped[2][[2, 1]]                                      # a row_of entry swapped
    names(V.check_present_rows(tuple(map(_t, swapped)), _t(crop), _t(paste), 3, 2), "row_of", "2 elements")
    short = [w.copy() for w in want]
    short[0][1] -= 1
    fig = names(V.check_present_rows(tuple(map(_t, short)), _t(crop), _t(paste), 3, 2), "count")
    assert fig["worst_frame"] == 1
    tail = [w.copy() for w in want]
    tail[4][5] = paste[5]                                                        # a window behind the present rows that is not zeros
    names(V.check_present_rows(tuple(map(_t, tail)), _t(crop), _t(paste), 3, 2), "paste_out")


# ---- the volumes' ends -----------------------------------------------------------------------------------------------------------------
def test_affine_grid3d_and_the_repacks():
    theta = _thetas(3, 9)
    size = (3, 5, 4)
    grid = torch.stack([R.theta_grid_fp64(theta[n], size).float() for n in range(3)])
    clean(V.check_affine_grid3d(grid, theta, size), 3)
    clean(V.check_affine_grid3d(torch.stack([R.theta_grid_f32(theta[n], size) for n in range(3)]), theta, size), 3)      # the reference's own bmm
    off = grid.clone()
    off[1, 2, 3, 1, 0] += 4 * 2.0 ** -23 * off[1, 2, 3, 1, 0].abs()              # four ulps in one coordinate
    names(V.check_affine_grid3d(off, theta, size), "frame 1")
    names(V.check_affine_grid3d(grid[[0, 2, 1]], theta, size), "frame")
    g = torch.Generator().manual_seed(10)
    cl = torch.randn(2, 3, 4, 5, 6, generator=g)                                  # [N,D,H,W,C]
    cf = cl.permute(0, 4, 1, 2, 3).contiguous()
    clean(V.check_volume_to_channels_first(cf, cl), 2)
    names(V.check_volume_to_channels_first(cl.permute(0, 4, 1, 3, 2).reshape(cf.shape).contiguous(), cl), "differ")
    bank = torch.randn(4, 3, 4, 5, 6, generator=g)
    row = torch.tensor([3, 7, 0], dtype=torch.int32)                             # (7: outside the bank, nothing is written)
    vol = torch.randn(3, 6, 3, 4, 5, generator=g)
    after = bank.clone()
    after[3], after[0] = vol[0].permute(1, 2, 3, 0), vol[2].permute(1, 2, 3, 0)
    clean(V.check_volume_to_channels_last_indexed(after, vol, bank, row), 3)
    names(V.check_volume_to_channels_last_indexed(bank, vol, bank, row), "differ")                 # nothing was written
    stray = after.clone()
    stray[1, 0, 0, 0, 0] += 1
    names(V.check_volume_to_channels_last_indexed(stray, vol, bank, row), "no `row` names")
    swapped = after.clone()
    swapped[3], swapped[0] = after[0], after[3]
    names(V.check_volume_to_channels_last_indexed(swapped, vol, bank, row), "differ")


def test_grid_sample3d_on_a_given_grid():
    g = torch.Generator().manual_seed(12)
    vol, grid = torch.randn(2, 4, 3, 5, 6, generator=g), torch.rand(2, 3, 4, 5, 3, generator=g) * 2.4 - 1.2
    for pm in ("zeros", "border"):
        out = F.grid_sample(vol, grid, mode="bilinear", padding_mode=pm, align_corners=False)
        fig = clean(V.check_grid_sample3d_grid(out, vol, grid, pm), 2)
        assert fig["max_ratio"] == 1.0
        names(V.check_grid_sample3d_grid(F.grid_sample(vol, grid.flip(-1), padding_mode=pm, align_corners=False), vol, grid, pm), "max err")
    names(V.check_grid_sample3d_grid(F.grid_sample(vol, grid, padding_mode="border", align_corners=False), vol, grid, "zeros"), "err")
