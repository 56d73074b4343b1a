"""Every launch the video path makes, against its reference, on every row.

emoportraits_amd/infer.py (animate_frames, _animate_clip, _track_chunk, animate_streams, the control launches, forward, animate,
enrolment) and frames.py (crops_of, paste_into) build their launches from windows the tracker computed, compacted rows, frame_of
runs with gaps, arena frames and row masks.  Here every ops.<name> they call is wrapped with the OpLaunchChecker of
test_op_launches_fp64_gpu.py while the wrapper of the tiny fixture runs EAGERLY (a captured sequence replays without Python): each
launch runs on the caller's own tensors -- what it writes in place is copied first -- and is compared at once, row by row, with
the references of tests/video_reference.py: fp64 restatements for the crops, the packs and the pastes, the host contracts of
hostglue.py bit for bit for the controls and the trackers.  The launches the hot path makes underneath (add, grid_sample3d,
mat4_inverse, volume_to_channels_last from nets.py, pose_theta from the stand-in regressor) pass through the same wrappers and are
checked with the rest.

One test per configuration, one PARITY line each: the worst figure per operation and the inventory (operation, form, shape) ->
launches.  MAX_BYTE_DIFF is judged per launch and per row; the share of differing bytes is judged per test over all its paste
launches, beside the share of torch's fp32 evaluation of the same restatement, which is asserted as the premise.

Windows the tracker makes have even sides (hostglue.crop_track: size -= size % 2, side -= side % 2), so D and E assert odd and even
origins, three of the four byte-address residues of a window row's first pixel, and that every side is even; odd sides are held in
A and C, whose windows the caller gives.

The guard at the end runs without a GPU: every ops.<name>( call of infer.py and frames.py is wrapped here, exempt with a reason,
or held by a named test that exists."""
import os

import numpy as np
import pytest
import torch

import video_reference as V
import yuv420_reference as Y
from emoportraits_amd import frames as frames_mod
from emoportraits_amd import hostglue, infer, ops
from guarded_outputs import guarded_outputs  # noqa: F401  (every output ops allocates: poisoned, between guards; the GPU tests ask for it)
from test_head_pose_controls_gpu import make_wrapper, project, tiny  # noqa: F401  (the tiny fixture's wrapper: toy embedders, a 2-slot bank)
from test_op_launches_fp64_gpu import OpLaunchChecker, ops_called, register

DEV = "cuda:0"
VIDEO_OPS = ("unpack_rgb8", "pack_rgb8", "mul_mask", "resize2d", "pose_theta", "mat4_inverse", "grid_sample3d", "add",
             "volume_to_channels_last", "resize2d_windows", "yuv420_windows", "crop_faces_mixed", "pack_yuv420", "paste_windows",
             "paste_windows_yuv420", "paste_faces_mixed", "mixing_theta", "theta_ema_scan", "expression_controls", "head_pose_controls",
             "crop_track", "track_assign", "present_rows", "affine_grid3d", "volume_to_channels_first", "volume_to_channels_last_indexed")
register(VIDEO_OPS)
EXEMPT = {"yuv420_dtype": "a table lookup: the dtype of a format's frames, no launch",
          "yuv420_name": "a table lookup: the format's name in a message, no launch",
          "yuv420_geometry": "a host check of a frame tensor's shape and strides, no launch",
          "windows_host": "the host check of a window list: no device, no upload",
          "DeviceWindows": "a holder of an int32 [M,4] device tensor: no launch; the ops that take it are wrapped",
          "overflow_events": "a host read of the overflow words: no launch"}
HELD_ELSEWHERE = {}                   # name -> "tests/<file>::<test> (why configuration F cannot reach the call)": none is needed today
PASTES = ("paste_windows", "paste_windows_yuv420", "paste_faces_mixed")
S, BATCH = 64, 4                      # the tiny fixture's image_size; rows (and frames) per batch
BIG, SMALL = (96, 128), (64, 96)      # the two frame sizes (H, W)


def _device_windows(w):
    return isinstance(w, ops.DeviceWindows) or isinstance(w, torch.Tensor) and w.is_cuda


def _window_form(a, frames_n):
    """host | device windows, frame_of (gaps: a frame of the batch without a row), absent (a window without a side)"""
    if a.get("windows") is None:
        return "whole frames"
    wins = V.windows_of(a["windows"])
    form = ("device" if _device_windows(a["windows"]) else "host") + " windows"
    if a.get("frame_of") is not None:
        fof = [int(v) for v in a["frame_of"]]
        form += " frame_of" + (" gaps" if set(range(frames_n)) - set(fof) else "") + (" several" if len(set(fof)) < len(fof) else "")
    if any(w[2] <= 0 for w in wins):
        form += " absent"
    return form


class VideoLaunchChecker(OpLaunchChecker):
    """OpLaunchChecker over the operations infer.py and frames.py launch; keeps the windows it saw and the pastes' byte counts"""
    wrapped = VIDEO_OPS
    title = "video launches"
    modules = (infer, frames_mod)
    mutated = dict(paste_windows=("frames_u8",), paste_windows_yuv420=("frames",), paste_faces_mixed=("frames",),
                   theta_ema_scan=("state", "has_state"), expression_controls=("anchor", "has_anchor", "ema", "has_ema"),
                   head_pose_controls=("anchor", "has_anchor"), crop_track=("state", "has_state", "last"), track_assign=("ref", "age"),
                   volume_to_channels_last_indexed=("bank",))

    def __init__(self, tag):
        super().__init__(tag)
        self.windows = []             # (op, x0, y0, side, byte address of the window's first sample mod 4) of every present window

    def _saw(self, op, wins, fof, address_of):
        for w, f in zip(wins, fof):
            if w[2] > 0:
                self.windows.append((op, w[0], w[1], w[2], address_of(f, w) % 4))

    # ---- taken as they are: ops_reference's checks ---------------------------------------------------------------------------
    def _check_unpack_rgb8(self, a, out):
        return "", tuple(a["frames_u8"].shape[1:]), V.check_unpack_rgb8(out, a["frames_u8"])

    def _check_pack_rgb8(self, a, out):
        return "", tuple(a["img"].shape[1:]), V.check_pack_rgb8(out, a["img"])

    def _check_mul_mask(self, a, out):
        return "", tuple(a["img"].shape[1:]), V.check_mul_mask(out, a["img"], a["mask"])

    def _check_resize2d(self, a, out):
        form = f"{a['mode']} -> {tuple(a['size'])}" + (" window" if a["window"] is not None else "") + (" clamp01" if a["clamp01"] else "")
        return form, tuple(a["x"].shape[1:]), V.check_resize2d(out, a["x"], a["size"], a["mode"], a["window"], a["clamp01"])

    def _check_pose_theta(self, a, out):
        return f"scale [{a['scale'].shape[1]}]", (4, 4), V.check_pose_theta(out, a["scale"], a["rotation"], a["translation"])

    def _check_grid_sample3d(self, a, out):
        if a["grid"] is not None and a["in_layout"] == a["out_layout"] == "ncdhw" and a["vol_index"] is None:
            return "grid ncdhw->ncdhw", tuple(a["vol"].shape[1:]), V.check_grid_sample3d_grid(out, a["vol"], a["grid"], a["padding_mode"])
        return super()._check_grid_sample3d(a, out)

    # ---- crops -------------------------------------------------------------------------------------------------------------------
    def _check_resize2d_windows(self, a, out):
        x = a["x"]
        wins = V.windows_of(a["windows"])
        fof = V.frames_of(a["frame_of"], x.shape[0], len(wins))
        # (x is the fp32 picture of rgb8 frames [N,H,W,3]: the bytes under a window begin 3 * (y0 * W + x0) into their frame)
        self._saw("resize2d_windows", wins, fof, lambda f, w: 3 * ((f * x.shape[2] + w[1]) * x.shape[3] + w[0]))
        fig = V.check_resize2d_windows(out, x, a["size"], a["windows"], a["mode"], a["clamp01"], a["frame_of"])
        return _window_form(a, x.shape[0]), tuple(x.shape[1:]), fig

    def _check_yuv420_windows(self, a, out):
        fr = a["frames"]
        if a["windows"] is not None:
            wins = V.windows_of(a["windows"])
            self._saw("yuv420_windows", wins, V.frames_of(a["frame_of"], fr.shape[0], len(wins)),
                      lambda f, w: fr.data_ptr() + (f * fr.stride(0) + w[1] * fr.stride(1) + w[0]) * fr.element_size())
        fig = V.check_yuv420_windows(out, fr, a["frame_format"], a["size"], a["windows"], a["colorspace"], a["full_range"], a["frame_of"])
        return f"{a['frame_format']} {_window_form(a, fr.shape[0])}", tuple(fr.shape[1:]), fig

    def _check_crop_faces_mixed(self, a, out):
        frames, rgb = a["frames"], a["frame_format"] == "rgb8"
        self._saw("crop_faces_mixed", V.windows_of(a["windows"]), [int(v) for v in a["frame_of"]],
                  lambda f, w: frames[f].data_ptr() + (w[1] * frames[f].stride(0) + (3 if rgb else 1) * w[0]) * frames[f].element_size())
        fig = V.check_crop_faces_mixed(out, frames, a["size"], a["windows"], a["frame_of"], a["frame_format"], a["colorspace"], a["full_range"])
        sizes = tuple(sorted({tuple(t.shape[:2]) for t in frames}))
        return f"{a['frame_format']} {_window_form(a, len(frames))}", sizes, fig

    def _check_pack_yuv420(self, a, out):
        return a["frame_format"], tuple(a["img"].shape[1:]), V.check_pack_yuv420(out, a["img"], a["frame_format"], a["colorspace"], a["full_range"])

    # ---- pastes (in place: the frames from before the launch are the input) ---------------------------------------------------------
    def _paste_form(self, a, frames_n):
        return _window_form(a, frames_n) + (" matte" if a["matte"] is not None else "") + f" feather {a['feather']:g}"

    def _check_paste_windows(self, a, out):
        after, before = a["after"]["frames_u8"], a["frames_u8"]
        assert out is after
        wins = V.windows_of(a["windows"])
        self._saw("paste_windows", wins, V.frames_of(a["frame_of"], after.shape[0], len(wins)),
                  lambda f, w: after.data_ptr() + f * after.stride(0) + w[1] * after.stride(1) + 3 * w[0])
        fig = V.check_paste_windows(after, before, a["img"], a["windows"], a["feather"], a["matte"], a["frame_of"])
        return self._paste_form(a, after.shape[0]), tuple(after.shape[1:]), fig

    def _check_paste_windows_yuv420(self, a, out):
        after, before = a["after"]["frames"], a["frames"]
        assert out is after
        wins = V.windows_of(a["windows"])
        self._saw("paste_windows_yuv420", wins, V.frames_of(a["frame_of"], after.shape[0], len(wins)),
                  lambda f, w: after.data_ptr() + (f * after.stride(0) + w[1] * after.stride(1) + w[0]) * after.element_size())
        fig = V.check_paste_windows_yuv420(after, before, a["frame_format"], a["img"], a["windows"], a["feather"], a["matte"], a["colorspace"],
                                           a["full_range"], a["frame_of"])
        return f"{a['frame_format']} {self._paste_form(a, after.shape[0])}", tuple(after.shape[1:]), fig

    def _check_paste_faces_mixed(self, a, out):
        after, before, rgb = a["after"]["frames"], a["frames"], a["frame_format"] == "rgb8"
        assert out is after
        self._saw("paste_faces_mixed", V.windows_of(a["windows"]), [int(v) for v in a["frame_of"]],
                  lambda f, w: after[f].data_ptr() + (w[1] * after[f].stride(0) + (3 if rgb else 1) * w[0]) * after[f].element_size())
        fig = V.check_paste_faces_mixed(after, before, a["img"], a["windows"], a["frame_of"], a["feather"], a["matte"], a["frame_format"],
                                        a["colorspace"], a["full_range"])
        sizes = tuple(sorted({tuple(t.shape[:2]) for t in after}))
        return f"{a['frame_format']} {self._paste_form(a, len(after))}", sizes, fig

    def paste_share(self):
        """(differing touched samples / touched samples, the same for torch's fp32 evaluation of the restatement, touched samples,
        the share of them that the launches changed) over every paste launch of the run"""
        d = d32 = n = c = 0
        for r in self.rows:
            if r["op"] in PASTES:
                d, d32, n, c = d + r["extra"][0], d32 + r["extra"][1], n + r["extra"][2], c + r["extra"][3]
        return d / max(n, 1), d32 / max(n, 1), n, c / max(n, 1)

    # ---- controls ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _masks_form(a, zeros):
        return ("tracks" if a["restart"] is not None or a["present"] is not None else "plain") + (" over zero rows" if zeros else "")

    def _check_mixing_theta(self, a, out):
        form = ("indexed" if a["index"] is not None else "one source") + (" mix_old" if a["mix_old"] else "")
        return form, (4, 4), V.check_mixing_theta(out, a["target"], a["source_bank"], a["index"], a["mix_old"])

    def _check_theta_ema_scan(self, a, out):
        fig = V.check_theta_ema_scan(out, a["values"], a["stream_of"], a["state"], a["has_state"], a["momentum"], a["restart"], a["present"],
                                     after=a["after"])
        return self._masks_form(a, not bool(a["values"].any())) + f" K={a['state'].shape[0]}", (4, 4), fig

    def _check_expression_controls(self, a, out):
        fig = V.check_expression_controls(out, a["values"], a["stream_of"], a["neutral"], a["gain"], a["offset"], a["anchor"], a["has_anchor"],
                                          a["ema"], a["has_ema"], a["relative"], a["momentum"], a["restart"], a["present"], after=a["after"])
        form = self._masks_form(a, not bool(a["values"].any())) + (" relative" if a["relative"] else "") + \
            (" smooth" if a["momentum"] is not None else "") + (" gain" if a["gain"] is not None else "") + (" offset" if a["offset"] is not None else "")
        return form, tuple(a["values"].shape[1:]), fig

    def _check_head_pose_controls(self, a, result):
        fig = V.check_head_pose_controls(result, a["scale"], a["rotation"], a["translation"], a["stream_of"], a["source"], a["gain"],
                                         a["rotation_offset"], a["translation_offset"], a["zoom"], a["anchor"], a["has_anchor"], a["relative"],
                                         a["frontal"], a["restart"], a["present"], after=a["after"])
        form = self._masks_form(a, not bool(a["scale"].any())) + (" relative" if a["relative"] else "") + (" frontal" if a["frontal"] else "") + \
            "".join(f" {k}" for k in ("gain", "rotation_offset", "translation_offset", "zoom") if a[k] is not None)
        return form, (a["scale"].shape[1],), fig

    # ---- trackers ----------------------------------------------------------------------------------------------------------------
    def _check_crop_track(self, a, result):
        fig = V.check_crop_track(result, a["boxes"], a["stream_of"], a["size"], a["state"], a["has_state"], a["last"], a["momentum"], a["smooth"],
                                 a["fixed"], a["scale"], a["box_format"], a["missing"], a["min_side"], a["K"], a["restart"], after=a["after"])
        size = a["size"]
        per_row = not (isinstance(size, (tuple, list)) and len(size) == 2 and not isinstance(size[0], (tuple, list)))
        form = ("sizes per row" if per_row else "one size") + (" restart" if a["restart"] is not None else "") + (" smooth" if a["smooth"] else "") + \
            f" min_side {a['min_side']}"
        return form, (tuple(a["boxes"].shape[1:])), fig

    def _check_track_assign(self, a, result):
        fig = V.check_track_assign(result, a["dets"], a["stream_of"], a["ref"], a["age"], a["min_iou"], a["max_missed"], a["box_format"],
                                   after=a["after"])
        return f"P={a['age'].shape[1]} max_missed {a['max_missed']}", tuple(a["dets"].shape[1:]), fig

    def _check_present_rows(self, a, result):
        return f"P={a['P']}", (4,), V.check_present_rows(result, a["crop"], a["paste"], a["F"], a["P"])

    # ---- the volumes' ends -----------------------------------------------------------------------------------------------------
    def _check_affine_grid3d(self, a, out):
        return "", tuple(a["size"]), V.check_affine_grid3d(out, a["theta"].float(), a["size"])

    def _check_volume_to_channels_first(self, a, out):
        return "", tuple(a["vol"].shape[1:]), V.check_volume_to_channels_first(out, a["vol"])

    def _check_volume_to_channels_last_indexed(self, a, out):
        fig = V.check_volume_to_channels_last_indexed(a["after"]["bank"], a["vol"], a["bank"], a["row"])
        fig["batch"] = a["vol"].shape[0]                                           # (the result is the bank: its rows are the volumes')
        return f"K={a['bank'].shape[0]}", tuple(a["vol"].shape[1:]), fig


# ---- running a configuration -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapper(project, tiny):  # noqa: F811
    assert tiny["cfg"]["image_size"] == S
    return make_wrapper(project, tiny, K=2, use_graphs=False)


def _fresh(w):
    w.reset_crop_state(), w.reset_pose_state(), w.reset_expression_state()


def _run(monkeypatch, tag, fn, pastes=False):
    """fn under the checker -> (the checker, its inventory, fn's result); with pastes: the share of differing touched bytes over all
    paste launches, judged for the run, and the premise that torch's fp32 evaluation of the restatement stays under MAX_SHARE"""
    chk = VideoLaunchChecker(tag)
    with monkeypatch.context() as mp:
        chk.install(mp)
        result = fn()
    torch.cuda.synchronize()
    inv = chk.report()
    if pastes:
        share, share32, touched, changed = chk.paste_share()
        print(f"PARITY pastes [{tag}]: {touched} touched samples, {changed:.3f} of them changed by the launches; share that differ from "
              f"the fp64 restatement {share:.2e} (torch fp32 against fp64: {share32:.2e}; MAX_SHARE {V.MAX_SHARE:g})")
        assert touched > 0 and share32 <= V.MAX_SHARE, (touched, share32)
        assert changed > 0.25, f"the pastes changed {changed:.3f} of the samples under their windows: the rendered image or the matte is degenerate"
        assert share <= V.MAX_SHARE, share
    chk.assert_clean()
    return chk, inv, result


def _consume(gen):
    """what a video generator yields, cloned (a yielded tensor is valid only until the generator is resumed)"""
    out = []
    for item in gen:
        out.append([(s, t, o.clone()) for s, t, o in item] if isinstance(item, list) else (item[0], item[1].clone()))
    return out


def _rgb_clip(n, hw, seed):
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _yuv_clip(n, hw, fmt, seed):
    """n frames of random legal-ish codes in the layout, junk in the ignored bits of the 10-bit words"""
    g = torch.Generator().manual_seed(seed)
    top = 1 << Y.BITS[fmt]
    codes = torch.randint(top // 16, top - top // 16, (n, hw[0] * 3 // 2, hw[1]), generator=g, dtype=torch.int32)
    return Y.tensor_of(codes, fmt, Y.junk_like(codes, fmt, seed))


def _same(a, b):
    """equal, element for element (through numpy: 16-bit words too)"""
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _matte(img):
    """a matte that follows the picture and never lets the frame through untouched"""
    return (0.3 + img.mean(dim=1, keepdim=True)).clamp(0, 1)


def _assert_window_spread(windows, even_sides_only, residues=True):
    """odd and even x0 and y0, three of the four byte-address residues of a window row's first sample (residues=False: 16-bit samples
    have two) -- and the sides: tracker-made windows are even by hostglue.crop_track's rule, a caller's list holds both"""
    assert windows
    assert {w[1] & 1 for w in windows} == {0, 1} and {w[2] & 1 for w in windows} == {0, 1}, sorted({(w[1], w[2]) for w in windows})
    assert not residues or len({w[4] for w in windows}) >= 3, sorted({w[4] for w in windows})
    sides = {w[3] & 1 for w in windows}
    assert sides == ({0} if even_sides_only else {0, 1}), sorted({w[3] for w in windows})


# ---- A: rgb8, a host list of windows, paste_back with a matte, mix and smooth_pose per identity --------------------------------------
A_WINDOWS = [(1, 3, 33), (2, 0, 64), (7, 5, 81), (32, 0, 96), (13, 11, 70), (0, 1, 95), (63, 31, 65), (30, 2, 16), (5, 6, 47), (18, 9, 80)]


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_a_rgb8_host_windows_paste_back_every_launch(wrapper, monkeypatch):
    """10 frames of 96 x 128 in chunks of 6 + 4, batches of 4: odd and even origins and sides, a side of S / 4, the frame's full
    height; identities over both slots, so the EMA state of each slot crosses the batches and the chunk boundary"""
    w, N = wrapper, 10
    clip = _rgb_clip(N, BIG, 201)
    assert all(x + s <= BIG[1] and y + s <= BIG[0] and 4 * s >= S for x, y, s in A_WINDOWS) and len(A_WINDOWS) == N
    ids = [0, 1, 1, 0, 1, 0, 0, 1, 0, 1]
    _fresh(w)
    chk, inv, out = _run(monkeypatch, "A rgb8 windows paste_back", lambda: _consume(w.animate_frames(
        iter([clip[:6], clip[6:]]), batch_size=BATCH, windows=A_WINDOWS, to_host=False, paste_back=True, paste_matte=_matte, identities=ids,
        mix=True, smooth_pose=True, smooth_per_identity=True)), pastes=True)
    assert sum(o.shape[0] for _, o in out) == N
    assert chk.has("unpack_rgb8") and chk.has("resize2d_windows", "host windows") and chk.has("mixing_theta", "indexed mix_old"), inv
    assert chk.has("paste_windows", lambda f: f.startswith("host windows matte")), inv
    assert sum(r["frames"] for r in chk.has("paste_windows")) == N == sum(r["frames"] for r in chk.has("resize2d_windows")), inv
    assert len(chk.has("theta_ema_scan", "plain K=2")) == 2, inv                    # (one scan per chunk, over all its rows)
    _assert_window_spread([x for x in chk.windows if x[0] == "paste_windows"], even_sides_only=False)


# ---- B: NV12 whole frames, out_format given ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_b_nv12_whole_frames_and_both_packs_every_launch(wrapper, monkeypatch):
    """8 frames of 96 x 128 as NV12 in chunks of 5 + 3, no windows: the whole-frame crop resized to S; out_format 'rgb8', 'nv12' and
    'yuv420p10' give pack_rgb8 and pack_yuv420 at 8 and at 10 bits.  Then 4 frames of S x S: the whole frame at its own size is the
    plain conversion, held under D_TOL"""
    w, N = wrapper, 8
    clip = _yuv_clip(N, BIG, "nv12", 211)
    own = _yuv_clip(4, (S, S), "nv12", 212)

    def calls():
        for out_format in ("rgb8", "nv12", "yuv420p10"):
            _fresh(w)
            out = _consume(w.animate_frames(iter([clip[:5], clip[5:]]), batch_size=BATCH, to_host=False, frame_format="nv12", colorspace="bt601",
                                            full_range=True, out_format=out_format))
            assert sum(o.shape[0] for _, o in out) == N and out[0][1].dtype == ops.yuv420_dtype(out_format)
        _consume(w.animate_frames(own, batch_size=BATCH, to_host=False, frame_format="nv12", out_format="nv12"))
    chk, inv, _ = _run(monkeypatch, "B nv12 whole frames", calls)
    whole = chk.has("yuv420_windows", "nv12 whole frames")
    assert {r["shape"] for r in whole} == {(144, 128), (96, 64)} and sum(r["frames"] for r in whole) == 3 * N + 4, inv
    assert chk.has("pack_rgb8") and chk.has("pack_yuv420", "nv12") and chk.has("pack_yuv420", "yuv420p10"), inv
    assert not chk.has("unpack_rgb8") and not chk.has("resize2d_windows"), inv


# ---- C: faces= with a frame of no face and overlapping faces, paste_back, planar 8-bit and interleaved 10-bit -------------------------------
C_FACES = [[(1, 3, 33), (10, 8, 64)], [], [(20, 0, 96), (40, 20, 48), (31, 1, 71)], [(64, 32, 64)], [(0, 0, 16)], [(5, 7, 80), (3, 2, 47)],
           [], [(17, 15, 66)]]


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
@pytest.mark.parametrize("fmt", ["yuv420p", "p010"])
def test_c_faces_paste_back_yuv_every_launch(wrapper, monkeypatch, fmt):
    """8 frames of 96 x 128 in chunks of 5 + 3, 10 faces: two- and three-way overlaps pasted in list order, frames without a face
    inside a batch, odd origins and sides (a chroma sample shared with the frame), a side of S / 4; p010 with junk in the six
    ignored bits of every word"""
    w, N = wrapper, len(C_FACES)
    clip = _yuv_clip(N, BIG, fmt, 221)
    flat = [f for of_frame in C_FACES for f in of_frame]
    assert all(x + s <= BIG[1] and y + s <= BIG[0] and 4 * s >= S for x, y, s in flat)
    ids = [(3 * m + m // 3) % 2 for m in range(len(flat))]
    _fresh(w)
    chk, inv, out = _run(monkeypatch, f"C {fmt} faces paste_back", lambda: _consume(w.animate_frames(
        iter([clip[:5], clip[5:]]), batch_size=BATCH, faces=C_FACES, to_host=False, paste_back=True, feather=0.125, identities=ids,
        frame_format=fmt, colorspace="bt709", full_range=False, smooth_pose=True, smooth_per_identity=True)), pastes=True)
    got = [f for _, o in out for f in o]
    assert len(got) == N and all(_same(got[i], clip[i]) == (not C_FACES[i]) for i in range(N))
    assert chk.has("yuv420_windows", lambda f: f.startswith(f"{fmt} host windows frame_of") and "several" in f), inv
    assert chk.has("yuv420_windows", lambda f: "gaps" in f) and chk.has("paste_windows_yuv420", lambda f: "gaps" in f and "several" in f), inv
    assert sum(r["frames"] for r in chk.has("paste_windows_yuv420")) == len(flat), inv
    _assert_window_spread([x for x in chk.windows if x[0] == "paste_windows_yuv420"], even_sides_only=False, residues=fmt != "p010")


# ---- D: detections with dropouts, a death and a rebirth; follow_tracks, with and without skip_absent; the controls that carry state ------
def d_detections():
    """10 frames of 96 x 128 in chunks of 6 + 4, two track slots, three detection rows in no stable order.  Face A is seen in frames
    0, 1 and 3 (a dropout in frame 2) and then leaves: with max_missed = 1 its track dies in frame 5.  Nobody is seen in frames 4 and
    5, which are a batch of their own.  C is born in frame 6 into the slot A freed, E in frame 7 into the other; C drops out in frame
    8.  -> (dets [10,3,4], the faces seen per frame)"""
    N, (H, W) = 10, BIG
    rng = np.random.default_rng(5)

    def walk(cx, cy, half):
        c = np.stack([cx + rng.integers(-6, 7, N), cy + rng.integers(-3, 4, N)], 1).astype(np.float64)
        h = half + rng.integers(-3, 4, (N, 2)) * 0.5
        return np.concatenate([c - h, c + h], 1)
    A, C, E = walk(47, 46, 17), walk(52, 49, 18), walk(85, 45, 16)
    dets = np.full((N, 3, 4), np.nan)
    for t in (0, 1, 3):
        dets[t, (t + 1) % 3] = A[t]
    for t in (6, 7, 9):
        dets[t, t % 3] = C[t]
    for t in (7, 8, 9):
        dets[t, (t + 2) % 3] = E[t]
    return dets, [1, 1, 0, 1, 0, 0, 1, 2, 1, 2]


D_TRACKING = dict(smooth=True, momentum=0.5, tracks=2, min_iou=0.2, max_missed=1, follow_tracks=True)
D_CONTROLS = dict(smooth_pose=True, smooth_per_identity=True, expression=dict(relative=True, smooth=True, momentum=0.4),
                  head_pose=dict(relative=True))


def d_host_account(dets, chunks=(6, 4)):
    """what hostglue says the trackers do with d_detections(), chunk by chunk as the clip loop calls them: (restart [N,2], the
    paste windows [N,2,4] with min_side = S / 4)"""
    ref, age = np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32)
    st, has, last = np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros((2, 4), np.int32)
    restarts, pastes, base = [], [], 0
    for n in chunks:
        boxes, restart, _ = hostglue.track_assign(dets[base:base + n], None, ref, age, D_TRACKING["min_iou"], D_TRACKING["max_missed"])
        _, paste, _ = hostglue.crop_track(boxes.reshape(-1, 4), np.tile(np.arange(2), n), (BIG[1], BIG[0]), st, has, last,
                                          momentum=D_TRACKING["momentum"], smooth=True, min_side=S // 4, restart=restart.reshape(-1))
        restarts.append(restart), pastes.append(paste.reshape(n, 2, 4))
        base += n
    return np.concatenate(restarts), np.concatenate(pastes)


def test_d_detections_are_what_the_configuration_is_there_for():
    """no GPU: hostglue's account of the detections -- the death in the batch nobody is in, the rebirth into the freed slot, every
    present window with a side of at least 32, odd and even origins and three of the four byte residues"""
    dets, seen = d_detections()
    restart, paste = d_host_account(dets)
    present = paste[:, :, 2] > 0
    assert present.sum(1).tolist() == seen
    assert restart[:, 0].tolist() == [1, 0, 0, 0, 0, 1, 1, 0, 0, 0] and restart[:, 1].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert frames_mod.face_spans(seen[:6], 0, 6, BATCH) == [(0, 4), (4, 6)] and not sum(seen[4:6])        # the death: in an empty batch
    wins = paste[present]
    assert wins[:, 2].min() >= 32 and not (wins[:, 2] & 1).any()
    assert set((wins[:, 0] & 1).tolist()) == {0, 1} and set((wins[:, 1] & 1).tolist()) == {0, 1}
    assert len(set(((3 * wins[:, 0]) % 4).tolist())) >= 3                           # (rows of 3 * 128 bytes: the residue is 3 * x0 mod 4)


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
@pytest.mark.parametrize("skip_absent", [True, False], ids=["skip_absent", "every_row"])
def test_d_tracked_detections_with_the_state_carrying_controls_every_launch(wrapper, monkeypatch, skip_absent):
    """rgb8 paste_back.  skip_absent: the crop, the networks and the paste see the kept rows only (compacted device windows, frame_of
    with gaps), the controls run over the full rows, and the batch nobody is in still launches them over zeros so that the death
    in it reaches its stream.  every_row: absent rows are rendered from the centred square and their paste windows have no side"""
    w, N = wrapper, 10
    dets, seen = d_detections()
    want_restart, want_paste = d_host_account(dets)
    clip, td = _rgb_clip(N, BIG, 231), torch.from_numpy(dets).to(DEV)
    _fresh(w)
    chk, inv, out = _run(monkeypatch, f"D detections skip_absent={skip_absent}", lambda: _consume(w.animate_frames(
        iter([clip[:6], clip[6:]]), batch_size=BATCH, detections=iter([td[:6], td[6:]]), tracking=dict(D_TRACKING, skip_absent=skip_absent),
        identities=[0, 1] * N, to_host=False, paste_back=True, **D_CONTROLS)), pastes=True)
    got = torch.cat([o for _, o in out]).cpu()
    assert got.shape == clip.shape and [torch.equal(got[i], clip[i]) for i in range(N)] == [c == 0 for c in seen]
    assert np.array_equal(w.tracked_assignment[1].cpu().numpy(), want_restart[6:])                     # (the last chunk's)
    assert np.array_equal(w.tracked_windows[0].cpu().numpy().reshape(-1, 2, 4), want_paste[6:])
    assert len(chk.has("track_assign", "P=2 max_missed 1")) == 2 == len(chk.has("crop_track", lambda f: f.startswith("one size restart smooth"))), inv
    for op in ("theta_ema_scan", "expression_controls", "head_pose_controls"):
        assert chk.has(op, lambda f: f.startswith("tracks")), (op, inv)
    if skip_absent:
        assert len(chk.has("present_rows", "P=2")) == 2, inv
        assert chk.has("resize2d_windows", lambda f: f.startswith("device windows frame_of") and "gaps" in f), inv
        for what in ("gaps", "several"):                                         # (a frame nobody is kept in; two kept rows of one frame)
            assert chk.has("paste_windows", lambda f: f.startswith("device windows frame_of") and what in f), (what, inv)
        assert chk.has("expression_controls", lambda f: "over zero rows" in f) and chk.has("head_pose_controls", lambda f: "over zero rows" in f), inv
        assert sum(r["frames"] for r in chk.has("paste_windows")) == sum(seen), inv
    else:
        assert not chk.has("present_rows"), inv
        assert chk.has("paste_windows", lambda f: f.startswith("device windows frame_of") and "absent" in f), inv
        assert sum(r["frames"] for r in chk.has("paste_windows")) == 2 * N == sum(r["frames"] for r in chk.has("resize2d_windows")), inv
    _assert_window_spread([x for x in chk.windows if x[0] == "paste_windows"], even_sides_only=True)
    assert min(x[3] for x in chk.windows if x[0] == "paste_windows") >= 32


# ---- E: animate_streams over two frame sizes with boxes, paste_back ----------------------------------------------------------------------
def e_boxes():
    """the face boxes of two streams, 5 frames of 96 x 128 and 4 of 64 x 96 (one of them missing): wandering, sides 40 ... 60"""
    rng = np.random.default_rng(11)
    out = []
    for n, (H, W) in ((5, BIG), (4, SMALL)):
        c = np.stack([W / 2 + rng.integers(-9, 10, n), H / 2 + rng.integers(-4, 5, n)], 1).astype(np.float64)
        h = 12 + rng.integers(0, 7, (n, 2)) * 0.5
        out.append(np.concatenate([c - h, c + h], 1))
    out[1][2] = np.nan
    return out


def e_host_account(boxes):
    """hostglue.crop_track per stream (smooth, min_side S / 4) -> the paste windows of each stream"""
    out = []
    for b, (H, W) in zip(boxes, (BIG, SMALL)):
        st = np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((1, 4), np.int32)
        out.append(hostglue.crop_track(b, None, (W, H), *st, momentum=0.5, smooth=True, min_side=S // 4)[1])
    return out


def test_e_boxes_are_what_the_configuration_is_there_for():
    """no GPU: hostglue's account -- one absent row, every present window with a side of at least 32, odd and even origins"""
    pastes = np.concatenate(e_host_account(e_boxes()))
    present = pastes[:, 2] > 0
    assert present.tolist() == [True] * 7 + [False, True]
    wins = pastes[present]
    assert wins[:, 2].min() >= 32 and not (wins[:, 2] & 1).any()
    assert set((wins[:, 0] & 1).tolist()) == {0, 1} and set((wins[:, 1] & 1).tolist()) == {0, 1}
    assert len(set((wins[:, 0] % 4).tolist())) >= 3          # (NV12 rows of even width: x0 mod 4 is the residue; rgb8: 3 * x0 mod 4)


@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_e_streams_of_two_frame_sizes_with_boxes_every_launch(wrapper, monkeypatch, fmt):
    """two streams, 5 + 4 frames, the first one's frames in chunks of 2 + 3, host frames: every batch lives in an arena whose frames
    begin at 256-byte offsets, the tracker's windows are per-row device windows with per-row frame sizes, one row is absent"""
    w = wrapper
    boxes = e_boxes()
    want = e_host_account(boxes)
    clips = [_rgb_clip(5, BIG, 241), _rgb_clip(4, SMALL, 242)] if fmt == "rgb8" else [_yuv_clip(5, BIG, fmt, 241), _yuv_clip(4, SMALL, fmt, 242)]
    streams = [dict(frames=iter([clips[0][:2], clips[0][2:]]), boxes=torch.from_numpy(boxes[0]), identities=0),
               dict(frames=clips[1], boxes=torch.from_numpy(boxes[1]).to(DEV), identities=[1, 0, 1, 1])]
    fkw = {} if fmt == "rgb8" else dict(frame_format=fmt, colorspace="bt601", full_range=True)
    _fresh(w)
    chk, inv, out = _run(monkeypatch, f"E {fmt} streams boxes paste_back", lambda: _consume(w.animate_streams(
        streams, batch_size=BATCH, to_host=False, paste_back=True, paste_matte=_matte, tracking=dict(smooth=True, momentum=0.5),
        smooth_pose=True, mix=True, **fkw)), pastes=True)
    items = {(s, t): o.cpu() for batch in out for s, t, o in batch}
    assert sorted(items) == [(0, t) for t in range(5)] + [(1, t) for t in range(4)]
    assert all(_same(items[(s, t)], clips[s][t]) == (want[s][t][2] == 0) for s, t in items)
    tracked = chk.has("crop_track", lambda f: f.startswith("sizes per row smooth"))
    assert tracked and sum(r["frames"] for r in tracked) == 9, inv
    assert chk.has("crop_faces_mixed", lambda f: f.startswith(f"{fmt} device windows frame_of"), lambda s: s == tuple(sorted({BIG if fmt == "rgb8" else (144, 128), SMALL if fmt == "rgb8" else (96, 96)}))), inv
    assert chk.has("paste_faces_mixed", lambda f: "absent" in f) and chk.has("paste_faces_mixed", lambda f: "matte" in f), inv
    assert chk.has("theta_ema_scan", "plain K=2") and chk.has("mixing_theta", "indexed mix_old"), inv
    _assert_window_spread([x for x in chk.windows if x[0] == "paste_faces_mixed"], even_sides_only=True)
    assert min(x[3] for x in chk.windows if x[0] == "paste_faces_mixed") >= 32


# ---- F: what only forward, enrolment and animate launch -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.usefixtures("guarded_outputs")
def test_f_forward_enrolment_and_animate_every_launch(wrapper, tiny, monkeypatch):  # noqa: F811
    """forward with a source and a driver picture that are not S x S (resize2d, the source's inverse theta and its rotation warp,
    pack_rgb8) and a driver found by a face detector (the windowed resize2d); the seams of HipModel that add the lattice and sample a
    given grid; enrol_identities over both slots from uint8 frames with windows (mul_mask, the indexed repack) and load_identity (the
    repack back); animate with the head-pose and expression controls over a whole stream and a 10-bit output"""
    from test_identity_bank_gpu import _drivers
    w = wrapper
    g = torch.Generator().manual_seed(251)
    src, drv = torch.rand(3, 80, 72, generator=g), torch.rand(3, 96, 128, generator=g)
    c, d, s = (w.cfg[k] for k in ("latent_volume_channels", "latent_volume_depth", "latent_volume_size"))
    pose, srt = _drivers(tiny, 6)

    def calls():
        w.embedders["face_detector"] = lambda img: (0.2, 0.15, 0.5, 0.6)
        try:
            w.forward(source_image=src, driver_image=drv, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=tiny["idt_embed"])
            w.forward(driver_image=drv, crop=True)
        finally:
            del w.embedders["face_detector"]
        emb = w.hot_path.embed(w.pred_source_pose_embed.float().contiguous(), w.idt_embed.float().contiguous())
        warp, delta = w.model.xy_generator_nw({"orig": emb})
        w.model.grid_sample(torch.rand(1, c, d, s, s, generator=g).to(DEV), warp.contiguous())
        frames = _rgb_clip(2, BIG, 252)
        slots = w.enrol_identities(frames, source_masks=torch.ones(2, 1, S, S), slots=[1, 0], windows=[(3, 1, 90), (40, 16, 64)], batch_size=1,
                                   custome_idt_embed=torch.cat([tiny["idt_embed"]] * 2), custome_source_pose_embed=torch.cat([tiny["source_pose_embed"]] * 2),
                                   custome_source_theta_embed=tuple(torch.cat([t, t + 0.01]) for t in _drivers(tiny, 1)[1]))
        assert slots == [1, 0]
        w.load_identity(1)
        _fresh(w)
        n = sum(o.shape[0] for _, o in _consume(w.animate(pose, srt, batch_size=BATCH, identities=[0, 1, 1, 0, 1, 0], mix=True, smooth_pose=True,
                                                          smooth_per_identity=True, out_format="p010", head_pose=dict(relative=True, gain=0.7, zoom=1.1),
                                                          expression=dict(relative=True, smooth=True, gain=0.8))))
        assert n == 6
    chk, inv, _ = _run(monkeypatch, "F forward, enrolment, animate", calls)
    assert chk.has("resize2d", "bicubic -> (64, 64)") and chk.has("resize2d", "bicubic -> (64, 64) window clamp01"), inv
    assert chk.has("mat4_inverse") and chk.has("affine_grid3d") and chk.has("volume_to_channels_last") and chk.has("pack_rgb8"), inv
    assert chk.has("grid_sample3d", "theta ndhwc->ndhwc") and chk.has("grid_sample3d", "delta ndhwc->ncdhw") and chk.has("grid_sample3d", "grid ncdhw->ncdhw"), inv
    assert chk.has("add", f"period {3 * d * s * s}") and chk.has("mul_mask"), inv
    assert len(chk.has("volume_to_channels_last_indexed", "K=2")) == 2 and chk.has("volume_to_channels_first"), inv
    assert chk.has("resize2d_windows", "device windows") and chk.has("unpack_rgb8"), inv       # (enrolment uploads its checked windows itself)
    assert chk.has("head_pose_controls", "plain relative gain zoom") and chk.has("expression_controls", "plain relative smooth gain"), inv
    assert chk.has("theta_ema_scan", "plain K=2") and chk.has("pose_theta") and chk.has("pack_yuv420", "p010"), inv


# ---- the guard (no GPU) ------------------------------------------------------------------------------------------------------------
def unaccounted(called):
    """the names of `called` that are in none of the three places, and those in more than one"""
    places = (set(VIDEO_OPS), set(EXEMPT), set(HELD_ELSEWHERE))
    return sorted(n for n in called if not any(n in p for p in places)), sorted(n for n in called if sum(n in p for p in places) > 1)


def test_every_ops_call_of_the_video_path_is_checked_exempt_or_held_elsewhere():
    """a launch added to infer.py or frames.py later cannot go unchecked without someone deciding so"""
    called = ops_called(infer, frames_mod)
    assert {"crop_faces_mixed", "present_rows", "paste_windows"} <= called, called             # (the pattern still finds the calls)
    missing, twice = unaccounted(called)
    assert not missing, f"ops called by infer.py / frames.py that no launch checker wraps and nothing exempts: {missing}"
    assert not twice, f"names in more than one of VIDEO_OPS, EXEMPT, HELD_ELSEWHERE: {twice}"
    assert unaccounted(called | {"foo"})[0] == ["foo"]                                          # (a new call is found)
    for name in VIDEO_OPS:
        assert callable(getattr(VideoLaunchChecker, "_check_" + name, None)) and callable(getattr(ops, name)), name
        assert callable(getattr(V, "check_" + name, None)), name
    assert all(reason for reason in EXEMPT.values()) and all(callable(getattr(ops, name)) for name in EXEMPT)
    stale = sorted((set(EXEMPT) | set(HELD_ELSEWHERE)) - called)
    assert not stale, f"exempt or held elsewhere, but no longer called: {stale}"
    for reason in HELD_ELSEWHERE.values():                                                      # the named tests exist
        path, name = reason.split(" ")[0].split("::")
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)) as f:
            assert f"def {name}(" in f.read(), reason
