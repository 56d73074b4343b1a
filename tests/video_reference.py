"""TEST INFRASTRUCTURE ONLY -- one check_<op>(result, arguments ...) -> figures per operation the video path launches
(emoportraits_amd/infer.py and frames.py), in the shape tests/test_op_launches_fp64_gpu.OpLaunchChecker expects: 'worst',
'worst_frame', 'unit', 'frames', 'failures' (and 'batch' where the result does not carry its rows).

Every check is an adapter over a reference the suite has already -- ops_reference's fp64 checks, the restatements of
paste_back_reference / nv12_reference / yuv420_reference evaluated in fp64, faces_reference.sequential, and the host contracts of
emoportraits_amd/hostglue.py -- applied ROW BY ROW to the arguments a launch was really given: each face against its own frame and
its own window, each control row against the stream it walks.  No arithmetic is stated here that is not stated there, with two
exceptions that are written out where they stand: the crop of a YUV frame through a window that is no square (yuv_crop: yuv420_reference.crop's
expression with (w, h) in place of (s, s); the CPU test holds the two equal on squares) and the bound of the affine 3-D grid
(grid3d_frames: ops_reference.warp2d_frames' derivation with one more term).  Every bound is the constant of the operation's own
kernel test, imported.

Tensors may lie on any device; what the restatements need on the host is copied there.  In-place launches are checked from a copy
of their arguments taken before the launch (`before`) and the caller's own objects as the launch left them (`after`)."""
import numpy as np
import torch
import torch.nn.functional as F

import faces_reference as FR
import nv12_reference as NV
import ops_reference as R
import paste_back_reference as PB
import yuv420_reference as Y
from emoportraits_amd import hostglue

F64, F32 = torch.float64, torch.float32
C_TOL, D_TOL = NV.C_TOL, NV.D_TOL
MAX_BYTE_DIFF, MAX_SHARE = PB.MAX_BYTE_DIFF, PB.MAX_SHARE
MIX_ULPS = 1                        # test_pose_controls_emul.test_mixing_kernel_matches_hostglue_within_one_ulp: each element within 1 fp32 ulp

# ---- the operations ops_reference holds already: taken as they are ---------------------------------------------------------------
check_unpack_rgb8 = R.check_unpack_rgb8
check_pack_rgb8 = R.check_pack_rgb8
check_mul_mask = R.check_mul_mask
check_resize2d = R.check_resize2d
check_pose_theta = R.check_pose_theta
check_mat4_inverse = R.check_mat4_inverse
check_grid_sample3d = R.check_grid_sample3d
check_add = R.check_add
check_volume_to_channels_last = R.check_channels_last


# ---- what the adapters share -----------------------------------------------------------------------------------------------------
def windows_of(windows):
    """a host sequence, an int32 [M,4] tensor or an ops.DeviceWindows -> [(x0, y0, w, h)] of ints"""
    t = getattr(windows, "tensor", windows)
    if isinstance(t, torch.Tensor):
        return [tuple(int(v) for v in row) for row in t.detach().cpu().reshape(-1, 4).tolist()]
    return [tuple(int(v) for v in w) for w in windows]


def frames_of(frame_of, F_, M):
    """frame_of (a host sequence or None: row m is frame m) -> [M] ints"""
    return list(range(M)) if frame_of is None else [int(v) for v in frame_of]


def crop_window_ok(w, W, H):
    """a window a crop reads: it has two sides and lies inside its W x H frame (nv12_window_ok of csrc/resample.hip)"""
    return w[2] > 0 and w[3] > 0 and w[0] >= 0 and w[1] >= 0 and w[0] <= W - w[2] and w[1] <= H - w[3]


def paste_window_ok(w, S, W, H):
    """paste_window_ok of csrc/resample.hip: a square inside its frame, downscaling by at most 4 -- the rule by which a paste
    leaves a window out"""
    return w[2] == w[3] and hostglue.window_inside(w[0], w[1], w[2], W, H) and 4 * w[2] >= S


def _np(t):
    if t is None:
        return None
    t = getattr(t, "tensor", t)
    return t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _differing(got, want):
    """elements per row whose bits differ (a shape that differs: every element)"""
    got, want = _np(got), np.asarray(want)
    if got.shape != want.shape:
        return np.full((max(want.shape[0], 1) if want.ndim else 1,), max(want.size, 1), np.int64)
    if got.dtype != want.dtype:
        raise ValueError(f"result of {got.dtype}, the contract's of {want.dtype}")
    d = _bits(got) != _bits(want)
    return d.reshape(d.shape[0], -1).sum(1) if d.ndim else d.reshape(1).astype(np.int64)


def _rows_fig(per_row, unit, failures, batch=None, **more):
    """figures from one number per row of the launch (larger is worse)"""
    per_row = [float(v) for v in per_row]
    n = len(per_row)
    w = max(range(n), key=lambda i: per_row[i]) if n else None
    fig = dict(frames=list(range(n)), frame_fig=per_row, unit=unit, worst=per_row[w] if n else 0.0, worst_frame=w, failures=list(failures))
    if batch is not None:              # (only where the launch's result does not carry its rows)
        fig["batch"] = batch
    fig.update(more)
    return fig


def _merge(figs, labels, unit):
    """the figures of single-row checks (ops_reference checks called on one row each) as the figures of the launch"""
    failures = [f"{lab}: {f}" for fig, lab in zip(figs, labels) for f in fig["failures"]]
    held = [f for f in figs if f.get("max_ratio") is not None]         # (the rows held to the yardstick: not the zero rows)
    return _rows_fig([f["worst"] for f in figs], unit, failures, max_ratio=max((f["max_ratio"] for f in held), default=0.0),
                     mean_ratio=max((f["mean_ratio"] for f in held), default=0.0), yardstick="ATen fp32")


def _zeros_fig(row, what):
    """a row that must be zeros, exactly (an absent window, a frame outside the batch): held like a checked row, bound 0"""
    bad = int((row != 0).sum())                                          # (a NaN is not zero either)
    return dict(worst=float("inf") if bad else 0.0, failures=[f"{what}: {bad} elements of a row that must be zeros are not"] if bad else [])


def _state_failures(pairs):
    """[(name, what the launch left, what the contract leaves[, live])] -> the arrays that differ in a bit.  live: the rows whose
    flag the contract leaves set -- a stream's values are its state only under a set flag (has_state, has_anchor, has_ema, age >= 0):
    the contracts clear a stream by its flag and say nothing of the values under a cleared one, and the kernels' own tests
    (test_head_pose_controls_gpu, test_track_assign_gpu, test_skip_absent_gpu) hold 'the state under a set flag'.  The flags
    themselves are held everywhere."""
    out = []
    for name, got, want, *live in pairs:
        if want is None:
            continue
        d = _differing(got, want)
        d = int(d[np.asarray(live[0], bool)].sum() if live and d.shape[0] == len(live[0]) else d.sum())
        if d:
            out.append(f"state {name}: {d} elements differ from what the host contract leaves behind")
    return out


# ---- crops -----------------------------------------------------------------------------------------------------------------------
def check_resize2d_windows(out, x, size, windows, mode="bicubic", clamp01=False, frame_of=None):
    """row m against ops_reference.check_resize2d of ITS frame x[frame_of[m]] through ITS window; a row whose window has no side, or
    whose frame lies outside [0, F), is zeros"""
    wins = windows_of(windows)
    N, _, H, W = x.shape
    fof = frames_of(frame_of, N, len(wins))
    if out.shape[0] != len(wins) or len(fof) != len(wins):
        raise ValueError(f"{out.shape[0]} rows, {len(wins)} windows, {len(fof)} entries of frame_of")
    figs, labels = [], []
    for m, (w, f) in enumerate(zip(wins, fof)):
        labels.append(f"row {m} (frame {f}, window {w})")
        if not 0 <= f < N or w[2] <= 0 or w[3] <= 0:
            figs.append(_zeros_fig(out[m], "resize2d_windows"))
        elif not crop_window_ok(w, W, H):
            figs.append(dict(worst=float("inf"), failures=[f"the window leaves its {W}x{H} frame: the launch read outside it"]))
        else:
            figs.append(R.check_resize2d(out[m:m + 1], x[f:f + 1], size, mode, w, clamp01))
    return _merge(figs, labels, "x allowed max err")


def yuv_crop(codes, f, w, size, colorspace, full_range, bits, dt):
    """yuv420_reference.crop for one row, the window (x0, y0, w, h) of frame f resized to size = (Ho, Wo): the same expression
    (crop's `s` twice is (w, h), its `size` twice is (Ho, Wo))"""
    rgb = Y.decode(codes[f:f + 1], colorspace, full_range, bits, dt)
    x0, y0, ww, wh = w
    return F.interpolate(rgb[:, :, y0:y0 + wh, x0:x0 + ww], size=tuple(size), mode="bicubic", align_corners=False).clamp(0, 1)[0]


def _yuv_rows(out, codes_of_frame, sizes, size, wins, fof, fmt, colorspace, full_range, whole, what):
    """rows of a YUV crop: |out - fp64 restatement| <= C_TOL (D_TOL for a whole frame at its own size), nothing outside [0, 1],
    zeros for an absent row.  codes_of_frame(f) -> codes [1, 3H/2, W]; sizes[f] = (H, W)"""
    per_row, failures = [], []
    got = out.detach().cpu()
    for m, (w, f) in enumerate(zip(wins, fof)):
        lab = f"{what} row {m} (frame {f}, window {w})"
        if not 0 <= f < len(sizes) or not crop_window_ok(w, sizes[f][1], sizes[f][0]):
            z = _zeros_fig(got[m], lab)
            per_row.append(z["worst"])
            failures += z["failures"]
            continue
        ref = yuv_crop(codes_of_frame(f), 0, w, size, colorspace, full_range, Y.BITS[fmt], F64)
        tol = D_TOL if whole and tuple(size) == tuple(sizes[f]) else C_TOL
        err = torch.nan_to_num((got[m].double() - ref).abs(), nan=float("inf")).max().item()
        outside = int((~((got[m] >= 0) & (got[m] <= 1))).sum())
        per_row.append(err / tol)
        if err > tol:
            failures.append(f"{lab}: max abs err {err:.3e} > {tol:g}")
        if outside:
            failures.append(f"{lab}: {outside} outputs outside [0, 1]")
    return _rows_fig(per_row, "x tolerance (C_TOL; D_TOL for a whole frame at its size)", failures)


def check_yuv420_windows(out, frames, frame_format, size=None, windows=None, colorspace="bt709", full_range=False, frame_of=None):
    """yuv420_reference.from_layout + the crop restated in fp64, row by row; windows None: the whole frame of every row"""
    codes = Y.from_layout(frames.detach().cpu().numpy(), frame_format)[0]
    N, rows, W = codes.shape
    H = rows // 3 * 2
    whole = windows is None
    wins = [(0, 0, W, H)] * N if whole else windows_of(windows)
    fof = frames_of(frame_of, N, len(wins))
    size = (H, W) if size is None else tuple(size)
    if out.shape[0] != len(wins):
        raise ValueError(f"{out.shape[0]} rows for {len(wins)} windows")
    return _yuv_rows(out, lambda f: codes[f:f + 1], [(H, W)] * N, size, wins, fof, frame_format, colorspace, full_range, whole, "yuv420_windows")


def check_crop_faces_mixed(out, frames, size, windows, frame_of, frame_format="rgb8", colorspace="bt709", full_range=False):
    """every face against its OWN frame of the list: rgb8 -- the fp64 of byte / 255 through ops_reference.check_resize2d (bicubic,
    clamp01); a YUV layout -- check_yuv420_windows' rows"""
    wins, fof = windows_of(windows), [int(v) for v in frame_of]
    size = (size, size) if isinstance(size, int) else tuple(size)
    if out.shape[0] != len(wins) or len(fof) != len(wins):
        raise ValueError(f"{out.shape[0]} rows, {len(wins)} windows, {len(fof)} entries of frame_of")
    if frame_format != "rgb8":
        sizes = [(t.shape[0] // 3 * 2, t.shape[1]) for t in frames]
        return _yuv_rows(out, lambda f: Y.from_layout(frames[f][None].detach().cpu().numpy(), frame_format)[0], sizes, size, wins, fof,
                         frame_format, colorspace, full_range, False, "crop_faces_mixed")
    figs, labels = [], []
    for m, (w, f) in enumerate(zip(wins, fof)):
        labels.append(f"face {m} (frame {f}, window {w})")
        if not 0 <= f < len(frames) or not crop_window_ok(w, frames[f].shape[1], frames[f].shape[0]):
            figs.append(_zeros_fig(out[m], "crop_faces_mixed"))
        else:
            x = (frames[f].to(out.device).to(F64) / 255.0).permute(2, 0, 1)[None]
            figs.append(R.check_resize2d(out[m:m + 1], x, size, "bicubic", w, True))
    return _merge(figs, labels, "x allowed max err")


# ---- packing ---------------------------------------------------------------------------------------------------------------------
def check_pack_yuv420(out, img, frame_format, colorspace="bt709", full_range=False):
    """yuv420_reference.encode in fp64 and compare_codes, frame by frame: every code within MAX_BYTE_DIFF, at most MAX_SHARE of a
    frame's samples different where torch's fp32 evaluation of the restatement stays under that share itself (the premise of the
    kernel's own test), and zeros in the format's unused bits"""
    codes, ignored = Y.from_layout(out.detach().cpu().numpy(), frame_format)
    img = img.detach().cpu()
    bits = Y.BITS[frame_format]
    ref64, ref32 = Y.encode(img.double(), colorspace, full_range, bits, F64), Y.encode(img, colorspace, full_range, bits, F32)
    per_row, failures = [], []
    for n in range(img.shape[0]):
        worst, share, share32 = Y.compare_codes(codes[n], ref64[n], ref32[n], codes[n].numel())
        per_row.append(worst)
        if worst > MAX_BYTE_DIFF:
            failures.append(f"pack_yuv420 frame {n}: a code {worst} from the fp64 restatement's (> {MAX_BYTE_DIFF})")
        if share32 > MAX_SHARE:
            failures.append(f"pack_yuv420 frame {n}: the premise fails, torch's fp32 restatement differs in {share32:.2e} of the samples")
        if share > MAX_SHARE:
            failures.append(f"pack_yuv420 frame {n}: {share:.2e} of the samples differ (> {MAX_SHARE})")
        if bool(ignored[n].any()):
            failures.append(f"pack_yuv420 frame {n}: {int((ignored[n] != 0).sum())} samples with bits set outside their code")
    return _rows_fig(per_row, "codes from the fp64 restatement", failures)


# ---- pastes ----------------------------------------------------------------------------------------------------------------------
def _check_paste(what, before, after, img, matte, wins, fof, S, sizes, paste_one, touched_of, rect_of, ignored=None):
    """The pastes' shared body, frame by frame.  before / after: per frame a [1, ...] integer tensor of bytes or codes (ignored:
    per frame (before, after) of the bits outside the codes); wins[m] goes into frame fof[m] of size sizes[f] = (H, W);
    paste_one(dt) -> faces_reference.sequential's paste_one evaluated in dt; touched_of(f, windows (x0, y0, s) of the frame) ->
    bool mask like the frame; rect_of(frame, window) -> the samples of one window, for the row's own figure.
    -> figures: per row the largest difference to the fp64 restatement inside the row's window (<= MAX_BYTE_DIFF), every sample
    outside the touched mask as it was, 'extra' = (differing touched samples, the same for the fp32 evaluation, touched samples,
    touched samples the launch changed: a paste that leaves its windows as they were is no paste)."""
    img, matte = img.detach().cpu(), None if matte is None else matte.detach().cpu()
    M = len(wins)
    if img.shape[0] != M or len(fof) != M:
        raise ValueError(f"{img.shape[0]} images, {M} windows, {len(fof)} entries of frame_of")
    valid = [0 <= f < len(sizes) and paste_window_ok(w, S, sizes[f][1], sizes[f][0]) for w, f in zip(wins, fof)]
    per_row, failures, counts = [0.0] * M, [], [0, 0, 0, 0]
    if any(fof[m] > fof[m + 1] for m in range(M - 1)):
        failures.append(f"{what}: frame_of is not non-decreasing")
    for f in range(len(sizes)):
        rows = [m for m in range(M) if fof[m] == f]
        skip = [j for j, m in enumerate(rows) if not valid[m]]
        w3 = [wins[m][:3] for m in rows]
        refs = []
        for dt in (F64, F32):
            refs.append(FR.sequential(paste_one(dt), before[f], img[rows], None if matte is None else matte[rows], w3, [0] * len(rows), skip)
                        if rows else before[f].clone())
        ref64, ref32 = refs
        touched = touched_of(f, [w for j, w in enumerate(w3) if j not in skip])
        diff = (after[f].int() - ref64.int()).abs()
        if not torch.equal(after[f][~touched], before[f][~touched]):
            failures.append(f"{what}: frame {f}: {int((after[f][~touched] != before[f][~touched]).sum())} samples outside the touched mask changed")
        counts[0] += int(diff[touched].ne(0).sum())
        counts[1] += int((ref32.int() - ref64.int())[touched].ne(0).sum())
        counts[2] += int(touched.sum())
        counts[3] += int((after[f] != before[f])[touched].sum())
        for j, m in enumerate(rows):
            if valid[m]:
                per_row[m] = float(rect_of(diff, w3[j]).max())
                if per_row[m] > MAX_BYTE_DIFF:
                    failures.append(f"{what}: face {m} (frame {f}, window {wins[m]}): a sample {int(per_row[m])} from the fp64 restatement's "
                                    f"(> {MAX_BYTE_DIFF})")
        if ignored is not None:
            ib, ia = ignored[f]
            if not torch.equal(ia[~touched], ib[~touched]):
                failures.append(f"{what}: frame {f}: the ignored bits of {int((ia[~touched] != ib[~touched]).sum())} untouched samples changed")
            if bool(ia[touched].any()):
                failures.append(f"{what}: frame {f}: {int((ia[touched] != 0).sum())} touched samples with bits set outside their code")
    return _rows_fig(per_row, "bytes / codes from the fp64 restatement", failures, batch=M, extra=tuple(counts))


def _rgb_paste(what, before, after, img, wins, fof, feather, matte):
    sizes = [(t.shape[1], t.shape[2]) for t in before]
    S = img.shape[-1]

    def touched_of(f, w3):
        mask = torch.zeros(before[f].shape, dtype=torch.bool)
        for x0, y0, s in w3:
            mask[0, y0:y0 + s, x0:x0 + s] = True
        return mask
    paste_one = lambda dt: (lambda fr, im, ma, w: PB.paste(fr, im, [w], feather, ma, dt))
    return _check_paste(what, before, after, img, matte, wins, fof, S, sizes, paste_one, touched_of,
                        lambda d, w: d[0, w[1]:w[1] + w[2], w[0]:w[0] + w[2]])


def _yuv_paste(what, before, after, img, wins, fof, feather, matte, fmt, colorspace, full_range):
    cb, ca = ([Y.from_layout(t.detach().cpu().numpy(), fmt) for t in side] for side in (before, after))
    sizes = [(c[0].shape[1] // 3 * 2, c[0].shape[2]) for c in cb]
    bits = Y.BITS[fmt]
    paste_one = lambda dt: (lambda fr, im, ma, w: Y.paste(fr, im, [w], feather, ma, colorspace, full_range, bits, dt))
    touched_of = lambda f, w3: Y.touched_mask(tuple(cb[f][0].shape), w3, [0] * len(w3))

    def rect_of(d, w):
        h = d.shape[1] // 3 * 2
        cx0, cy0, cx1, cy1 = NV.chroma_rect(*w)
        return torch.cat([d[0, w[1]:w[1] + w[2], w[0]:w[0] + w[2]].reshape(-1), d[0, h + cy0:h + cy1, 2 * cx0:2 * cx1].reshape(-1)])
    return _check_paste(what, [c[0] for c in cb], [c[0] for c in ca], img, matte, wins, fof, img.shape[-1], sizes, paste_one, touched_of, rect_of,
                        ignored=[(b[1], a[1]) for b, a in zip(cb, ca)] if fmt in Y.IGNORED else None)


def check_paste_windows(after, before, img, windows, feather=0.0, matte=None, frame_of=None):
    """paste_back_reference.paste in fp64, face after face in list order (faces_reference.sequential), on the frames as they were
    before the launch; a window that fails paste_window_ok is left out"""
    before, after = before.detach().cpu(), after.detach().cpu()
    wins = windows_of(windows)
    fof = frames_of(frame_of, before.shape[0], len(wins))
    split = lambda t: [t[f:f + 1] for f in range(t.shape[0])]
    return _rgb_paste("paste_windows", split(before), split(after), img, wins, fof, feather, matte)


def check_paste_windows_yuv420(after, before, frame_format, img, windows, feather=0.0, matte=None, colorspace="bt709", full_range=False,
                               frame_of=None):
    """yuv420_reference.paste in fp64 on the codes of the frames as they were, face after face; the 10-bit layouts' ignored bits
    stay where no window touches and are zero where one does"""
    wins = windows_of(windows)
    fof = frames_of(frame_of, before.shape[0], len(wins))
    split = lambda t: [t[f:f + 1] for f in range(t.shape[0])]
    return _yuv_paste("paste_windows_yuv420", split(before), split(after), img, wins, fof, feather, matte, frame_format, colorspace, full_range)


def check_paste_faces_mixed(after, before, img, windows, frame_of, feather=0.0, matte=None, frame_format="rgb8", colorspace="bt709",
                            full_range=False):
    """the two checks above on a list of frames of different sizes: every face into its OWN frame"""
    wins, fof = windows_of(windows), [int(v) for v in frame_of]
    one = lambda side: [t[None].detach().cpu() for t in side]
    if frame_format == "rgb8":
        return _rgb_paste("paste_faces_mixed", one(before), one(after), img, wins, fof, feather, matte)
    return _yuv_paste("paste_faces_mixed", one(before), one(after), img, wins, fof, feather, matte, frame_format, colorspace, full_range)


# ---- the pose and expression controls ----------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = (np.ascontiguousarray(t, dtype=np.float32).view(np.int32).astype(np.int64) for t in (a, b))
    a, b = np.where(a < 0, -(a & 0x7FFFFFFF), a), np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def check_mixing_theta(out, target, source_bank, index=None, mix_old=True):
    """row n within MIX_ULPS fp32 ulp of hostglue.mixing_theta(source_bank[index[n]], target[n]) rounded to fp32, row 3 exactly
    (0, 0, 0, 1); the fallbacks exactly: an index outside the bank, or a source whose linear part is not finite, hands the target on"""
    got, tgt, bank = _np(out), _np(target), _np(source_bank)
    idx = np.zeros(tgt.shape[0], np.int64) if index is None else _np(index)
    per_row, failures = [], []
    for n in range(tgt.shape[0]):
        k = int(idx[n])
        if not 0 <= k < bank.shape[0]:
            d = int((_bits(got[n]) != _bits(tgt[n])).sum())
            per_row.append(float("inf") if d else 0.0)
            failures += [f"mixing_theta row {n}: index {k} lies outside the bank and the target did not pass through ({d} elements)"] if d else []
            continue
        want = np.zeros((4, 4), np.float32)
        want[:3] = hostglue.mixing_theta(bank[k][None], tgt[n][None], mix_old)[0]
        want[3, 3] = 1
        exact = not np.isfinite(bank[k][:3, :3]).all()
        u = _ulps(got[n], want)
        u = np.where(np.isnan(got[n]) != np.isnan(want), 1 << 31, u)
        lim = 0 if exact else MIX_ULPS
        per_row.append(float(u.max()))
        if u.max() > lim or _ulps(got[n][3], want[3]).max() > 0:
            failures.append(f"mixing_theta row {n} (source {k}): {int(u.max())} ulp from hostglue's (allowed {lim}; row 3 exact)")
    return _rows_fig(per_row, "fp32 ulp", failures)


def _bitwise_rows(what, got, want, inside=None):
    """rows held bit for bit; a row the contract leaves unwritten (stream outside [0, K): NaN there) must still be NaN"""
    got, want = _np(got), np.asarray(want)
    if got.shape != want.shape:
        raise ValueError(f"{what}: result {got.shape} vs the contract's {want.shape}")
    per_row, failures = [], []
    for i in range(want.shape[0]):
        if inside is not None and not inside[i]:
            d = int((~np.isnan(got[i])).sum())
            msg = f"{what} row {i}: its stream lies outside the bank and {d} elements were written"
        else:
            d = int((_bits(got[i]) != _bits(want[i])).sum())
            msg = f"{what} row {i}: {d} elements differ from the host contract's bits"
        per_row.append(d)
        if d:
            failures.append(msg)
    return per_row, failures


def _inside(stream_of, n, K):
    so = _np(stream_of)
    return np.ones(n, bool) if so is None else (so >= 0) & (so < K)


def check_theta_ema_scan(out, values, stream_of, state, has_state, momentum, restart=None, present=None, after=None):
    """hostglue.ema_scan_tracks on copies of the state from before the launch: the smoothed rows and the state left behind, bit
    for bit.  after = dict(state=, has_state=): the caller's arrays as the launch left them"""
    st, has = _np(state), _np(has_state)
    want = hostglue.ema_scan_tracks(_np(values), _np(stream_of), st, has, momentum, _np(restart), _np(present))
    per_row, failures = _bitwise_rows("theta_ema_scan", out, want, _inside(stream_of, want.shape[0], st.shape[0]))
    failures += _state_failures([("state", after["state"], st, has != 0), ("has_state", after["has_state"], has)])
    return _rows_fig(per_row, "differing elements", failures)


def _per_row_values(v, n, width=None):
    """a scalar or [n] -> [n]; width: a [width] or [n, width] tensor -> [n, width] (what the ops wrapper broadcasts)"""
    if v is None:
        return None
    if width is None:
        return _np(v).astype(np.float32) if isinstance(v, torch.Tensor) and v.dim() == 1 else np.full(n, float(v), np.float32)
    a = _np(v).astype(np.float32)
    return np.tile(a, (n, 1)) if a.ndim == 1 else a


def check_expression_controls(out, values, stream_of=None, neutral=None, gain=None, offset=None, anchor=None, has_anchor=None, ema=None,
                              has_ema=None, relative=False, momentum=None, restart=None, present=None, after=None):
    """hostglue.expression_controls on copies of the streams' state from before the launch: rows and state bit for bit.  The
    state a control that is off does not see is handed to neither (ops.expression_controls passes no pointer for it)"""
    v = _np(values)
    n, E = v.shape
    smooth = momentum is not None
    an, han = (_np(anchor), _np(has_anchor)) if relative else (None, None)
    em, hem = (_np(ema), _np(has_ema)) if smooth else (None, None)
    want = hostglue.expression_controls(v, _np(stream_of), _np(neutral), _per_row_values(gain, n), _per_row_values(offset, n, E), an, han, em, hem,
                                        relative, momentum, _np(restart), _np(present))
    K = next((a.shape[0] for a in (_np(neutral), an, em) if a is not None), 1)
    per_row, failures = _bitwise_rows("expression_controls", out, want, _inside(stream_of, n, K))
    after = after or {}
    left = lambda name, on: _np(after.get(name)) if on and after.get(name) is not None else None
    failures += _state_failures([("anchor", left("anchor", relative), an, han), ("has_anchor", left("has_anchor", relative), han),
                                 ("ema", left("ema", smooth), em, hem), ("has_ema", left("has_ema", smooth), hem)])
    for name, on in (("anchor", relative), ("has_anchor", relative), ("ema", smooth), ("has_ema", smooth)):
        # a state array of a control that is off is not the launch's to write
        before = dict(anchor=anchor, has_anchor=has_anchor, ema=ema, has_ema=has_ema)[name]
        if not on and before is not None and after.get(name) is not None:
            failures += _state_failures([(f"{name} (its control is off)", after[name], _np(before))])
    return _rows_fig(per_row, "differing elements", failures)


def check_head_pose_controls(result, scale, rotation, translation, stream_of=None, source=None, gain=None, rotation_offset=None,
                             translation_offset=None, zoom=None, anchor=None, has_anchor=None, relative=False, frontal=False, restart=None,
                             present=None, after=None):
    """hostglue.head_pose_controls on copies of the anchors from before the launch: the edited rows and the state bit for bit; the
    returned theta through ops_reference.check_pose_theta of the edited rows (the device's sinf / cosf: a yardstick, not bits)"""
    srt, theta = result
    n = scale.shape[0]
    an, han = (_np(anchor), _np(has_anchor)) if relative else (None, None)
    with np.errstate(all="ignore"):      # (rows left out arrive as zeros: 0 / 0 under `relative`, in the contract as in the kernel)
        want, _ = hostglue.head_pose_controls(_np(scale), _np(rotation), _np(translation), _np(stream_of), _np(source), _per_row_values(gain, n),
                                              _per_row_values(rotation_offset, n, 3), _per_row_values(translation_offset, n, 3),
                                              _per_row_values(zoom, n), an, han, relative, frontal, None, _np(restart), _np(present))
    K = next((a.shape[0] for a in (_np(source), an) if a is not None), 1)
    inside = _inside(stream_of, n, K)
    per_row, failures = _bitwise_rows("head_pose_controls", srt, want, inside)
    after = after or {}
    if relative:
        failures += _state_failures([("anchor", after.get("anchor"), an, han), ("has_anchor", after.get("has_anchor"), han)])
    elif anchor is not None and after.get("anchor") is not None:
        failures += _state_failures([("anchor (relative is off)", after["anchor"], _np(anchor)),
                                     ("has_anchor (relative is off)", after["has_anchor"], _np(has_anchor))])
    # (a row whose edit is not finite -- zeros scattered where a row was left out divide 0 by 0 under `relative` -- has no theta to hold)
    finite = np.isfinite(_np(srt)).all(1)
    rows = [i for i in range(n) if inside[i] and finite[i]]
    fig = R.check_pose_theta(theta, srt[:, 0:3].contiguous(), srt[:, 3:6].contiguous(), srt[:, 6:9].contiguous(), frames=rows) if rows else None
    unwritten = int((~torch.isnan(theta.detach().cpu()[torch.from_numpy(~inside)])).sum()) if not inside.all() else 0
    if unwritten:
        failures.append(f"head_pose_controls: {unwritten} theta elements of rows outside the bank were written")
    out = _rows_fig(per_row, "differing elements of the edited rows", failures + (fig["failures"] if fig else []))
    out.update(theta_worst=fig["worst"] if fig else 0.0, max_ratio=fig["max_ratio"] if fig else 0.0,
               mean_ratio=fig["mean_ratio"] if fig else 0.0, yardstick="torch fp32")
    return out


# ---- the trackers ----------------------------------------------------------------------------------------------------------------
def check_crop_track(result, boxes, stream_of=None, size=None, state=None, has_state=None, last=None, momentum=0.01, smooth=False,
                     fixed=False, scale=1.0, box_format="xyxy", missing="skip", min_side=2, K=None, restart=None, after=None):
    """hostglue.crop_track on copies of the tracker's state: the crop and paste windows, face_scale and every state array bit for bit"""
    st, has, la = _np(state), _np(has_state), _np(last)
    want = hostglue.crop_track(_np(boxes).astype(np.float64), _np(stream_of), _np(size), st if smooth else None, has if smooth else None, la,
                               momentum, smooth, fixed, scale, box_format, missing, min_side, K, restart=_np(restart))
    names = ("crop", "paste", "face_scale")
    per = [_differing(g, w) for g, w in zip(result, want)]
    per_row = sum(per)
    failures = [f"crop_track row {i}: {', '.join(nm for nm, p in zip(names, per) if p[i])} differ from hostglue.crop_track "
                f"(got {[_np(g)[i].tolist() for g in result[:2]]}, want {[w[i].tolist() for w in want[:2]]})" for i in np.nonzero(per_row)[0]]
    after = after or {}
    failures += _state_failures([("state", after.get("state"), st if state is not None else None, has if has is not None else np.ones(0 if st is None else len(st))),
                                 ("has_state", after.get("has_state"), has), ("last", after.get("last"), la)])
    return _rows_fig(per_row, "differing outputs of the row", failures)


def check_track_assign(result, dets, stream_of=None, ref=None, age=None, min_iou=0.3, max_missed=15, box_format="xyxy", after=None):
    """hostglue.track_assign on copies of the tracks: boxes (NaN rows included), restart, track_of, ref and age bit for bit"""
    r, a = _np(ref), _np(age)
    want = hostglue.track_assign(_np(dets).astype(np.float64), _np(stream_of), r, a, min_iou, max_missed, box_format)
    names = ("boxes", "restart", "track_of")
    per = [_differing(g, w) for g, w in zip(result, want)]
    per_row = sum(per)
    failures = [f"track_assign frame {i}: {', '.join(nm for nm, p in zip(names, per) if p[i])} differ from hostglue.track_assign"
                for i in np.nonzero(per_row)[0]]
    after = after or {}
    live = a >= 0
    failures += _state_failures([("ref", np.where(live[..., None], _np(after.get("ref")), 0), np.where(live[..., None], r, 0)),
                                 ("age", after.get("age"), a)])
    return _rows_fig(per_row, "differing outputs of the frame", failures)


def check_present_rows(result, crop, paste, F_, P):
    """hostglue.present_rows: count, first, row_of and the compacted windows, every element"""
    want = hostglue.present_rows(_np(crop), _np(paste), F_, P)
    names = ("count", "first", "row_of", "crop_out", "paste_out")
    failures = []
    for nm, g, w in zip(names, result, want):
        d = int(_differing(g, w).sum())
        if d:
            failures.append(f"present_rows {nm}: {d} elements differ from hostglue.present_rows (got {_np(g).tolist()}, want {w.tolist()})")
    return _rows_fig(_differing(result[0], want[0]), "differing counts of the frame", failures)


# ---- the volumes' ends ---------------------------------------------------------------------------------------------------------
def grid3d_frames(theta, size):
    """yields (n, fp64 grid [D, H, W, 3] = ops_reference.theta_grid_fp64, fp64 bound without TINY).  affine_row of csrc/gs3d_coord.h
    computes, per coordinate j, p^ = fl(x t[j][0]), q^ = fl(fma(y, t[j][1], p^)), r^ = fl(fma(z, t[j][2], q^)) and g^ =
    fl(fma(1, t[j][3], r^)): four roundings, one more than ops_reference.warp2d_frames' three, and its derivation goes on one
    step: on the exact intermediates p, q, r, g the error is at most u (1 + u)^3 (|p| + |q| + |r| + |g|)."""
    for n in range(theta.shape[0]):
        pts = R._lattice_points(tuple(size), theta.device, F64)
        t = theta[n][:3].to(F64)
        p = pts[..., 0:1] * t[:, 0]
        q = pts[..., 1:2] * t[:, 1] + p
        r = pts[..., 2:3] * t[:, 2] + q
        g = t[:, 3] + r
        yield n, g, R.U * (1.0 + R.U) ** 3 * (p.abs() + q.abs() + r.abs() + g.abs())


def check_affine_grid3d(out, theta, size):
    """every coordinate against the fp64 product of the fp32 lattice and theta, under grid3d_frames' bound + TINY"""
    rows = []
    for n, g, bound in grid3d_frames(theta, size):
        ref = R.theta_grid_fp64(theta[n], tuple(size))
        assert (g - ref).abs().max() <= 1e-12 * (1 + ref.abs().max())           # (the bound's own product is that grid)
        rows.append(R._bounded_row(out[n], ref, bound + R.TINY))
    return R._bounded_fig(rows, list(range(theta.shape[0])), "affine_grid3d")


def check_volume_to_channels_first(out, vol):
    """[N,D,H,W,C] -> [N,C,D,H,W]: the permutation check_channels_last holds, read the other way round"""
    return R.check_channels_last(vol, out)


def check_volume_to_channels_last_indexed(after, vol, before, row):
    """bank[row[n]] is the channels-last form of vol[n] bit for bit (ops_reference.check_channels_last); every other row of the
    bank, and everything where row[n] lies outside it, is as it was"""
    rows = [int(v) for v in _np(row)]
    K = before.shape[0]
    valid = [n for n, k in enumerate(rows) if 0 <= k < K]
    per_row, failures = [0.0] * len(rows), []
    if valid:
        fig = R.check_channels_last(after[[rows[n] for n in valid]], vol[valid])
        for n, v in zip(valid, fig["frame_fig"]):
            per_row[n] = v
        failures += [f"volume_to_channels_last_indexed: {f}" for f in fig["failures"]]
    others = [k for k in range(K) if k not in set(rows)]
    if others:
        d = int((after[others].contiguous().view(torch.int32) != before[others].contiguous().view(torch.int32)).sum())
        if d:
            failures.append(f"volume_to_channels_last_indexed: {d} elements of bank rows no `row` names changed")
    return _rows_fig(per_row, "differing elements", failures)


def check_grid_sample3d_grid(out, vol, grid, padding_mode="zeros"):
    """the grid= form ('ncdhw' -> 'ncdhw'), which ops_reference.grid_sample3d_frames does not serve: its construction on a given
    grid -- F.grid_sample in fp64 on the fp32 grid against ATen's fp32 CPU kernel on the same inputs, with the sampler's margins"""
    N = grid.shape[0]
    rows = []
    for n in range(N):
        v = vol[n if vol.shape[0] > 1 else 0]
        ref = F.grid_sample(v.to(F64)[None], grid[n].to(F64)[None], mode="bilinear", padding_mode=padding_mode, align_corners=False)[0]
        yard = F.grid_sample(v.float().cpu()[None], grid[n].float().cpu()[None], mode="bilinear", padding_mode=padding_mode, align_corners=False)[0]
        rows.append(R._yardstick_row(out[n], ref, yard, n))
    return R._yardstick_fig(rows, list(range(N)), "grid_sample3d grid=")
