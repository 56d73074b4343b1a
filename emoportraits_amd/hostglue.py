"""Host-side scalar logic of the wrapper around the hot path: face-box -> square crop window with
its tracking state, and the source/driver pose mixing.  In the reference these are numpy / scipy code on the host as well
(notebooks/infer.py); here they are kept apart from the kernels so that they can be pinned on CPU against outputs of the
reference's own methods (tests/golden/hostglue.pt, oracle/make_golden.py).
"""
import numpy as np


def detection_to_face(rel_xmin, rel_ymin, rel_width, rel_height, img_w, img_h):
    """mediapipe relative bounding box -> the pixel box the reference crops around (notebooks/infer.py:385-391, :529-536):
    the top edge is pulled up (ymin * 0.9), the bottom edge pushed down (height * 1.2) and clamped to the image"""
    return np.array([img_w * rel_xmin,
                     img_h * rel_ymin * 0.9,
                     img_w * (rel_xmin + rel_width),
                     min(img_h * (rel_ymin + rel_height * 1.2), img_h - 1)])


def remove_overflow(center, size, w, h):
    """notebooks/infer.py:243-261: shrink a square window symmetrically until it fits the w x h image; returns the new
    (even) side length"""
    half = size / 2
    box = np.asarray([center[0] - half, center[1] - half, center[0] + half, center[1] + half], dtype=np.float64)
    over = max(0.0 if box[0] >= 0 else -box[0], 0.0 if box[1] >= 0 else -box[1],
               0.0 if box[2] <= w else box[2] - w, 0.0 if box[3] <= h else box[3] - h)
    box[:2] += over
    box[2:] -= over
    side = int((box[2] - box[0] + box[3] - box[1]) / 2)
    return side - side % 2


class CropTracker:
    """state of `use_smoothed_crop` (notebooks/infer.py:317-327): exponential moving average of the box centre and size
    over the frame sequence; `fixed_bounding_box` freezes the first one"""

    def __init__(self, momentum=0.01, fixed_bounding_box=False):
        self.momentum, self.fixed = momentum, fixed_bounding_box
        self.center = self.size = None

    def reset(self):
        self.center = self.size = None

    def update(self, center, size):
        if self.center is None:
            self.center, self.size = center, size
        elif not self.fixed:
            self.center = center * self.momentum + self.center * (1 - self.momentum)
            self.size = size * self.momentum + self.size * (1 - self.momentum)
        return self.center, self.size


def crop_window(face, img_w, img_h, tracker=None, scale=1):
    """notebooks/infer.py:301-352 (crop_image), the per-frame arithmetic: face box (x0, y0, x1, y1) -> (x_lo, y_lo, side,
    face_scale) of the square that is then resized to image_size.  Returns None for a missing face."""
    if face is None:
        return None
    center = np.asarray([(face[2] + face[0]) // 2, (face[3] + face[1]) // 2])
    size = (face[2] - face[0] + face[3] - face[1]) * scale
    if tracker is not None:
        center, size = tracker.update(center, size)
    center = center.round().astype(int)
    size = int(round(size))
    size -= size % 2
    side = remove_overflow(center, size, img_w, img_h)
    return int(center[0] - side // 2), int(center[1] - side // 2), side, side / size


CROP_BOX_FORMATS = {"xyxy": 0, "relative": 1}
CROP_MISSING = {"skip": 0, "hold": 1}
_CROP_RANGE = float(1 << 30)


def window_inside(x_lo, y_lo, side, img_w, img_h, min_side=1):
    """the integer test of a square window against its frame: the predicate of ops.windows_host (and of nv12_window_ok in
    csrc/resample.hip), and a side of at least min_side"""
    return side > 0 and x_lo >= 0 and y_lo >= 0 and x_lo <= img_w - side and y_lo <= img_h - side and side >= min_side


def crop_track(boxes, stream_of, size, state, has, last, momentum=0.01, smooth=False, fixed=False, scale=1.0, box_format="xyxy",
               missing="skip", min_side=2, K=None, why=None, restart=None):
    """Face boxes -> crop and paste windows for a whole batch of rows, one row after another: crop_window with a CropTracker per
    stream (notebooks/infer.py:301-352, crop_image's arithmetic), plus what a batch needs that one frame did not -- a row whose
    face is missing or whose window does not fit still gets a window that can be read, and says so.  The contract that
    emo_crop_track_f64 (ops.crop_track) is held to bit for bit.  Everything is float64 until a value has passed its range test.
    boxes [M,4] float64, row order = frame order; stream_of [M] ints or None (every row: stream 0); size = (W, H) of every
    row's frame, or [M,2]; state [K,3] float64 = (cx, cy, size), has [K] int32 and last [K,4] int32 (the stream's last present
    window, side 0 = none) are the streams' state, UPDATED IN PLACE (state and has may be None without `smooth`; last may be
    None without missing='hold', and is then not kept; K: the number of streams where no state says it, default 1); momentum in
    (0, 1], with om = 1 - momentum formed in float64.
    box_format 'xyxy': the pixel box (x0, y0, x1, y1); 'relative': mediapipe's (xmin, ymin, width, height), through
    detection_to_face's arithmetic in its order of operations.  -> (crop [M,4] int32, paste [M,4] int32, face_scale [M] float64).
    Row i of stream k in a W x H frame:
        missing: a component of the box (after the format conversion) is not finite or has magnitude >= 2^30, or k is outside
            [0, K).  A missing row does not touch the tracker (the reference: `face is None` -> face_check = False); a k outside
            [0, K) touches no state at all.
        cx = floor((x1 + x0) / 2), cy = floor((y1 + y0) / 2), size = (((x1 - x0) + y1) - y0) * scale
        smooth: a stream without state takes (cx, cy, size) as its state; otherwise, unless `fixed`, state = v * m + state * om,
            each product and the sum rounded on its own; the row goes on with the state.
        cx, cy, size = rint of each (half to even); size -= size % 2; absent unless size is finite and >= 2
        side = remove_overflow((cx, cy), size, W, H) before its last line, truncated towards zero; side -= side % 2; absent
            unless side >= 2; absent unless |cx|, |cy| and side are below 2^30 -- only now do they become integers
        x_lo = cx - side / 2, y_lo = cy - side / 2
        present: window_inside(x_lo, y_lo, side, W, H, min_side).  Then crop = paste = (x_lo, y_lo, side, side), last[k] is that
            window and face_scale = side / size.
        missing or absent: face_scale = 0, and with missing='hold', if last[k] has a side and is window_inside this row's frame
            with min_side, crop = paste = last[k]; otherwise crop is the centred square of side min(W, H) at ((W - side) // 2,
            (H - side) // 2), which can always be read, and paste = (0, 0, 0, 0), which every paste kernel skips.
    why: a list that receives, per row, 'present' or what made the row missing ('stream', 'box') or absent ('size', 'side',
    'min_side'; 'guard' = the range test of the centre and the side or the inside test, which no finite box below 2^30 in a frame
    below 2^30 reaches: they are made so that no value is trusted).
    restart [M] ints or None (emo_crop_track_restarts_f64; track_assign's, flattened to the rows): a row i of a stream in [0, K)
    with restart[i] != 0 first clears its stream -- has[k] = 0 under `smooth`, last[k] = 0 where last is given -- and is then
    processed as above: a birth starts the EMA at its own box, a track that died is no longer held."""
    b = np.ascontiguousarray(boxes, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes must be [M,4], got {b.shape}")
    if box_format not in CROP_BOX_FORMATS:
        raise ValueError(f"box_format {box_format!r}: 'xyxy' or 'relative'")
    if missing not in CROP_MISSING:
        raise ValueError(f"missing {missing!r}: 'skip' or 'hold'")
    m = float(momentum)
    if not 0.0 < m <= 1.0:
        raise ValueError(f"crop momentum {momentum} is not in (0, 1]")
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError(f"crop scale {scale} is not finite")
    if smooth and (state is None or has is None):
        raise ValueError("smoothing needs state and has")
    hold = missing == "hold"
    if hold and last is None:
        raise ValueError("missing='hold' needs last")
    if int(min_side) < 1:
        raise ValueError(f"min_side {min_side} is below 1")
    M = b.shape[0]
    K = next((a.shape[0] for a in (state, has, last) if a is not None), 1 if K is None else K)
    sizes = np.asarray(size, dtype=np.int64)
    sizes = np.broadcast_to(sizes, (M, 2)) if sizes.ndim == 1 else sizes
    if sizes.shape != (M, 2) or (sizes < 1).any():
        raise ValueError("size: the (W, H) of every frame, or one per row, all positive")
    om = 1.0 - m
    crop, paste, face_scale = np.zeros((M, 4), np.int32), np.zeros((M, 4), np.int32), np.zeros(M, np.float64)
    with np.errstate(all="ignore"):                      # (inf and nan boxes are inputs here, not accidents)
        for i in range(M):
            W, H = int(sizes[i, 0]), int(sizes[i, 1])
            k = 0 if stream_of is None else int(stream_of[i])
            in_range = 0 <= k < K
            if restart is not None and in_range and int(restart[i]) != 0:
                if smooth:
                    has[k] = 0
                if last is not None:
                    last[k] = 0
            if box_format == "relative":
                x0, y0, x1, y1 = (np.float64(v) for v in detection_to_face(b[i, 0], b[i, 1], b[i, 2], b[i, 3], W, H))
            else:
                x0, y0, x1, y1 = b[i]
            window, cause = None, "stream" if not in_range else "box"
            if in_range and all(np.isfinite(v) and abs(v) < _CROP_RANGE for v in (x0, y0, x1, y1)):
                v = np.array([np.floor((x1 + x0) / 2), np.floor((y1 + y0) / 2), (((x1 - x0) + y1) - y0) * scale])
                if smooth:
                    if not has[k]:
                        state[k] = v
                        has[k] = 1
                    elif not fixed:
                        state[k] = v * m + state[k] * om
                    v = state[k].copy()
                cx, cy, sz = np.rint(v)
                cause = "size"
                if np.isfinite(sz) and sz >= 2:
                    sz = sz - np.fmod(sz, 2.0)
                    half = sz / 2
                    b0, b1, b2, b3 = cx - half, cy - half, cx + half, cy + half
                    over = max(0.0 if b0 >= 0 else -b0, 0.0 if b1 >= 0 else -b1, 0.0 if b2 <= W else b2 - W, 0.0 if b3 <= H else b3 - H)
                    b0, b1, b2, b3 = b0 + over, b1 + over, b2 - over, b3 - over
                    side = np.trunc((b2 - b0 + b3 - b1) / 2)
                    side = side - np.fmod(side, 2.0)
                    cause = "side" if not side >= 2 else "guard"
                    if side >= 2 and side < _CROP_RANGE and abs(cx) < _CROP_RANGE and abs(cy) < _CROP_RANGE:
                        side_i = int(side)
                        x_lo, y_lo = int(cx) - side_i // 2, int(cy) - side_i // 2
                        if window_inside(x_lo, y_lo, side_i, W, H, min_side):
                            window, cause = (x_lo, y_lo, side_i, side_i), "present"
                            face_scale[i] = side / sz
                        elif window_inside(x_lo, y_lo, side_i, W, H):
                            cause = "min_side"
            if why is not None:
                why.append(cause)
            if window is not None:
                crop[i] = paste[i] = window
                if last is not None:
                    last[k] = window
                continue
            if hold and in_range and window_inside(int(last[k, 0]), int(last[k, 1]), int(last[k, 2]), W, H, min_side):
                crop[i] = paste[i] = last[k]
                continue
            side_i = min(W, H)
            crop[i] = ((W - side_i) // 2, (H - side_i) // 2, side_i, side_i)
    return crop, paste, face_scale


TRACK_MAX_TRACKS, TRACK_MAX_DETECTIONS = 16, 32
_QUIET_NAN = np.uint64(0x7ff8000000000000)


def box_iou(a, b):
    """IoU of two boxes (x0, y0, x1, y1) of float64, in the order of operations of include/emo_hip.h (ABI 25)"""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return np.float64(0.0)
    inter = iw * ih
    return inter / (((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter)


def track_assign(dets, stream_of, ref, age, min_iou=0.3, max_missed=15, box_format="xyxy"):
    """Unordered detections -> ordered track rows, one frame after another: greedy IoU association of the detections of every frame
    to the P track slots of its video stream.  The contract that emo_track_assign_f64 (ops.track_assign) is held to bit for bit;
    include/emo_hip.h (ABI 25) has the same text.
    dets [F,D,4] float64, frame order, D <= 32, NaN rows = padding; stream_of [F] ints or None (every frame: stream 0); ref [K,P,4]
    float64 = each track's last matched box (x0, y0, x1, y1) and age [K,P] int32 (-1: the slot is free; >= 0: live, that many
    consecutive frames without a match) are the streams' state, UPDATED IN PLACE (numpy arrays), P <= 16; min_iou in (0, 1];
    max_missed >= 0; box_format 'xyxy', or 'relative' = (xmin, ymin, width, height), whose box is (d0, d1, d0 + d2, d1 + d3): IoU does
    not change under a scaling of an axis, so neither the frame size nor detection_to_face's 0.9 / 1.2 enter here.
    -> (boxes [F,P,4] float64, restart [F,P] int32, track_of [F,D] int32).  A frame of stream k:
        usable: a detection whose box is finite and below 2^30 in all four values, with x1 > x0 and y1 > y0
        1. match: repeat -- among the live tracks without a match in this frame and the usable detections without a track, the
           pair of the largest box_iou(ref[k,p], box), ties to the smaller p, then the smaller d; stop when there is none or its IoU
           < min_iou.  ref[k,p] = the box, age[k,p] = 0, boxes[f,p] = dets[f,d] bit for bit, restart[f,p] = 0, track_of[f,d] = p
        2. age: every live track without a match: age += 1; past max_missed it dies: age = -1, restart[f,p] = 1.  Its row is NaN
        3. birth: the usable detections without a track, in ascending d, each into the lowest free slot (those freed in step 2
           included): ref, age = 0, boxes[f,p] = dets[f,d], restart[f,p] = 1, track_of[f,d] = p; -1 with no slot left
        4. every other slot: a NaN row, restart 0; every other detection: track_of = -1
    NaN rows are the quiet NaN 0x7ff8000000000000.  A frame whose stream lies outside [0, K) gets NaN rows, restart 0, track_of
    -1 and touches no state."""
    d = np.ascontiguousarray(dets, dtype=np.float64)
    if d.ndim != 3 or d.shape[2] != 4 or d.shape[0] == 0 or not 0 < d.shape[1] <= TRACK_MAX_DETECTIONS:
        raise ValueError(f"dets must be [F,D,4] with 1 <= D <= {TRACK_MAX_DETECTIONS}, got {d.shape}")
    if box_format not in CROP_BOX_FORMATS:
        raise ValueError(f"box_format {box_format!r}: 'xyxy' or 'relative'")
    if ref.ndim != 3 or ref.shape[2] != 4 or age.shape != ref.shape[:2] or not 0 < ref.shape[1] <= TRACK_MAX_TRACKS or ref.shape[0] == 0:
        raise ValueError(f"ref [K,P,4] and age [K,P] with 1 <= P <= {TRACK_MAX_TRACKS}, got {ref.shape} and {age.shape}")
    min_iou = np.float64(min_iou)
    if not 0.0 < min_iou <= 1.0:
        raise ValueError(f"min_iou {min_iou} is not in (0, 1]")
    if int(max_missed) != max_missed or max_missed < 0:
        raise ValueError(f"max_missed {max_missed} is not an integer >= 0")
    F, D = d.shape[:2]
    K, P = age.shape
    boxes = np.empty((F, P, 4), np.float64)
    boxes.view(np.uint64)[:] = _QUIET_NAN
    restart, track_of = np.zeros((F, P), np.int32), np.full((F, D), -1, np.int32)
    with np.errstate(all="ignore"):
        for f in range(F):
            k = 0 if stream_of is None else int(stream_of[f])
            if not 0 <= k < K:
                continue
            box = d[f].copy()
            if box_format == "relative":
                box[:, 2], box[:, 3] = d[f, :, 0] + d[f, :, 2], d[f, :, 1] + d[f, :, 3]
            usable = [bool(all(np.isfinite(v) and abs(v) < _CROP_RANGE for v in b) and b[2] > b[0] and b[3] > b[1]) for b in box]
            iou = {(p, j): box_iou(ref[k, p], box[j]) for p in range(P) if age[k, p] >= 0 for j in range(D) if usable[j]}
            matched = set()
            while True:
                best = None
                for (p, j), v in sorted(iou.items()):                              # (ascending p, then d: the first of equals wins)
                    if p not in matched and track_of[f, j] < 0 and v >= 0 and (best is None or v > best[0]):
                        best = (v, p, j)
                if best is None or not best[0] >= min_iou:
                    break
                _, p, j = best
                ref[k, p], age[k, p], boxes[f, p], track_of[f, j] = box[j], 0, d[f, j], p
                matched.add(p)
            for p in range(P):
                if age[k, p] >= 0 and p not in matched:
                    age[k, p] += 1
                    if age[k, p] > max_missed:
                        age[k, p], restart[f, p] = -1, 1
            for j in range(D):
                if usable[j] and track_of[f, j] < 0:
                    free = [p for p in range(P) if age[k, p] < 0]
                    if not free:
                        break
                    p = free[0]
                    ref[k, p], age[k, p], boxes[f, p], restart[f, p], track_of[f, j] = box[j], 0, d[f, j], 1, p
    return boxes, restart, track_of


PRESENT_MAX_ROWS = 1 << 24


def present_rows(crop, paste, F, P):
    """The present rows of the tracker's windows, first and in order: a stable compaction of the M = F * P frame-major rows.  The
    contract that emo_present_rows_i32 (ops.present_rows) is held to bit for bit; include/emo_hip.h (ABI 27) has the same text.
    crop, paste [M,4] int32 as crop_track returns them; row i is present iff paste[i][2] > 0.
    -> (count [F], first [F + 1], row_of [M], crop_out [M,4], paste_out [M,4]), int32: first[f] = the present rows with an index <
    f * P (first[F] = T, their total), count[f] = first[f + 1] - first[f]; for j < T row_of[j] = the index of the j-th present row,
    crop_out[j] = crop[row_of[j]], paste_out[j] = paste[row_of[j]]; for T <= j < M row_of[j] = -1 and both windows (0, 0, 0, 0)."""
    F, P = int(F), int(P)
    if F <= 0 or not 1 <= P <= TRACK_MAX_TRACKS or F * P > PRESENT_MAX_ROWS:
        raise ValueError(f"present_rows: F = {F} frames of P = {P} rows: F >= 1, 1 <= P <= {TRACK_MAX_TRACKS}, F * P <= 2^24")
    M = F * P
    crop, paste = (np.ascontiguousarray(w, dtype=np.int32) for w in (crop, paste))
    if crop.shape != (M, 4) or paste.shape != (M, 4):
        raise ValueError(f"present_rows: crop and paste must be [{M},4], got {crop.shape} and {paste.shape}")
    present = paste[:, 2] > 0
    rows = np.nonzero(present)[0].astype(np.int32)
    T = rows.shape[0]
    count = present.reshape(F, P).sum(axis=1).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    row_of = np.full((M,), -1, np.int32)
    crop_out, paste_out = np.zeros((M, 4), np.int32), np.zeros((M, 4), np.int32)
    row_of[:T], crop_out[:T], paste_out[:T] = rows, crop[rows], paste[rows]
    return count, first, row_of, crop_out, paste_out


def mixing_theta(source_theta, target_theta, mix_old=True):
    """notebooks/infer.py:686-736 (get_mixing_theta): keep the source's stretch (scale/shear from the polar decomposition of
    its linear part) and take rotation + translation from the driver.  numpy [B,>=3,4] x [B*T,>=3,4] -> float64 [B*T,3,4].
    As in the reference the driver poses are rolled by one along the batch axis of the sources (a no-op for one source)."""
    from scipy import linalg
    source_theta = np.asarray(source_theta, dtype=np.float64)[:, :3, :]
    target_theta = np.asarray(target_theta, dtype=np.float64)[:, :3, :]
    B = source_theta.shape[0]
    T = target_theta.shape[0] // B
    target_theta = np.roll(target_theta.reshape(B, T, 3, 4), 1, axis=0).reshape(B * T, 3, 4)

    def homogeneous(t):
        m = np.tile(np.eye(4), (t.shape[0], 1, 1))
        m[:, :3, :] = t
        return m

    src, tgt = homogeneous(source_theta), homogeneous(target_theta)
    translation = np.tile(np.eye(4), (B * T, 1, 1))
    translation[:, :3, 3] = tgt[:, :3, 3]
    src_lin, tgt_lin = src.copy(), tgt.copy()
    src_lin[:, :3, 3] = 0
    tgt_lin[:, :3, 3] = 0
    out = []
    for b in range(B):
        try:
            _, src_stretch = linalg.polar(src_lin[b])
        except Exception:                                   # decomposition failed: fall back to the driver pose (:718-719)
            out += [tgt[b * T + t] for t in range(T)]
            continue
        for t in range(T):
            i = b * T + t
            try:
                tgt_rot, tgt_stretch = linalg.polar(tgt_lin[i])
            except Exception:
                out.append(src_stretch)                                                     # :724-725
                continue
            if mix_old:
                out.append(translation[i] @ tgt_rot @ src_stretch)                          # :727-728
            else:
                out.append(src_stretch * tgt_stretch.mean() / src_stretch.mean() @ tgt_rot @ translation[i])   # :729-730
    return np.stack(out)[:, :3]


def ema_scan(values, state, momentum):
    """The `smooth_pose` recurrence of notebooks/infer.py:571-581 over a whole clip on the host:
        theta_i = pred[i] * momentum + theta_{i-1} * (1 - momentum),   theta_{-1} = state, or pred[0] on the first call
    values [n, ...] fp32 (n x 16 floats: cheap), state [...] or None -> (smoothed [n, ...], new state).  fp32 element for
    element in the reference's operation order (two rounded products, one rounded sum; `1 - momentum` formed in double and
    rounded to fp32 once, as torch does with a Python scalar), so the result is bit-identical to the reference's per-frame loop
    of device ops -- and, being a scan over the FRAME ORDER, it has to run before the frames are sharded across ranks
    (SURVEY.md section 8e)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    m, om = np.float32(momentum), np.float32(1 - momentum)
    cur = v[0].copy() if state is None else np.asarray(state, dtype=np.float32).reshape(v.shape[1:])
    out = np.empty_like(v)
    for i in range(v.shape[0]):
        cur = v[i] * m + cur * om
        out[i] = cur
    return out, cur


def _row_mask(mask, n, name):
    """a row mask of the control streams: None, or n ints -> None or a bool [n] array (!= 0)"""
    if mask is None:
        return None
    mask = np.asarray(mask)
    if mask.shape != (n,):
        raise ValueError(f"{name} must have one entry per row ({n}), got {mask.shape}")
    return mask != 0


def ema_scan_tracks(values, stream_of, state, has_state, momentum, restart=None, present=None):
    """ema_scan over the rows of K streams that follow face tracks -- the contract that emo_theta_ema_scan_tracks_f32
    (ops.theta_ema_scan(restart=, present=)) is held to bit for bit; include/emo_hip.h (ABI 26) has the same text.
    values [n, ...] fp32 in frame order; stream_of [n] ints or None (every row: stream 0); state [K, ...] fp32 and has_state [K]
    are the streams' states, UPDATED IN PLACE (numpy arrays); restart, present: [n] ints or None (no restarts; every row
    present).  Row i of a stream k in [0, K), within the stream in row order:
        1. restart[i] != 0: has_state[k] = 0, before the row is looked at and whether or not it is present
        2. present: a stream without state starts at the row's value; cur = v * m + cur * fp32(1 - m); state[k] = cur,
           has_state[k] = 1; out[i] = cur  (ema_scan's recurrence)
        3. absent: out[i] = v * m + cur * fp32(1 - m) with cur = state[k], or = v where the stream has none; nothing is written
    -> out [n, ...]; a row whose stream lies outside [0, K) is left unwritten (NaN here), touches no state, and its masks are
    not looked at.  With both masks None every stream is ema_scan of its rows."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    n, K = v.shape[0], state.shape[0]
    restart, present = _row_mask(restart, n, "restart"), _row_mask(present, n, "present")
    m, om = np.float32(momentum), np.float32(1 - momentum)
    out = np.full_like(v, np.nan)
    for i in range(n):
        k = 0 if stream_of is None else int(stream_of[i])
        if not 0 <= k < K:
            continue
        if restart is not None and restart[i]:
            has_state[k] = 0
        cur = state[k].reshape(v.shape[1:]) if has_state[k] else v[i]
        cur = v[i] * m + cur * om
        if present is None or present[i]:
            state[k] = cur.reshape(state.shape[1:])
            has_state[k] = 1
        out[i] = cur
    return out


def expression_controls(values, stream_of, neutral, gain, offset, anchor, has_anchor, ema, has_ema, relative, momentum,
                        restart=None, present=None):
    """The expression controls of the batched entry points on the host, one row after another -- the contract that
    emo_expr_controls_f32 (ops.expression_controls) is held to bit for bit, as ema_scan is for the theta scan.  The reference has
    no such controls beyond the `custome_target_pose_embed` override (notebooks/infer.py:603-604).
    values [n,E] fp32 in frame order; stream_of [n] ints or None (every row: stream 0); neutral [K,E] or None; gain [n] or None;
    offset [n,E] or None; anchor, ema [K,E] and has_anchor, has_ema [K] are the streams' states, UPDATED IN PLACE (numpy arrays;
    None where the control that needs them is off); momentum None = no smoothing.  Row i of stream k, every operation in fp32
    and rounded on its own:
        with neutral:  r = neutral[k], or with `relative` the stream's anchor (its first row);  e = neutral[k] + (e - r) * gain[i]
        with offset:   e = e + offset[i]
        with momentum: the smooth_pose recurrence, cur = e * m + cur * fp32(1 - m), started at the stream's first e
    restart, present: [n] ints or None (emo_expr_controls_tracks_f32; include/emo_hip.h, ABI 26, has the same text): a row with
    restart[i] != 0 first clears its stream's has_anchor (under `relative`) and has_ema (with momentum), whether or not it is
    present; a present row (present None or present[i] != 0) is processed as above; an absent row is computed from a private copy
    of the stream's state -- it is its own anchor where the stream has none, and its EMA starts at itself where the stream has
    none -- and writes nothing of the stream.  With both None this is the function as it always was.
    -> out [n,E]; a row whose stream lies outside [0, K) is left unwritten (NaN here), touches no state, and its masks are not
    looked at."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    restart, present = _row_mask(restart, v.shape[0], "restart"), _row_mask(present, v.shape[0], "present")
    if v.ndim != 2:
        raise ValueError(f"values must be [n,E], got {v.shape}")
    smooth = momentum is not None
    if (relative or gain is not None) and neutral is None:
        raise ValueError("relative transfer and gain work about a neutral expression: neutral is missing")
    if relative and (anchor is None or has_anchor is None):
        raise ValueError("relative transfer needs anchor and has_anchor")
    if smooth and (ema is None or has_ema is None):
        raise ValueError("smoothing needs ema and has_ema")
    K = next((a.shape[0] for a in (neutral, anchor, ema) if a is not None), 1)
    f32 = lambda a: None if a is None else np.asarray(a, dtype=np.float32)
    neutral, gain, offset = f32(neutral), f32(gain), f32(offset)
    if smooth:
        m, om = np.float32(momentum), np.float32(1 - momentum)
    out = np.full_like(v, np.nan)
    for i in range(v.shape[0]):
        k = 0 if stream_of is None else int(stream_of[i])
        if not 0 <= k < K:
            continue
        if restart is not None and restart[i]:
            if relative:
                has_anchor[k] = 0
            if smooth:
                has_ema[k] = 0
        here = present is None or bool(present[i])
        e = v[i].copy()
        if neutral is not None:
            r = neutral[k]
            if relative:
                if not has_anchor[k] and here:
                    anchor[k] = e
                    has_anchor[k] = 1
                r = anchor[k] if has_anchor[k] else e
            t = e - r
            if gain is not None:
                t = t * gain[i]
            e = neutral[k] + t
        if offset is not None:
            e = e + offset[i]
        if smooth:
            cur = ema[k] if has_ema[k] else e
            e = e * m + cur * om
            if here:
                ema[k] = e
                has_ema[k] = 1
        out[i] = e
    return out


_POSE_CLAMP = (np.float32(-np.float32(3.14159265358979323846) / np.float32(2)), np.float32(3.14159265358979323846))


def srt_theta(srt):
    """get_transform_matrix (utils/point_transforms.py:188-242) of rows [n,9] = [scale | yaw pitch roll | translation] in
    float64 -> theta [n,4,4] float64 = S R T, the rotation clamped to [-pi/2, pi]: what emo_pose_theta_f32 forms in fp32"""
    p = np.asarray(srt, dtype=np.float64).reshape(-1, 9)
    out = np.zeros((p.shape[0], 4, 4))
    for i, r in enumerate(p):
        yaw, pitch, roll = np.clip(r[3:6], -np.pi / 2, np.pi)
        yc, ys, pc, ps, rc, rs = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        R = np.array([[yc * pc, yc * ps * rs - ys * rc, yc * ps * rc + ys * rs],
                      [ys * pc, ys * ps * rs + yc * rc, ys * ps * rc - yc * rs],
                      [-ps, pc * rs, pc * rc]])
        SR = np.diag(r[0:3]) @ R
        out[i, :3, :3] = SR
        out[i, :3, 3] = SR @ r[6:9]
        out[i, 3, 3] = 1.0
    return out


def head_pose_controls(scale, rotation, translation, stream_of, source, gain, rotation_offset, translation_offset, zoom, anchor,
                       has_anchor, relative, frontal, K=None, restart=None, present=None):
    """The head-pose controls of the batched entry points on the host, one row after another -- the contract that
    emo_head_pose_controls_f32 (ops.head_pose_controls) is held to bit for bit.  frontal and the rotation offsets are the
    reference's `normalize`, `delta_yaw` and `delta_pitch` (ExpressionEmbed.forward_image, expression_embedder.py:302-316: the
    rotation clamped to [-pi/2, pi], yaw = pitch = 0 and translation = 0, then the deltas added); the rest has no counterpart
    there.  scale [n,1] or [n,3] (one column is broadcast to three), rotation and translation [n,3], frame order; stream_of [n]
    ints or None (every row: stream 0); source [K,9] or None; gain, zoom [n] or None; rotation_offset, translation_offset [n,3]
    or None; anchor [K,9] and has_anchor [K] are the streams' state, UPDATED IN PLACE (numpy arrays; None without `relative`);
    K: the number of streams where neither source nor anchor says it (default 1).
    A row is p = [sx sy sz | yaw pitch roll | tx ty tz]; row i of stream k, every operation in fp32 and rounded on its own:
        0. p.rot = clamp(p.rot, -pi/2, pi), the fp32 constants of emo_pose_theta_f32
        1. frontal:  yaw = pitch = 0, p.trans = 0
        2. with source:  q = source[k], q.rot clamped;  ref = q, or with `relative` the stream's anchor (its first row after
           step 0);  p.rot = q.rot + (p.rot - ref.rot) * gain[i],  p.trans = q.trans + (p.trans - ref.trans) * gain[i] (no
           product without gain);  with `relative` only:  p.scale = q.scale * (p.scale / ref.scale)
        3. p.rot += rotation_offset[i];  p.trans += translation_offset[i];  p.scale *= zoom[i]  (each where given)
    restart, present: [n] ints or None (emo_head_pose_controls_tracks_f32; include/emo_hip.h, ABI 26, has the same text): under
    `relative` a row with restart[i] != 0 first clears its stream's has_anchor, whether or not it is present; a present row
    (present None or present[i] != 0) is processed as above; an absent row never becomes the anchor, and where the stream has none
    it is its own reference (ref = the row after step 0).  Without `relative` there is no state and the masks change nothing; with
    both None this is the function as it always was.
    -> (rows [n,9] fp32, theta [n,4,4] = srt_theta(rows) rounded to fp32); a row whose stream lies outside [0, K) is left
    unwritten (NaN here), touches no state, and its masks are not looked at."""
    f32 = lambda a: None if a is None else np.asarray(a, dtype=np.float32)
    scale, rotation, translation = (np.ascontiguousarray(a, dtype=np.float32) for a in (scale, rotation, translation))
    if scale.ndim != 2 or scale.shape[1] not in (1, 3) or rotation.shape != (scale.shape[0], 3) or translation.shape != rotation.shape:
        raise ValueError(f"scale [n,1] or [n,3], rotation and translation [n,3]: got {scale.shape}, {rotation.shape}, {translation.shape}")
    if relative and frontal:
        raise ValueError("frontal zeroes what relative transfers")
    if (relative or gain is not None) and source is None:
        raise ValueError("relative transfer and gain work about a source pose: source is missing")
    if relative and (anchor is None or has_anchor is None):
        raise ValueError("relative transfer needs anchor and has_anchor")
    K = next((a.shape[0] for a in (source, anchor) if a is not None), 1 if K is None else K)
    source, gain, zoom = f32(source), f32(gain), f32(zoom)
    rotation_offset, translation_offset = f32(rotation_offset), f32(translation_offset)
    lo, hi = _POSE_CLAMP
    n = scale.shape[0]
    restart, present = _row_mask(restart, n, "restart"), _row_mask(present, n, "present")
    out = np.full((n, 9), np.nan, np.float32)
    for i in range(n):
        k = 0 if stream_of is None else int(stream_of[i])
        if not 0 <= k < K:
            continue
        p = np.empty(9, np.float32)
        p[0:3] = scale[i]
        p[3:6] = np.clip(rotation[i], lo, hi)
        p[6:9] = translation[i]
        if relative and restart is not None and restart[i]:
            has_anchor[k] = 0
        if relative and not has_anchor[k] and (present is None or present[i]):
            anchor[k] = p
            has_anchor[k] = 1
        own = p.copy()
        if frontal:
            p[3] = p[4] = 0.0
            p[6:9] = 0.0
        if source is not None:
            q = source[k].copy()
            q[3:6] = np.clip(q[3:6], lo, hi)
            ref = (anchor[k] if has_anchor[k] else own) if relative else q
            d = p[3:9] - ref[3:9]
            if gain is not None:
                d = d * gain[i]
            if relative:
                p[0:3] = q[0:3] * (p[0:3] / ref[0:3])
            p[3:9] = q[3:9] + d
        if rotation_offset is not None:
            p[3:6] = p[3:6] + rotation_offset[i]
        if translation_offset is not None:
            p[6:9] = p[6:9] + translation_offset[i]
        if zoom is not None:
            p[0:3] = p[0:3] * zoom[i]
        out[i] = p
    theta = np.full((n, 4, 4), np.nan, np.float32)
    done = np.ones(n, dtype=bool) if stream_of is None else np.array([0 <= int(k) < K for k in stream_of], dtype=bool)
    if done.any():
        theta[done] = srt_theta(out[done]).astype(np.float32)
    return out, theta


def bank_slot(slot, capacity):
    """a slot of an identity bank of `capacity` slots as an int; ValueError unless it is an integer (not a bool) in range"""
    import operator
    try:
        slot = operator.index(slot) if not isinstance(slot, bool) else None
    except TypeError:
        slot = None
    if slot is None or not 0 <= slot < capacity:
        raise ValueError(f"slot {slot!r} is not in [0, {capacity})")
    return slot


def enrolment_plan(used, n_sources, slots=None, batch_size=8, world=1):
    """InferenceWrapper.enrol_identities on the host, before anything is launched -> (slots, chunks, owners).
    used: the occupied flag of every bank slot.  slots=None takes the n_sources lowest free slots; an explicit list may name
    occupied slots (they are overwritten, as store_identity(slot) overwrites).  Chunk j is the sources
    [j * batch_size, (j + 1) * batch_size) whatever the world size, and rank r owns the contiguous chunk range
    parallel.shard_range(len(chunks), r, world); owners[j] is the rank that computes chunk j.  ValueError for a bank without
    slots, no sources, too few free slots, a duplicate or out-of-range slot and a batch size below 1.  A pure function of its
    arguments: every rank passes the same ones and takes the same decision."""
    from .parallel import shard_range
    capacity = len(used)
    if capacity == 0:
        raise ValueError("this wrapper has no identity bank: construct it with identity_capacity=K")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    if n_sources == 0:
        raise ValueError("no sources to enrol")
    if slots is None:
        free = [k for k, u in enumerate(used) if not u]
        if len(free) < n_sources:
            raise ValueError(f"{n_sources} sources, {len(free)} free identity slots of {capacity}: drop_identity some or pass slots=")
        slots = free[:n_sources]
    else:
        slots = [bank_slot(k, capacity) for k in slots]
        if len(slots) != n_sources:
            raise ValueError(f"{len(slots)} slots for {n_sources} sources")
        if len(set(slots)) != len(slots):
            raise ValueError(f"slots {slots} name a slot twice")
    n_chunks = -(-n_sources // batch_size)
    chunks = [(j * batch_size, min((j + 1) * batch_size, n_sources)) for j in range(n_chunks)]
    owners = [0] * n_chunks
    for r in range(world):
        lo, hi = shard_range(n_chunks, r, world)
        owners[lo:hi] = [r] * (hi - lo)
    return slots, chunks, owners
