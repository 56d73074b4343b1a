"""The per-row controls of the batched entry points that carry state along the frame order -- smooth_pose, expression=, head_pose=
-- beside InferenceWrapper (emoportraits_amd/infer.py): the state of a set of streams (StreamStates) and the host-side checks of
the two keywords (expression_plan, head_pose_plan, and stream_expression / stream_head_pose for animate_streams).  The value types
are in controls.py, which stays pure Python; the arithmetic is ops.theta_ema_scan / expression_controls / head_pose_controls.
Crop tracking (boxes=, tracking=) has its own store, CropStates -- its streams are tracks of the video, not identities -- its own
checks, crop_plan, and BoxFeed, which hands out the boxes as the frames come; the arithmetic is ops.crop_track.  detections= (unordered
detections in place of ordered boxes) adds TrackStates, the tracks that ops.track_assign associates the detections to.  With
tracking follow_tracks=True the streams of StreamStates follow those tracks: row_masks hands the tracker's restart flags and its
"this row has a face" to the three controls, which restart a stream at a birth and keep a row without a face out of it."""
import itertools
from argparse import Namespace

import torch

from .controls import CropTracking, ExpressionControls, HeadPoseControls


class StreamStates:
    """The state of K streams of rows, on the device: per stream the smooth_pose EMA `theta` [K,4,4], the relative-pose anchor
    `pose_anchor` [K,9], the expression controls' relative-transfer anchor `expr_anchor` and EMA `expr_ema` [K,E], each with an int32
    flag vector `*_has` [K]: 0 until the stream's first row (the kernels set it), and 0 again after a restart -- restart() here, or
    under tracking follow_tracks=True a row at which the row's face track restarts (the kernels clear it).  The expression rows
    are allocated at the first use (expression()), from the width of the row at hand; until then they and their flags are None.
    InferenceWrapper holds two: `_bank_streams`, one stream per slot of the identity bank (None without a bank), and `_stream`, the
    one stream of the current identity, which the calls without identities= walk.

    Which event restarts which streams (restart() is the only place that does it); "pose" = theta EMA + pose anchor, "all" = pose +
    expression:
        event                                         bank streams                       the single stream
        forward(source_image=...), a new source       --                                 pose anchor
        load_identity(slot)                           --                                 pose anchor
        share_source(), on every rank                 --                                 pose anchor
        store_identity(slot)                          slot: all  (= _bank_write)         --
        _bank_write(slot, ...)                        slot: all                          --
        drop_identity(slot)                           slot: all                          --
        enrol_identities(..., slots)                  the enrolled slots: all            --
        share_identity(slot), on a receiver           slot: all  (= _bank_write)         --
        share_identity(slot), on the source rank      --                                 --
        reset_pose_state(None | slots)                every slot | slots: pose           pose | --
        reset_expression_state(None | slots)          every slot | slots: expression     expression | --
        forward(reset_tracking=True)                  every slot: all                    all
    So a new current identity restarts the single stream's relative pose but neither its smooth_pose EMA (the reference carries
    `self.theta` across sources) nor its expression anchor and EMA: those run on until reset_expression_state() or
    reset_tracking."""

    def __init__(self, K, device, what="the identity bank"):
        self.K, self.device, self.what = K, device, what
        self.theta = torch.zeros((K, 4, 4), device=device, dtype=torch.float32)
        self.pose_anchor = torch.zeros((K, 9), device=device, dtype=torch.float32)
        self.theta_has, self.pose_anchor_has = (torch.zeros((K,), device=device, dtype=torch.int32) for _ in range(2))
        self.expr_anchor = self.expr_ema = self.expr_anchor_has = self.expr_ema_has = None

    def expression(self, E):
        """the expression rows, allocated at the first use from the width E of the row at hand; every later row has that width"""
        if self.expr_anchor is None:
            self.expr_anchor, self.expr_ema = (torch.zeros((self.K, E), device=self.device, dtype=torch.float32) for _ in range(2))
            self.expr_anchor_has, self.expr_ema_has = (torch.zeros((self.K,), device=self.device, dtype=torch.int32) for _ in range(2))
        elif self.expr_anchor.shape[1] != E:
            raise ValueError(f"an expression row of width {E}: {self.what} holds rows of width {self.expr_anchor.shape[1]}")

    def restart(self, rows=None, pose_ema=False, pose_anchor=False, expression=False):
        """The streams `rows` (host ints or a device index tensor; None: all of them) begin again at their next row: device fills of
        the flags, no host synchronisation"""
        if rows is not None and not isinstance(rows, torch.Tensor):
            rows = torch.tensor(list(rows), dtype=torch.int64).to(self.device)
        for has, on in ((self.theta_has, pose_ema), (self.pose_anchor_has, pose_anchor), (self.expr_anchor_has, expression),
                        (self.expr_ema_has, expression)):
            if on and has is not None:                   # (None: expression rows that no call has used yet)
                if rows is None:
                    has.zero_()
                else:
                    has.index_fill_(0, rows, 0)


# ---- the checks of expression= and head_pose=, before anything is launched ------------------------------------------------------
def _scalar(v):
    return isinstance(v, torch.Tensor) and v.dim() == 0 or not isinstance(v, torch.Tensor) and not hasattr(v, '__len__')


def _rows(v, n_rows, name, dims, expected, width=None):
    """"one row, or one per row": v as a host fp32 tensor of one of `dims` dimensions (of `width` columns where given; `expected`
    says so in words), with max(dims) dimensions one row per row of the call"""
    t = torch.as_tensor(v).detach().float()
    if t.dim() not in dims or width is not None and t.shape[-1] != width:
        raise ValueError(f"{name}: {expected}, got {tuple(t.shape)}")
    if t.dim() == max(dims) and n_rows is not None and t.shape[0] != n_rows:
        raise ValueError(f"{name} has {t.shape[0]} rows for {n_rows} rows of the call")
    return t


def _per_row(v, n_rows, name, expected):
    """"a float, or one value per row" -> None for 1.0, a float, or a host [rows] tensor"""
    if _scalar(v):
        return None if float(v) == 1.0 else float(v)
    return _rows(v, n_rows, name, (1,), expected)


def _sources(ids, source, has_source, no_current, no_slot):
    """what relative / gain work about is there: the current identity's `source` row, or one in every slot of `ids`"""
    if ids is None and source is None:
        raise ValueError(no_current)
    missing = [] if ids is None else [k for k in sorted(set(ids.tolist())) if not has_source[k]]
    if missing:
        raise ValueError(no_slot.format(missing[0]))


def rows_of(t, r0, m, name, whole=None):
    """the rows r0 ... r0 + m of a per-row value; a float, None or a `whole`-dimensional tensor (one value for every row) as it is"""
    if not isinstance(t, torch.Tensor) or t.dim() == whole:
        return t
    if t.shape[0] < r0 + m:
        raise ValueError(f"{name} has {t.shape[0]} rows, the frames run past it")
    return t[r0:r0 + m]


def expression_plan(expression, n_rows, ids, where, faces, device, source, has_source, bank_width):
    """The checks of expression= (an ExpressionControls or a mapping with its fields), before anything is launched -> None
    (no control: nothing will be launched, no state touched) or what InferenceWrapper._expression_controls needs: relative, smooth,
    momentum (None without smooth), gain (None = 1.0 | a float | a device [rows]), offset (None | a device [E] or [rows,E]), override
    (None | a device [rows,E]), step1 = the part about the neutral runs, scan = a control that walks the frame order.
    n_rows: the rows of the call where known; ids: the per-row slots (host tensor) or None = the current identity, whose source
    expression is `source` (None: it has none); has_source[k]: slot k has one; bank_width: E of the bank's rows, None before the first."""
    ex = ExpressionControls.of(expression)
    if ex is None:
        return None
    m = float(ex.momentum)
    if not 0.0 < m <= 1.0:
        raise ValueError(f"expression momentum {ex.momentum} is not in (0, 1]")
    relative, smooth = bool(ex.relative), bool(ex.smooth)
    gain = _per_row(ex.gain, n_rows, "expression gain", "a tensor of 1 dimensions")
    offset = None if ex.offset is None else _rows(ex.offset, n_rows, "expression offset", (1, 2), "a tensor of 1 or 2 dimensions")
    override = None if ex.override is None else _rows(ex.override, n_rows, "expression override", (2,), "a tensor of 2 dimensions")
    if override is not None and where != 'animate_frames':
        raise ValueError(f"expression override= replaces the expression embedder of animate_frames: {where}"
                         + ("'s expressions are inputs already" if where == 'animate' else " takes none"))
    if not (relative or smooth or gain is not None or offset is not None or override is not None):
        return None
    step1 = relative or gain is not None
    if (relative or smooth) and ids is None and (faces or where == 'animate_streams'):
        raise ValueError("expression relative / smooth follow every face track as its identity's stream: give identities")
    widths = {t.shape[-1] for t in (offset, override) if t is not None}
    if step1:
        _sources(ids, source, has_source,
                 "expression relative / gain work about the current identity's source expression, which is missing: "
                 "call forward with a source_image (or load_identity a slot that has one) first",
                 "expression relative / gain work about each identity's source expression: slot {} has none")
        if ids is None:
            widths.add(source.numel())
    if ids is not None and (step1 or smooth) and bank_width is not None:
        widths.add(bank_width)
    if len(widths) > 1:
        raise ValueError(f"expression rows of different widths: {sorted(widths)}")
    up = lambda t: t.to(device).contiguous() if isinstance(t, torch.Tensor) else t
    return Namespace(relative=relative, smooth=smooth, momentum=m if smooth else None, step1=step1, scan=relative or smooth,
                     gain=up(gain), offset=up(offset), override=up(override))


def head_pose_plan(head_pose, n_rows, ids, where, target_theta, faces, device, source, has_source):
    """The checks of head_pose= (a HeadPoseControls or a mapping with its fields), before anything is launched -> None (no
    control: nothing will be launched, no state touched) or what InferenceWrapper._head_pose_controls needs: relative, frontal, gain
    and zoom (None = 1.0 | a float | a device [rows]), rotation_offset and translation_offset (None | a device [3] or [rows,3]),
    step1 = the part about the source pose runs.  n_rows, ids, source (the current identity's [1,9] row), has_source: as
    expression_plan's."""
    hp = HeadPoseControls.of(head_pose)
    if hp is None:
        return None
    relative, frontal = bool(hp.relative), bool(hp.frontal)
    gain, zoom = (_per_row(getattr(hp, name), n_rows, f"head_pose {name}", "a float or one value per row") for name in ('gain', 'zoom'))
    rot, trans = (None if v is None else _rows(v, n_rows, f"head_pose {name}", (1, 2), "[3] or [rows,3]", 3)
                  for name, v in (('rotation_offset', hp.rotation_offset), ('translation_offset', hp.translation_offset)))
    if not (relative or frontal or gain is not None or zoom is not None or rot is not None or trans is not None):
        return None
    if frontal and relative:
        raise ValueError("head_pose frontal zeroes the yaw, pitch and translation that relative transfers: choose one")
    if not target_theta:
        raise ValueError("head_pose= edits the driver's head pose, target_theta=False renders in the source's: nothing of the "
                         "edit would be rendered")
    step1 = relative or gain is not None
    if relative and ids is None and (faces or where == 'animate_streams'):
        raise ValueError("head_pose relative follows every face track as its identity's stream: give identities")
    if step1:
        _sources(ids, source, has_source,
                 "head_pose relative / gain work about the current identity's source (scale, rotation, translation), "
                 "which is missing: call forward with a source_image and the head-pose regressor, or a "
                 "custome_source_theta_embed given as the triple, first",
                 "head_pose relative / gain work about each identity's source (scale, rotation, translation): slot {} has none")
    up = lambda t: t.to(device).contiguous() if isinstance(t, torch.Tensor) else t
    return Namespace(relative=relative, frontal=frontal, step1=step1, gain=up(gain), zoom=up(zoom), rotation_offset=up(rot),
                     translation_offset=up(trans))


# ---- animate_streams: the call's values and the streams' own -> the values of the call's rows -------------------------------------
def _merge_streams(kind, call, per_stream, n_faces, order, scalars, offsets, width):
    """The per-stream merge of a control's per-row fields.  call: the controls of the call, whose `scalars` are one float and whose
    `offsets` one [width] row ([E] with width=None); per_stream[s]: stream s's own mapping of those fields or None, in place of the
    call's values for its n_faces[s] faces; order = (stream, first face, end) of every frame of the batch order.  -> None where no
    stream brings its own (the call's values stay as they are), else {field: the value of every row of the call}: the stream's
    value or the call's expanded to the stream's faces, concatenated in batch order -- zero rows for a stream without an offset
    where another has one, a scalar 1.0 again where every row's is 1."""
    one = "[E]" if width is None else f"[{width}]"
    for name in scalars:
        if not _scalar(getattr(call, name)):
            raise ValueError(f"animate_streams' {kind} {name} is one float: per-face values belong to a stream's '{kind}'")
    for name in offsets:
        v = getattr(call, name)
        if v is not None and (torch.as_tensor(v).dim() != 1 if width is None else tuple(torch.as_tensor(v).shape) != (width,)):
            raise ValueError(f"animate_streams' {kind} {name} is one {one} row: per-face rows belong to a stream's '{kind}'")
    if all(p is None for p in per_stream):
        return None
    fields = scalars + offsets
    takes = " and ".join([", ".join(repr(f) for f in fields[:-1]), repr(fields[-1])])
    cols = {name: [] for name in fields}
    for s, p in enumerate(per_stream):
        p, n = {} if p is None else dict(p), n_faces[s]
        unknown = sorted(set(p) - set(fields))
        if unknown:
            raise ValueError(f"stream {s}: its '{kind}' takes {takes}, not {unknown[0]!r}")
        for name in scalars:
            g = torch.as_tensor(p.get(name, getattr(call, name))).detach().float()
            if g.dim() > 1 or g.dim() == 1 and g.shape[0] != n:
                raise ValueError(f"stream {s}: {kind} {name} {tuple(g.shape)} is not a float or one per face ({n})")
            cols[name].append(g.expand(n))
        for name in offsets:
            o = p.get(name, getattr(call, name))
            if o is not None:
                o = torch.as_tensor(o).detach().float()
                if o.dim() not in (1, 2) or width is not None and o.shape[-1] != width or o.dim() == 2 and o.shape[0] != n:
                    raise ValueError(f"stream {s}: {kind} {name} {tuple(o.shape)} is not {one} or one row per face "
                                     f"({n}{'' if width is None else f', {width}'})")
                o = o.expand(n, o.shape[-1])
            cols[name].append(o)
    out = {}
    for name in scalars:
        v = torch.cat([cols[name][s][a:b] for s, a, b in order]) if order else torch.zeros(0)
        out[name] = v if bool((v != 1.0).any()) else 1.0
    for name in offsets:
        widths = {o.shape[1] for o in cols[name] if o is not None}
        if len(widths) > 1:
            raise ValueError(f"{kind} {name}s of different widths: {sorted(widths)}")
        rows = [torch.zeros((n_faces[s], *widths)) if o is None else o for s, o in enumerate(cols[name])] if widths else None
        out[name] = torch.cat([rows[s][a:b] for s, a, b in order]) if order and rows is not None else None
    return out


def stream_expression(expression, per_stream, n_faces, order):
    """animate_streams' expression= and the streams' own 'expression' mappings ({'gain', 'offset'}) -> the ExpressionControls of the
    call's rows (_merge_streams)"""
    ex = ExpressionControls.of(expression)
    if ex is not None and ex.override is not None:
        raise ValueError("expression override= replaces the expression embedder of animate_frames: animate_streams takes none")
    call = ex or ExpressionControls()
    merged = _merge_streams('expression', call, per_stream, n_faces, order, ('gain',), ('offset',), None)
    return ex if merged is None else ExpressionControls(relative=call.relative, smooth=call.smooth, momentum=call.momentum, **merged)


def stream_head_pose(head_pose, per_stream, n_faces, order):
    """animate_streams' head_pose= and the streams' own 'head_pose' mappings ({'gain', 'zoom', 'rotation_offset',
    'translation_offset'}) -> the HeadPoseControls of the call's rows (_merge_streams)"""
    hp = HeadPoseControls.of(head_pose)
    call = hp or HeadPoseControls()
    merged = _merge_streams('head_pose', call, per_stream, n_faces, order, ('gain', 'zoom'), ('rotation_offset', 'translation_offset'), 3)
    return hp if merged is None else HeadPoseControls(relative=call.relative, frontal=call.frontal, **merged)


# ---- crop tracking: boxes= and tracking= -----------------------------------------------------------------------------------------
class CropStates:
    """The crop tracker's state of K tracks of a video, on the device: `state` [K,3] float64 = the EMA of (cx, cy, size), its flags
    `has` [K] int32 (0 until the track's first box; ops.crop_track sets it) and `last` [K,4] int32, the track's last present
    window (side 0: none).  Allocated at the first use.  Apart from StreamStates: a track is a face of the video, not an identity,
    so bank events do not touch it; InferenceWrapper restarts it with reset_crop_state() and forward(reset_tracking=True)."""

    def __init__(self, K, device):
        self.K, self.device = K, device
        self.state = self.has = self.last = None

    def arrays(self):
        if self.state is None:
            self.state = torch.zeros((self.K, 3), device=self.device, dtype=torch.float64)
            self.has = torch.zeros((self.K,), device=self.device, dtype=torch.int32)
            self.last = torch.zeros((self.K, 4), device=self.device, dtype=torch.int32)
        return self.state, self.has, self.last

    def restart(self, rows=None):
        """the tracks `rows` (host ints; None: all of them) begin again at their next box: device fills, no host synchronisation"""
        if self.state is None:
            return
        if rows is None:
            self.has.zero_()
            self.last.zero_()
        else:
            rows = torch.tensor([int(k) for k in rows], dtype=torch.int64)
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= self.K):
                raise ValueError(f"a track outside the {self.K} being tracked")
            rows = rows.to(self.device)
            self.has.index_fill_(0, rows, 0)
            self.last.index_fill_(0, rows, 0)


class TrackStates:
    """The tracks of K video streams that detections= are associated to (ops.track_assign), on the device: `ref` [K,P,4] float64 =
    each track's last matched box and `age` [K,P] int32 (-1: the slot is free; >= 0: live, that many consecutive frames without a
    detection).  Beside CropStates, whose stream p is the crop tracker of track p; restarted with it."""

    def __init__(self, K, P, device):
        self.K, self.P, self.device = K, P, device
        self.ref = torch.zeros((K, P, 4), device=device, dtype=torch.float64)
        self.age = torch.full((K, P), -1, device=device, dtype=torch.int32)

    def restart(self, tracks=None):
        """the slots `tracks` of every stream (host ints; None: all of them) are free again: device fills, no host synchronisation"""
        if tracks is None:
            self.age.fill_(-1)
        else:
            cols = torch.tensor([int(p) for p in tracks], dtype=torch.int64)
            if cols.numel() and (int(cols.min()) < 0 or int(cols.max()) >= self.P):
                raise ValueError(f"a track outside the {self.P} being tracked")
            self.age.index_fill_(1, cols.to(self.device), -1)


def check_boxes(t, what):
    """one tensor of boxes: floating point, [n,4] or [n,P,4] -> P (None: one box per frame)"""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be a float32 or float64 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() not in (2, 3) or t.shape[-1] != 4 or t.dim() == 3 and t.shape[1] == 0:
        raise ValueError(f"{what} must be [N,4] or [N,P,4], got {tuple(t.shape)}")
    return t.shape[1] if t.dim() == 3 else None


class BoxFeed:
    """boxes= handed out as the frames come: one tensor for the whole call (rows [base, base + n) of it), or an iterable that
    yields one tensor per chunk of frames, consumed in lockstep.  take() returns the boxes of a chunk on the device, as they are
    (ops.crop_track widens float32 exactly)."""

    def __init__(self, boxes, device, tracks=None, what="boxes"):
        self.device, self.what, self.tracks = device, what, tracks
        self.whole = boxes if isinstance(boxes, torch.Tensor) else None
        self.chunks = None if self.whole is not None else iter(boxes)

    def take(self, n, base):
        if self.whole is not None:
            if self.whole.shape[0] < base + n:
                raise ValueError(f"{self.what} has {self.whole.shape[0]} rows, the frames run past it")
            t = self.whole[base:base + n]
        else:
            t = next(self.chunks, None)
            if t is None:
                raise ValueError(f"{self.what} ended before the frames did: the chunk of frames {base} ... {base + n} has none")
            if check_boxes(t, f"a chunk of {self.what}") != self.tracks:
                raise ValueError(f"a chunk of {self.what} is {tuple(t.shape)}: {'[n,4]' if self.tracks is None else f'[n,{self.tracks},4]'} "
                                 f"like the others")
            if t.shape[0] != n:
                raise ValueError(f"a chunk of {self.what} has {t.shape[0]} rows for a chunk of {n} frames")
        return t.to(self.device)


def row_masks(masks, r0, m):
    """The row masks of the control streams under tracking follow_tracks=True, for the rows r0 ... r0 + m of the call: masks =
    None (the streams do not follow the tracks: {}) or (restart int32 [rows] on the device or None, present int32 [rows], the
    first row of the chunk they belong to) -> the restart= and present= of ops.theta_ema_scan / expression_controls /
    head_pose_controls: slices of the chunk's tensors, no launch"""
    if masks is None:
        return {}
    restart, present, first = masks
    if r0 < first or r0 + m > first + present.shape[0]:
        raise ValueError(f"the rows {r0} ... {r0 + m} are not rows of the chunk last tracked ({first} ... {first + present.shape[0]})")
    a = r0 - first
    return dict(restart=None if restart is None else restart[a:a + m], present=present[a:a + m])


def crop_plan(boxes, tracking, n_frames, other, batch_size, default_momentum, device, what="boxes", detections=None):
    """The checks of boxes= and tracking= (a CropTracking or a mapping with its fields), before anything is launched -> None (no
    boxes: nothing will be launched) or what InferenceWrapper._track_chunk needs: the tracker's settings, tracks = P of boxes
    [N,P,4] (None: [N,4]) and feed, the BoxFeed.  n_frames: the frames of the call where known; other: the name of a keyword given
    beside boxes that also says where the faces are ('windows' | 'faces'), or None; default_momentum: the wrapper's crop momentum.
    detections: unordered detections [N,D,4] (or an iterable of chunks) in place of boxes -- mutually exclusive with it and with
    `other`; tracking.tracks = P <= min(16, batch_size) says how many track slots a frame has, D <= 32.  The plan then has
    detections = D (None: boxes=), tracks = P, min_iou and max_missed, and its feed hands out the detections.  follow_tracks: the
    control streams follow the tracks (row_masks).  skip_absent: the rows without a face are left out of the render
    (InferenceWrapper._animate_clip; boxes [N,P,4] or detections= only)."""
    tr = CropTracking.of(tracking)
    if detections is not None:
        if boxes is not None:
            raise ValueError("detections= (unordered, the tracks are formed on the device) and boxes= (ordered tracks) are mutually exclusive")
        boxes, what = detections, "detections"
    elif tr is not None and tr.tracks is not None:
        raise ValueError("tracking tracks= says how many tracks detections= are associated to: detections= is missing")
    if boxes is None:
        if tr is not None:
            raise ValueError("tracking= says how boxes= become windows: boxes= is missing" +
                             (" (skip_absent=True leaves out rows the tracker found empty: it needs boxes= or detections=)"
                              if tr.skip_absent else ""))
        return None
    if other is not None:
        raise ValueError(f"{what}= (the tracker forms the windows) and {other}= (ready windows) are mutually exclusive")
    tr = tr or CropTracking()
    from .hostglue import CROP_BOX_FORMATS, CROP_MISSING
    if tr.box_format not in CROP_BOX_FORMATS:
        raise ValueError(f"tracking box_format {tr.box_format!r}: 'xyxy' or 'relative'")
    if tr.missing not in CROP_MISSING:
        raise ValueError(f"tracking missing {tr.missing!r}: 'skip' or 'hold'")
    m = float(default_momentum if tr.momentum is None else tr.momentum)
    if not 0.0 < m <= 1.0:
        raise ValueError(f"crop momentum {tr.momentum} is not in (0, 1]")
    scale = float(tr.scale)
    if scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError(f"crop scale {tr.scale} is not finite")
    n_dets = min_iou = max_missed = None
    if detections is not None:
        from .hostglue import TRACK_MAX_DETECTIONS, TRACK_MAX_TRACKS
        P = tr.tracks
        if P is None:
            raise ValueError("detections= needs tracking tracks=P: the number of track slots per frame")
        if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= TRACK_MAX_TRACKS:
            raise ValueError(f"tracking tracks {P!r} is not an integer in 1 ... {TRACK_MAX_TRACKS}")
        if P > batch_size:
            raise ValueError(f"tracking tracks={P}: more tracks per frame than batch_size={batch_size}")
        min_iou, max_missed = float(tr.min_iou), tr.max_missed
        if not 0.0 < min_iou <= 1.0:
            raise ValueError(f"tracking min_iou {tr.min_iou} is not in (0, 1]")
        if isinstance(max_missed, bool) or not isinstance(max_missed, int) or max_missed < 0:
            raise ValueError(f"tracking max_missed {max_missed!r} is not an integer >= 0")
    tracks = None
    if isinstance(boxes, torch.Tensor):
        tracks = check_boxes(boxes, what)
        if n_frames is not None and boxes.shape[0] != n_frames:
            raise ValueError(f"{what} has {boxes.shape[0]} rows for {n_frames} frames")
    elif not hasattr(boxes, "__iter__"):
        raise ValueError(f"{what} must be a tensor [N,4] or [N,P,4], or an iterable of one such tensor per chunk of frames")
    else:
        # (a generator: its first chunk is taken now, so that the form is known before anything is launched)
        boxes = iter(boxes)
        head = next(boxes, None)
        if head is None:
            raise ValueError(f"{what} ended before the frames did: it is empty")
        tracks = check_boxes(head, f"a chunk of {what}")
        boxes = itertools.chain([head], boxes)
    if detections is not None:
        if tracks is None:
            raise ValueError("detections must be [N,D,4], D detections per frame padded with NaN rows: got [N,4]")
        if tracks > TRACK_MAX_DETECTIONS:
            raise ValueError(f"detections has D = {tracks} per frame: at most {TRACK_MAX_DETECTIONS} are served")
        n_dets, tracks = tracks, tr.tracks
    elif tracks is not None and tracks > batch_size:
        raise ValueError(f"{what} has {tracks} tracks per frame: more than batch_size={batch_size}")
    if tr.skip_absent and tracks is None:
        raise ValueError(f"tracking skip_absent=True leaves out the rows of {what} [N,P,4] that have no face: skipping lives on the "
                         f"faces path, pass [N,1,4] for one track per frame")
    return Namespace(smooth=bool(tr.smooth), fixed=bool(tr.fixed), momentum=m, scale=scale, box_format=tr.box_format, missing=tr.missing,
                     tracks=tracks, detections=n_dets, min_iou=min_iou, max_missed=max_missed, follow_tracks=bool(tr.follow_tracks),
                     skip_absent=bool(tr.skip_absent),
                     feed=BoxFeed(boxes, device, tracks if n_dets is None else n_dets, what))
