"""The value types of the public keywords that are more than a flag (pure Python: importing the package stays cheap)."""
import dataclasses
from collections.abc import Mapping


@dataclasses.dataclass
class ExpressionControls:
    """The `expression=` keyword of InferenceWrapper.animate / animate_frames / animate_streams: what happens to the driver's
    expression vectors between the expression embedder and the render, on the device (ops.expression_controls).  A row is a
    frame, or a face with faces=.
    relative: source expression + (driver_t - driver_first): the driver's resting face stays out of the avatar.
    gain: a float, or one value per row -- damps (< 1) or exaggerates (> 1) the expression about the identity's source expression.
    offset: [E] or [rows,E], added to the expression (an emotion direction, constant or per row).
    smooth, momentum: the smooth_pose recurrence on the expression, e = e * momentum + previous * (1 - momentum), 0 < momentum <= 1.
    override: [rows,E] in place of the expression embedder's output (the batched `custome_target_pose_embed`); the embedder is
        then not run.
    All defaults = no control: nothing is launched and no state is touched."""
    relative: bool = False
    gain: object = 1.0
    offset: object = None
    smooth: bool = False
    momentum: float = 0.5
    override: object = None

    @classmethod
    def of(cls, value):
        """None | ExpressionControls | a mapping with the same fields -> ExpressionControls or None"""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, Mapping):
            unknown = sorted(set(value) - {f.name for f in dataclasses.fields(cls)})
            if unknown:
                raise ValueError(f"expression= has no field {unknown[0]!r}")
            return cls(**value)
        raise ValueError("expression= takes an ExpressionControls or a mapping with its fields")


@dataclasses.dataclass
class HeadPoseControls:
    """The `head_pose=` keyword of InferenceWrapper.animate / animate_frames / animate_streams: what happens to the driver's
    head pose -- the (scale, rotation, translation) the head-pose regressor returns -- before theta is formed, on the device
    (ops.head_pose_controls).  A row is a frame, or a face with faces=.
    relative: source pose + (driver_t - driver_first): the avatar keeps its own head pose and follows the driver's head motion.
    gain: a float, or one value per row -- damps (< 1) or exaggerates (> 1) rotation and translation about the identity's source pose.
    rotation_offset: [3] or [rows,3], yaw, pitch, roll in radians, added to the rotation (the reference's delta_yaw / delta_pitch,
        expression_embedder.py:302-316, plus roll).
    translation_offset: [3] or [rows,3], added to the translation.
    zoom: a float, or one value per row, multiplies the scale.
    frontal: the reference's `normalize`: yaw = pitch = 0 and translation = 0; roll and scale stay the driver's.
    All defaults = no control: nothing is launched and no state is touched."""
    relative: bool = False
    gain: object = 1.0
    rotation_offset: object = None
    translation_offset: object = None
    zoom: object = 1.0
    frontal: bool = False

    @classmethod
    def of(cls, value):
        """None | HeadPoseControls | a mapping with the same fields -> HeadPoseControls or None"""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, Mapping):
            unknown = sorted(set(value) - {f.name for f in dataclasses.fields(cls)})
            if unknown:
                raise ValueError(f"head_pose= has no field {unknown[0]!r}")
            return cls(**value)
        raise ValueError("head_pose= takes a HeadPoseControls or a mapping with its fields")


@dataclasses.dataclass
class CropTracking:
    """The `tracking=` keyword of InferenceWrapper.animate_frames / animate_streams, beside `boxes=`: how the face boxes of a
    detector become crop windows, on the device (ops.crop_track; the arithmetic is crop_image's, notebooks/infer.py:301-352, and
    hostglue.crop_track states it).  A row is a frame, or a track of a frame with boxes [N,P,4].
    smooth: the reference's use_smoothed_crop: an EMA of the box centre and size along each track, started at the track's first box.
    momentum: the EMA's, 0 < momentum <= 1; None = the wrapper's crop momentum (`momentum`, 0.01), what crop_image uses.
    fixed: the reference's fixed_bounding_box: with smooth, every row takes the track's first centre and size.
    scale: multiplies the box size (crop_image's `scale`).
    box_format: 'xyxy' = pixel boxes (x0, y0, x1, y1); 'relative' = mediapipe's (xmin, ymin, width, height) relative to the frame,
        made a pixel box as forward(crop=True) makes it (hostglue.detection_to_face).
    missing: what a row without a usable window is given: 'skip' = it is not pasted (paste_back returns its frame as it came) and
        is rendered, where crops are returned, from the centred square of its frame; 'hold' = the track's last window, where it
        has one that fits the row's frame.
    tracks, min_iou, max_missed: for `detections=` only (unordered detections [N,D,4] in place of boxes=; ops.track_assign,
        hostglue.track_assign states it).  tracks = P, the number of track slots per frame, 1 ... min(16, batch_size): column p of
        the rows is one face from frame to frame, rendered as the identity given for column p.  A detection continues the track
        whose last matched box it overlaps most, if their IoU is at least min_iou (in (0, 1]); a track that finds no detection
        for more than max_missed consecutive frames is dropped and its slot is free for the next new face.  0.3 and 15 are
        taste defaults, not measured optima.
    follow_tracks: animate_frames only.  The per-identity control streams -- the smooth_pose EMA, the expression controls' relative
        anchor and EMA, the head-pose controls' relative anchor -- follow the tracks: a row at which detections= restarts its track
        (a birth, a death) first restarts the stream its identity walks, and a row without a face (a paste window of side 0) is
        still rendered, from a copy of the stream's state, but leaves no mark on the stream: it is neither an anchor nor a step of
        an EMA.  False: every row enters its stream, as before the field existed.
    skip_absent: animate_frames only, with boxes [N,P,4] or detections=.  A row without a face (a paste window of side 0) is not
        cropped, not embedded, not rendered, not refined and not returned: one more launch per chunk (ops.present_rows,
        hostglue.present_rows states it) puts the present rows first, the number of faces of every frame comes to the host (the
        one host wait per chunk the field adds), and the batches hold at most batch_size present rows.  The controls still run
        over all rows of a batch's frames, so a control that carries state needs follow_tracks=True beside it.  False: every
        row is rendered, as before the field existed.
    All defaults = the reference's per-frame window (use_smoothed_crop=False)."""
    smooth: bool = False
    momentum: object = None
    fixed: bool = False
    scale: float = 1.0
    box_format: str = "xyxy"
    missing: str = "skip"
    tracks: object = None
    min_iou: float = 0.3
    max_missed: int = 15
    follow_tracks: bool = False
    skip_absent: bool = False

    @classmethod
    def of(cls, value):
        """None | CropTracking | a mapping with the same fields -> CropTracking or None"""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, Mapping):
            unknown = sorted(set(value) - {f.name for f in dataclasses.fields(cls)})
            if unknown:
                raise ValueError(f"tracking= has no field {unknown[0]!r}")
            return cls(**value)
        raise ValueError("tracking= takes a CropTracking or a mapping with its fields")
