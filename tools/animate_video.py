"""Frames in -> frames out through the device-resident path (the reference loops
`InferenceWrapper.forward(driver_image=frame)` over decoded video frames, notebooks/infer.py:511-644).

    python tools/animate_video.py --project <project_dir> --experiment <exp> --checkpoint <file> \
        --source source.png --frames <dir of PNG/JPG frames | frames.npy (uint8 [N,H,W,3])> --out <dir> [--batch 16]
        [--windows windows.json]   # optional per-frame crop windows [[x_lo, y_lo, side], ...] from a face detector
        [--faces faces.json [--sources a.png,b.png --identities ids.json]]   # several faces per frame: [[[x_lo, y_lo, side], ...],
         ...], one list per frame in paste order ([]: no face); --sources enrols several source images into an identity bank
         (slots 0, 1, ... in that order) and ids.json names the slot of every face, flattened in frame order
        [--mix [--mix-new]] [--source-pose] [--smooth-pose]   # forward()'s pose controls (mix, mix_old=False, target_theta=False)
        [--relative-pose] [--pose-gain G] [--yaw R --pitch R --roll R] [--pose-zoom Z] [--frontal]   # the head-pose controls
         (animate_frames' head_pose=): keep the avatar's own head pose and follow the driver's motion, damp it, turn the head, look ahead
        [--boxes boxes.json|.npy|.pt [--box-format relative] [--smooth-crop [--crop-momentum M] [--fixed-crop]] [--crop-scale S]
         [--hold-missing]]   # in place of --windows / --faces: the detector's face boxes, [N,4] (x0, y0, x1, y1) in pixels (or mediapipe's
         relative (xmin, ymin, width, height)), or [N,P,4] for P tracks per frame; the windows are formed on the device
         (animate_frames' boxes= / tracking=: crop_image's arithmetic with its smoothed-crop tracker); a frame whose box is NaN has
         no face: it is not pasted, or with --hold-missing pasted at the track's last window
        [--detections dets.json|.npy|.pt --tracks P [--min-iou X] [--max-missed N]]   # in place of --boxes, with its options: the
         detector's output as it comes, up to 32 boxes per frame in no stable order ([N,D,4], or a JSON list per frame of any length:
         rows are padded with NaN); they are associated to P track slots on the device (animate_frames' detections=), and track p is
         rendered as the identity that --identities names for column p
        [--follow-tracks]   # with --boxes / --detections: --smooth-pose, --relative-expression / --smooth-expression and
         --relative-pose follow the face tracks (tracking follow_tracks=True): a new face in a freed slot starts its own streams, and a
         frame without a face leaves no mark on them
        [--skip-absent]     # with --boxes [N,P,4] / --detections: a track slot without a face is not rendered (tracking
         skip_absent=True); the controls that carry state then need --follow-tracks
        [--paste-back [--feather F]]   # with --windows: write the FULL frames, the rendered head pasted back where its window was
        [--stage2-experiment <exp2> --stage2-checkpoint <file> [--cloth]       # refine every batch with the stage-2 model
         (--embedders module:factory | --refine-everywhere)]                   # (<project>/logs_s2/<exp2>), inside the same path
        [--frame-format nv12|yuv420p|p010|yuv420p10 --frame-size WxH [--colorspace bt709|bt601] [--full-range]]   # raw NV12 video in and out:
         --frames clip.nv12 (or .yuv) as `ffmpeg -pix_fmt nv12 -f rawvideo` writes it; --out a file, raw NV12 of the frames
         (with --paste-back) or of the crops, which e.g. `ffmpeg -f rawvideo -pix_fmt nv12 -s WxH -i <out>` reads back

Frame I/O is host work (PIL / numpy): decoded frames are handed to InferenceWrapper.animate_frames as uint8 chunks in pinned
memory; crop, bicubic resize, both embedders, the hot path and the uint8 packing run on the GPU without a host sync, and
finished batches come back through the pinned D2H ring while the next ones are being computed.  Face detection, parsing
and matting are third-party networks without sources in the reference tree: the source image must come with its mask
(--source-mask, default all ones) and crop windows, if any, are precomputed.  For the same reason stage 2's matte (MODNet)
and face mask (BiSeNet) come from the caller: --embedders names a `module:factory` whose call returns {'matting': fn,
'face_parsing': fn}, each img [b,3,S2,S2] -> [b,1,S2,S2] on the device; --refine-everywhere sets both masks to ones (the
residual is then added over the whole crop, background included).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_frames(path, chunk):
    """yields pinned uint8 [n,H,W,3] chunks"""
    if path.endswith(".npy"):
        arr = np.load(path, mmap_mode="r")
        for a in range(0, arr.shape[0], chunk):
            yield torch.from_numpy(np.ascontiguousarray(arr[a:a + chunk])).pin_memory()
        return
    from PIL import Image
    names = sorted(f for f in os.listdir(path) if f.lower().endswith((".png", ".jpg", ".jpeg")))
    for a in range(0, len(names), chunk):
        imgs = [np.asarray(Image.open(os.path.join(path, f)).convert("RGB")) for f in names[a:a + chunk]]
        yield torch.from_numpy(np.stack(imgs)).pin_memory()


def load_nv12(path, width, height, chunk, frame_format="nv12"):
    """yields pinned uint8 [n, 3H/2, W] chunks of a raw NV12 file (frame after frame: H rows of Y, H/2 rows of interleaved U, V);
    frame_format 'yuv420p': the same of a planar file (H rows of Y, the U plane, the V plane); 'p010' / 'yuv420p10': uint16
    chunks of a file of 16-bit little-endian samples -- a frame is 3HW/2 samples of 1 or 2 bytes"""
    dtype = np.dtype("<u2") if frame_format in ("p010", "yuv420p10") else np.dtype(np.uint8)
    per = width * height * 3 // 2 * dtype.itemsize
    size = os.path.getsize(path)
    if size == 0 or size % per:
        raise SystemExit(f"{path}: {size} bytes is not a whole number of {width}x{height} {frame_format.upper() if frame_format == 'nv12' else frame_format} "
                         f"frames of {per} bytes")
    arr = np.memmap(path, dtype=dtype, mode="r").reshape(-1, 3 * height // 2, width)
    for a in range(0, arr.shape[0], chunk):
        yield torch.from_numpy(np.array(arr[a:a + chunk])).pin_memory()          # (a copy: the map is read-only)


def load_boxes(path):
    """face boxes [N,4] or [N,P,4] from a .pt, .npy or .json file as a floating-point tensor; a JSON null is a missing coordinate
    (NaN: a frame whose box is [null, null, null, null] has no face)"""
    if path.endswith(".pt"):
        t = torch.load(path, map_location="cpu")
    elif path.endswith(".npy"):
        t = torch.from_numpy(np.load(path))
    else:
        t = torch.from_numpy(np.array(json.load(open(path)), dtype=np.float64))
    return t if t.dtype in (torch.float32, torch.float64) else t.double()


def load_detections(path):
    """detections [N,D,4] from a .pt, .npy or .json file; a JSON file may hold a list of any length per frame ([]: nobody), which
    is padded to the longest with NaN rows"""
    if not path.endswith(".json"):
        return load_boxes(path)
    frames = json.load(open(path))
    D = max(1, max((len(f) for f in frames), default=1))
    out = np.full((len(frames), D, 4), np.nan)
    for i, f in enumerate(frames):
        for j, box in enumerate(f):
            out[i, j] = [np.nan if v is None else v for v in box]
    return torch.from_numpy(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--project", required=True)
    ap.add_argument("--experiment", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--folder", default="logs")
    ap.add_argument("--head-pose-regressor", default=None)
    ap.add_argument("--source", required=True)
    ap.add_argument("--source-mask", default=None)
    ap.add_argument("--frames", required=True)
    ap.add_argument("--windows", default=None)
    ap.add_argument("--faces", default=None, help="several faces per frame: a JSON list per frame of [x_lo, y_lo, side], in paste order")
    ap.add_argument("--boxes", default=None, help="face boxes [N,4] (or [N,P,4]) as .json, .npy or .pt: windows formed on the device")
    ap.add_argument("--box-format", default="xyxy", choices=["xyxy", "relative"], help="pixel (x0, y0, x1, y1), or mediapipe's relative box")
    ap.add_argument("--smooth-crop", action="store_true", help="the reference's use_smoothed_crop: an EMA of the box centre and size")
    ap.add_argument("--crop-momentum", type=float, default=None, help="with --smooth-crop: 0 < M <= 1 (default: the wrapper's 0.01)")
    ap.add_argument("--fixed-crop", action="store_true", help="with --smooth-crop: every frame takes the first box (fixed_bounding_box)")
    ap.add_argument("--crop-scale", type=float, default=1.0, help="multiplies the box size (crop_image's scale)")
    ap.add_argument("--hold-missing", action="store_true", help="a frame without a usable box takes the track's last window")
    ap.add_argument("--detections", default=None, help="unordered detections [N,D,4] (or a JSON list per frame) in place of --boxes: "
                                                       "associated to --tracks track slots on the device")
    ap.add_argument("--tracks", type=int, default=None, help="with --detections: P, the track slots per frame (<= 16 and <= --batch)")
    ap.add_argument("--min-iou", type=float, default=0.3, help="with --detections: a detection continues a track from this IoU on")
    ap.add_argument("--max-missed", type=int, default=15, help="with --detections: frames a track may go without a detection")
    ap.add_argument("--follow-tracks", action="store_true", help="with --boxes / --detections: the pose and expression streams restart at a "
                                                                 "track's birth and skip the frames without a face")
    ap.add_argument("--skip-absent", action="store_true", help="with --boxes [N,P,4] / --detections: render only the track slots that hold "
                                                               "a face")
    ap.add_argument("--sources", default=None, help="comma-separated source images enrolled into bank slots 0, 1, ... (--identities)")
    ap.add_argument("--identities", default=None, help="JSON list: the bank slot of every frame, or with --faces of every face")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--graphs", action="store_true")
    ap.add_argument("--mix", action="store_true", help="keep the source's face stretch, take the driver's rotation + translation")
    ap.add_argument("--mix-new", action="store_true", help="with --mix: the reference's mix_old=False formula")
    ap.add_argument("--source-pose", action="store_true", help="render in the source's own head pose (target_theta=False)")
    ap.add_argument("--smooth-pose", action="store_true", help="EMA over the driver head poses (smooth_pose=True)")
    ap.add_argument("--relative-expression", action="store_true",
                    help="relative expression transfer: source expression + (driver_t - driver_first)")
    ap.add_argument("--expression-gain", type=float, default=1.0, help="damp (< 1) or exaggerate (> 1) the expression about the source's")
    ap.add_argument("--expression-offset", default=None, help="a .pt file with an [E] row, or one row per frame (face), added to the expression")
    ap.add_argument("--smooth-expression", action="store_true", help="EMA over the expression vectors (see --expression-momentum)")
    ap.add_argument("--expression-momentum", type=float, default=None, help="with --smooth-expression: 0 < M <= 1 (default 0.5)")
    ap.add_argument("--relative-pose", action="store_true", help="relative head pose: source pose + (driver_t - driver_first)")
    ap.add_argument("--pose-gain", type=float, default=1.0, help="damp (< 1) or exaggerate (> 1) the head motion about the source's pose")
    ap.add_argument("--yaw", type=float, default=0.0, help="radians added to the yaw (the reference's delta_yaw)")
    ap.add_argument("--pitch", type=float, default=0.0, help="radians added to the pitch (the reference's delta_pitch)")
    ap.add_argument("--roll", type=float, default=0.0, help="radians added to the roll")
    ap.add_argument("--pose-zoom", type=float, default=1.0, help="multiplies the head pose's scale")
    ap.add_argument("--frontal", action="store_true", help="look straight ahead: yaw = pitch = 0, translation = 0 (the reference's normalize)")
    ap.add_argument("--paste-back", action="store_true", help="write the full frames with the rendered crops pasted back (needs --windows, --faces or --boxes)")
    ap.add_argument("--feather", type=float, default=0.0625, help="with --paste-back: blended edge as a fraction of the window side")
    ap.add_argument("--stage2-experiment", default=None, help="refine with the stage-2 model <project>/logs_s2/<this>")
    ap.add_argument("--stage2-checkpoint", default=None)
    ap.add_argument("--cloth", action="store_true", help="stage 2: no face mask (all ones), as infer_s2.py's cloth=True")
    ap.add_argument("--embedders", default=None, help="module:factory returning {'matting': fn, 'face_parsing': fn} for stage 2")
    ap.add_argument("--refine-everywhere", action="store_true", help="stage 2 with both masks all ones (no matting / parsing nets)")
    ap.add_argument("--frame-format", default="rgb8", choices=["rgb8", "nv12", "yuv420p", "p010", "yuv420p10"],
                    help="a YUV 4:2:0 format (ffmpeg's -pix_fmt names; p010 is p010le, yuv420p10 is yuv420p10le): --frames and --out are raw files")
    ap.add_argument("--frame-size", default=None, help="with --frame-format nv12: WxH of the frames in --frames")
    ap.add_argument("--colorspace", default="bt709", choices=["bt709", "bt601"])
    ap.add_argument("--full-range", action="store_true", help="NV12 in full range (Y 0 ... 255) instead of limited (16 ... 235)")
    a = ap.parse_args()
    nv12 = a.frame_format != "rgb8"                                # (any of the raw YUV 4:2:0 formats)
    if nv12:
        try:
            width, height = (int(v) for v in (a.frame_size or "").lower().split("x"))
        except ValueError:
            ap.error("--frame-format nv12 needs --frame-size WxH")
        if width <= 0 or height <= 0 or width % 2 or height % 2:
            ap.error("--frame-size: NV12 frames have an even width and height")
        if not a.frames.lower().endswith((".nv12", ".yuv", ".p010")):
            ap.error("--frame-format nv12 reads a raw .nv12 / .yuv file")
    elif a.frame_size or a.full_range or a.colorspace != "bt709":
        ap.error("--frame-size / --colorspace / --full-range belong to --frame-format nv12")
    if a.faces and a.windows:
        ap.error("--faces and --windows are mutually exclusive")
    if a.boxes and (a.faces or a.windows):
        ap.error("--boxes (windows formed on the device) and --windows / --faces (ready windows) are mutually exclusive")
    if a.detections and (a.boxes or a.faces or a.windows):
        ap.error("--detections (tracks formed on the device) and --boxes / --windows / --faces are mutually exclusive")
    if bool(a.detections) != (a.tracks is not None) or not a.detections and (a.min_iou != 0.3 or a.max_missed != 15):
        ap.error("--detections and --tracks go together; --min-iou / --max-missed belong to them")
    if not (a.boxes or a.detections) and (a.box_format != "xyxy" or a.smooth_crop or a.fixed_crop or a.crop_scale != 1.0 or a.hold_missing):
        ap.error("--box-format / --smooth-crop / --fixed-crop / --crop-scale / --hold-missing belong to --boxes / --detections")
    if a.follow_tracks and not (a.boxes or a.detections):
        ap.error("--follow-tracks belongs to --boxes / --detections")
    if a.skip_absent and not (a.boxes or a.detections):
        ap.error("--skip-absent belongs to --boxes / --detections")
    if (a.crop_momentum is not None or a.fixed_crop) and not a.smooth_crop:
        ap.error("--crop-momentum / --fixed-crop belong to --smooth-crop")
    if a.crop_momentum is not None and not 0.0 < a.crop_momentum <= 1.0:
        ap.error("--crop-momentum: 0 < M <= 1")
    if (a.sources is None) != (a.identities is None):
        ap.error("--sources (the images of the bank's slots) and --identities (the slot of every face or frame) go together")
    if a.smooth_pose and a.faces and not a.identities:
        ap.error("--smooth-pose with --faces smooths every face track as its identity's stream: it needs --sources / --identities")
    if a.expression_momentum is not None and not a.smooth_expression:
        ap.error("--expression-momentum belongs to --smooth-expression")
    if a.expression_momentum is not None and not 0.0 < a.expression_momentum <= 1.0:
        ap.error("--expression-momentum: 0 < M <= 1")
    if (a.relative_expression or a.smooth_expression) and a.faces and not a.identities:
        ap.error("--relative-expression / --smooth-expression with --faces follow every face track as its identity's stream: "
                 "they need --sources / --identities")
    if a.relative_pose and a.frontal:
        ap.error("--frontal zeroes what --relative-pose transfers: choose one")
    if a.relative_pose and a.faces and not a.identities:
        ap.error("--relative-pose with --faces follows every face track as its identity's stream: it needs --sources / --identities")
    head_pose = dict(relative=a.relative_pose, gain=a.pose_gain, zoom=a.pose_zoom, frontal=a.frontal,
                     rotation_offset=[a.yaw, a.pitch, a.roll] if a.yaw or a.pitch or a.roll else None)
    if a.source_pose and (a.relative_pose or a.frontal or a.pose_gain != 1.0 or a.pose_zoom != 1.0 or head_pose["rotation_offset"]):
        ap.error("--source-pose renders in the source's head pose: nothing of --relative-pose / --pose-gain / --yaw / --pitch / --roll / "
                 "--pose-zoom / --frontal would be rendered")
    sources = a.sources.split(",") if a.sources else []
    refine = a.stage2_experiment is not None
    if refine and (a.stage2_checkpoint is None or (a.embedders is None) == (not a.refine_everywhere)):
        ap.error("--stage2-experiment needs --stage2-checkpoint and one of --embedders module:factory / --refine-everywhere")
    if not refine and (a.stage2_checkpoint or a.embedders or a.refine_everywhere or a.cloth):
        ap.error("--stage2-checkpoint / --embedders / --refine-everywhere / --cloth belong to --stage2-experiment")
    from PIL import Image
    from notebooks.infer import InferenceWrapper
    w = InferenceWrapper(experiment_name=a.experiment, model_file_name=a.checkpoint, project_dir=a.project, folder=a.folder,
                         head_pose_regressor_path=a.head_pose_regressor, use_graphs=a.graphs,
                         identity_capacity=len(sources))
    refine_masks = None
    if refine:
        from notebooks.infer_s2 import InferenceWrapper as InferenceWrapperS2
        embedders = None
        if a.embedders:
            import importlib
            module, _, factory = a.embedders.partition(":")
            embedders = getattr(importlib.import_module(module), factory)()
        else:
            def refine_masks(img):
                ones = torch.ones((img.shape[0], 1) + tuple(img.shape[2:]), device=img.device)
                return ones, ones
        w.attach_stage2(InferenceWrapperS2(experiment_name=a.stage2_experiment, model_file_name=a.stage2_checkpoint,
                                           project_dir=a.project, cloth=a.cloth, embedders=embedders))
    S = w.cfg["image_size"]
    src = Image.open(a.source).convert("RGB")
    mask = torch.ones(1, 1, S, S) if a.source_mask is None else \
        torch.from_numpy(np.asarray(Image.open(a.source_mask).convert("L").resize((S, S)), dtype=np.float32) / 255.0)[None, None]
    w.forward(source_image=src, crop=False, source_mask=mask)
    windows = json.load(open(a.windows)) if a.windows else None
    faces = json.load(open(a.faces)) if a.faces else None
    boxes = tracking = None
    if a.boxes:
        boxes = load_boxes(a.boxes)
        tracking = dict(smooth=a.smooth_crop, momentum=a.crop_momentum, fixed=a.fixed_crop, scale=a.crop_scale, box_format=a.box_format,
                        missing="hold" if a.hold_missing else "skip", follow_tracks=a.follow_tracks, skip_absent=a.skip_absent)
    detections = None
    if a.detections:
        detections = load_detections(a.detections)
        tracking = dict(smooth=a.smooth_crop, momentum=a.crop_momentum, fixed=a.fixed_crop, scale=a.crop_scale, box_format=a.box_format,
                        missing="hold" if a.hold_missing else "skip", tracks=a.tracks, min_iou=a.min_iou, max_missed=a.max_missed,
                        follow_tracks=a.follow_tracks, skip_absent=a.skip_absent)
    identities = None
    if sources:
        w.enrol_identities([Image.open(f).convert("RGB") for f in sources], slots=list(range(len(sources))), batch_size=a.batch)
        identities = json.load(open(a.identities))
    expression = dict(relative=a.relative_expression, gain=a.expression_gain, smooth=a.smooth_expression,
                      momentum=0.5 if a.expression_momentum is None else a.expression_momentum,
                      offset=None if a.expression_offset is None else torch.load(a.expression_offset, map_location="cpu"))
    t0, n = time.perf_counter(), 0
    if nv12:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        frames = load_nv12(a.frames, width, height, 8 * a.batch, a.frame_format)
        sink = open(a.out, "wb")
        fmt = dict(frame_format=a.frame_format, colorspace=a.colorspace, full_range=a.full_range)
    else:
        os.makedirs(a.out, exist_ok=True)
        frames = load_frames(a.frames, 8 * a.batch)
        sink, fmt = None, {}
    # (without --paste-back the crops of --faces come face by face: `first` then counts faces, not frames)
    for first, u8 in w.animate_frames(frames, batch_size=a.batch, windows=windows, faces=faces, identities=identities, mix=a.mix,
                                      mix_old=not a.mix_new, target_theta=not a.source_pose, smooth_pose=a.smooth_pose,
                                      smooth_per_identity=identities is not None, paste_back=a.paste_back,
                                      feather=a.feather, refine=refine, refine_masks=refine_masks, expression=expression,
                                      head_pose=head_pose, boxes=boxes, tracking=tracking, detections=detections, **fmt):
        arr = u8.numpy()
        if nv12:
            sink.write(arr.tobytes())                             # batches come in frame order (one rank)
        else:
            for j in range(arr.shape[0]):
                Image.fromarray(arr[j]).save(os.path.join(a.out, f"{first + j:06d}.png"))
        n += arr.shape[0]
    if sink is not None:
        sink.close()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(frames=n, seconds=round(dt, 3), fps=round(n / dt, 2), image_size=S, batch=a.batch, refine=refine)))


if __name__ == "__main__":
    main()
