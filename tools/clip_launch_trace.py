"""What the video paths do between their checks and their yields, as a record that can be held against another commit's.

InferenceWrapper.animate_frames / animate / animate_streams run as they are on the bare wrapper of tests/bare_wrapper.py: CPU
tensors, the host-compiled kernels (tests/emul/emulibs.stream), the head-pose regressor and the expression embedder fixed
functions of the crop, the driver pass a recorder, the uploads plain copies.  Every combination of keywords of COMBOS runs on one
rank and on two (two spawned processes, gloo), with the crop budget EMO_SMOOTH_KEEP_GB at its default and at 0 (the budget is
read at import: it is set in the child's environment).  A run leaves, per combination:
  events   in call order: the name of every C entry called; ["head_pose" | "expression" | "drive", rows] from the stand-ins;
           ["upload", frames] from frames.uploaded / uploaded_mixed; ["gather", local rows, total rows] from parallel.gather_rows
  rows     the (pose, theta) of every row handed to the driver pass, in the order of the rank's rows
  states   every array of _bank_streams, _stream and _crop_streams after the call
  yields   what the generator yielded, and whether the caller's frames are as they were
Only the events go into the fixture tests/golden/clip_launch_trace.json -- names and integers, no float and no hash of one (the
host-compiled kernels may round differently on another CPU); tests/test_clip_launch_trace.py holds the rest of one run against
another of the same session.

    python tools/clip_launch_trace.py                  the fixture, to stdout
    python tools/clip_launch_trace.py --write [PATH]   the fixture, to a file (default: the committed one)
    python tools/clip_launch_trace.py --list           the keys
"""
import json
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emul")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "clip_launch_trace.json")
N, HW, CHUNKS, BATCH, K, E = 13, (16, 16), (7, 6), 3, 3, 6
IDS = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]
# 0, 1 or 2 faces per frame: batches of whole frames, one of them without a face on one rank (frames 3 ... 5) and on two (frame 3)
FACE_COUNTS = [1, 2, 0, 0, 0, 0, 1, 2, 1, 0, 1, 2, 1]
FACE_IDS = [0, 1, 2, 0, 1, 2, 2, 0, 1, 1, 0]
RUNS = ((1, "default"), (1, "0"), (2, "default"), (2, "0"))          # (world, EMO_SMOOTH_KEEP_GB)
# two tracks per frame (boxes [N,2,4], detections= with tracks=2), the rows without a face planted: MISSING[frame] = its tracks without
# a box, KEPT_COUNTS[frame] = 2 - their number, written out.  In batches of 3 kept rows / 3 frames and chunks of 7 + 6 that leaves the
# frames 3 ... 5 a batch of their own on one rank and frame 3 one on rank 0 of two, and nobody in rank 1's shard of the second chunk
# (frames 10 ... 12); tests/test_clip_launch_trace.py asserts it
MISSING = {0: (1,), 1: (0,), 2: (1,), 3: (0, 1), 4: (0, 1), 5: (0, 1), 8: (0,), 10: (0, 1), 11: (0, 1), 12: (0, 1)}
KEPT_COUNTS = [1, 1, 1, 0, 0, 0, 2, 2, 1, 2, 0, 0, 0]
TRACK_IDS = [0, 2] * N                                                # one slot per row: track p of every frame is one identity
# detections=: which frames each face is seen in and where.  With max_missed=1 A's track (slot 0) dies in frame 3 and B's (slot 1) in
# frame 4, both in frames nobody is in; C and D are born in frame 6 into the slots they freed and stay to the end (so every stream
# ends with a state that can be compared), C dropping out in frame 8.  SEEN_COUNTS[frame] = the faces seen in it, written out
SEEN = dict(A=((0, 1), (1, 1, 8, 8)), B=((2,), (8, 7, 15, 15)), C=((6, 7, 9, 10, 11, 12), (1, 6, 9, 14)),
            D=((6, 7, 8, 9, 10, 11, 12), (8, 1, 15, 8)))
SEEN_COUNTS = [1, 1, 1, 0, 0, 0, 2, 2, 1, 2, 2, 2, 2]


class _Resident(torch.Tensor):
    """a chunk that says it lies on the device: the clip loop then clones the spans it pastes into"""
    is_cuda = property(lambda self: True)


def _clip(n, hw, seed):
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _chunks(t):
    return iter(torch.split(t, CHUNKS))


def _faces():
    g = torch.Generator().manual_seed(7)
    out = []
    for c in FACE_COUNTS:
        of_frame = []
        for _ in range(c):
            side = int(torch.randint(6, 13, (1,), generator=g))
            x, y = (int(v) for v in torch.randint(0, 17 - side, (2,), generator=g))
            of_frame.append((x, y, side))
        out.append(of_frame)
    return out


def _boxes(n, tracks=None, seed=11):
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if tracks is None else (n, tracks)
    lo = torch.rand(shape + (2,), generator=g, dtype=torch.float64) * 5 + 1
    side = torch.rand(shape + (1,), generator=g, dtype=torch.float64) * 4 + 5
    return torch.cat([lo, lo + side], dim=-1)


def _dropout_boxes():
    """boxes [N,2,4] of two faces, NaN where MISSING says the track has none"""
    boxes = _boxes(N, 2)
    for frame, tracks in MISSING.items():
        boxes[frame, list(tracks)] = float("nan")
    return boxes


def _detections():
    """detections [N,4,4] of the faces of SEEN, each drifting a little, in a shuffled order per frame, NaN rows the padding"""
    g = torch.Generator().manual_seed(17)
    dets = torch.full((N, 4, 4), float("nan"), dtype=torch.float64)
    for t in range(N):
        at = torch.randperm(4, generator=g).tolist()
        for k, (frames, box) in enumerate(SEEN.values()):
            if t in frames:
                dets[t, at[k]] = torch.tensor(box, dtype=torch.float64) + 0.05 * t
    return dets


def _per_row(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * 2, 0.2 * torch.randn(n, 3, generator=g)


def _frames_combo(counts=None, **kw):
    """an animate_frames call over the 13-frame clip in chunks of 7 + 6; counts: the rows of every frame (None: one)"""
    def call(w):
        clip = _clip(N, HW, 80)
        kw_ = dict(kw)
        frames = clip.as_subclass(_Resident) if kw_.pop("resident", False) else clip
        for name in ("boxes", "detections"):
            if isinstance(kw_.get(name), torch.Tensor):
                kw_[name] = _chunks(kw_[name])
        return w.animate_frames(_chunks(frames), batch_size=kw_.pop("batch_size", BATCH), to_host=False, **kw_), [clip, clip.clone()]
    return dict(call=call, counts=counts or [1] * N, chunks=CHUNKS, paste=bool(kw.get("paste_back")))


def _animate_combo(**kw):
    def call(w):
        g = torch.Generator().manual_seed(90)
        pose = torch.randn(N, E, generator=g)
        srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.9 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
        return w.animate(pose, srt, batch_size=BATCH, as_uint8=False, **kw), None
    return dict(call=call, counts=[1] * N, chunks=(N,), paste=False)


def _streams_combo():
    def call(w):
        a, b = _clip(5, (16, 16), 85), _clip(3, (20, 24), 86)
        gain, rot = _per_row(3, 87)
        streams = [dict(frames=iter([a[:2], a[2:]]), boxes=_boxes(5, seed=12), identities=0, head_pose=dict(gain=0.5)),
                   dict(frames=b, boxes=_boxes(3, seed=13), identities=[1, 2, 1], head_pose=dict(gain=gain, rotation_offset=rot))]
        return w.animate_streams(streams, batch_size=BATCH, to_host=False, as_uint8=False, smooth_pose=True, tracking=dict(smooth=True),
                                 head_pose=dict(relative=True, zoom=1.1)), None
    return dict(call=call, counts=None, chunks=None, paste=False, local=True)


def _combos():
    gain, rot = _per_row(N, 81)
    over = torch.randn(N, E, generator=torch.Generator().manual_seed(82))
    per_id = dict(smooth_pose=True, smooth_per_identity=True)
    faces7 = dict(faces=_faces(), identities=FACE_IDS, head_pose=dict(relative=True), expression=dict(relative=True), mix=True, **per_id)
    f32 = dict(as_uint8=False)
    over2 = torch.randn(2 * N, E, generator=torch.Generator().manual_seed(83))
    tracked = dict(identities=TRACK_IDS, expression=dict(relative=True, smooth=True), head_pose=dict(relative=True), **per_id)
    return {
        "1 identities, head_pose relative per row, expression relative smooth gain, smooth_pose, mix": _frames_combo(
            identities=IDS, head_pose=dict(relative=True, gain=gain, rotation_offset=rot),
            expression=dict(relative=True, smooth=True, gain=0.8), mix=True, **per_id, **f32),
        "2 identities, head_pose frontal zoom, expression relative, mix": _frames_combo(
            identities=IDS, head_pose=dict(frontal=True, zoom=1.2), expression=dict(relative=True), mix=True, **f32),
        "3 identities, expression smooth override": _frames_combo(identities=IDS, expression=dict(smooth=True, override=over), **f32),
        "4 identities, head_pose relative": _frames_combo(identities=IDS, head_pose=dict(relative=True), **f32),
        "5 identities, expression relative, smooth_pose": _frames_combo(identities=IDS, expression=dict(relative=True), **per_id, **f32),
        "6 boxes [N,4] smoothed, expression smooth, smooth_pose": _frames_combo(
            boxes=_boxes(N), tracking=dict(smooth=True), expression=dict(smooth=True), smooth_pose=True, **f32),
        "7 faces, identities, head_pose relative, expression relative, smooth_pose, mix": _frames_combo(FACE_COUNTS, **faces7, **f32),
        "8 faces as 7, paste_back": _frames_combo(FACE_COUNTS, paste_back=True, **faces7),
        "9 windows, paste_back, resident chunk, identities, smooth_pose": _frames_combo(
            windows=[(i % 4, (2 * i) % 5, 8 + i % 5) for i in range(N)], paste_back=True, resident=True, identities=IDS, **per_id),
        "10 boxes [N,2,4], identities, expression relative, smooth_pose": _frames_combo(
            [2] * N, boxes=_boxes(N, 2), batch_size=4, identities=(IDS + IDS[::-1]), expression=dict(relative=True), **per_id, **f32),
        "11 animate, identities, head_pose, expression, smooth_pose": _animate_combo(
            identities=IDS, head_pose=dict(relative=True, gain=gain), expression=dict(relative=True, smooth=True), mix=True, **per_id),
        "12 animate, head_pose, expression, smooth_pose": _animate_combo(
            head_pose=dict(relative=True, gain=gain), expression=dict(relative=True, smooth=True), smooth_pose=True),
        "13 animate_streams, two frame sizes, boxes, smooth_pose, per-stream head_pose": _streams_combo(),
        "14 boxes [N,2,4] with dropouts, follow_tracks, head_pose relative, expression relative smooth, smooth_pose": _frames_combo(
            [2] * N, boxes=_dropout_boxes(), tracking=dict(follow_tracks=True, smooth=True), **tracked, **f32),
        "15 as 14, skip_absent": _frames_combo(
            KEPT_COUNTS, boxes=_dropout_boxes(), tracking=dict(follow_tracks=True, smooth=True, skip_absent=True), **tracked),
        "16 detections [N,4,4] shuffled, tracks=2 max_missed=1, follow_tracks, skip_absent, controls as 14, paste_back": _frames_combo(
            SEEN_COUNTS, detections=_detections(), tracking=dict(tracks=2, follow_tracks=True, skip_absent=True, max_missed=1),
            paste_back=True, **tracked),
        "17 as 15, expression override over the full rows, mix": _frames_combo(
            KEPT_COUNTS, boxes=_dropout_boxes(), tracking=dict(follow_tracks=True, smooth=True, skip_absent=True), mix=True,
            **dict(tracked, expression=dict(relative=True, smooth=True, override=over2))),
    }


COMBOS = tuple(_combos())


def expected_rows(combo, world, rank):
    """the rows of the call that `rank` of `world` renders, in its order: per chunk, the rows of its shard of the chunk's frames"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import parallel
    c = _combos()[combo]
    first, rows, base = frames_mod.face_offsets(c["counts"]), [], 0
    for n in c["chunks"]:
        lo, hi = parallel.shard_range(n, rank, world)
        rows += range(first[base + lo], first[base + hi])
        base += n
    return rows


class _Builds:
    """the association and the compaction (a wave exchange, a block barrier) from the threaded host build, every other entry point from
    the loop build, which runs the crops and the pastes of whole frames in reasonable time"""
    THREADED = ("emo_track_assign_f64", "emo_present_rows_i32")

    def __init__(self, loop, threads):
        self._loop, self._threads = loop, threads

    def __getattr__(self, name):
        return getattr(self._threads if name in self.THREADED else self._loop, name)


def _rig(patch, rank, world):
    """the wrapper of one combination: a filled 3-slot bank and a current identity, the stand-ins writing their events into
    w.lib.order between the C entries"""
    import bare_wrapper
    import emulibs
    from counting_lib import CountingLib
    from emoportraits_amd import ops, parallel
    lib = CountingLib(_Builds(emulibs.stream(False), emulibs.stream(True)))
    events = lib.order
    bare_wrapper.host_uploads(patch, lambda n: events.append(("upload", n)))
    w = bare_wrapper.bare_wrapper(patch, lib, K, lpe_output_channels_expression=E)
    w.rank, w.world = rank, world
    g = torch.Generator().manual_seed(70)
    sources = torch.cat([1 + 0.1 * torch.randn(K, 3, generator=g), 0.4 * torch.randn(K, 3, generator=g), 0.05 * torch.randn(K, 3, generator=g)], 1)
    neutrals = torch.randn(K, E, generator=g)
    thetas = ops.pose_theta(*(sources[:, i:i + 3].contiguous() for i in (0, 3, 6)))
    for k in range(K):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), thetas[k], neutrals[k], sources[k])
    w._canonical_cl = torch.zeros(1, 2, 2, 2, 4)
    w.pred_source_theta, w.pred_source_pose_embed, w.pred_source_srt = thetas[:1].clone(), neutrals[:1].clone(), sources[:1].clone()

    def head_pose(crops):
        events.append(("head_pose", crops.shape[0]))
        f = crops.flatten(1)[:, 3::17][:, :9] - 0.5
        srt = (1 + 0.2 * f[:, 0:3]).contiguous(), (4.0 * f[:, 3:6]).contiguous(), (0.2 * f[:, 6:9]).contiguous()
        return (ops.pose_theta(*srt),) + srt

    def expression(crops, theta, what):
        events.append(("expression", crops.shape[0]))
        return (crops.flatten(1)[:, 5::31][:, :E] * 4 - 2 + theta.flatten(1)[:, :E]).contiguous(), None     # (what it aligns by shows)
    record = w._drive_bank

    def drive(pose, theta, ident=None):
        events.append(("drive", pose.shape[0]))
        return record(pose, theta, ident)
    w._head_pose, w._expression, w._drive_bank, w._drive = head_pose, expression, drive, lambda pose, theta: drive(pose, theta)
    gather_rows = parallel.gather_rows

    def gather(local, counts, rank=None, world=None):
        events.append(("gather", local.shape[0], sum(int(c) for c in counts)))
        return gather_rows(local, counts, rank, world)
    patch.setattr(parallel, "gather_rows", gather)
    lib.calls.clear()
    return w


def _arrays(w):
    out = []
    for st in (w._bank_streams, w._stream):
        out += [getattr(st, name) for name in ("theta", "theta_has", "pose_anchor", "pose_anchor_has", "expr_anchor", "expr_anchor_has",
                                               "expr_ema", "expr_ema_has")]
    cs = w._crop_streams
    out += [None] * 3 if cs is None else [cs.state, cs.has, cs.last]
    return [None if t is None else t.numpy().copy() for t in out]


def run_combo(combo, rank=0, world=1):
    """one combination on a fresh rig -> dict(events, rows, states, yields, untouched)"""
    import pytest
    c = _combos()[combo]
    with pytest.MonkeyPatch.context() as patch:
        w = _rig(patch, rank if not c.get("local") else 0, world if not c.get("local") else 1)
        gen, frames = c["call"](w)
        yields = []
        for item in gen:
            if isinstance(item, list):                                           # (animate_streams: [(stream, frame, out)])
                yields += [((s, t), out.numpy().copy()) for s, t, out in item]
            else:
                yields.append((item[0], item[1].numpy().copy()))
        events = [e if isinstance(e, str) else list(e) for e in w.lib.order]
        rows = (torch.cat([r[0] for r in w.recorded]).numpy(), torch.cat([r[1] for r in w.recorded]).numpy())
        return dict(events=events, rows=rows, states=_arrays(w), yields=yields,
                    untouched=frames is None or torch.equal(frames[0], frames[1]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), EMO_PIN_CORES="0")
    torch.set_num_threads(1)
    if world > 1:
        torch.distributed.init_process_group(backend="gloo", init_method="env://")
    out = {}
    for combo in COMBOS:
        if world == 1 or not _combos()[combo].get("local"):
            out[combo] = run_combo(combo, rank, world)
    q.put((world, os.environ["EMO_SMOOTH_KEEP_GB"], rank, out))
    if world > 1:
        torch.distributed.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_all():
    """every combination at every (world, budget) of RUNS, each rank a spawned process -> {(world, budget, rank): {combo: run_combo's}}"""
    import emulibs
    emulibs.stream(False), emulibs.stream(True)                                  # (built once, before the children load them)
    ctx = mp.get_context("spawn")
    q, procs, before = ctx.Queue(), [], os.environ.get("EMO_SMOOTH_KEEP_GB")
    try:
        for world, keep in RUNS:
            os.environ["EMO_SMOOTH_KEEP_GB"] = "16" if keep == "default" else keep
            port = _free_port()
            for rank in range(world):
                procs.append(ctx.Process(target=_worker, args=(rank, world, port, q)))
                procs[-1].start()
    finally:
        if before is None:
            os.environ.pop("EMO_SMOOTH_KEEP_GB", None)
        else:
            os.environ["EMO_SMOOTH_KEEP_GB"] = before
    out = {}
    for _ in procs:
        world, keep, rank, res = q.get(timeout=300)
        out[(world, "default" if keep == "16" else keep, rank)] = res
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0, f"a rank ended with {p.exitcode}"
    return out


def key(combo, world, keep, rank):
    return f"{combo} | world {world} rank {rank} keep {keep}"


def traces(runs):
    """the fixture of run_all()'s result: {key: events}, in the order of COMBOS and RUNS"""
    return {key(combo, world, keep, rank): runs[(world, keep, rank)][combo]["events"]
            for combo in COMBOS for world, keep in RUNS for rank in range(world) if combo in runs[(world, keep, rank)]}


def dumps(fixture):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in fixture.items()) + "\n}\n"


def main(argv):
    if "--list" in argv:
        print("\n".join(key(c, w, k, r) for c in COMBOS for w, k in RUNS for r in range(w) if w == 1 or not _combos()[c].get("local")))
        return
    text = dumps(traces(run_all()))
    if "--write" in argv:
        at = argv.index("--write") + 1
        with open(argv[at] if at < len(argv) else FIXTURE, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
