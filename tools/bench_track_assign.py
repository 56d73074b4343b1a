"""Frames/s of InferenceWrapper.animate_frames fed with a detector's unordered output (detections=: one launch of ops.track_assign
per chunk in front of the crop tracker's) against the same call with boxes=[N,2,4] holding the same two tracks in order.

    python tools/bench_track_assign.py [--reps 2] [--frames 384] [--crops] [--out profiles/track_assign_bench.jsonl]

Released architecture at R512 with seeded weights (as tools/bench_crop_track.py), hipGraph replay, B = 16, 1080p uint8 frames in
pinned host memory -> the frames with both rendered heads pasted back, in pinned host memory (--crops: the crops instead), one
identity.  Two faces wander about the left and the right half of the frame; the detections are those two boxes at a random two of
D = 4 rows per frame, the other rows NaN.  Settings, alternated A B A2, A B A2 ... in one process:
    A    boxes=<the ordered [N,2,4]>, tracking=dict(smooth=True, momentum=0.5)
    B    detections=<the permuted [N,4,4]>, tracking=dict(smooth=True, momentum=0.5, tracks=2, min_iou=0.2)
    A2   A once more: the A/A pair of the repetition
Every repetition writes one JSONL record, and a last record sums up: `a_spread` = max(A, A2) / min(A, A2) - 1 over all repetitions
is the run-to-run spread of A against A on this box, `a2_over_a` the ratio of the means of the pair, `b_over_a` the ratio of B's
mean to the mean of A and A2.  The claim to check is that B is not distinguishable from A beyond `a_spread`.  --parent measures A
alone: this file copied into a checkout of the parent commit gives the parent's frames/s for the same boxes= call on the same box.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emoportraits_amd import config, random_init  # noqa: E402
from emoportraits_amd import embedders as E  # noqa: E402
from emoportraits_amd.infer import InferenceWrapper  # noqa: E402

MOMENTUM, MIN_IOU, TRACKS, D = 0.5, 0.2, 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=384)
    ap.add_argument("--crops", action="store_true", help="yield the crops instead of the pasted frames")
    ap.add_argument("--parent", action="store_true", help="a checkout without detections=: measure A alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_assign_bench.jsonl"))
    a = ap.parse_args()
    S, B, H, W = 512, 16, 1080, 1920
    cfg = config.hot_path_config(overrides={"image_size": S})
    ecfg = E.embedder_config()
    sd = random_init.random_state_dict(cfg, seed=0)
    sd.update(E.random_state_dict(E.idt_schema(ecfg), 1))
    sd.update(E.random_state_dict(E.expression_schema(ecfg), 2))
    hp_sd = E.random_state_dict(E.head_pose_schema(), 3)
    hp_sd["fc.weight"] *= 0.05
    hp_sd["fc.bias"] = torch.tensor([1.0, 1.0, 1.0, 0.1, -0.2, 0.05, 0.02, -0.03, 0.01])
    root = tempfile.mkdtemp()
    os.makedirs(os.path.join(root, "logs", "exp", "checkpoints"))
    with open(os.path.join(root, "logs", "exp", "args.txt"), "wt") as f:
        for k, v in {**cfg, **ecfg}.items():
            f.write(f"{k}: {v}\n")
    torch.save(hp_sd, os.path.join(root, "hp.pth"))
    w = InferenceWrapper(experiment_name="exp", model_file_name="x", project_dir=root, folder="logs", state_dict=sd,
                         print_params=False, head_pose_regressor_path=os.path.join(root, "hp.pth"), use_graphs=True)
    g = torch.Generator().manual_seed(5)
    w.forward(source_image=torch.rand(1, 3, S, S, generator=g), crop=False, source_mask=torch.ones(1, 1, S, S))
    n = a.frames - a.frames % B
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
    rng = np.random.default_rng(6)
    tracks = []
    for at in (0.3, 0.7):                                         # a face in the left and one in the right half: they never overlap
        cx = W * (at + 0.01 * rng.standard_normal(n)).clip(at - 0.03, at + 0.03)
        cy = H * (0.5 + 0.015 * rng.standard_normal(n)).clip(0.46, 0.54)
        half = rng.uniform(0.13, 0.16, (2, n)) * H
        tracks.append(np.stack([cx - half[0], cy - half[1], cx + half[0], cy + half[1]], 1))
    boxes = np.stack(tracks, 1)                                   # [n,2,4]
    dets = np.full((n, D, 4), np.nan)
    for t in range(n):
        dets[t, np.arange(TRACKS) if t == 0 else rng.permutation(D)[:TRACKS]] = boxes[t]
    if not a.parent:                       # the association gives the ordered boxes back: both settings render the same faces
        from emoportraits_amd import hostglue
        ordered = hostglue.track_assign(dets, None, np.zeros((1, TRACKS, 4)), np.full((1, TRACKS), -1, np.int32), MIN_IOU, 15)[0]
        assert np.array_equal(ordered, boxes), "the detections do not associate to the two tracks"
    track = dict(smooth=True, momentum=MOMENTUM)
    kw_all = dict(paste_back=not a.crops)
    runs = {"A": dict(boxes=torch.from_numpy(boxes), tracking=track)}
    if not a.parent:
        runs.update({"B": dict(detections=torch.from_numpy(dets), tracking=dict(track, tracks=TRACKS, min_iou=MIN_IOU)), "A2": runs["A"]})

    def run(kw, count=n):
        kw = {k: (v[:count] if k in ("boxes", "detections") else v) for k, v in kw.items()}
        w.reset_crop_state()
        got = 0
        for _, out in w.animate_frames(frames[:count], batch_size=B, **kw_all, **kw):
            got += out.shape[0]
        return got

    def timed(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert run(kw) == (n if not a.crops else TRACKS * n)
        return round(n / (time.perf_counter() - t0), 2)

    for kw in runs.values():               # warm-up: every signature captured
        run(kw, 3 * B)
    torch.cuda.synchronize()
    if not a.parent:                       # the two settings track the same faces: B's windows of the warm-up are A's
        run(runs["A"], 3 * B)
        wins_a = w.tracked_windows[0].clone()
        run(runs["B"], 3 * B)
        assert torch.equal(w.tracked_windows[0], wins_a) and bool((wins_a[:, 2] > 0).all()), "the two settings do not render the same windows"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        every = {name: [] for name in runs}
        for rep in range(a.reps):
            rec = {"tool": "bench_track_assign", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": S, "batch": B,
                   "frames": n, "faces_per_frame": TRACKS, "detections_per_frame": D, "frame_size": [W, H], "paste_back": not a.crops,
                   "graphs": True, "precision": w.hot_path.precision, "parent": bool(a.parent)}
            rec["frames_per_s"] = {name: timed(kw) for name, kw in runs.items()}          # A B A2, A B A2, ...
            for name, v in rec["frames_per_s"].items():
                every[name].append(v)
            if "B" in runs:
                rec["b_over_a"] = round(rec["frames_per_s"]["B"] / rec["frames_per_s"]["A"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        mean = {name: sum(v) / len(v) for name, v in every.items()}
        rec = {"tool": "bench_track_assign", "summary": True, "parent": bool(a.parent), "reps": a.reps, "paste_back": not a.crops,
               "mean_frames_per_s": {k: round(v, 2) for k, v in mean.items()},
               "a_spread": round(max(every["A"] + every.get("A2", [])) / min(every["A"] + every.get("A2", [])) - 1, 4)}   # A against A
        if "B" in runs:
            rec["a2_over_a"] = round(mean["A2"] / mean["A"], 4)
            rec["b_over_a"] = round(2 * mean["B"] / (mean["A"] + mean["A2"]), 4)
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
