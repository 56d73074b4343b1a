"""Frames/s of InferenceWrapper.animate_frames(detections=) with the control streams following the face tracks (tracking
follow_tracks=True: the three control launches take two int32 row masks) against the same call without the field.

    python tools/bench_track_controls.py [--reps 2] [--frames 384] [--crops] [--out profiles/track_controls_bench.jsonl]

Released architecture at R512 with seeded weights (as tools/bench_track_assign.py), hipGraph replay, B = 16, 1080p uint8 frames in
pinned host memory -> the frames with both rendered heads pasted back, in pinned host memory (--crops: the crops instead), a bank
of two identities.  Two faces wander about the left and the right half of the frame and come as a detector delivers them, at a
random two of D = 4 rows per frame; the detector drops the right face for 3 frames in every 40, and once for 24 frames, so that
its track dies (max_missed = 15) and is born again: the masks are not all ones.  smooth_pose, a relative expression and a relative
head pose are on in every setting.  Settings, alternated A B A2, A B A2 ... in one process:
    A    tracking=dict(smooth=True, momentum=0.5, tracks=2, min_iou=0.2)
    B    A with follow_tracks=True
    A2   A once more: the A/A pair of the repetition
Every repetition writes one JSONL record, and a last record sums up: `a_spread` = max(A, A2) / min(A, A2) - 1 over all repetitions
is the run-to-run spread of A against A on this box, `a2_over_a` the ratio of the means of the pair, `b_over_a` the ratio of B's
mean to the mean of A and A2.  No speed-up is claimed: the expectation to check is that B is not distinguishable from A beyond
`a_spread`.  --parent measures A alone: this file copied into a checkout of the parent commit gives the parent's frames/s for the
same detections= call on the same box.
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

MOMENTUM, MIN_IOU, TRACKS, D, MAX_MISSED = 0.5, 0.2, 2, 4, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=384)
    ap.add_argument("--crops", action="store_true", help="yield the crops instead of the pasted frames")
    ap.add_argument("--parent", action="store_true", help="a checkout without follow_tracks: measure A alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_controls_bench.jsonl"))
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
                         print_params=False, head_pose_regressor_path=os.path.join(root, "hp.pth"), use_graphs=True,
                         identity_capacity=TRACKS)
    g = torch.Generator().manual_seed(5)
    w.enrol_identities(torch.rand(TRACKS, 3, S, S, generator=g), source_masks=[torch.ones(1, 1, S, S)] * TRACKS, batch_size=TRACKS)
    n = a.frames - a.frames % (B // TRACKS)
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
    rng = np.random.default_rng(6)
    tracks = []
    for at in (0.3, 0.7):                                         # a face in the left and one in the right half: they never overlap
        cx = W * (at + 0.01 * rng.standard_normal(n)).clip(at - 0.03, at + 0.03)
        cy = H * (0.5 + 0.015 * rng.standard_normal(n)).clip(0.46, 0.54)
        half = rng.uniform(0.13, 0.16, (2, n)) * H
        tracks.append(np.stack([cx - half[0], cy - half[1], cx + half[0], cy + half[1]], 1))
    boxes = np.stack(tracks, 1)                                   # [n,2,4]
    gone = np.zeros(n, bool)                                      # the frames in which the detector has no right face
    for t in range(20, n, 40):
        gone[t:t + 3] = True
    gone[n // 2:n // 2 + 24] = True
    dets = np.full((n, D, 4), np.nan)
    for t in range(n):
        at = np.arange(TRACKS) if t == 0 else rng.permutation(D)[:TRACKS]
        dets[t, at[0]] = boxes[t, 0]
        if not gone[t]:
            dets[t, at[1]] = boxes[t, 1]
    track = dict(smooth=True, momentum=MOMENTUM, tracks=TRACKS, min_iou=MIN_IOU, max_missed=MAX_MISSED)
    kw_all = dict(paste_back=not a.crops, detections=torch.from_numpy(dets), identities=[0, 1] * n, smooth_pose=True, smooth_per_identity=True,
                  expression=dict(relative=True), head_pose=dict(relative=True))
    runs = {"A": dict(tracking=track)}
    if not a.parent:
        runs.update({"B": dict(tracking=dict(track, follow_tracks=True)), "A2": runs["A"]})

    def run(kw, count=n):
        more = {k: (v[:count] if k == "detections" else v[:TRACKS * count] if k == "identities" else v) for k, v in kw_all.items()}
        w.reset_crop_state(), w.reset_pose_state(), w.reset_expression_state()
        got = 0
        for _, out in w.animate_frames(frames[:count], batch_size=B, **more, **kw):
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
    masks = None
    if not a.parent:                       # what the masks of the whole clip hold: B has something to follow
        run(runs["B"])
        present = w.tracked_present[0].reshape(n, TRACKS)
        restart = w.tracked_assignment[1]
        masks = {"absent_rows": int((present == 0).sum()), "restarts": int(restart.sum())}
        assert masks["absent_rows"] >= int(gone.sum()) and masks["restarts"] >= 4, masks
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        every = {name: [] for name in runs}
        for rep in range(a.reps):
            rec = {"tool": "bench_track_controls", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": S, "batch": B,
                   "frames": n, "faces_per_frame": TRACKS, "detections_per_frame": D, "frame_size": [W, H], "paste_back": not a.crops,
                   "graphs": True, "precision": w.hot_path.precision, "parent": bool(a.parent), "masks": masks}
            rec["frames_per_s"] = {name: timed(kw) for name, kw in runs.items()}          # A B A2, A B A2, ...
            for name, v in rec["frames_per_s"].items():
                every[name].append(v)
            if "B" in runs:
                rec["b_over_a"] = round(rec["frames_per_s"]["B"] / rec["frames_per_s"]["A"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        mean = {name: sum(v) / len(v) for name, v in every.items()}
        rec = {"tool": "bench_track_controls", "summary": True, "parent": bool(a.parent), "reps": a.reps, "paste_back": not a.crops,
               "mean_frames_per_s": {k: round(v, 2) for k, v in mean.items()},
               "a_spread": round(max(every["A"] + every.get("A2", [])) / min(every["A"] + every.get("A2", [])) - 1, 4)}   # A against A
        if "B" in runs:
            rec["a2_over_a"] = round(mean["A2"] / mean["A"], 4)
            rec["b_over_a"] = round(2 * mean["B"] / (mean["A"] + mean["A2"]), 4)
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
