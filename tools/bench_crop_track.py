"""Frames/s of InferenceWrapper.animate_frames with crop tracking on the device (boxes= with the smoothed crop: one launch of
ops.crop_track per chunk, in front of the batch loop) against the same call with windows= holding the same windows as a host list.

    python tools/bench_crop_track.py [--reps 2] [--frames 384] [--crops] [--out profiles/crop_track_bench.jsonl]

Released architecture at R512 with seeded weights (as tools/bench_head_pose_controls.py), hipGraph replay, B = 16, 1080p uint8
frames in pinned host memory -> the frames with the rendered head pasted back, in pinned host memory (--crops: the crops instead),
one identity.  The boxes are a face that wanders about the middle of the frame; the windows of A are what the tracker makes of them,
formed on the host by the loop of hostglue.crop_window + CropTracker that a user without boxes= would write.  Settings, alternated
A B A2, A B A2 ... in one process:
    A    windows=<those windows>
    B    boxes=<the boxes>, tracking=dict(smooth=True, momentum=0.5)
    A2   A once more: the A/A pair of the repetition
Every repetition writes one JSONL record, and a last record sums up: `a_spread` = max(A, A2) / min(A, A2) - 1 over all repetitions
is the run-to-run spread of A against A on this box, `a2_over_a` the ratio of the means of the pair, `b_over_a` the ratio of B's
mean to the mean of A and A2.  --parent measures A alone: this file copied into a checkout of the parent commit gives the parent's
frames/s for the same windows= call on the same box.
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
from emoportraits_amd import config, hostglue, random_init  # noqa: E402
from emoportraits_amd import embedders as E  # noqa: E402
from emoportraits_amd.infer import InferenceWrapper  # noqa: E402

MOMENTUM = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=384, help="frames of a timed run: 384 are a second (96 measured the scheduler)")
    ap.add_argument("--crops", action="store_true", help="yield the crops instead of the pasted frames")
    ap.add_argument("--parent", action="store_true", help="a checkout without boxes=: measure A alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_track_bench.jsonl"))
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
    cx, cy = W * (0.5 + 0.05 * rng.standard_normal(n)).clip(0.4, 0.6), H * (0.5 + 0.05 * rng.standard_normal(n)).clip(0.4, 0.6)
    half = rng.uniform(0.2, 0.3, (2, n)) * H
    boxes = np.stack([cx - half[0], cy - half[1], cx + half[0], cy + half[1]], 1)
    tracker, windows = hostglue.CropTracker(MOMENTUM), []
    for box in boxes:                                             # (from fresh state: every timed run of B restarts the tracker)
        x_lo, y_lo, side, _ = hostglue.crop_window(box, W, H, tracker)
        windows.append((x_lo, y_lo, side))
    assert all(s >= S // 4 and x >= 0 and y >= 0 and x + s <= W and y + s <= H for x, y, s in windows)
    kw_all = dict(paste_back=not a.crops)
    runs = {"A": dict(windows=windows)}
    if not a.parent:
        runs.update({"B": dict(boxes=torch.from_numpy(boxes), tracking=dict(smooth=True, momentum=MOMENTUM)), "A2": dict(windows=windows)})

    def run(kw, count=n):
        kw = {k: (v[:count] if k in ("windows", "boxes") else v) for k, v in kw.items()}
        if "boxes" in kw:
            w.reset_crop_state()
        got = 0
        for _, out in w.animate_frames(frames[:count], batch_size=B, **kw_all, **kw):
            got += out.shape[0]
        return got

    def timed(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert run(kw) == n
        return round(n / (time.perf_counter() - t0), 2)

    for kw in runs.values():               # warm-up: every signature captured
        run(kw, 3 * B)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        every = {name: [] for name in runs}
        for rep in range(a.reps):
            rec = {"tool": "bench_crop_track", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": S, "batch": B,
                   "frames": n, "frame_size": [W, H], "paste_back": not a.crops, "graphs": True, "precision": w.hot_path.precision,
                   "parent": bool(a.parent)}
            rec["frames_per_s"] = {name: timed(kw) for name, kw in runs.items()}          # A B A2, A B A2, ...
            for name, v in rec["frames_per_s"].items():
                every[name].append(v)
            if "B" in runs:
                rec["b_over_a"] = round(rec["frames_per_s"]["B"] / rec["frames_per_s"]["A"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        mean = {name: sum(v) / len(v) for name, v in every.items()}
        rec = {"tool": "bench_crop_track", "summary": True, "parent": bool(a.parent), "reps": a.reps, "paste_back": not a.crops,
               "mean_frames_per_s": {k: round(v, 2) for k, v in mean.items()},
               "a_spread": round(max(every["A"] + every.get("A2", [])) / min(every["A"] + every.get("A2", [])) - 1, 4)}   # A against A
        if "B" in runs:
            rec["a2_over_a"] = round(mean["A2"] / mean["A"], 4)
            rec["b_over_a"] = round(2 * mean["B"] / (mean["A"] + mean["A2"]), 4)
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
