"""Frames/s and rendered rows/s of InferenceWrapper.animate_frames(detections=, tracking=dict(tracks=2)) with the rows without a
face left out (tracking skip_absent=True: one ops.present_rows launch and one host wait per chunk, batches of kept rows) against
the same call without the field.

    python tools/bench_skip_absent.py [--reps 2] [--frames 384] [--scenarios half,full,full_32] [--out profiles/skip_absent_bench.jsonl]

Released architecture at R512 with seeded weights (as tools/bench_track_controls.py), hipGraph replay, B = 16, 1080p uint8 frames
in pinned host memory -> the frames with the rendered heads pasted back, in pinned host memory, a bank of two identities, two
track slots, detections at a random two of D = 4 rows per frame.  Scenarios:
    half        the left face in every frame, the right face on screen for 24 frames in every 96 (a quarter): 1.25 n present rows
                of 2 n.  If the path is bound by rows, skipping is worth 2 n / 1.25 n = 1.6 in frames/s: the expectation, not a
                threshold
    scattered   (on request) the right face in a random quarter of the frames, as a detector that flickers: the kept rows of a
                batch vary, so B meets batch shapes that A does not
    full        both faces in every frame: nothing to skip, B against A is the price of the launch and of the host wait per chunk
    full_32     `full` with the clip handed over as chunks of 32 frames: a host wait every 32 frames
Settings, alternated A B A2, A B A2 ... in one process:
    A    tracking=dict(smooth=True, momentum=0.5, tracks=2, min_iou=0.2)
    B    A with skip_absent=True
    A2   A once more: the A/A pair of the repetition
Every scenario writes one JSONL record per repetition and a summary: frames/s and rendered rows/s of every setting, `a_spread` =
max(A, A2) / min(A, A2) - 1 over the repetitions, `b_over_a` = B's mean over the mean of A and A2, `rows_ratio` = rows A renders /
rows B renders, and `graphs` = per setting how many batch shapes were captured as hipGraphs while the scenario warmed up (all
sequences together) and the seconds their capture took -- the kept counts vary, so B meets more shapes than A.  --parent measures
A alone: this file copied into a checkout of the parent commit gives the parent's frames/s for the same calls on the same box.
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
from emoportraits_amd import config, graphs, random_init  # noqa: E402
from emoportraits_amd import embedders as E  # noqa: E402
from emoportraits_amd.infer import InferenceWrapper  # noqa: E402

MOMENTUM, MIN_IOU, TRACKS, D, MAX_MISSED, CHUNK = 0.5, 0.2, 2, 4, 15, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=384)
    ap.add_argument("--scenarios", default="half,full,full_32", help="comma-separated: half, scattered, full, full_32")
    ap.add_argument("--parent", action="store_true", help="a checkout without skip_absent: measure A alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_absent_bench.jsonl"))
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
    n = a.frames - a.frames % CHUNK
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
    rng = np.random.default_rng(6)
    tracks = []
    for at in (0.3, 0.7):                                         # a face in the left and one in the right half: they never overlap
        cx = W * (at + 0.01 * rng.standard_normal(n)).clip(at - 0.03, at + 0.03)
        cy = H * (0.5 + 0.015 * rng.standard_normal(n)).clip(0.46, 0.54)
        half = rng.uniform(0.13, 0.16, (2, n)) * H
        tracks.append(np.stack([cx - half[0], cy - half[1], cx + half[0], cy + half[1]], 1))
    boxes = np.stack(tracks, 1)                                   # [n,2,4]

    def detections(there):
        """the left face in every frame, the right one where there[t]; each at a random row of the D"""
        dets = np.full((n, D, 4), np.nan)
        for t in range(n):
            at = np.arange(TRACKS) if t == 0 else rng.permutation(D)[:TRACKS]
            dets[t, at[0]] = boxes[t, 0]
            if there[t]:
                dets[t, at[1]] = boxes[t, 1]
        return torch.from_numpy(dets)

    quarter = np.arange(n) % 96 < 24
    scenarios = {"half": (detections(quarter), None), "full": (detections(np.ones(n, bool)), None)}
    scenarios["full_32"] = (scenarios["full"][0], CHUNK)
    scenarios["scattered"] = (detections(np.random.default_rng(7).random(n) < 0.25), None)
    scenarios = {name: scenarios[name] for name in a.scenarios.split(",")}
    track = dict(smooth=True, momentum=MOMENTUM, tracks=TRACKS, min_iou=MIN_IOU, max_missed=MAX_MISSED)
    runs = {"A": dict(tracking=track)}
    if not a.parent:
        runs.update({"B": dict(tracking=dict(track, skip_absent=True)), "A2": runs["A"]})

    captures = {"n": 0, "s": 0.0}
    capture = graphs.Graphed._capture

    def timed_capture(self, tensors):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = capture(self, tensors)
        torch.cuda.synchronize()
        captures["n"], captures["s"] = captures["n"] + 1, captures["s"] + time.perf_counter() - t0
        return out
    graphs.Graphed._capture = timed_capture

    def run(dets, chunk, kw):
        """-> (frames out, rows rendered)"""
        w.reset_crop_state()
        clip = frames if chunk is None else (frames[i:i + chunk] for i in range(0, n, chunk))
        got = rows = 0
        drive = w._drive_bank

        def counted(pose, theta, ident):
            nonlocal rows
            rows += pose.shape[0]
            return drive(pose, theta, ident)
        w._drive_bank = counted
        try:
            for _, out in w.animate_frames(clip, batch_size=B, paste_back=True, detections=dets, identities=[0, 1] * n, **kw):
                got += out.shape[0]
        finally:
            w._drive_bank = drive
        return got, rows

    def timed(dets, chunk, kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got, rows = run(dets, chunk, kw)
        dt = time.perf_counter() - t0
        assert got == n
        return round(n / dt, 2), round(rows / dt, 2), rows

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for scenario, (dets, chunk) in scenarios.items():
            warm = {}
            for name, kw in runs.items():          # warm-up: the whole clip twice, so that every batch shape it holds is captured
                if name == "A2":
                    continue
                captures["n"], captures["s"] = 0, 0.0
                run(dets, chunk, kw), run(dets, chunk, kw)
                warm[name] = {"shapes_captured": captures["n"], "capture_s": round(captures["s"], 3)}
            torch.cuda.synchronize()
            every = {name: [] for name in runs}
            rows_of = {}
            base = {"tool": "bench_skip_absent", "scenario": scenario, "image_size": S, "batch": B, "frames": n, "chunk": chunk,
                    "tracks": TRACKS, "detections_per_frame": D, "frame_size": [W, H], "paste_back": True, "graphs": True,
                    "precision": w.hot_path.precision, "parent": bool(a.parent)}
            for rep in range(a.reps):
                captures["n"] = 0
                rec = dict(base, time=time.strftime("%Y-%m-%dT%H:%M:%S"), rep=rep, frames_per_s={}, rows_per_s={})
                for name, kw in runs.items():                                             # A B A2, A B A2, ...
                    fps, rps, rows_of[name] = timed(dets, chunk, kw)
                    rec["frames_per_s"][name], rec["rows_per_s"][name] = fps, rps
                    every[name].append(fps)
                rec["captures_while_timed"] = captures["n"]
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
            mean = {name: sum(v) / len(v) for name, v in every.items()}
            pair = every["A"] + every.get("A2", [])
            rec = dict(base, summary=True, reps=a.reps, mean_frames_per_s={k: round(v, 2) for k, v in mean.items()},
                       rows_rendered=rows_of, mean_rows_per_s={k: round(v * rows_of[k] / n, 2) for k, v in mean.items()},
                       a_spread=round(max(pair) / min(pair) - 1, 4), graphs=warm)
            if "B" in runs:
                rec["a2_over_a"] = round(mean["A2"] / mean["A"], 4)
                rec["b_over_a"] = round(2 * mean["B"] / (mean["A"] + mean["A2"]), 4)
                rec["rows_ratio"] = round(rows_of["A"] / rows_of["B"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
