"""Frames/s of InferenceWrapper.animate_frames with the head-pose controls on (relative transfer, gain, rotation offset: one
launch of ops.head_pose_controls per batch, nine floats per row), against the same call with the defaults.

    python tools/bench_head_pose_controls.py [--reps 4] [--frames 192] [--out profiles/head_pose_controls_bench.jsonl]

Released architecture at R512 with seeded weights (as tools/bench_pose_controls.py), hipGraph replay, B = 16, uint8 frames in pinned
host memory -> uint8 frames in pinned host memory, one identity.  Settings, alternated A B A B ... in one process:
    A    the defaults (no `head_pose`)
    B    head_pose=dict(relative=True, gain=0.5, rotation_offset=[0.2, -0.1, 0.0])
    A2   A once more: the A/A pair of the repetition
Every repetition writes one JSONL record, and a last record sums up: `a_spread` = max(A, A2) / min(A, A2) - 1 over all repetitions
is the run-to-run spread of A against A on this box, `a2_over_a` the ratio of the means of the pair, `b_over_a` the ratio of B's
mean to the mean of A and A2.  --parent measures A alone: this file copied into
a checkout of the parent commit gives the parent's frames/s for the same call on the same box.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emoportraits_amd import config, random_init  # noqa: E402
from emoportraits_amd import embedders as E  # noqa: E402
from emoportraits_amd.infer import InferenceWrapper  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--parent", action="store_true", help="a checkout without head_pose=: measure A alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_pose_controls_bench.jsonl"))
    a = ap.parse_args()
    S, B = 512, 16
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
    frames = (torch.rand(n, S, S, 3, generator=g) * 255).to(torch.uint8).pin_memory()
    runs = {"A": {}} if a.parent else {"A": {}, "B": dict(head_pose=dict(relative=True, gain=0.5, rotation_offset=[0.2, -0.1, 0.0])), "A2": {}}

    def run(kw, count=n):
        got = 0
        for _, out in w.animate_frames(frames[:count], batch_size=B, **kw):
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
            rec = {"tool": "bench_head_pose_controls", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": S,
                   "batch": B, "frames": n, "graphs": True, "precision": w.hot_path.precision, "parent": bool(a.parent)}
            rec["frames_per_s"] = {name: timed(kw) for name, kw in runs.items()}          # A B A2, A B A2, ...
            for name, v in rec["frames_per_s"].items():
                every[name].append(v)
            if "B" in runs:
                rec["b_over_a"] = round(rec["frames_per_s"]["B"] / rec["frames_per_s"]["A"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        mean = {name: sum(v) / len(v) for name, v in every.items()}
        rec = {"tool": "bench_head_pose_controls", "summary": True, "parent": bool(a.parent), "reps": a.reps,
               "mean_frames_per_s": {k: round(v, 2) for k, v in mean.items()},
               "a_spread": round(max(every["A"] + every.get("A2", [])) / min(every["A"] + every.get("A2", [])) - 1, 4)}   # A against A
        if "B" in runs:
            rec["a2_over_a"] = round(mean["A2"] / mean["A"], 4)
            rec["b_over_a"] = round(2 * mean["B"] / (mean["A"] + mean["A2"]), 4)
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
