"""Frames/s of InferenceWrapper.animate_frames with forward()'s pose controls on (mix, smooth_pose, target_theta), against the
same call with the defaults -- the controls are two tiny launches per batch (ops.mixing_theta, ops.theta_ema_scan) or a gather.

    python tools/bench_pose_controls.py [--reps 4] [--frames 192] [--out profiles/pose_controls_bench.jsonl]

Released architecture at R512 with seeded weights (as tools/bench_pipeline.py), hipGraph replay, B = 16, uint8 frames in pinned
host memory -> uint8 frames in pinned host memory.  Settings:
    defaults          one identity, no control
    mix               one identity, mix=True
    source_pose       one identity, target_theta=False
    bank16            16 identities, one frame each per batch, no control
    bank16_smooth     16 identities, smooth_pose=True (one stream per slot, scanned on the device)
    bank16_mix_smooth 16 identities, mix=True and smooth_pose=True
The settings are interleaved within each repetition (one process); every repetition writes one JSONL record.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_controls_bench.jsonl"))
    a = ap.parse_args()
    S, B, K = 512, 16, 16
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
                         identity_capacity=K)
    g = torch.Generator().manual_seed(5)
    for k in range(K):                      # K identities with their own images (and so their own regressed source thetas)
        w.forward(source_image=torch.rand(1, 3, S, S, generator=g), crop=False, source_mask=torch.ones(1, 1, S, S))
        w.store_identity(k)
    n = a.frames - a.frames % B
    frames = (torch.rand(n, S, S, 3, generator=g) * 255).to(torch.uint8).pin_memory()
    ids = [i % K for i in range(n)]
    runs = {
        "defaults": {},
        "mix": dict(mix=True),
        "source_pose": dict(target_theta=False),
        "bank16": dict(identities=ids),
        "bank16_smooth": dict(identities=ids, smooth_pose=True, smooth_per_identity=True),
        "bank16_mix_smooth": dict(identities=ids, mix=True, smooth_pose=True, smooth_per_identity=True),
    }

    def run(kw, count=n):
        got = 0
        for _, out in w.animate_frames(frames[:count], batch_size=B, **kw):
            got += out.shape[0]
        return got

    for kw in runs.values():               # warm-up: every signature captured
        kw_w = dict(kw, identities=ids[:3 * B]) if "identities" in kw else kw
        run(kw_w, 3 * B)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rep in range(a.reps):
            rec = {"tool": "bench_pose_controls", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": S,
                   "batch": B, "frames": n, "graphs": True, "precision": w.hot_path.precision, "frames_per_s": {}}
            for name, kw in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert run(kw) == n
                rec["frames_per_s"][name] = round(n / (time.perf_counter() - t0), 2)
            fps = rec["frames_per_s"]
            rec["ratio_to_defaults"] = {k: round(v / fps["defaults"], 4) for k, v in fps.items() if k != "defaults"}
            rec["bank16_smooth_over_bank16"] = round(fps["bank16_smooth"] / fps["bank16"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
