"""Frames/s of mixed-identity driver batches (the identity bank: HotPath.driver_pass(identity=...)) against the single-identity
step and the per-call loop a server without the bank would run.

    python tools/bench_identities.py [--reps 5] [--iters 20] [--out profiles/identity_bank_bench.jsonl]

Seeded trained-like R512 checkpoint (random_init.trained_like_state_dict, the bench's), default precision, B = 16:
    k1_plain   one identity through today's path (what bench.py times)
    bank_k1    the bank path, every frame on identity 0
    bank_k4    the bank path, 4 distinct identities per batch
    bank_k16   the bank path, 16 distinct identities per batch (one frame each)
    b1_loop    16 graph-replayed B = 1 passes, one per identity (16 frames)
Timed with events after warm-up; the variants are interleaved within each repetition (A B A B, one process), and every
repetition writes one JSONL record.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_bank_bench.jsonl"))
    a = ap.parse_args()
    from emoportraits_amd import config, graphs, nets, ops, random_init
    dev = "cuda:0"
    cfg = config.hot_path_config(overrides={"image_size": 512})
    sd = random_init.trained_like_state_dict(cfg, seed=0, with_source=False)
    hp = nets.HotPath(sd, cfg, dev, with_source=False)
    c, d, s = cfg["latent_volume_channels"], cfg["latent_volume_depth"], cfg["latent_volume_size"]
    K, B = 16, 16
    g = torch.Generator().manual_seed(1)
    bank_cl = torch.cat([hp.prepare_canonical(torch.randn(1, c, d, s, s, generator=g).to(dev)) for _ in range(K)])
    bank_idt = torch.randn(K, cfg["gen_max_channels"], 4, 4, generator=g).to(dev)
    pose = torch.randn(B, cfg["lpe_output_channels_expression"], generator=g).to(dev)
    srt = [t.to(dev) for t in (1 + 0.05 * torch.randn(B, 3, generator=g), 0.3 * torch.randn(B, 3, generator=g),
                              0.05 * torch.randn(B, 3, generator=g))]
    theta = ops.pose_theta(*srt)
    ident = {k: torch.tensor([i % k for i in range(B)], dtype=torch.int32, device=dev) for k in (1, 4, 16)}
    one_cl, one_idt = bank_cl[:1].contiguous(), bank_idt[:1].contiguous()
    loop = [graphs.Graphed(lambda p, t, k=k: hp.driver_pass(bank_cl[k:k + 1], bank_idt[k:k + 1], p, t), clone_outputs=False)
            for k in range(K)]

    def b1_loop():
        for k in range(K):
            loop[k](pose[k:k + 1], theta[k:k + 1])

    runs = {
        "k1_plain": lambda: hp.driver_pass(one_cl, one_idt, pose, theta),
        "bank_k1": lambda: hp.driver_pass(bank_cl, bank_idt, pose, theta, identity=ident[1]),
        "bank_k4": lambda: hp.driver_pass(bank_cl, bank_idt, pose, theta, identity=ident[4]),
        "bank_k16": lambda: hp.driver_pass(bank_cl, bank_idt, pose, theta, identity=ident[16]),
        "b1_loop": b1_loop,
    }
    for fn in runs.values():                # warm-up: lazy packing, allocator, graph capture
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rep in range(a.reps):
            rec = {"tool": "bench_identities", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": 512,
                   "batch": B, "precision": hp.precision, "iters": a.iters, "frames_per_s": {}, "ms_per_16_frames": {}}
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1) / a.iters
                rec["ms_per_16_frames"][name] = round(ms, 4)
                rec["frames_per_s"][name] = round(16 * 1e3 / ms, 2)
            fps = rec["frames_per_s"]
            rec["bank_k16_over_k1_plain"] = round(fps["bank_k16"] / fps["k1_plain"], 4)
            rec["bank_k16_over_b1_loop"] = round(fps["bank_k16"] / fps["b1_loop"], 4)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
