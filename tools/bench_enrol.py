"""Enrolment of K = 16 source identities into the identity bank: the per-identity loop against the batched entry point.

    python tools/bench_enrol.py [--reps 4] [--out profiles/enrol_bench.jsonl]

Seeded trained-like R512 checkpoint (random_init.trained_like_state_dict, the bench's), default precision, 16 synthetic sources
with their embeddings given through the custome_* arguments (so both sides time the same work: masks, source pass, bank write):
    loop        forward(source_image=...) + store_identity(k), once per identity
    enrol_bs4   enrol_identities(..., batch_size=4)       (and bs8, bs16)
Device-synchronised wall time; the variants alternate within each repetition (one process), and every repetition writes one
JSONL record with ms per identity and the peak device memory of each variant.  A last record times the bare
HotPath.source_pass: 8 calls at B = 1 against one call at B = 8.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enrol_bench.jsonl"))
    a = ap.parse_args()
    from emoportraits_amd import config, random_init
    from notebooks.infer import InferenceWrapper
    S, K = 512, 16
    cfg = config.hot_path_config(overrides={"image_size": S})
    root = tempfile.mkdtemp()
    os.makedirs(os.path.join(root, "logs", "exp", "checkpoints"))
    with open(os.path.join(root, "logs", "exp", "args.txt"), "wt") as f:
        for k, v in cfg.items():
            f.write(f"{k}: {v}\n")
    sd = random_init.trained_like_state_dict(cfg, seed=0)
    w = InferenceWrapper(experiment_name="exp", model_file_name="x", project_dir=root, folder="logs", state_dict=sd,
                         print_params=False, use_graphs=False, identity_capacity=K)
    dev = w.device
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand(K, 3, S, S, generator=g)
    masks = [torch.ones(1, 1, S, S)] * K
    idt = torch.randn(K, cfg["gen_max_channels"], 4, 4, generator=g)
    pose = torch.randn(K, cfg["lpe_output_channels_expression"], generator=g)
    srt = (1 + 0.05 * torch.randn(K, 3, generator=g), 0.3 * torch.randn(K, 3, generator=g), 0.05 * torch.randn(K, 3, generator=g))
    from emoportraits_amd import ops
    theta = ops.pose_theta(*[t.to(dev).contiguous() for t in srt]).cpu()

    def loop():
        for k in range(K):
            w.forward(source_image=imgs[k:k + 1], crop=False, source_mask=masks[k], custome_idt_embed=idt[k:k + 1],
                      custome_source_pose_embed=pose[k:k + 1], custome_source_theta_embed=theta[k:k + 1])
            w.store_identity(k)

    def enrol(bs):
        return lambda: w.enrol_identities(imgs, source_masks=masks, slots=list(range(K)), batch_size=bs, custome_idt_embed=idt,
                                          custome_source_pose_embed=pose, custome_source_theta_embed=theta)

    runs = {"loop": loop, "enrol_bs4": enrol(4), "enrol_bs8": enrol(8), "enrol_bs16": enrol(16)}
    for fn in runs.values():                 # warm-up: lazy packing, allocator
        fn()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rep in range(a.reps):
            rec = {"tool": "bench_enrol", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "rep": rep, "image_size": S, "identities": K,
                   "precision": w.hot_path.precision, "ms_per_identity": {}, "peak_mib": {}}
            for name, fn in runs.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                rec["ms_per_identity"][name] = round((time.perf_counter() - t0) * 1e3 / K, 3)
                rec["peak_mib"][name] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
            m = rec["ms_per_identity"]
            rec["loop_over_enrol"] = {k: round(m["loop"] / m[k], 4) for k in m if k != "loop"}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        # the bare source pass: 8 identities at B = 1 against one B = 8 call
        hp = w.hot_path
        masked = imgs[:8].to(dev)
        args8 = (masked, idt[:8].to(dev).contiguous(), pose[:8].to(dev).contiguous(), theta[:8].to(dev).contiguous())
        one = lambda: [hp.source_pass(*(t[k:k + 1] for t in args8)) for k in range(8)]
        eight = lambda: hp.source_pass(*args8)
        for fn in (one, eight):
            fn()
        rec = {"tool": "bench_enrol", "time": time.strftime("%Y-%m-%dT%H:%M:%S"), "source_pass_ms_per_identity": {"b1": [], "b8": []}}
        for rep in range(a.reps):
            for name, fn in (("b1", one), ("b8", eight)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                rec["source_pass_ms_per_identity"][name].append(round((time.perf_counter() - t0) * 1e3 / 8, 3))
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
