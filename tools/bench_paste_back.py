"""Frames in -> frames out: animate_frames with the rendered crops pasted back into the full driver frames, against the crop-out
path it extends, and the paste kernel alone against a copy of the same bytes.

    python tools/bench_paste_back.py [--reps 4] [--frames 256] [--variants ABC] [--label TEXT] [--out profiles/paste_back_bench.jsonl]

Seeded trained-like R512 checkpoint (random_init.trained_like_state_dict, the bench's) with seeded embedder weights, default
precision and graphs, B = 16, a 1080 x 1920 clip in pinned host memory, one crop window per frame with sides spread over
300 ... 900 at seeded positions.  One JSON line each, the variants alternating A B A B within one process:
    A   animate_frames(frames, windows=...)                    uint8 crops out, as before
    B   animate_frames(frames, windows=..., paste_back=True)   uint8 full frames out
    C   ops.paste_windows on one batch by events, beside a copy_ of exactly the bytes it touches (window bytes read + written, the
        fp32 images read): bytes_touched, kernel_ms, copy_ms_same_bytes
    S   (on request) the kernel by window side: 16 windows of one side, 1080 ... 128, without and with feather and matte
and a last line with B / A and kernel / copy.  --variants A runs on a tree without paste_back (the same-box comparison of A with
the commit before).  Wall time around the whole generator, device-synchronised; one warm-up run per variant (graph capture,
lazy packing, pinned ring).
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
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--variants", default="ABC")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paste_back_bench.jsonl"))
    a = ap.parse_args()
    from emoportraits_amd import config, ops, random_init
    from emoportraits_amd import embedders as E
    from emoportraits_amd.infer import InferenceWrapper
    S, B, Hf, Wf, N = 512, 16, 1080, 1920, a.frames
    cfg = config.hot_path_config(overrides={"image_size": S})
    ecfg = E.embedder_config()
    sd = random_init.trained_like_state_dict(cfg, seed=0)
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
                         print_params=False, head_pose_regressor_path=os.path.join(root, "hp.pth"))
    dev = w.device
    g = torch.Generator().manual_seed(5)
    w.forward(source_image=torch.rand(1, 3, S, S, generator=g), crop=False, source_mask=torch.ones(1, 1, S, S))
    distinct = torch.randint(0, 256, (32, Hf, Wf, 3), generator=g, dtype=torch.uint8)
    frames = torch.empty((N, Hf, Wf, 3), dtype=torch.uint8, pin_memory=True)
    for i in range(0, N, 32):
        frames[i:i + 32].copy_(distinct[:min(32, N - i)])
    windows = []
    for i in range(N):
        s = 300 + (600 * (i % B)) // (B - 1)                      # every batch holds the whole spread of sides
        windows.append((int(torch.randint(0, Wf - s + 1, (1,), generator=g)), int(torch.randint(0, Hf - s + 1, (1,), generator=g)), s))

    def run(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for _, out in w.animate_frames(frames, batch_size=B, windows=windows, **kw):
            got += out.shape[0]
        torch.cuda.synchronize()
        assert got == N
        return time.perf_counter() - t0

    variants = {"A": dict(), "B": dict(paste_back=True)}
    order = [v for v in "AB" if v in a.variants]
    base = {"tool": "bench_paste_back", "label": a.label, "image_size": S, "batch": B, "frames": N, "frame_size": [Hf, Wf],
            "precision": w.hot_path.precision, "graphs": w.use_graphs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    fps = {v: [] for v in order}
    with open(a.out, "a") as f:
        def emit(rec):
            rec = {**base, "time": time.strftime("%Y-%m-%dT%H:%M:%S"), **rec}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()

        for v in order:
            run(**variants[v])                                     # warm-up
        for rep in range(a.reps):
            for v in order:
                dt = run(**variants[v])
                fps[v].append(N / dt)
                emit({"variant": v, "rep": rep, "fps": round(N / dt, 2), "ms_per_batch": round(dt * 1e3 / (N / B), 3),
                      "out": "full frames" if v == "B" else "crops"})
        summary = {}
        if "C" in a.variants:
            u8 = frames[:B].to(dev)
            img = torch.rand(B, 3, S, S, generator=g).to(dev)
            wins = [(x, y, s, s) for x, y, s in windows[:B]]
            touched = sum(2 * 3 * s * s for _, _, s, _ in wins) + img.numel() * 4
            src = torch.empty(touched // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)

            def timed(fn, iters=20):
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / iters

            for rep in range(a.reps):
                k_ms = timed(lambda: ops.paste_windows(u8, img, wins, 0.0625))
                c_ms = timed(lambda: dst.copy_(src))
                emit({"variant": "C", "rep": rep, "feather": 0.0625, "bytes_touched": touched, "kernel_ms": round(k_ms, 4),
                      "copy_ms_same_bytes": round(c_ms, 4), "kernel_gb_per_s": round(touched / k_ms / 1e6, 1)})
                summary.setdefault("kernel_over_copy", []).append(round(k_ms / c_ms, 3))
        if "S" in a.variants:
            # the kernel by window side: 16 windows of one side each, upscaling (side > 512), scale 1 and the antialiased downscaling
            u8 = frames[:B].to(dev)
            img = torch.rand(B, 3, S, S, generator=g).to(dev)
            matte = torch.rand(B, 1, S, S, generator=g).to(dev)
            for side in (1080, 900, 513, 512, 511, 400, 300, 200, 128):
                wins = [(7 * n + 1, 0, side, side) for n in range(B)]
                for feather, m in ((0.0, None), (0.0625, None), (0.0625, matte)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    for it in range(23):
                        if it == 3:
                            e0.record()
                        ops.paste_windows(u8, img, wins, feather, m)
                    e1.record()
                    e1.synchronize()
                    ms = e0.elapsed_time(e1) / 20
                    emit({"variant": "S", "side": side, "feather": feather, "matte": m is not None, "kernel_ms": round(ms, 4),
                          "ns_per_window_pixel": round(ms * 1e6 / (B * side * side), 3)})
        med = lambda xs: sorted(xs)[len(xs) // 2]
        for v in order:
            summary[f"fps_{v}_median"] = round(med(fps[v]), 2)
            summary[f"fps_{v}_spread"] = [round(min(fps[v]), 2), round(max(fps[v]), 2)]
        if "A" in fps and "B" in fps:
            summary["B_over_A"] = round(med(fps["B"]) / med(fps["A"]), 4)
        if summary:
            emit({"variant": "summary", **summary})


if __name__ == "__main__":
    main()
