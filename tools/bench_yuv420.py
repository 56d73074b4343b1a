"""Video in -> video out in the four YUV 4:2:0 formats: animate_frames(paste_back=True) on full 1080p frames in NV12, yuv420p, p010
and yuv420p10, and each kernel instantiation of the three new layouts alone beside a copy of the bytes it moves.

    python tools/bench_yuv420.py [--reps 4] [--frames 256] [--variants ABCDK] [--label TEXT] [--out profiles/yuv420_bench.jsonl]

tools/bench_nv12.py's wrapper, clip and windows (seeded trained-like R512 checkpoint, default precision and graphs, B = 16, a
1080 x 1920 clip in pinned host memory).  The clips of B, C and D are re-layouts of A's samples; the 10-bit clips hold the codes
4 * byte.  One JSON line each, the variants alternating A B C D within one process:
    A   animate_frames(nv12 frames, windows=..., paste_back=True, frame_format='nv12')            uint8  [b,1620,1920] out
    B   the same with frame_format='yuv420p'                                                      uint8  [b,1620,1920] out
    C   the same with frame_format='p010'                                                         uint16 [b,1620,1920] out
    D   the same with frame_format='yuv420p10'                                                    uint16 [b,1620,1920] out
    K   ops.yuv420_windows, ops.pack_yuv420 and ops.paste_windows_yuv420 of every new format (and the NV12 ops) on one batch by
        events, each beside a copy_ of exactly the bytes it moves (read + written): bytes_moved, kernel_ms, copy_ms_same_bytes
and a last line with the medians, the spreads and every variant over A.  Wall time around the whole generator,
device-synchronised; one warm-up run per variant (graph capture, lazy packing, pinned ring).
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

FORMAT = {"A": "nv12", "B": "yuv420p", "C": "p010", "D": "yuv420p10"}


def relayout(nv12, frame_format):
    """NV12 uint8 [n, 3H/2, W] -> the same samples in frame_format (the 10-bit formats: the codes 4 * byte), on the host"""
    n, rows, w = nv12.shape
    h = rows // 3 * 2
    x = nv12
    if frame_format in ("yuv420p", "yuv420p10"):
        uv = nv12[:, h:].reshape(n, h // 2, w // 2, 2)
        x = torch.cat([nv12[:, :h].reshape(n, -1), uv[..., 0].reshape(n, -1), uv[..., 1].reshape(n, -1)], dim=1).reshape(n, rows, w)
    if frame_format == "p010":
        return (x.to(torch.int32) << 8).to(torch.uint16)
    if frame_format == "yuv420p10":
        return (x.to(torch.int32) << 2).to(torch.uint16)
    return x.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--variants", default="ABCDK")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv420_bench.jsonl"))
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
    nv12 = torch.cat([ops.pack_nv12(ops.unpack_rgb8(distinct[i:i + 8].to(dev))).cpu() for i in range(0, 32, 8)])
    order = [v for v in "ABCD" if v in a.variants]
    clips = {}
    for v in order:
        src = relayout(nv12, FORMAT[v])
        clips[v] = torch.empty((N, 3 * Hf // 2, Wf), dtype=src.dtype, pin_memory=True)
        for i in range(0, N, 32):
            clips[v][i:i + 32].copy_(src[:min(32, N - i)])
    windows = []
    for i in range(N):
        s = 300 + (600 * (i % B)) // (B - 1)                      # every batch holds the whole spread of sides
        windows.append((int(torch.randint(0, Wf - s + 1, (1,), generator=g)), int(torch.randint(0, Hf - s + 1, (1,), generator=g)), s))

    def run(v):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for _, out in w.animate_frames(clips[v], batch_size=B, windows=windows, paste_back=True, frame_format=FORMAT[v]):
            got += out.shape[0]
        torch.cuda.synchronize()
        assert got == N
        return time.perf_counter() - t0

    base = {"tool": "bench_yuv420", "label": a.label, "image_size": S, "batch": B, "frames": N, "frame_size": [Hf, Wf],
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
            run(v)                                                 # warm-up
        for rep in range(a.reps):
            for v in order:
                dt = run(v)
                fps[v].append(N / dt)
                emit({"variant": v, "rep": rep, "fps": round(N / dt, 2), "ms_per_batch": round(dt * 1e3 / (N / B), 3),
                      "frames_in_out": FORMAT[v], "bytes_per_frame_each_way": clips[v][0].numel() * clips[v].element_size()})
        if "K" in a.variants:
            img = torch.rand(B, 3, S, S, generator=g).to(dev)
            wins = [(x, y, s, s) for x, y, s in windows[:B]]
            win_px = sum(s * s for _, _, s, _ in wins)
            f32 = img.numel() * 4

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

            # name -> (callable, bytes it moves: read + written)
            kernels = {}
            for fmt in ("nv12", "yuv420p", "p010", "yuv420p10"):
                fr = relayout(nv12[:B], fmt).to(dev)
                sb = fr.element_size()
                kernels[f"yuv420_windows[{fmt}]"] = (lambda fr=fr, fmt=fmt: ops.yuv420_windows(fr, fmt, (S, S), wins), win_px * 3 // 2 * sb + f32)
                kernels[f"pack_yuv420[{fmt}]"] = (lambda fmt=fmt: ops.pack_yuv420(img, fmt), f32 + B * S * S * 3 // 2 * sb)
                kernels[f"paste_windows_yuv420[{fmt}]"] = (lambda fr=fr, fmt=fmt: ops.paste_windows_yuv420(fr, fmt, img, wins, 0.0625),
                                                           2 * (win_px * 3 // 2) * sb + f32)
            for rep in range(a.reps):
                for name, (fn, moved) in kernels.items():
                    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                    dst = torch.empty_like(src)
                    k_ms = timed(fn)
                    c_ms = timed(lambda: dst.copy_(src))
                    emit({"variant": "K", "kernel": name, "rep": rep, "bytes_moved": moved, "kernel_ms": round(k_ms, 4),
                          "copy_ms_same_bytes": round(c_ms, 4), "kernel_over_copy": round(k_ms / c_ms, 3)})
        med = lambda xs: sorted(xs)[len(xs) // 2]
        summary = {}
        for v in order:
            summary[f"fps_{v}_median"] = round(med(fps[v]), 2)
            summary[f"fps_{v}_spread"] = [round(min(fps[v]), 2), round(max(fps[v]), 2)]
            if v != "A" and "A" in fps:
                summary[f"{v}_over_A"] = round(med(fps[v]) / med(fps["A"]), 4)
        if summary:
            emit({"variant": "summary", **summary})


if __name__ == "__main__":
    main()
