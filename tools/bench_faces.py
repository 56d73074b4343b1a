"""Several faces per frame in the video path: animate_frames(faces=..., paste_back=True) on 1080p frames against what the commit
before it offers for the same frames.

    python tools/bench_faces.py [--reps 4] [--frames 256] [--cases ab] [--formats rgb8,nv12] [--label TEXT] [--out profiles/faces_bench.jsonl]

Seeded trained-like R512 checkpoint with seeded embedder weights (tools/bench_nv12.py's), default precision and graphs, B = 16,
1080 x 1920 frames in pinned host memory, a bank of 4 identities.  One JSON line per run, the two variants of a case alternating
A B A B within one process after one warm-up run each; a summary line per case and format; the clock implied by a bare MFMA
stream (bench.py's sustained_mfma form, 0.3 s) in front of and behind every case.
  case a, one face per frame, --frames frames, sides 300 ... 900 at seeded places:
    A   animate_frames(frames, windows=wins, paste_back=True)                 the single-window path, unchanged by the feature
    B   animate_frames(frames, faces=[[w] for w in wins], paste_back=True)    the same frames through the faces entry points
    summary: B / A beside the spread A shows against itself in the same alternation (max / min of its runs)
  case b, 4 faces per frame whose windows overlap pairwise (sides 420 ... 600 around the frame's centre), --frames / 4 frames, one
  bank slot per face, batches of 4 frames = 16 faces in both variants:
    C   animate_frames(frames, faces=..., identities=..., paste_back=True)
    D   the way without the feature: every frame duplicated per face (the copies made outside the timed region),
        animate_frames(frames[frame_of], windows=flat, identities=..., as_uint8=False, to_host=False), then per batch one
        paste_back call per face layer in order (layer k = face k of each of the batch's frames) and the frames brought to the host
    summary: fps of output frames for both, C / D, the bytes uploaded per output frame (computed from the shapes), and whether
    the two produced the same bytes on the first batch (checked outside the timed region)
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


def implied_clock_ghz(ops, dev, seconds=0.3):
    sink = torch.empty(256 * ops.device_cu_count(), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_mfma = ops.mfma_stream(4000, False, sink)
    torch.cuda.synchronize()
    reps = max(2, int(seconds / max(1e-4, time.perf_counter() - t0)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.mfma_stream(4000, False, sink)
    e1.record()
    torch.cuda.synchronize()
    return round(n_mfma * reps * 32.0 / (e0.elapsed_time(e1) * 1e-3) / (ops.device_cu_count() * 4) / 1e9, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--cases", default="ab")
    ap.add_argument("--formats", default="rgb8,nv12")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faces_bench.jsonl"))
    a = ap.parse_args()
    from emoportraits_amd import config, ops, random_init
    from emoportraits_amd import embedders as E
    from emoportraits_amd.infer import InferenceWrapper
    S, B, Hf, Wf, N, K = 512, 16, 1080, 1920, a.frames, 4
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
                         print_params=False, head_pose_regressor_path=os.path.join(root, "hp.pth"), identity_capacity=K)
    dev = w.device
    g = torch.Generator().manual_seed(5)
    w.enrol_identities(torch.rand(K, 3, S, S, generator=g), source_masks=[torch.ones(1, 1, S, S)] * K, batch_size=K)
    w.load_identity(0)
    distinct = torch.randint(0, 256, (32, Hf, Wf, 3), generator=g, dtype=torch.uint8)
    pictures = {"rgb8": distinct,
                "nv12": torch.cat([ops.pack_nv12(ops.unpack_rgb8(distinct[i:i + 8].to(dev))).cpu() for i in range(0, 32, 8)])}

    def clip(fmt, n):
        out = torch.empty((n,) + tuple(pictures[fmt].shape[1:]), dtype=torch.uint8, pin_memory=True)
        for i in range(0, n, 32):
            out[i:i + 32].copy_(pictures[fmt][:min(32, n - i)])
        return out

    wins = []
    for i in range(N):
        s = 300 + (600 * (i % B)) // (B - 1)                      # every batch holds the whole spread of sides
        wins.append((int(torch.randint(0, Wf - s + 1, (1,), generator=g)), int(torch.randint(0, Hf - s + 1, (1,), generator=g)), s))
    n4 = N // K
    faces4 = []
    for i in range(n4):                                           # four windows around the centre: every pair overlaps
        of_frame = []
        for k in range(K):
            s = 420 + 60 * ((i + k) % K)
            of_frame.append((Wf // 2 - s // 2 + (120 if k & 1 else -120) + i % 7, Hf // 2 - s // 2 + (90 if k & 2 else -90) - i % 5, s))
        assert all(abs(p[0] - q[0]) < min(p[2], q[2]) and abs(p[1] - q[1]) < min(p[2], q[2]) for p in of_frame for q in of_frame)
        faces4.append(of_frame)
    flat4 = [f for of_frame in faces4 for f in of_frame]
    frame_of4 = [i for i in range(n4) for _ in range(K)]
    ids4 = [m % K for m in range(len(flat4))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return got, time.perf_counter() - t0

    def stream(frames, keep=0, **kw):
        """drain animate_frames -> (frames yielded, the first `keep` of them copied)"""
        n, kept = 0, []
        for _, out in w.animate_frames(frames, batch_size=B, paste_back=True, **kw):
            if n < keep:
                kept.append(out.clone())
            n += out.shape[0]
        return n, kept

    def parent_way(frames, dup, fkw, keep=0):
        n, kept = 0, []
        for m0, img in w.animate_frames(dup, batch_size=B, windows=flat4, identities=ids4, as_uint8=False, to_host=False, **fkw):
            f0, nf = m0 // K, img.shape[0] // K
            cur = frames[f0:f0 + nf]
            for k in range(K):                                     # layer k: face k of each of the batch's frames
                cur = w.paste_back(cur, img[k::K], [flat4[m0 + K * j + k] for j in range(nf)], **fkw)
            out = cur.cpu()
            if n < keep:
                kept.append(out)
            n += nf
        return n, kept

    base = {"tool": "bench_faces", "label": a.label, "image_size": S, "batch": B, "frame_size": [Hf, Wf],
            "precision": w.hot_path.precision, "graphs": w.use_graphs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    with open(a.out, "a") as f:
        def emit(rec):
            rec = {**base, "time": time.strftime("%Y-%m-%dT%H:%M:%S"), **rec}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()

        for fmt in a.formats.split(","):
            fkw = dict(frame_format="nv12") if fmt == "nv12" else {}
            frame_bytes = pictures[fmt][0].numel()
            variants, extra, n_out = {}, {}, N
            for case in a.cases:
                if case == "a":
                    frames = clip(fmt, N)
                    variants = {"A": lambda: stream(frames, windows=wins, **fkw)[0],
                                "B": lambda: stream(frames, faces=[[x] for x in wins], **fkw)[0]}
                    n_out, extra = N, {"faces_per_frame": 1}
                else:
                    frames = clip(fmt, n4)
                    dup = torch.empty((len(flat4),) + tuple(frames.shape[1:]), dtype=torch.uint8, pin_memory=True)
                    dup.copy_(frames[frame_of4])
                    variants = {"C": lambda: stream(frames, faces=faces4, identities=ids4, **fkw)[0],
                                "D": lambda: parent_way(frames, dup, fkw)[0]}
                    same = torch.equal(torch.cat(stream(frames, keep=B // K, faces=faces4, identities=ids4, **fkw)[1])[:B // K],
                                       torch.cat(parent_way(frames, dup, fkw, keep=B // K)[1])[:B // K])
                    n_out = n4
                    extra = {"faces_per_frame": K, "same_bytes_first_batch": same,
                             "bytes_uploaded_per_output_frame": {"C": frame_bytes, "D": (K + 1) * frame_bytes}}
                clock_before = implied_clock_ghz(ops, dev)
                fps = {v: [] for v in variants}
                for v, fn in variants.items():
                    assert fn() == n_out                              # warm-up
                for rep in range(a.reps):
                    for v, fn in variants.items():
                        got, dt = timed(fn)
                        assert got == n_out
                        fps[v].append(n_out / dt)
                        emit({"case": case, "format": fmt, "variant": v, "rep": rep, "frames": n_out, "fps": round(n_out / dt, 2)})
                x, y = list(variants)
                emit({"case": case, "format": fmt, "variant": "summary", "frames": n_out, **extra,
                      f"fps_{x}_median": round(med(fps[x]), 2), f"fps_{x}_runs": [round(v, 2) for v in fps[x]],
                      f"fps_{y}_median": round(med(fps[y]), 2), f"fps_{y}_runs": [round(v, 2) for v in fps[y]],
                      f"{'B_over_A' if case == 'a' else 'C_over_D'}": round(med(fps["B" if case == "a" else "C"]) / med(fps[x if case == "a" else y]), 4),
                      f"{x}_max_over_min": round(max(fps[x]) / min(fps[x]), 4),
                      "implied_clock_ghz_before_after": [clock_before, implied_clock_ghz(ops, dev)]})


if __name__ == "__main__":
    main()
