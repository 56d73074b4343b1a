"""Video streams of different frame sizes in one driver batch: InferenceWrapper.animate_streams against what the commit before it
offers for the same frames.

    python tools/bench_streams.py [--reps 4] [--ticks 8] [--cases ab] [--formats rgb8,nv12] [--label TEXT] [--out profiles/streams_bench.jsonl]

Seeded trained-like R512 checkpoint with seeded embedder weights (tools/bench_faces.py's), default precision and graphs, B = 16,
16 streams of --ticks frames each in pinned host memory, one face per frame (sides 300 ... 900 clipped to the frame, at seeded
places), a bank of 4 identities, stream k on slot k % 4.  One JSON line per run, the variants of a case alternating within one
process after one warm-up run each; a summary line per case, format and output; the clock implied by a bare MFMA stream in front
of and behind every case.  Every case runs with the crops coming out through the ring ('crops') and with paste_back=True ('paste').
  case a, the control -- all 16 streams 1080 x 1920:
    A   animate_frames(clip, windows=..., identities=...)   the same frames as ONE clip in tick order: the uniform path, unchanged
    B   animate_streams(streams)                            the same frames through the frame table and the arena
    summary: B / A beside the spread A shows against itself in the same alternation (max / min of its runs)
  case b, mixed -- 4 streams each of 480 x 640, 720 x 1280, 1080 x 1920 and 2160 x 3840:
    C   animate_streams(streams)                            one batch of 16 faces per tick
    D   the way without the feature, for throughput: each stream through its own animate_frames(batch_size=16), one after another
    E   the way without the feature, for latency: per tick 16 calls of animate_frames on one frame each
    summary: frames/s of C and D, C / D, and the time per tick of C and E
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_faces import implied_clock_ghz  # noqa: E402

SIZES = {"a": [(1080, 1920)] * 16, "b": [(480, 640)] * 4 + [(720, 1280)] * 4 + [(1080, 1920)] * 4 + [(2160, 3840)] * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--ticks", type=int, default=8)
    ap.add_argument("--cases", default="ab")
    ap.add_argument("--formats", default="rgb8,nv12")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_bench.jsonl"))
    a = ap.parse_args()
    from emoportraits_amd import config, ops, random_init
    from emoportraits_amd import embedders as E
    from emoportraits_amd.infer import InferenceWrapper
    S, B, T, K = 512, 16, a.ticks, 4
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

    def make_streams(sizes, fmt):
        """16 streams of T frames in pinned memory: two distinct random pictures per size, repeated; one window per frame"""
        streams, pictures = [], {}
        for k, (H, W) in enumerate(sizes):
            if (H, W) not in pictures:
                rgb = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
                pictures[(H, W)] = rgb if fmt == "rgb8" else ops.pack_nv12(ops.unpack_rgb8(rgb.to(dev))).cpu()
            pic = pictures[(H, W)]
            frames = torch.empty((T,) + tuple(pic.shape[1:]), dtype=torch.uint8, pin_memory=True)
            for t in range(T):
                frames[t].copy_(pic[(t + k) % 2])
            wins = []
            for t in range(T):
                s = min(300 + (600 * ((t + k) % B)) // (B - 1), H, W)
                wins.append((int(torch.randint(0, W - s + 1, (1,), generator=g)), int(torch.randint(0, H - s + 1, (1,), generator=g)), s))
            streams.append(dict(frames=frames, windows=wins, identities=k % K))
        return streams

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return got, time.perf_counter() - t0

    def frames_out(gen):
        return sum(t.shape[0] for _, t in gen)

    base = {"tool": "bench_streams", "label": a.label, "image_size": S, "batch": B, "streams": 16, "ticks": T,
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
            for case in a.cases:
                streams = make_streams(SIZES[case], fmt)
                n_out = 16 * T
                for output, okw in (("crops", {}), ("paste", dict(paste_back=True))):
                    kw = dict(batch_size=B, **okw, **fkw)
                    mixed = lambda: sum(len(batch) for batch in w.animate_streams(streams, **kw))
                    if case == "a":
                        clip = torch.empty((n_out,) + tuple(streams[0]["frames"].shape[1:]), dtype=torch.uint8, pin_memory=True)
                        for t in range(T):
                            for k, st in enumerate(streams):
                                clip[16 * t + k].copy_(st["frames"][t])
                        wins = [st["windows"][t] for t in range(T) for st in streams]
                        ids = [st["identities"] for t in range(T) for st in streams]
                        variants = {"A": lambda: frames_out(w.animate_frames(clip, windows=wins, identities=ids, **kw)), "B": mixed}
                    else:
                        def per_stream():
                            return sum(frames_out(w.animate_frames(st["frames"], windows=st["windows"], identities=[st["identities"]] * T, **kw))
                                       for st in streams)

                        def per_tick():
                            return sum(frames_out(w.animate_frames(st["frames"][t:t + 1], windows=st["windows"][t:t + 1],
                                                                    identities=[st["identities"]], **kw))
                                       for t in range(T) for st in streams)
                        variants = {"C": mixed, "D": per_stream, "E": per_tick}
                    clock_before = implied_clock_ghz(ops, dev)
                    secs = {v: [] for v in variants}
                    for v, fn in variants.items():
                        assert fn() == n_out                          # warm-up
                    for rep in range(a.reps):
                        for v, fn in variants.items():
                            got, dt = timed(fn)
                            assert got == n_out
                            secs[v].append(dt)
                            emit({"case": case, "format": fmt, "output": output, "variant": v, "rep": rep, "frames": n_out,
                                  "fps": round(n_out / dt, 2), "ms_per_tick": round(1e3 * dt / T, 3)})
                    fps = {v: [n_out / dt for dt in secs[v]] for v in variants}
                    x, y = list(variants)[:2]
                    rec = {"case": case, "format": fmt, "output": output, "variant": "summary", "frames": n_out,
                           "sizes": sorted(set(SIZES[case])), "implied_clock_ghz_before_after": [clock_before, implied_clock_ghz(ops, dev)]}
                    for v in variants:
                        rec[f"fps_{v}_median"] = round(med(fps[v]), 2)
                        rec[f"fps_{v}_runs"] = [round(r, 2) for r in fps[v]]
                        rec[f"ms_per_tick_{v}_median"] = round(1e3 * med(secs[v]) / T, 3)
                    if case == "a":
                        rec["B_over_A"] = round(med(fps["B"]) / med(fps["A"]), 4)
                        rec["A_max_over_min"] = round(max(fps["A"]) / min(fps["A"]), 4)
                    else:
                        rec["C_over_D"] = round(med(fps["C"]) / med(fps["D"]), 4)
                        rec["tick_E_over_C"] = round(med(secs["E"]) / med(secs["C"]), 4)
                    emit(rec)
                del streams


if __name__ == "__main__":
    main()
