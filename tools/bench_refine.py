"""Refined video, frames in -> frames out: stage 2 inside animate_frames against stage 2 called by hand after it.

    python tools/bench_refine.py [--mode all|separate|inpath|stage1] [--frames 192] [--batch 16] [--rounds 3] [--size 512]

Seeded random weights of the released shapes (the wrapper bench.py builds: hot path + both native embedders + head-pose
regressor; stage 2 at --size), full frames of (size + 64) x (size + 192) bytes with one size x size crop window each, toy mask
callables (a few torch element-wise launches per batch, the same in every mode).  One JSON line per measurement:
  separate   what refined video took before refine=True existed, written with those calls only (so this file runs on an older
             checkout with --mode separate): animate_frames(as_uint8=False, to_host=False) -> clone -> stage2.InferenceWrapper
             .forward -> the refined bytes D2H through two pinned buffers
  inpath     animate_frames(refine=True): crops through the pinned ring; and the same with paste_back=True (full frames)
  stage1     animate_frames alone (no refinement), for the ratio
  all        stage1 once, then separate / inpath alternated --rounds times, and a summary line with the spread of each
Every mode first runs three batches (eager call, graph capture, replay) that are not timed.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def matting(img):
    return (img.mean(1, keepdim=True) * 1.6 - 0.3).clamp(0, 1)


def face_parsing(img):
    return (img[:, 1:2] > 0.35).float()


def build(S):
    from emoportraits_amd import config, random_init, stage2
    from emoportraits_amd import embedders as E
    from notebooks.infer import InferenceWrapper
    cfg = config.hot_path_config(overrides={"image_size": S})
    ecfg = E.embedder_config()
    full = dict(random_init.trained_like_state_dict(cfg, seed=0))
    full.update(E.random_state_dict(E.idt_schema(ecfg), 1))
    full.update(E.random_state_dict(E.expression_schema(ecfg), 2))
    hp_sd = E.random_state_dict(E.head_pose_schema(), 3)
    hp_sd["fc.weight"] *= 0.05
    hp_sd["fc.bias"] = torch.tensor([1.0, 1.0, 1.0, 0.1, -0.2, 0.05, 0.02, -0.03, 0.01])
    root = tempfile.mkdtemp()
    os.makedirs(os.path.join(root, "logs", "exp", "checkpoints"))
    with open(os.path.join(root, "logs", "exp", "args.txt"), "wt") as f:
        for k, v in {**cfg, **ecfg}.items():
            f.write(f"{k}: {v}\n")
    torch.save(hp_sd, os.path.join(root, "hp.pth"))
    w = InferenceWrapper(experiment_name="exp", model_file_name="x", project_dir=root, folder="logs", state_dict=full,
                         print_params=False, head_pose_regressor_path=os.path.join(root, "hp.pth"))
    g = torch.Generator().manual_seed(13)
    w.forward(source_image=torch.rand(1, 3, S, S, generator=g), crop=False, source_mask=torch.ones(1, 1, S, S))
    s2cfg = stage2.stage2_config(overrides=dict(output_size_s2=S))
    os.makedirs(os.path.join(root, "logs_s2", "exp2", "checkpoints"))
    with open(os.path.join(root, "logs_s2", "exp2", "args.txt"), "wt") as f:
        for k, v in s2cfg.items():
            f.write(f"{k}: {v}\n")
    w2 = stage2.InferenceWrapper(experiment_name="exp2", model_file_name="x", project_dir=root,
                                 state_dict=stage2.random_state_dict(s2cfg, seed=0),
                                 embedders={"matting": matting, "face_parsing": face_parsing})
    return w, w2


def timed(run, frames, B, n_warm=3):
    """frames/s of run(frames) after n_warm untimed batches; run returns the number of frames it delivered to the host"""
    run(frames[:n_warm * B])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = run(frames)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "separate", "inpath", "stage1"])
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    S, B = a.size, a.batch
    w, w2 = build(S)
    Hf, Wf = S + 64, S + 192
    frames = torch.randint(0, 256, (a.frames, Hf, Wf, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).pin_memory()
    wins = [(96, 32, S)] * a.frames
    pinned = [torch.empty((B, S, S, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]

    def separate(fr):
        events, n = [None, None], 0
        for k, (b0, img) in enumerate(w.animate_frames(fr, batch_size=B, windows=wins[:fr.shape[0]], to_host=False, as_uint8=False)):
            u8 = w2.forward(img.clone())[2]
            slot = k % 2
            if events[slot] is not None:
                events[slot].synchronize()                      # (the host has consumed this buffer's previous batch)
            pinned[slot][:u8.shape[0]].copy_(u8, non_blocking=True)
            events[slot] = torch.cuda.Event()
            events[slot].record()
            n += u8.shape[0]
        return n

    def inpath(fr, **kw):
        return sum(o.shape[0] for _, o in w.animate_frames(fr, batch_size=B, windows=wins[:fr.shape[0]], refine=True, **kw))

    def stage1(fr):
        return sum(o.shape[0] for _, o in w.animate_frames(fr, batch_size=B, windows=wins[:fr.shape[0]]))

    base = dict(image_size=S, batch=B, frames=a.frames, frame_bytes=[Hf, Wf, 3], precision=w.hot_path.precision,
                device=torch.cuda.get_device_name(0))
    emit = lambda what, fps, **kw: print(json.dumps(dict(base, what=what, fps=round(fps, 2), **kw)), flush=True)
    if a.mode in ("inpath", "all"):
        w.attach_stage2(w2)
    if a.mode == "separate":
        emit("separate", timed(separate, frames, B))
    elif a.mode == "inpath":
        emit("inpath", timed(inpath, frames, B))
        emit("inpath_paste_back", timed(lambda fr: inpath(fr, paste_back=True), frames, B))
    elif a.mode == "stage1":
        emit("stage1", timed(stage1, frames, B))
    else:
        emit("stage1", timed(stage1, frames, B))
        runs = {"separate": [], "inpath": [], "inpath_paste_back": []}
        for r in range(a.rounds):
            for what, fn in (("separate", separate), ("inpath", inpath), ("inpath_paste_back", lambda fr: inpath(fr, paste_back=True))):
                runs[what].append(timed(fn, frames, B))
                emit(what, runs[what][-1], round=r)
        summary = {k: dict(min=round(min(v), 2), max=round(max(v), 2), mean=round(sum(v) / len(v), 2)) for k, v in runs.items()}
        print(json.dumps(dict(base, what="summary", rounds=a.rounds, fps=summary)), flush=True)


if __name__ == "__main__":
    main()
