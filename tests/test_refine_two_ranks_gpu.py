"""animate_frames(refine=True, paste_back=True) under world size 2 (the pattern of tests/test_paste_back_two_ranks_gpu.py: two
fresh processes, gloo on ONE GPU).  32 full frames in two chunks, batch_size=4, smooth_pose=True: each rank renders, refines and
pastes its own contiguous shard of every chunk -- the stage-2 pass adds no collective -- and the union of the two ranks' full
frames equals the one-rank result BIT FOR BIT (shards of 8 frames: the same batches of 4 in both runs)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

N_FRAMES = 32
WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emoportraits_amd import parallel
import torch
from notebooks.infer import InferenceWrapper
from notebooks.infer_s2 import InferenceWrapper as InferenceWrapperS2
from test_infer_gpu import _toy_embedders
from test_refine_gpu import MASKS
tiny = torch.load(os.path.join(%(root)r, "tests", "golden", "tiny_hotpath.pt"), weights_only=False)
num_gpus = int(os.environ["WORLD_SIZE"])
w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=%(project)r, folder="logs",
                     print_params=False, num_gpus=num_gpus, use_graphs=True)
w.embedders.update(_toy_embedders(tiny, w.device))
w2 = InferenceWrapperS2(experiment_name="exp2", model_file_name="m.pth", project_dir=%(project)r, embedders=MASKS)
assert w2.device == w.device
w.attach_stage2(w2)
S = tiny["cfg"]["image_size"]
if w.rank == 0:
    w.forward(source_image=tiny["img"], crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=tiny["idt_embed"],
              custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=tiny["theta_src"])
if num_gpus > 1:
    w.share_source(src_rank=0)
N = %(n)d
Hf, Wf = S + S // 2 + 3, 2 * S + 5
g = torch.Generator().manual_seed(29)
frames = torch.randint(0, 256, (N, Hf, Wf, 3), generator=g, dtype=torch.uint8)
wins = []
for n in range(N):
    s = S // 2 + ((Hf - S // 2) * n) // (N - 1)
    wins.append((min(Wf - s, 3 * n + 1), min(Hf - s, 2 * n), s))
before = frames.clone()
out = {}
for b0, full in w.animate_frames([frames[:N // 2], frames[N // 2:]], batch_size=4, ring=2, windows=wins, smooth_pose=True,
                                 refine=True, paste_back=True):
    for j in range(full.shape[0]):
        out[b0 + j] = full[j].clone()
assert torch.equal(frames, before)
plain = {}
if num_gpus == 1:
    w.theta = None
    for b0, full in w.animate_frames([frames[:N // 2], frames[N // 2:]], batch_size=4, ring=2, windows=wins, smooth_pose=True,
                                     paste_back=True):
        for j in range(full.shape[0]):
            plain[b0 + j] = full[j].clone()
torch.save(dict(frames=out, plain=plain, input=frames, wins=wins), os.path.join(%(project)r, "refine_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def test_two_ranks_refine_and_paste_back_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from emoportraits_amd import parallel
    from test_two_ranks_gpu import _free_port, _project
    project = _project(tmp_path, golden_dir)
    tiny2 = torch.load(os.path.join(golden_dir, "tiny_stage2.pt"), weights_only=False)
    exp2 = tmp_path / "logs_s2" / "exp2"
    (exp2 / "checkpoints").mkdir(parents=True)
    with open(exp2 / "args.txt", "wt") as f:
        for k, v in tiny2["cfg"].items():
            f.write(f"{k}: {v}\n")
    torch.save(tiny2["state_dict"], exp2 / "checkpoints" / "m.pth")

    def spawn(world):
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port))
            for k in ("EMO_DIST_BACKEND", "EMO_FORCE_DEVICE", "EMO_DIST_FORCE_INIT"):
                env.pop(k, None)
            if world > 1:
                env.update(EMO_FORCE_DEVICE="0", EMO_DIST_BACKEND="gloo")
            procs.append(subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT, project=project, n=N_FRAMES)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=300)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0 and "WORKER_OK" in o, o[-4000:]
        return [torch.load(os.path.join(project, f"refine_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    single = spawn(1)[0]
    ranks = spawn(2)
    assert sorted(single["frames"]) == list(range(N_FRAMES))
    half = N_FRAMES // 2
    covered = []
    for r, out in enumerate(ranks):
        want = []
        for base in (0, half):
            lo, hi = parallel.shard_range(half, r, 2)
            want += list(range(base + lo, base + hi))
        assert sorted(out["frames"]) == want, (r, sorted(out["frames"]))                     # its shard of every chunk, nothing else
        for i, frame in out["frames"].items():
            assert torch.equal(frame, single["frames"][i]), f"frame {i} of rank {r} differs from the single-rank run"
        covered += list(out["frames"])
    assert sorted(covered) == list(range(N_FRAMES))
    # (and the frames were refined and pasted into: inside its window a frame differs from the input and from the unrefined paste,
    # outside it does not)
    for i, (x0, y0, s) in enumerate(single["wins"]):
        got, src = single["frames"][i], single["input"][i]
        assert tuple(got.shape) == tuple(src.shape)
        mask = torch.ones(src.shape[:2], dtype=torch.bool)
        mask[y0:y0 + s, x0:x0 + s] = False
        assert torch.equal(got[mask], src[mask]) and not torch.equal(got, src), i
        assert not torch.equal(got, single["plain"][i]), i
