"""The identity bank under world size 2 (the pattern of tests/test_two_ranks_gpu.py: two fresh processes, gloo on one GPU): rank 0
enrols three identities and share_identity() broadcasts each slot; both ranks run animate and animate_frames with per-frame
identities.  The union of the shards must equal BIT FOR BIT one rank walking the same shards itself."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

N_FRAMES = 33

WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emoportraits_amd import parallel
import torch
from notebooks.infer import InferenceWrapper
from test_infer_gpu import _toy_embedders
tiny = torch.load(os.path.join(%(root)r, "tests", "golden", "tiny_hotpath.pt"), weights_only=False)
num_gpus = int(os.environ["WORLD_SIZE"])
w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=%(project)r, folder="logs",
                     print_params=False, num_gpus=num_gpus, use_graphs=True, identity_capacity=3)
w.embedders.update(_toy_embedders(tiny, w.device))
S = tiny["cfg"]["image_size"]
g = torch.Generator().manual_seed(23)
for k in range(3):
    idt = (tiny["idt_embed"] + 0.2 * k * torch.randn(tiny["idt_embed"].shape, generator=g)).contiguous()
    if w.rank == 0:
        img = (tiny["img"] + 0.1 * k * torch.randn(tiny["img"].shape, generator=g)).clamp(0, 1).contiguous()
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=tiny["theta_src"])
        assert w.store_identity(k) == k
    if num_gpus > 1:
        w.share_identity(k, src_rank=0)
assert w.identities() == [0, 1, 2]
N = %(n)d
g = torch.Generator().manual_seed(17)
pose = torch.randn(N, tiny["target_pose_embed"].shape[1], generator=g) * 0.5
srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.3 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
frames = (torch.rand(N, S, S, 3, generator=g) * 255).to(torch.uint8)
ids = torch.tensor([(7 * i + i // 5) %% 3 for i in range(N)])
out = {"animate": {}, "animate_frames": {}}
emulate = int(os.environ.get("EMULATE_WORLD", "0"))
spans = [parallel.shard_range(N, r, emulate) for r in range(emulate)] if emulate else [None]
for span in spans:
    sl = slice(None) if span is None else slice(*span)
    off = 0 if span is None else span[0]
    for rep in range(2):                 # second sweep: graph replay
        for b0, u8 in w.animate(pose[sl], [t[sl] for t in srt], batch_size=4, identities=ids[sl]):
            for j in range(u8.shape[0]):
                out["animate"][off + b0 + j] = u8[j].cpu()
    for b0, u8 in w.animate_frames(frames[sl], batch_size=4, ring=2, identities=ids[sl]):
        for j in range(u8.shape[0]):
            out["animate_frames"][off + b0 + j] = u8[j].clone()
torch.save(out, os.path.join(%(project)r, "bank_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def test_two_ranks_bank_share_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from emoportraits_amd import parallel
    from test_two_ranks_gpu import _free_port, _project
    project = _project(tmp_path, golden_dir)

    def spawn(world, emulate=0):
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), EMULATE_WORLD=str(emulate))
            for k in ("EMO_DIST_BACKEND", "EMO_FORCE_DEVICE", "EMO_DIST_FORCE_INIT"):
                env.pop(k, None)
            if world > 1:
                env.update(EMO_FORCE_DEVICE="0", EMO_DIST_BACKEND="gloo")
            procs.append(subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT, project=project, n=N_FRAMES)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=600)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0 and "WORKER_OK" in o, o[-4000:]
        return [torch.load(os.path.join(project, f"bank_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    single = spawn(1, emulate=2)[0]
    ranks = spawn(2)
    for kind in ("animate", "animate_frames"):
        assert sorted(single[kind]) == list(range(N_FRAMES))
        covered = []
        for r, out in enumerate(ranks):
            lo, hi = parallel.shard_range(N_FRAMES, r, 2)
            assert sorted(out[kind]) == list(range(lo, hi)), (kind, r)
            covered += list(out[kind])
            for i, frame in out[kind].items():
                assert torch.equal(frame, single[kind][i]), f"{kind}: frame {i} of rank {r} differs from the single-rank run"
        assert sorted(covered) == list(range(N_FRAMES))
