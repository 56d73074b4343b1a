"""animate_frames(faces=, paste_back=True, smooth_pose=True) under world size 2 (the pattern of
tests/test_paste_back_two_ranks_gpu.py: two fresh processes, gloo on ONE GPU).  Two chunks of the irregular clip -- 2, 0, 3, 1, 0, 2
faces per frame -- with a 2-slot bank, one slot per face, per-identity smoothing: the ranks shard every chunk by FRAMES (3 + 3), take
the faces of their frames (5 + 3), gather the per-face thetas (parallel.gather_rows) and paste their own frames; the union of the
two ranks' frames equals the one-rank result BIT FOR BIT.  batch_size=3 makes the batches of both runs the same -- frames (0,2)
(2,3) (3,6) of a chunk -- so that every face is rendered by the same launches in both."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

COUNTS = [2, 0, 3, 1, 0, 2]
WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emoportraits_amd import parallel
import torch
from notebooks.infer import InferenceWrapper
from test_infer_gpu import _toy_embedders
from test_faces_gpu import faces_clip
tiny = torch.load(os.path.join(%(root)r, "tests", "golden", "tiny_hotpath.pt"), weights_only=False)
num_gpus = int(os.environ["WORLD_SIZE"])
w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=%(project)r, folder="logs",
                     print_params=False, num_gpus=num_gpus, use_graphs=True, identity_capacity=2)
w.embedders.update(_toy_embedders(tiny, w.device))
S = tiny["cfg"]["image_size"]
g = torch.Generator().manual_seed(23)
for k in range(2):
    idt = (tiny["idt_embed"] + 0.2 * k * torch.randn(tiny["idt_embed"].shape, generator=g)).contiguous()
    if w.rank == 0:
        img = (tiny["img"] + 0.1 * k * torch.randn(tiny["img"].shape, generator=g)).clamp(0, 1).contiguous()
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=tiny["theta_src"])
        assert w.store_identity(k) == k
    if num_gpus > 1:
        w.share_identity(k, src_rank=0)
counts = %(counts)r
a, fa = faces_clip(S, counts, seed=41)
b, fb = faces_clip(S, counts, seed=43)
faces = fa + fb
ids = [(3 * m + m // 3) %% 2 for m in range(2 * sum(counts))]
before = (a.clone(), b.clone())
out = {}
for b0, full in w.animate_frames([a, b], batch_size=3, ring=2, faces=faces, identities=ids, mix=True, smooth_pose=True,
                                 smooth_per_identity=True, paste_back=True):
    for j in range(full.shape[0]):
        out[b0 + j] = full[j].clone()
assert torch.equal(a, before[0]) and torch.equal(b, before[1])
torch.save(dict(frames=out, input=torch.cat([a, b])), os.path.join(%(project)r, "faces_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def test_two_ranks_faces_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import parallel
    from test_two_ranks_gpu import _free_port, _project
    n = len(COUNTS)
    one_rank = frames_mod.face_spans(COUNTS, 0, n, 3)
    assert one_rank == [(0, 2), (2, 3), (3, 6)]                       # the premise: both runs form the same batches
    assert one_rank == sum((frames_mod.face_spans(COUNTS, *parallel.shard_range(n, r, 2), 3) for r in range(2)), [])
    project = _project(tmp_path, golden_dir)

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
            procs.append(subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT, project=project, counts=COUNTS)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=300)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0 and "WORKER_OK" in o, o[-4000:]
        return [torch.load(os.path.join(project, f"faces_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    single = spawn(1)[0]
    ranks = spawn(2)
    assert sorted(single["frames"]) == list(range(2 * n))
    covered = []
    for r, out in enumerate(ranks):
        lo, hi = parallel.shard_range(n, r, 2)
        assert sorted(out["frames"]) == list(range(lo, hi)) + list(range(n + lo, n + hi)), (r, sorted(out["frames"]))
        for i, frame in out["frames"].items():
            assert torch.equal(frame, single["frames"][i]), f"frame {i} of rank {r} differs from the single-rank run"
        covered += list(out["frames"])
    assert sorted(covered) == list(range(2 * n))
    # frames without a face come back as they went in, the others were pasted into
    for i in range(2 * n):
        assert torch.equal(single["frames"][i], single["input"][i]) == (COUNTS[i % n] == 0), i
