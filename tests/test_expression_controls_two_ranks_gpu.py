"""animate_frames(expression=) under world size 2 (the pattern of tests/test_faces_two_ranks_gpu.py: fresh processes, gloo on ONE
GPU).  Relative transfer and smoothing walk the frame order, so on two ranks the expressions of both shards are gathered in row
order (parallel.gather_rows) and scanned on every rank: the controlled expressions, the frames and the slots' states after the
call equal the one-rank run BIT FOR BIT.  Two chunks of 12 frames with batch_size=3: the ranks' shards (6 + 6) form the batches of
the one-rank run, so every frame is rendered by the same launches in both.  The first call also smooths the pose (the thetas come
from the gathered scan), the second does not (the expression pass regresses them), and continues the first one's streams."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

N = 12
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
                     print_params=False, num_gpus=num_gpus, use_graphs=True, identity_capacity=2)
w.embedders.update(_toy_embedders(tiny, w.device))
S, E = tiny["cfg"]["image_size"], tiny["cfg"]["lpe_output_channels_expression"]
g = torch.Generator().manual_seed(23)
for k in range(2):
    idt = (tiny["idt_embed"] + 0.2 * k * torch.randn(tiny["idt_embed"].shape, generator=g)).contiguous()
    neutral = (tiny["source_pose_embed"] + 0.3 * k * torch.randn(tiny["source_pose_embed"].shape, generator=g)).contiguous()
    img = (tiny["img"] + 0.1 * k * torch.randn(tiny["img"].shape, generator=g)).clamp(0, 1).contiguous()   # (every rank draws the same)
    if w.rank == 0:
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=neutral, custome_source_theta_embed=tiny["theta_src"])
        assert w.store_identity(k) == k
    if num_gpus > 1:
        w.share_identity(k, src_rank=0)
    assert torch.equal(w._bank_expr[k].cpu(), neutral[0]) and w._bank_expr_has[k]
n = %(n)d
clip = (torch.rand(2 * n, S, S, 3, generator=torch.Generator().manual_seed(31)) * 255).to(torch.uint8)
ids = [(3 * m + m // 5) %% 2 for m in range(2 * n)]
gain, offset = torch.rand(2 * n, generator=g) * 2, 0.2 * torch.randn(2 * n, E, generator=g)
last = {}
drive_bank = w._drive_bank
def recorded(pose, theta, ident):
    last["pose"] = pose.clone()
    return drive_bank(pose, theta, ident)
w._drive_bank = recorded
out = {}
for call, kw in enumerate((dict(mix=True, smooth_pose=True, smooth_per_identity=True), {})):
    ex = dict(relative=True, gain=gain, offset=offset, smooth=True, momentum=0.3)
    for b0, img in w.animate_frames([clip[:n], clip[n:]], batch_size=3, identities=ids, expression=ex, to_host=False, as_uint8=False, **kw):
        for j in range(img.shape[0]):
            out[(call, b0 + j)] = (last["pose"][j].cpu().clone(), img[j].cpu().clone())
state = [t.cpu().clone() for t in (w._bank_streams.expr_anchor, w._bank_streams.expr_anchor_has, w._bank_streams.expr_ema, w._bank_streams.expr_ema_has)]
torch.save(dict(rows=out, state=state), os.path.join(%(project)r, "expr_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def test_two_ranks_expression_controls_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from emoportraits_amd import parallel
    from test_two_ranks_gpu import _free_port, _project
    one_rank = [(b0, min(b0 + 3, N)) for b0 in range(0, N, 3)]
    two_ranks = [(b0, min(b0 + 3, hi)) for lo, hi in (parallel.shard_range(N, r, 2) for r in range(2)) for b0 in range(lo, hi, 3)]
    assert one_rank == two_ranks                                      # the premise: both runs form the same batches
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
            procs.append(subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT, project=project, n=N)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=300)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0 and "WORKER_OK" in o, "\n".join(t[-3000:] for t in outs)
        return [torch.load(os.path.join(project, f"expr_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    bits = lambda t: t.contiguous().view(torch.int32)
    single = spawn(1)[0]
    ranks = spawn(2)
    assert sorted(single["rows"]) == [(c, i) for c in range(2) for i in range(2 * N)]
    covered = []
    for r, out in enumerate(ranks):
        lo, hi = parallel.shard_range(N, r, 2)
        mine = list(range(lo, hi)) + list(range(N + lo, N + hi))
        assert sorted(out["rows"]) == [(c, i) for c in range(2) for i in mine], (r, sorted(out["rows"]))
        for key, (pose, img) in out["rows"].items():
            assert torch.equal(bits(pose), bits(single["rows"][key][0])), f"the expression of row {key} on rank {r} differs from the single-rank run"
            assert torch.equal(bits(img), bits(single["rows"][key][1])), f"frame {key} of rank {r} differs from the single-rank run"
        covered += list(out["rows"])
        for a, b in zip(out["state"], single["state"]):                   # the slots' anchors and EMAs: equal on both ranks
            assert torch.equal(a, b) if a.dtype == torch.int32 else torch.equal(bits(a), bits(b)), r
    assert len(covered) == 4 * N
    assert single["state"][1].tolist() == [1, 1] and single["state"][3].tolist() == [1, 1]
    # (the controls did something: the rows of the two calls differ although the frames are the same)
    assert not torch.equal(single["rows"][(0, 5)][0], single["rows"][(1, 5)][0])
