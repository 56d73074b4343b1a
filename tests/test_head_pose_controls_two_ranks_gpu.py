"""animate_frames(head_pose=) under world size 2 (the pattern of tests/test_expression_controls_two_ranks_gpu.py: fresh processes,
gloo on ONE GPU).  A relative head pose walks the frame order, so on two ranks the regressed (scale, rotation, translation) of
both shards are gathered in row order (parallel.gather_rows) and edited on every rank: the thetas every rank rendered with, on
one rank and on two, equal ops.pose_theta of hostglue.head_pose_controls over the whole clip BIT FOR BIT, across a chunk
boundary, and so do the slots' anchors.  Two chunks of 12 frames with batch_size=3: the ranks' shards (6 + 6) form the batches of
the one-rank run.  A second call also mixes and smooths the pose (the edited thetas go through the gathered scan) and continues
the first one's streams: there the two runs are compared with each other, frames included."""
import os
import sys

import numpy as np
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
from test_head_pose_controls_two_ranks_gpu import controls, source_of
tiny = torch.load(os.path.join(%(root)r, "tests", "golden", "tiny_hotpath.pt"), weights_only=False)
num_gpus = int(os.environ["WORLD_SIZE"])
w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=%(project)r, folder="logs",
                     print_params=False, num_gpus=num_gpus, use_graphs=True, identity_capacity=2)
w.embedders.update(_toy_embedders(tiny, w.device))
S = tiny["cfg"]["image_size"]
g = torch.Generator().manual_seed(23)
for k in range(2):
    idt = (tiny["idt_embed"] + 0.2 * k * torch.randn(tiny["idt_embed"].shape, generator=g)).contiguous()
    img = (tiny["img"] + 0.1 * k * torch.randn(tiny["img"].shape, generator=g)).clamp(0, 1).contiguous()   # (every rank draws the same)
    if w.rank == 0:
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=source_of(k))
        assert w.store_identity(k) == k
    if num_gpus > 1:
        w.share_identity(k, src_rank=0)
    assert torch.equal(w._bank_srt[k].cpu(), torch.cat(source_of(k), 1)[0]) and w._bank_srt_has[k]
n = %(n)d
clip = (torch.rand(2 * n, S, S, 3, generator=torch.Generator().manual_seed(31)) * 255).to(torch.uint8)
ids, gain, rot = controls(2 * n)
seen = dict(srt=[], theta=[])
drive_bank, head_pose = w._drive_bank, w._head_pose
def recorded(pose, theta, ident):
    seen["theta"].append(theta.clone())
    return drive_bank(pose, theta, ident)
def regressed(crops):
    out = head_pose(crops)
    seen["srt"].append(torch.cat([t.clone() for t in out[1:]], 1))
    return out
w._drive_bank, w._head_pose = recorded, regressed
out = {}
for call, kw in enumerate(({}, dict(mix=True, smooth_pose=True, smooth_per_identity=True))):
    seen["srt"].clear(), seen["theta"].clear()
    hp = dict(relative=True, gain=gain, rotation_offset=rot)
    rows, imgs = [], []
    for b0, img in w.animate_frames([clip[:n], clip[n:]], batch_size=3, identities=ids, head_pose=hp, to_host=False, as_uint8=False, **kw):
        rows += list(range(b0, b0 + img.shape[0]))
        imgs.append(img.cpu().clone())
    srt, theta, imgs = torch.cat(seen["srt"]).cpu(), torch.cat(seen["theta"]).cpu(), torch.cat(imgs)
    assert srt.shape[0] == theta.shape[0] == len(rows)
    for j, i in enumerate(rows):
        out[(call, i)] = (srt[j].clone(), theta[j].clone(), imgs[j].clone())
state = [t.cpu().clone() for t in (w._bank_streams.pose_anchor, w._bank_streams.pose_anchor_has)]
torch.save(dict(rows=out, state=state), os.path.join(%(project)r, "hp_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def source_of(k):
    """identity k's source (scale, rotation, translation)"""
    g = torch.Generator().manual_seed(60 + k)
    return 1 + 0.05 * torch.randn(1, 3, generator=g), 0.3 * torch.randn(1, 3, generator=g), 0.05 * torch.randn(1, 3, generator=g)


def controls(n):
    g = torch.Generator().manual_seed(29)
    return [(3 * m + m // 5) % 2 for m in range(n)], torch.rand(n, generator=g) * 2, 0.2 * torch.randn(n, 3, generator=g)


def test_two_ranks_head_pose_controls_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from emoportraits_amd import hostglue, ops, parallel
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
        return [torch.load(os.path.join(project, f"hp_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    bits = lambda t: t.contiguous().view(torch.int32)
    single = spawn(1)[0]
    ranks = spawn(2)
    assert sorted(single["rows"]) == [(c, i) for c in range(2) for i in range(2 * N)]
    # the restatement over the whole clip, from the rows the one-rank run regressed (both calls regress the same frames)
    ids, gain, rot = controls(2 * N)
    srt = torch.stack([single["rows"][(0, i)][0] for i in range(2 * N)]).numpy()
    sources = torch.cat([torch.cat(source_of(k), 1) for k in range(2)]).numpy()
    state = np.zeros((2, 9), np.float32), np.zeros(2, np.int32)
    rows, _ = hostglue.head_pose_controls(srt[:, 0:3], srt[:, 3:6], srt[:, 6:9], ids, sources, gain.numpy(), rot.numpy(), None, None, *state,
                                          True, False)
    dev = torch.from_numpy(rows).to("cuda:0")
    want = ops.pose_theta(*[dev[:, i:i + 3].contiguous() for i in (0, 3, 6)]).cpu()
    covered = []
    for world, outs in ((1, [single]), (2, ranks)):
        for r, out in enumerate(outs):
            lo, hi = parallel.shard_range(N, r, world)
            mine = list(range(lo, hi)) + list(range(N + lo, N + hi))
            assert sorted(out["rows"]) == [(c, i) for c in range(2) for i in mine], (world, r)
            for (call, i), (own, theta, img) in out["rows"].items():
                assert torch.equal(bits(own), bits(single["rows"][(call, i)][0])), f"row {i}: regressed differently on rank {r} of {world}"
                if call == 0:
                    assert torch.equal(bits(theta), bits(want[i])), f"the theta of row {i} on rank {r} of {world} is not the restatement's"
                assert torch.equal(bits(theta), bits(single["rows"][(call, i)][1])), f"the theta of row {(call, i)} on rank {r} differs"
                assert torch.equal(bits(img), bits(single["rows"][(call, i)][2])), f"frame {(call, i)} of rank {r} differs"
            if world == 2:
                covered += list(out["rows"])
            # the slots' anchors: the streams' first rows over the whole clip, on every rank
            assert out["state"][1].tolist() == [1, 1] and torch.equal(bits(out["state"][0]), bits(torch.from_numpy(state[0]))), (world, r)
    assert len(covered) == 4 * N
    # (the edit did something, and the second call's mix and smoothing too)
    assert not torch.equal(single["rows"][(0, 5)][1], single["rows"][(1, 5)][1])
