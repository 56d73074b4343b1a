"""animate_frames(tracking=dict(follow_tracks=True)) under world size 2 (the pattern of
tests/test_head_pose_controls_two_ranks_gpu.py: fresh processes, gloo on ONE GPU).  The birth clip of
tests/test_track_controls_gpu.py -- a face leaves, its track dies, another is born into its slot -- with smooth_pose, a relative
expression and a relative head pose: every rank tracks the whole chunk, so every rank holds the restart and present masks of all
its rows, and the three controls run over the gathered rows of the chunk on every rank.  The thetas and the expressions every rank
rendered with, and the frames, equal the one-rank run's BIT FOR BIT, and so do the streams' states.  12 frames with batches of
three frames (six rows): the ranks' shards (6 + 6) form the batches of the one-rank run."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

N, H, W = 12, 96, 128
WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emoportraits_amd import parallel
import torch
from notebooks.infer import InferenceWrapper
from test_infer_gpu import _toy_embedders
from test_head_pose_controls_two_ranks_gpu import source_of
from test_track_controls_two_ranks_gpu import birth_clip
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
clip, dets = birth_clip()
seen = dict(theta=[], pose=[])
drive_bank = w._drive_bank
def recorded(pose, theta, ident):
    seen["theta"].append(theta.clone()), seen["pose"].append(pose.clone())
    return drive_bank(pose, theta, ident)
w._drive_bank = recorded
rows, imgs = [], []
for m0, img in w.animate_frames(clip, detections=dets, tracking=dict(tracks=2, min_iou=0.2, max_missed=2, smooth=True, momentum=0.5,
                                                                      follow_tracks=True),
                                identities=[0, 1] * clip.shape[0], batch_size=6, smooth_pose=True, smooth_per_identity=True,
                                expression=dict(relative=True, smooth=True), head_pose=dict(relative=True), to_host=False, as_uint8=False):
    rows += list(range(m0, m0 + img.shape[0]))
    imgs.append(img.cpu().clone())
theta, pose, imgs = torch.cat(seen["theta"]).cpu(), torch.cat(seen["pose"]).cpu(), torch.cat(imgs)
assert theta.shape[0] == pose.shape[0] == len(rows)
out = {i: (theta[j].clone(), pose[j].clone(), imgs[j].clone()) for j, i in enumerate(rows)}
st = w._bank_streams
state = [t.cpu().clone() for t in (st.theta, st.theta_has, st.pose_anchor, st.pose_anchor_has, st.expr_anchor, st.expr_anchor_has, st.expr_ema,
                                   st.expr_ema_has)]
present = w.tracked_present[0].cpu().clone()
torch.save(dict(rows=out, state=state, present=present), os.path.join(%(project)r, "tc_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def birth_clip():
    """-> (clip uint8 [12,96,128,3], dets float64 [12,3,4]): face A in frames 0 ... 3, nobody in frames 4 ... 6, face C from frame 7
    (with max_missed = 2 born into A's slot), face E from frame 9"""
    from test_crop_track_gpu import _clip, _walk
    clip = _clip(N, H, W, "rgb8", 51)
    A, Cf, E = _walk(N, W, H, 52, 0.4, 0.5, -0.2), _walk(N, W, H, 53, 0.4, 0.5, 0.2), _walk(N, W, H, 60, 0.35, 0.45, -0.15)
    dets = np.full((N, 3, 4), np.nan)
    dets[:4, 1], dets[7:, 2], dets[9:, 0] = A[:4], Cf[7:], E[9:]
    return clip, torch.from_numpy(dets)


def test_two_ranks_follow_the_tracks_one_gpu_gloo(tmp_path, golden_dir):
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
            procs.append(subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT, project=project)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=300)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0 and "WORKER_OK" in o, "\n".join(t[-3000:] for t in outs)
        return [torch.load(os.path.join(project, f"tc_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    bits = lambda t: t.contiguous().view(torch.int32)
    single = spawn(1)[0]
    ranks = spawn(2)
    assert sorted(single["rows"]) == list(range(2 * N))
    assert single["present"].reshape(N, 2)[:, 0].tolist() == [1] * 4 + [0] * 3 + [1] * 5
    assert single["present"].reshape(N, 2)[:, 1].tolist() == [0] * 9 + [1] * 3
    assert single["state"][1].tolist() == [1, 1] and single["state"][3].tolist() == [1, 1]
    covered = []
    for r, out in enumerate(ranks):
        lo, hi = parallel.shard_range(N, r, 2)
        assert sorted(out["rows"]) == list(range(2 * lo, 2 * hi)), r
        assert torch.equal(out["present"], single["present"])          # every rank tracked the whole chunk
        for i, (theta, pose, img) in out["rows"].items():
            assert torch.equal(bits(theta), bits(single["rows"][i][0])), f"the theta of row {i} on rank {r} differs"
            assert torch.equal(bits(pose), bits(single["rows"][i][1])), f"the expression of row {i} on rank {r} differs"
            assert torch.equal(bits(img), bits(single["rows"][i][2])), f"row {i} of rank {r} was rendered differently"
        covered += list(out["rows"])
        for j in (1, 3, 5, 7):
            on = single["state"][j] != 0
            assert torch.equal(out["state"][j], single["state"][j]), (r, j)
            assert torch.equal(bits(out["state"][j - 1][on]), bits(single["state"][j - 1][on])), (r, j)
    assert sorted(covered) == list(range(2 * N))
