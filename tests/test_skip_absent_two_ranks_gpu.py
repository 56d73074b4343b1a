"""animate_frames(tracking=dict(skip_absent=True)) under world size 2 (the pattern of tests/test_track_controls_two_ranks_gpu.py:
fresh processes, gloo on ONE GPU).  Two faces as unordered detections with dropouts, follow_tracks with smooth_pose, a smoothed
relative expression and a relative head pose, pasted back: every rank tracks and compacts the whole chunk, the kept rows of every
rank are gathered (sized from `first`, which every rank has), scattered into the chunk's full rows and walked by the three controls
on every rank.  The union of the ranks' pasted frames is the one-rank call's BYTE FOR BYTE, and so are the streams' states.  10
frames, batches of at most 4 kept rows: the ranks' shards (5 + 5 frames) form the batches of the one-rank run."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

N, H, W = 10, 96, 128
COUNT = [1, 1, 1, 2, 1, 2, 1, 1, 2, 2]
WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emoportraits_amd import parallel
import torch
from notebooks.infer import InferenceWrapper
from test_infer_gpu import _toy_embedders
from test_head_pose_controls_two_ranks_gpu import source_of
from test_skip_absent_two_ranks_gpu import dropout_clip
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
clip, dets = dropout_clip()
frames = {}
for f0, out in w.animate_frames(clip, detections=dets, tracking=dict(tracks=2, min_iou=0.2, max_missed=15, smooth=True, momentum=0.5,
                                                                      follow_tracks=True, skip_absent=True),
                                identities=[0, 1] * clip.shape[0], batch_size=4, smooth_pose=True, smooth_per_identity=True,
                                expression=dict(relative=True, smooth=True, momentum=0.4), head_pose=dict(relative=True), to_host=False,
                                paste_back=True):
    for j in range(out.shape[0]):
        frames[f0 + j] = out[j].cpu().clone()
st = w._bank_streams
state = [t.cpu().clone() for t in (st.theta, st.theta_has, st.pose_anchor, st.pose_anchor_has, st.expr_anchor, st.expr_anchor_has, st.expr_ema,
                                   st.expr_ema_has)]
rows = (w.tracked_rows[0].cpu().clone(), w.tracked_rows[1], w.tracked_rows[2])
torch.save(dict(frames=frames, state=state, rows=rows), os.path.join(%(project)r, "sa_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def dropout_clip():
    """-> (clip uint8 [10,96,128,3], dets float64 [10,3,4]): two faces in changing detection rows, face a from frame 0 and dropped
    in frame 4, face b from frame 3 and dropped in frames 6 and 7; with max_missed = 15 no track dies"""
    from test_crop_track_gpu import _clip, _walk
    clip = _clip(N, H, W, "rgb8", 111)
    both = np.stack([_walk(N, W, H, 0, 0.35, 0.45, -0.2), _walk(N, W, H, 1, 0.4, 0.5, 0.2)], 1)
    both[[0, 1, 2, 6, 7], 1] = np.nan
    both[4, 0] = np.nan
    dets = np.full((N, 3, 4), np.nan)
    for t in range(N):
        dets[t, t % 3], dets[t, (t + 1) % 3] = both[t, 1], both[t, 0]
    return clip, torch.from_numpy(dets)


def test_two_ranks_skip_the_absent_rows_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import parallel
    from test_two_ranks_gpu import _free_port, _project
    one_rank = frames_mod.face_spans(COUNT, 0, N, 4)
    two_ranks = [sp for r in range(2) for sp in frames_mod.face_spans(COUNT, *parallel.shard_range(N, r, 2), 4)]
    assert one_rank == two_ranks == [(0, 3), (3, 5), (5, 8), (8, 10)]   # the premise: both runs form the same batches
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
        return [torch.load(os.path.join(project, f"sa_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    bits = lambda t: t.contiguous().view(torch.int32)
    single = spawn(1)[0]
    ranks = spawn(2)
    clip, _ = dropout_clip()
    assert sorted(single["frames"]) == list(range(N)) and single["rows"][1] == frames_mod.face_offsets(COUNT) and single["rows"][2] == 0
    assert all(not torch.equal(single["frames"][t], clip[t]) for t in range(N))     # (somebody in every frame)
    assert all(single["state"][j].tolist() == [1, 1] for j in (1, 3, 5, 7))
    covered = []
    for r, out in enumerate(ranks):
        lo, hi = parallel.shard_range(N, r, 2)
        assert sorted(out["frames"]) == list(range(lo, hi)), r
        assert torch.equal(out["rows"][0], single["rows"][0]) and out["rows"][1:] == single["rows"][1:]   # every rank compacted the whole chunk
        for t, frame in out["frames"].items():
            assert torch.equal(frame, single["frames"][t]), f"frame {t} of rank {r} differs"
        covered += list(out["frames"])
        for j in (1, 3, 5, 7):
            on = single["state"][j] != 0
            assert torch.equal(out["state"][j], single["state"][j]), (r, j)
            assert torch.equal(bits(out["state"][j - 1][on]), bits(single["state"][j - 1][on])), (r, j)
    assert sorted(covered) == list(range(N))
