"""enrol_identities under world size 2 (the pattern of tests/test_identity_bank_two_ranks_gpu.py: two fresh processes, gloo on one
GPU).  Both ranks enrol the same 5 sources with batch_size=2: chunks (0, 2), (2, 4), (4, 5), rank 0 computes the first two and
rank 1 the last, each chunk is broadcast by its owner and written by every rank.  Both banks -- volumes, idt_embed, thetas, used
slots -- must equal each other and a one-rank enrolment BIT FOR BIT."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emoportraits_amd import parallel
import torch
from notebooks.infer import InferenceWrapper
from test_infer_gpu import _toy_embedders
from test_enrol_gpu import _identities
tiny = torch.load(os.path.join(%(root)r, "tests", "golden", "tiny_hotpath.pt"), weights_only=False)
num_gpus = int(os.environ["WORLD_SIZE"])
w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=%(project)r, folder="logs",
                     print_params=False, num_gpus=num_gpus, use_graphs=True, identity_capacity=6)
w.embedders.update(_toy_embedders(tiny, w.device))
S = tiny["cfg"]["image_size"]
ids = _identities(tiny, 5)
slots = w.enrol_identities([i[0] for i in ids], source_masks=[torch.ones(1, 1, S, S)] * 5, batch_size=2,
                           custome_idt_embed=torch.cat([i[1] for i in ids]), custome_source_pose_embed=torch.cat([i[2] for i in ids]),
                           custome_source_theta_embed=torch.cat([i[3] for i in ids]))
assert slots == [0, 1, 2, 3, 4], slots
out = dict(cl=w._bank_cl.cpu(), idt=w._bank_idt.cpu(), theta=w._bank_theta.cpu(), used=list(w._bank_used),
           pose_has=w._bank_streams.theta_has.cpu())
torch.save(out, os.path.join(%(project)r, "enrol_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def test_two_ranks_enrol_one_gpu_gloo(tmp_path, golden_dir):
    import subprocess
    from test_two_ranks_gpu import _free_port, _project
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
        outs = [p.communicate(timeout=600)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0 and "WORKER_OK" in o, o[-4000:]
        return [torch.load(os.path.join(project, f"enrol_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    single = spawn(1)[0]
    ranks = spawn(2)
    assert single["used"] == [True] * 5 + [False]
    for r, out in enumerate(ranks):
        assert out["used"] == single["used"], r
        for key in ("cl", "idt", "theta", "pose_has"):
            assert torch.equal(out[key].view(torch.int32), single[key].view(torch.int32)), f"rank {r}: {key} differs from one rank"
    assert bool(single["cl"][:5].abs().sum(dim=(1, 2, 3, 4)).gt(0).all())             # (every enrolled row was written)
