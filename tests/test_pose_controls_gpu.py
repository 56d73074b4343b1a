"""forward()'s pose controls in the batched entry points, on the GPU: ops.mixing_theta and ops.theta_ema_scan (the device kernels
give the bits of their CPU emulation), animate_frames(mix=, mix_old=, target_theta=) against forward() on the same frames, the
identity bank with per-frame mixing and per-identity smoothing streams (eager and graph replay) against each identity's own
single-identity run, animate(smooth_pose=True) against hostglue.ema_scan, and 2 ranks against 1.  Tiny fixture, toy embedders."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"), reason="the CPU emulation needs ROCm's toolchain")
def test_kernels_give_the_bits_of_their_cpu_emulation():
    import emulibs
    import test_pose_controls_emul as E
    from emoportraits_amd import ops
    lib = emulibs.stream(False)
    th = E.corpus(lib)
    M = th.shape[0]
    rng = np.random.default_rng(3)
    tgt = th[rng.permutation(M)].copy()
    for n, v in ((5, np.nan), (9, np.inf)):                        # non-finite target linear parts
        tgt[n, 1, 1] = v
    bank = th.copy()
    bank[7, 0, 2] = np.nan                                         # a non-finite source
    idx = np.int32(rng.integers(0, M, M))
    idx[[3, 11, 20]] = [7, -1, M]                                  # ... and out-of-range slots
    for mix_old in (True, False):
        want = E.mix(lib, tgt, bank, idx, mix_old)
        got = ops.mixing_theta(torch.from_numpy(tgt).to(DEV), torch.from_numpy(bank).to(DEV),
                               torch.from_numpy(idx).to(DEV), mix_old).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), mix_old
        want0 = E.mix(lib, tgt, bank, None, mix_old)
        got0 = ops.mixing_theta(torch.from_numpy(tgt).to(DEV), torch.from_numpy(bank).to(DEV), None, mix_old).cpu().numpy()
        assert np.array_equal(got0.view(np.uint32), want0.view(np.uint32))
    vals = rng.standard_normal((40, 4, 4)).astype(np.float32)
    so = np.int32([(i * 5 + i // 4) % 3 for i in range(40)])
    st, has = np.zeros((4, 16), np.float32), np.int32([0, 1, 0, 0])
    st[1] = rng.standard_normal(16)
    dst, dhas = torch.from_numpy(st.reshape(4, 4, 4).copy()).to(DEV), torch.from_numpy(has.copy()).to(DEV)
    for lo, hi in ((0, 23), (23, 40)):
        want = E.scan(lib, vals[lo:hi], so[lo:hi], st, has, 0.3)
        got = ops.theta_ema_scan(torch.from_numpy(vals[lo:hi]).to(DEV), torch.from_numpy(so[lo:hi]).to(DEV), dst, dhas, 0.3)
        assert np.array_equal(got.cpu().numpy().reshape(-1, 16).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dst.cpu().numpy().reshape(4, 16).view(np.uint32), st.view(np.uint32))
    assert dhas.cpu().tolist() == has.tolist() == [1, 1, 1, 0]


# ---- the wrapper ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def project(tmp_path_factory, tiny):
    from emoportraits_amd import config
    root = tmp_path_factory.mktemp("proj")
    exp = root / "logs" / "exp"
    (exp / "checkpoints").mkdir(parents=True)
    cfg = config.hot_path_config(overrides=tiny["cfg"])
    with open(exp / "args.txt", "wt") as f:
        for k, v in cfg.items():
            f.write(f"{k}: {v}\n")
        f.write("experiment_name: exp\nuse_seg: True\n")
    torch.save(tiny["state_dict"], exp / "checkpoints" / "model.pth")
    return root


def _wrapper(project, tiny, **kw):
    from test_identity_bank_gpu import _wrapper as make
    return make(project, tiny, **kw)


def _frames(tiny, N, seed=3):
    S = tiny["cfg"]["image_size"]
    return (torch.rand(N, S, S, 3, generator=torch.Generator().manual_seed(seed)) * 255).to(torch.uint8)


def _collect(gen):
    out = {}
    for b0, u8 in gen:
        for j in range(u8.shape[0]):
            out[b0 + j] = u8[j].cpu().clone()
    return [out[i] for i in range(len(out))]


def _sources_with_poses(tiny, n):
    """n identities whose source thetas differ (stretch, shear, a reflection): mixing then differs per identity"""
    from test_identity_bank_gpu import _sources
    out = []
    shears = [torch.eye(4), torch.tensor([[1.1, 0.2, 0, 0], [0, 0.9, 0, 0], [0, 0, 1.05, 0], [0, 0, 0, 1]]),
              torch.diag(torch.tensor([-1.0, 1.0, 1.0, 1.0]))]
    for k, (img, idt, th) in enumerate(_sources(tiny, n)):
        out.append((img, idt, (th[0] @ shears[k % 3])[None].contiguous()))
    return out


@pytest.mark.parametrize("mix_old", [True, False])
def test_animate_frames_mix_and_source_pose_equal_forward(project, tiny, mix_old):
    """animate_frames(mix=True) / (target_theta=False) vs forward(driver_image=..., crop=False, mix=True / target_theta=False) on the
    same frames (the host scipy mixing there): <= 1 per uint8 byte, as test_animate_frames_is_device_resident_and_equals_forward"""
    w = _wrapper(project, tiny, use_graphs=False)
    S = tiny["cfg"]["image_size"]
    img, idt, th = _sources_with_poses(tiny, 2)[1]
    w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
              custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=th)
    N = 6
    frames = _frames(tiny, N)
    as_float = frames.permute(0, 3, 1, 2).float() / 255.0
    for kw in (dict(mix=True, mix_old=mix_old), dict(target_theta=False), dict(mix=True, mix_old=mix_old, target_theta=False)):
        got = _collect(w.animate_frames(frames, batch_size=3, ring=2, **kw))
        imgs, _ = w.forward(driver_image=as_float, crop=False, **kw)
        for i in range(N):
            assert np.abs(np.asarray(imgs[i]).astype(int) - got[i].numpy().astype(int)).max() <= 1, (kw, i)
    plain = _collect(w.animate_frames(frames, batch_size=3, ring=2))
    mixed = _collect(w.animate_frames(frames, batch_size=3, ring=2, mix=True, mix_old=mix_old))
    assert any(not torch.equal(a, b) for a, b in zip(plain, mixed))              # (the mixing does change the frames)


class _Recorder:
    """wraps the wrapper's driver calls: (pose, render theta, slots, image) of every batch; the expression embedder's theta"""

    def __init__(self, w):
        self.w, self.calls, self.expr = w, [], []
        drive_bank, drive, expression = w._drive_bank, w._drive, w._expression

        def bank(pose, theta, ident):
            img = drive_bank(pose, theta, ident)
            self.calls.append((pose.clone(), theta.clone(), ident.clone(), img.clone()))
            return img

        def single(pose, theta):
            img = drive(pose, theta)
            self.calls.append((pose.clone(), theta.clone(), None, img.clone()))
            return img

        def expr(crops, theta, what):
            self.expr.append(theta.clone())
            return expression(crops, theta, what)
        w._drive_bank, w._drive, w._expression = bank, single, expr

    def thetas(self):
        return torch.cat([c[1] for c in self.calls]), torch.cat(self.expr)

    def remove(self):
        for name in ("_drive_bank", "_drive", "_expression"):
            self.w.__dict__.pop(name, None)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_bank_mix_smooth_source_pose_equal_each_identitys_own_run(project, tiny, use_graphs):
    """a mixed-identity batch with mix, smooth_pose (and target_theta=False): every frame's thetas are bit for bit those of its
    identity's own single-identity run over that identity's frames, and every frame is bit for bit the same row of the
    single-identity driver pass at the same batch size (the _bank_vs_single pattern of test_identity_bank_gpu.py)"""
    w = _wrapper(project, tiny, use_graphs=use_graphs, identity_capacity=3)
    from test_identity_bank_gpu import _enrol
    srcs = _sources_with_poses(tiny, 3)
    assert _enrol(w, tiny, srcs) == [0, 1, 2]
    N, B = 24, 8
    frames = _frames(tiny, N, seed=11)
    ids = [(5 * i + i // 7) % 3 for i in range(N)]
    ids[:3] = [0, 0, 1]                                        # slot 2 begins mid-batch
    for target_theta in (True, False):
        w.reset_pose_state()
        rec = _Recorder(w)
        rounds = 2 if use_graphs else 1                        # graphs: the second round replays (streams carried on)
        for r in range(rounds):
            rec.calls.clear(), rec.expr.clear()
            _collect(w.animate_frames(frames, batch_size=B, ring=2, identities=ids, mix=True, smooth_pose=True,
                                      smooth_per_identity=True, target_theta=target_theta))
        render, expr = rec.thetas()
        state = (w._bank_streams.theta.clone(), w._bank_streams.theta_has.clone())
        # each identity's own run: load it, one stream from scratch (the host scan), its frames only
        singles = {}
        for k in range(3):
            sel = [i for i in range(N) if ids[i] == k]
            w.load_identity(k)
            w.reset_pose_state()
            rec.remove()
            one = _Recorder(w)
            for r in range(rounds):
                one.calls.clear(), one.expr.clear()
                _collect(w.animate_frames(frames[sel], batch_size=B, ring=2, mix=True, smooth_pose=True, target_theta=target_theta))
            r_k, e_k = one.thetas()
            assert _same(e_k, expr[sel]), (k, target_theta)                    # mixed + smoothed theta into the embedder
            assert _same(r_k, render[sel]), (k, target_theta)                  # what the frame is rendered with
            if not target_theta:
                assert _same(render[sel], w._bank_theta[k].expand(len(sel), 4, 4))
            singles[k] = e_k[-1]
            one.remove()
        for k in range(3):                                                     # slot states = each identity's last theta
            assert _same(state[0][k], singles[k]) and int(state[1][k]) == 1
        # frames: row b of the bank pass == row b of the single-identity pass of its identity over the same batch
        hp = w.hot_path
        for pose, theta, ident, img in rec.calls:
            for k in set(ident.tolist()):
                single = hp.driver_pass(w._bank_cl[k:k + 1], w._bank_idt[k:k + 1], pose, theta)
                for b in range(pose.shape[0]):
                    if int(ident[b]) == k:
                        assert _same(img[b], single[b]), (k, b)
    if use_graphs:
        assert len(w._graphed['driver_bank'].signatures()) == 1


def test_animate_smooth_pose_equals_the_host_scan(project, tiny):
    """animate(smooth_pose=True): the thetas of the whole stream from target_srt, scanned on the device, = hostglue.ema_scan;
    the frames = the driver pass fed those thetas; state carried into the next call through self.theta"""
    from emoportraits_amd import hostglue, ops
    from test_identity_bank_gpu import _drivers, _enrol
    w = _wrapper(project, tiny, use_graphs=False, identity_capacity=2)
    _enrol(w, tiny, _sources_with_poses(tiny, 2))
    w.load_identity(0)
    N = 20
    pose, srt = _drivers(tiny, N, seed=8)
    raw = ops.pose_theta(*[t.to(DEV).contiguous() for t in srt]).cpu().numpy().reshape(N, 16)
    want, st = hostglue.ema_scan(raw[:13], None, w.pose_momentum)
    want2, _ = hostglue.ema_scan(raw[13:], st, w.pose_momentum)
    rec = _Recorder(w)
    out = [u8 for _, u8 in w.animate(pose[:13], [t[:13] for t in srt], batch_size=8, smooth_pose=True)]
    out += [u8 for _, u8 in w.animate(pose[13:], [t[13:] for t in srt], batch_size=8, smooth_pose=True)]
    got = torch.cat([c[1] for c in rec.calls])
    assert np.array_equal(got.cpu().numpy().reshape(N, 16), np.concatenate([want, want2]))
    for pose_b, theta_b, _, img in rec.calls:
        assert _same(img, w.hot_path.driver_pass(w._canonical_cl, w.idt_embed, pose_b, theta_b))
    # with a bank: one stream per slot, the same scan per slot's subsequence
    ids = [i % 2 for i in range(N)]
    rec.calls.clear()
    list(w.animate(pose, srt, batch_size=8, identities=ids, smooth_pose=True, smooth_per_identity=True))
    got = torch.cat([c[1] for c in rec.calls]).cpu().numpy().reshape(N, 16)
    for k in range(2):
        sel = [i for i in range(N) if ids[i] == k]
        assert np.array_equal(got[sel], hostglue.ema_scan(raw[sel], None, w.pose_momentum)[0])


N_FRAMES = 32
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
shears = [torch.eye(4), torch.tensor([[1.1, 0.2, 0, 0], [0, 0.9, 0, 0], [0, 0, 1.05, 0], [0, 0, 0, 1]]),
          torch.diag(torch.tensor([-1.0, 1.0, 1.0, 1.0]))]
for k in range(3):
    idt = (tiny["idt_embed"] + 0.2 * k * torch.randn(tiny["idt_embed"].shape, generator=g)).contiguous()
    if w.rank == 0:
        img = (tiny["img"] + 0.1 * k * torch.randn(tiny["img"].shape, generator=g)).clamp(0, 1).contiguous()
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=tiny["source_pose_embed"],
                  custome_source_theta_embed=(tiny["theta_src"][0] @ shears[k])[None].contiguous())
        assert w.store_identity(k) == k
    if num_gpus > 1:
        w.share_identity(k, src_rank=0)
N = %(n)d
g = torch.Generator().manual_seed(17)
frames = (torch.rand(N, S, S, 3, generator=g) * 255).to(torch.uint8)
ids = torch.tensor([(7 * i + i // 5) %% 3 for i in range(N)])
out = {}
for b0, u8 in w.animate_frames([frames[:N // 2], frames[N // 2:]], batch_size=4, ring=2, identities=ids, smooth_pose=True,
                               smooth_per_identity=True, mix=True):
    for j in range(u8.shape[0]):
        out[b0 + j] = u8[j].clone()
torch.save(dict(frames=out, state=w._bank_streams.theta.cpu(), has=w._bank_streams.theta_has.cpu()),
           os.path.join(%(project)r, "pose_rank%%d_of%%d.pt" %% (w.rank, w.world)))
parallel.barrier()
parallel.shutdown()
print("WORKER_OK", w.rank, flush=True)
"""


def test_two_ranks_bank_smooth_mix_equal_one_rank(tmp_path, golden_dir, guarded_outputs):
    """animate_frames(identities=..., smooth_pose=True, mix=True) on 2 ranks (gloo, one GPU) = 1 rank: the same frames and the
    same slot states (every rank scans the whole gathered chunk); two chunks, so the streams carry across a chunk boundary"""
    import subprocess
    from emoportraits_amd import parallel
    from test_two_ranks_gpu import _free_port, _project as make_project
    guarded_outputs.may_serve_nothing("the ranks are child processes: this process launches nothing")
    project = make_project(tmp_path, golden_dir)

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
        return [torch.load(os.path.join(project, f"pose_rank{r}_of{world}.pt"), weights_only=False) for r in range(world)]

    single = spawn(1)[0]
    ranks = spawn(2)
    assert sorted(single["frames"]) == list(range(N_FRAMES))
    covered = []
    half = N_FRAMES // 2
    for r, out in enumerate(ranks):
        assert _same(out["state"], single["state"]) and torch.equal(out["has"], single["has"]), r
        for i, frame in out["frames"].items():
            assert torch.equal(frame, single["frames"][i]), f"frame {i} of rank {r} differs from the single-rank run"
        covered += list(out["frames"])
        for base in (0, half):
            lo, hi = parallel.shard_range(half, r, 2)
            assert all(base + i in out["frames"] for i in range(lo, hi))
    assert sorted(covered) == list(range(N_FRAMES))
