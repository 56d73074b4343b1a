"""Frames of several source identities in one driver batch, on the GPU: HotPath.driver_pass(identity=...) over a bank, and the
InferenceWrapper's identity bank (store / load / drop, animate(identities=...), graph replay).  Every frame must be BIT FOR BIT
the same row of the single-identity pass of its identity at the same batch size (same launch plans): only the uv sampler call and
the (pose + idt) * 0.5 add read the bank, both with the plain kernels' arithmetic."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bank_vs_single(hp, canon, idt, pose, theta, identity):
    """(mixed frames, single-identity frames per identity) for one bank; the overflow log of each pass must be empty"""
    single = []
    for k in range(len(canon)):
        single.append(hp.driver_pass(hp.prepare_canonical(canon[k]), idt[k], pose, theta))
        assert hp.overflow_events() == {}, k
    bank_cl = torch.cat([hp.prepare_canonical(c) for c in canon])
    ident = torch.tensor(identity, dtype=torch.int32, device=hp.device)
    mixed = hp.driver_pass(bank_cl, torch.cat(idt), pose, theta, identity=ident)
    assert hp.overflow_events() == {}
    return mixed, single


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3", "f32", "f16"])
def test_tiny_bank_pass_equals_each_identitys_own_pass(tiny, precision):
    from emoportraits_amd import config, nets
    cfg = config.hot_path_config(overrides=tiny["cfg"])
    hp = nets.HotPath(tiny["state_dict"], cfg, DEV, with_source=False, precision=precision)
    g = torch.Generator().manual_seed(4)
    c0 = tiny["source"]["canonical"]
    canon = [c0, c0.flip(-1).contiguous(), (0.7 * c0 + 0.1 * torch.randn(c0.shape, generator=g)).contiguous()]
    idt = [tiny["idt_embed"]] + [(tiny["idt_embed"] + 0.2 * torch.randn(tiny["idt_embed"].shape, generator=g)).contiguous()
                                 for _ in range(2)]
    canon, idt = [t.to(DEV) for t in canon], [t.to(DEV) for t in idt]
    B = 8
    pose = (0.5 * torch.randn(B, tiny["target_pose_embed"].shape[1], generator=g)).to(DEV)
    theta = tiny["theta_drv"][torch.arange(B) % tiny["theta_drv"].shape[0]].contiguous().to(DEV)
    identity = [0, 2, 1, 1, 0, 2, 2, 0]
    mixed, single = _bank_vs_single(hp, canon, idt, pose, theta, identity)
    for b, k in enumerate(identity):
        assert _same(mixed[b], single[k][b]), (precision, b, k)
    assert not _same(single[0][0], single[1][0])                       # (the identities do differ)


def test_r512_bank_pass_equals_each_identitys_own_pass():
    """the bench's checkpoint (seeded trained-like, R512), four seeded canonical volumes, B = 16, default mode"""
    from emoportraits_amd import config, nets, ops, random_init
    cfg = config.hot_path_config(overrides={"image_size": 512})
    sd = random_init.trained_like_state_dict(cfg, seed=0, with_source=False)
    hp = nets.HotPath(sd, cfg, DEV, with_source=False)
    c, d, s = cfg["latent_volume_channels"], cfg["latent_volume_depth"], cfg["latent_volume_size"]
    g = torch.Generator().manual_seed(1)
    canon = [torch.randn(1, c, d, s, s, generator=g).to(DEV) for _ in range(4)]
    idt = [torch.randn(1, cfg["gen_max_channels"], 4, 4, generator=g).to(DEV) for _ in range(4)]
    B = 16
    pose = torch.randn(B, cfg["lpe_output_channels_expression"], generator=g).to(DEV)
    srt = [t.to(DEV) for t in (1 + 0.05 * torch.randn(B, 3, generator=g), 0.3 * torch.randn(B, 3, generator=g),
                              0.05 * torch.randn(B, 3, generator=g))]
    theta = ops.pose_theta(*srt)
    identity = [3, 0, 1, 2, 2, 1, 0, 3, 0, 0, 2, 3, 1, 3, 2, 1]
    mixed, single = _bank_vs_single(hp, canon, idt, pose, theta, identity)
    for b, k in enumerate(identity):
        assert _same(mixed[b], single[k][b]), (b, k)


@pytest.mark.parametrize("row", [512 * 16, 1000, 64 * 256 + 300], ids=lambda r: f"row{r}")
def test_add_rows_indexed_equals_add_per_row(row):
    """ops.add_rows_indexed directly: row b is bit for bit ops.add(a[b], table[index[b]], alpha) -- the warp embedding's
    [B, 512 * 16] rows, a row length that is no multiple of 256, and one longer than the 64 * 256 elements the capped grid
    covers in one trip; repeated and permuted indices; an index outside the bank gives a zero row"""
    from emoportraits_amd import ops
    g = torch.Generator().manual_seed(row)
    B, K, alpha = 9, 4, 0.5
    a = torch.randn(B, row, 1, generator=g).to(DEV)
    table = torch.randn(K, row, 1, generator=g).to(DEV)
    for index in ([3, 1, 0, 2, 2, 2, 0, 3, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 4, 2, -1, 3, 0, 2 ** 31 - 1, 3, -2 ** 31]):
        idx = torch.tensor(index, dtype=torch.int32, device=DEV)
        out = ops.add_rows_indexed(a, table, idx, alpha)
        assert out.shape == a.shape
        for b, k in enumerate(index):
            want = ops.add(a[b], table[k], alpha) if 0 <= k < K else torch.zeros_like(a[b])
            assert _same(out[b], want), (row, index, b, k)
    # the rows differ from each other (a fixed row of the table for every b would not pass above), and out= is honoured
    assert not _same(ops.add(a[0], table[0], alpha), ops.add(a[0], table[1], alpha))
    buf = torch.full_like(a, 7.0)
    idx = torch.tensor([3, 1, 0, 2, 2, 2, 0, 3, 1], dtype=torch.int32, device=DEV)
    assert ops.add_rows_indexed(a, table, idx, alpha, out=buf) is buf and _same(buf, ops.add_rows_indexed(a, table, idx, alpha))


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
    from notebooks.infer import InferenceWrapper
    from test_infer_gpu import _toy_embedders
    w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=str(project), folder="logs",
                         print_params=False, **kw)
    w.embedders.update(_toy_embedders(tiny, w.device))
    return w


def _sources(tiny, n):
    """n distinct identities: (source image, idt_embed, source theta) -- the tiny fixture's, perturbed"""
    g = torch.Generator().manual_seed(23)
    out = []
    for k in range(n):
        img = (tiny["img"] if k == 0 else (tiny["img"] + 0.1 * torch.randn(tiny["img"].shape, generator=g)).clamp(0, 1)).contiguous()
        idt = tiny["idt_embed"] if k == 0 else (tiny["idt_embed"] + 0.2 * torch.randn(tiny["idt_embed"].shape, generator=g))
        out.append((img, idt.contiguous(), tiny["theta_src"]))
    return out


def _enrol(w, tiny, sources):
    S = tiny["cfg"]["image_size"]
    slots = []
    for img, idt, th in sources:
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=th)
        slots.append(w.store_identity())
    return slots


def _drivers(tiny, N, seed=17):
    g = torch.Generator().manual_seed(seed)
    pose = torch.randn(N, tiny["target_pose_embed"].shape[1], generator=g) * 0.5
    srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.3 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
    return pose, srt


def _animate(w, pose, srt, **kw):
    out = {}
    for b0, u8 in w.animate(pose, srt, batch_size=16, **kw):
        for j in range(u8.shape[0]):
            out[b0 + j] = u8[j].cpu()
    return [out[i] for i in range(len(out))]


def test_wrapper_bank_store_load_animate(project, tiny):
    w = _wrapper(project, tiny, use_graphs=False, identity_capacity=3)
    slots = _enrol(w, tiny, _sources(tiny, 3))
    assert slots == [0, 1, 2] and w.identities() == [0, 1, 2]
    N = 33
    pose, srt = _drivers(tiny, N)
    ids = torch.tensor([(5 * i + i // 7) % 3 for i in range(N)])
    per = []
    S = tiny["cfg"]["image_size"]
    frame = (torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(3)))
    first = []
    for k in range(3):
        w.load_identity(k)
        per.append(_animate(w, pose, srt))
        first.append(w.forward(driver_image=frame, crop=False)[1].cpu())
    # load_identity + forward(driver_image=...) renders that identity: the same frame as right after its own source call
    w2 = _wrapper(project, tiny, use_graphs=False)
    img, idt, th = _sources(tiny, 3)[1]
    w2.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
               custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=th)
    assert _same(w2.forward(driver_image=frame, crop=False)[1].cpu(), first[1])
    w.load_identity(1)
    assert _same(w.pred_source_theta.cpu(), w2.pred_source_theta.cpu())
    assert _same(w.idt_embed.cpu().reshape(-1), w2.idt_embed.cpu().reshape(-1))
    assert _same(w.target_latent_volume.cpu(), w2.target_latent_volume.cpu())
    mixed = _animate(w, pose, srt, identities=ids)
    for i in range(N):
        assert torch.equal(mixed[i], per[int(ids[i])][i]), i
    # drop + bad slots: ValueError on the host, before anything is launched
    w.drop_identity(1)
    assert w.identities() == [0, 2]
    for bad in ([0, 1], [0, 3], [-1, 0], [0, 2.0]):
        with pytest.raises(ValueError):
            next(w.animate(pose[:2], [t[:2] for t in srt], identities=torch.tensor(bad)))
    with pytest.raises(ValueError):
        w.load_identity(1)
    with pytest.raises(ValueError):
        next(w.animate(pose[:3], [t[:3] for t in srt], identities=[0, 0]))              # one slot per frame
    frames = (torch.rand(4, S, S, 3) * 255).to(torch.uint8)
    with pytest.raises(ValueError):
        next(w.animate_frames(frames, identities=[0, 0, 2, 2], smooth_pose=True))
    with pytest.raises(ValueError):
        next(w.animate_frames(frames, identities=[0, 0, 1, 2]))
    with pytest.raises(ValueError):
        _wrapper(project, tiny, use_graphs=False).store_identity()                    # no bank (and no identity yet)


def test_wrapper_bank_under_graph_replay(project, tiny):
    """use_graphs=True: new indices and a re-stored slot take effect on replay, with ONE captured signature for the bank pass"""
    w = _wrapper(project, tiny, use_graphs=True, identity_capacity=2)
    srcs = _sources(tiny, 3)
    _enrol(w, tiny, srcs[:2])
    ref = _wrapper(project, tiny, use_graphs=False, identity_capacity=3)
    _enrol(ref, tiny, srcs)
    N = 16
    pose, srt = _drivers(tiny, N, seed=5)
    per = []
    for k in range(3):
        ref.load_identity(k)
        per.append(_animate(ref, pose, srt))
    plans = [[i % 2 for i in range(N)], [(i // 3) % 2 for i in range(N)], [1 - (i % 2) for i in range(N)]]
    for call, plan in enumerate(plans * 2):
        if call == 4:                                       # re-store slot 1 with the third identity between replays
            S = tiny["cfg"]["image_size"]
            img, idt, th = srcs[2]
            w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                      custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=th)
            w.drop_identity(1)
            assert w.store_identity(1) == 1
        out = _animate(w, pose, srt, identities=plan)
        for i in range(N):
            k = plan[i] if not (call >= 4 and plan[i] == 1) else 2
            assert torch.equal(out[i], per[k][i]), (call, i)
    assert len(w._graphed['driver_bank'].signatures()) == 1
