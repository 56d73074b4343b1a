"""Batched enrolment of source identities on the GPU: HotPath.source_pass at B > 1 against the oracle, the row-indexed repack
(ops.volume_to_channels_last_indexed, ABI 14) on the device, and InferenceWrapper.enrol_identities.

Bounds.  The batched source pass is held per identity to oracle/restate.source_pass with the bounds of the B = 1 pass
(tests/test_nets_gpu.py: 1e-3 of max on the canonical volume).  A bank filled by enrol_identities is compared with one filled by
forward + store_identity: the launch plans of the small layers depend on the batch (pack.plan_launch splits the K loop
differently), so the two differ by rounding only.  Both are within 1e-3 of the oracle, so they are within 2e-3 of each other
(triangle inequality), and the frames rendered from them within 2 x 5e-3 abs (the image bound of the end-to-end parity tests).
Everything enrol_identities composes from the same chunks is compared bit for bit."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rel(got, ref):
    return (got.detach().cpu().double() - ref.detach().cpu().double()).abs().max().item() / (ref.double().abs().max().item() + 1e-30)


def _identities(tiny, n):
    """n distinct identities (masked source, idt_embed, source pose embedding, source theta): the tiny fixture's source plus
    perturbed ones (as test_identity_bank_gpu._sources makes them), each with a pose embedding and a head pose of its own"""
    from test_identity_bank_gpu import _sources
    g = torch.Generator().manual_seed(41)
    thetas = [tiny["theta_src"]] + [tiny["theta_drv"][k % tiny["theta_drv"].shape[0]][None] for k in range(n - 1)]
    out = []
    for k, (img, idt, _) in enumerate(_sources(tiny, n)):
        pose = tiny["source_pose_embed"] if k == 0 else tiny["source_pose_embed"] + 0.3 * torch.randn(tiny["source_pose_embed"].shape,
                                                                                                        generator=g)
        out.append((img, idt, pose.contiguous(), thetas[k].contiguous()))
    return out


@pytest.mark.parametrize("precision", ["f16x2", "f32"])
def test_tiny_batched_source_pass_vs_oracle(tiny, precision):
    import restate as O
    from emoportraits_amd import config, nets
    cfg = config.hot_path_config(overrides=tiny["cfg"])
    hp = nets.HotPath(tiny["state_dict"], cfg, DEV, precision=precision)
    ids = _identities(tiny, 3)
    cat = lambda i: torch.cat([x[i] for x in ids]).to(DEV)
    got = hp.source_pass(cat(0), cat(1), cat(2), cat(3), keep=True)
    assert hp.overflow_events() == {}
    assert got["canonical"].shape[0] == 3
    for k, (img, idt, pose, th) in enumerate(ids):
        with torch.no_grad():
            ref = O.source_pass(tiny["state_dict"], cfg, img, idt, pose, th)
        e = _rel(got["canonical"][k:k + 1], ref["canonical"])
        e_pre = _rel(got["pre_canonical"][k:k + 1], ref["pre_canonical"])
        one = hp.source_pass(img.to(DEV), idt.to(DEV), pose.to(DEV), th.to(DEV))
        assert hp.overflow_events() == {}
        e1 = _rel(got["canonical"][k:k + 1], one)
        print(f"PARITY batched source pass tiny {precision} identity {k}: canonical {e:.2e} pre_canonical {e_pre:.2e}, "
              f"to the B = 1 pass {e1:.2e}")
        assert e <= 1e-3 and e_pre <= 1e-3, (k, e, e_pre)


def test_batched_source_pass_released_architecture_vs_oracle():
    import restate as O
    from emoportraits_amd import nets
    from test_nets_gpu import _full_size, check
    cfg, sd, x = _full_size(256, 1, seed=11)
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s: torch.randn(*s, generator=g)
    second = dict(img=torch.rand(1, 3, 256, 256, generator=g), idt=rnd(1, 512, 4, 4), pose_s=rnd(1, 128),
                  th_s=O.get_transform_matrix(1 + 0.05 * rnd(1, 3), 0.3 * rnd(1, 3), 0.05 * rnd(1, 3)))
    ids = [x, second]
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    hp = nets.HotPath(sd, cfg, DEV)
    cat = lambda key: torch.cat([i[key] for i in ids]).float().to(DEV)
    got = hp.source_pass(cat("img"), cat("idt"), cat("pose_s"), cat("th_s"), keep=True)
    assert hp.overflow_events() == {}
    for k, i in enumerate(ids):
        with torch.no_grad():
            ref = O.source_pass(sd, cfg, i["img"], i["idt"], i["pose_s"], i["th_s"])
        row = lambda t: t[k:k + 1]
        e = [check("latents", row(got["latents"]), ref["latents"]),
             check("source_volume", row(got["source_volume"]), ref["source_volume"]),
             check("pre_canonical", row(got["pre_canonical"]), ref["pre_canonical"], 1e-3),
             check("canonical", row(got["canonical"]), ref["canonical"], 1e-3)]
        print(f"PARITY batched source pass R256 identity {k}:", [f"{v:.2e}" for v in e])


def test_indexed_repack_on_the_device():
    from emoportraits_amd import ops
    g = torch.Generator().manual_seed(5)
    vols = torch.randn(4, 70, 3, 5, 13, generator=g).to(DEV)
    sentinel = -7.25
    bank = torch.full((5, 3, 5, 13, 70), sentinel, device=DEV)
    rows = torch.tensor([3, -1, 0, 5], dtype=torch.int32, device=DEV)        # -1 and 5 (= num_rows) are skipped
    assert ops.volume_to_channels_last_indexed(vols, bank, rows) is bank
    torch.cuda.synchronize()
    assert _same(bank[3], ops.volume_to_channels_last(vols[0:1])[0])
    assert _same(bank[0], ops.volume_to_channels_last(vols[2:3])[0])
    for r in (1, 2, 4):
        assert bool((bank[r] == sentinel).all()), r
    with pytest.raises(ValueError):
        ops.volume_to_channels_last_indexed(vols, bank[:, :, :, :, :64].contiguous(), rows)
    with pytest.raises(ValueError):
        ops.volume_to_channels_last_indexed(vols, bank, rows.long())


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


def _bank_bytes(w):
    return [t.clone() for t in (w._bank_cl, w._bank_idt, w._bank_theta, w._bank_streams.theta_has)] + [list(w._bank_used)]


def _bank_equal(a, b):
    return all(_same(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _frames(w, tiny, ids, seed=17):
    from test_identity_bank_gpu import _drivers
    pose, srt = _drivers(tiny, len(ids), seed)
    out = {}
    for b0, img in w.animate(pose, srt, batch_size=8, identities=ids, as_uint8=False):
        for j in range(img.shape[0]):
            out[b0 + j] = img[j].cpu()
    return [out[i] for i in range(len(ids))]


def test_wrapper_enrol_identities(project, tiny):
    from emoportraits_amd import ops
    S = tiny["cfg"]["image_size"]
    ids = _identities(tiny, 5)
    imgs = [i[0] for i in ids]
    kw = dict(source_masks=[torch.ones(1, 1, S, S)] * 5, batch_size=2, custome_idt_embed=torch.cat([i[1] for i in ids]),
              custome_source_pose_embed=torch.cat([i[2] for i in ids]), custome_source_theta_embed=torch.cat([i[3] for i in ids]))
    w = _wrapper(project, tiny, use_graphs=False, identity_capacity=6)
    # the current identity, rendered before the enrolment
    cur = _identities(tiny, 1)[0]
    w.forward(source_image=cur[0], crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=cur[1],
              custome_source_pose_embed=cur[2], custome_source_theta_embed=cur[3])
    frame = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(3))
    before = w.forward(driver_image=frame, crop=False)[1].cpu()
    state = [t.clone() for t in (w._canonical_cl, w.idt_embed, w.pred_source_theta, w.target_latent_volume)]

    # every refusal: ValueError on the host, the bank bytes as they were
    empty = _bank_bytes(w)
    for bad in (dict(sources=[]), dict(sources=imgs + imgs[:2]), dict(slots=[0, 1, 2, 3, 3]), dict(slots=[0, 1, 2, 3, 6]),
                dict(source_masks=[torch.ones(1, 1, S, S)] * 4), dict(custome_idt_embed=kw["custome_idt_embed"][:4]),
                dict(custome_source_pose_embed=kw["custome_source_pose_embed"][:3]),
                dict(custome_source_theta_embed=kw["custome_source_theta_embed"][:, :3]), dict(batch_size=0),
                dict(windows=[(0, 0, S)] * 5)):
        args = dict(kw, **bad)
        with pytest.raises(ValueError):
            w.enrol_identities(args.pop("sources", imgs), **args)
        assert _bank_equal(_bank_bytes(w), empty), bad
    # crop=True and a source without a face: named, nothing enrolled
    no_face = lambda img: None if torch.equal(torch.as_tensor(img), imgs[3]) else (0.2, 0.2, 0.5, 0.5)
    w.embedders["face_detector"] = no_face
    with pytest.raises(ValueError, match="source 3"):
        w.enrol_identities(imgs, crop=True, **kw)
    assert _bank_equal(_bank_bytes(w), empty)
    del w.embedders["face_detector"]

    slots = w.enrol_identities(imgs, **kw)
    assert slots == [0, 1, 2, 3, 4] and w.identities() == slots
    # the current identity is untouched and renders as before
    for a, b in zip(state, (w._canonical_cl, w.idt_embed, w.pred_source_theta, w.target_latent_volume)):
        assert _same(a, b)
    assert _same(w.forward(driver_image=frame, crop=False)[1].cpu(), before)

    # rows == a manual composition of the same chunks (source_pass -> volume_to_channels_last), bit for bit
    hp = w.hot_path
    for a, b in ((0, 2), (2, 4), (4, 5)):
        cat = lambda i: torch.cat([x[i] for x in ids[a:b]]).to(DEV)
        canon = hp.source_pass(cat(0), cat(1), cat(2), cat(3))
        cl = ops.volume_to_channels_last(canon)
        for k in range(a, b):
            assert _same(w._bank_cl[k], cl[k - a]), k
            assert _same(w._bank_idt[k], cat(1)[k - a].reshape(w._bank_idt.shape[1:])), k
            assert _same(w._bank_theta[k], cat(3)[k - a]), k

    # against a bank filled by forward + store_identity: rounding of the batched launch plans only
    ref = _wrapper(project, tiny, use_graphs=False, identity_capacity=6)
    for img, idt, pose, th in ids:
        ref.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                    custome_source_pose_embed=pose, custome_source_theta_embed=th)
        ref.store_identity()
    for k in range(5):
        e = _rel(w._bank_cl[k], ref._bank_cl[k])
        print(f"PARITY enrolled vs forward + store_identity, identity {k}: canonical {e:.2e}")
        assert e <= 2e-3, (k, e)
        assert _same(w._bank_idt[k], ref._bank_idt[k]) and _same(w._bank_theta[k], ref._bank_theta[k])
    plan = [(3 * i + i // 4) % 5 for i in range(12)]
    got, want = _frames(w, tiny, plan), _frames(ref, tiny, plan)
    e_img = max((x - y).abs().max().item() for x, y in zip(got, want))
    print(f"PARITY enrolled vs stored bank, animate frames: max abs {e_img:.2e}")
    assert e_img <= 1e-2

    # uint8 frames + windows == the float path fed the same crops, bit for bit
    g = torch.Generator().manual_seed(8)
    H, W = S + 24, S + 40
    u8 = (torch.rand(5, H, W, 3, generator=g) * 255).to(torch.uint8)
    wins = [(3 * k, 2 * k + 1, S + 8 - 2 * k) for k in range(5)]
    crops = ops.resize2d_windows(ops.unpack_rgb8(u8.to(DEV)), (S, S), [(x, y, s, s) for x, y, s in wins], "bicubic",
                                 clamp01=True).cpu()
    wv = _wrapper(project, tiny, use_graphs=False, identity_capacity=6)
    assert wv.enrol_identities(u8, windows=wins, **kw) == slots
    wf = _wrapper(project, tiny, use_graphs=False, identity_capacity=6)
    assert wf.enrol_identities(crops, slots=[5, 4, 3, 2, 1], **kw) == [5, 4, 3, 2, 1]
    for k in range(5):
        assert _same(wv._bank_cl[k], wf._bank_cl[5 - k]) and _same(wv._bank_theta[k], wf._bank_theta[5 - k]), k

    # explicit slots overwrite occupied ones; every written slot starts a new smooth_pose stream
    w._bank_streams.theta_has.fill_(1)
    assert w.enrol_identities(imgs[:2], slots=[4, 5], **dict(kw, source_masks=kw["source_masks"][:2],
                                                            custome_idt_embed=kw["custome_idt_embed"][:2],
                                                            custome_source_pose_embed=kw["custome_source_pose_embed"][:2],
                                                            custome_source_theta_embed=kw["custome_source_theta_embed"][:2])) == [4, 5]
    assert w._bank_streams.theta_has.cpu().tolist() == [1, 1, 1, 1, 0, 0]
    assert _same(w._bank_cl[4], w._bank_cl[0]) and _same(w._bank_cl[5], w._bank_cl[1])     # (chunk (0, 2) again)
    with pytest.raises(ValueError):
        w.enrol_identities(imgs[:1], **dict(kw, source_masks=kw["source_masks"][:1],
                                            custome_idt_embed=kw["custome_idt_embed"][:1],
                                            custome_source_pose_embed=kw["custome_source_pose_embed"][:1],
                                            custome_source_theta_embed=kw["custome_source_theta_embed"][:1]))   # bank full


def test_wrapper_enrol_under_graph_replay(project, tiny):
    """a captured bank pass replays slots enrolled after the capture; its frames equal a non-graph wrapper's bit for bit"""
    S = tiny["cfg"]["image_size"]
    ids = _identities(tiny, 5)

    def kw(a, b):
        return dict(source_masks=[torch.ones(1, 1, S, S)] * (b - a), batch_size=2,
                    custome_idt_embed=torch.cat([i[1] for i in ids[a:b]]),
                    custome_source_pose_embed=torch.cat([i[2] for i in ids[a:b]]),
                    custome_source_theta_embed=torch.cat([i[3] for i in ids[a:b]]))
    imgs = [i[0] for i in ids]
    ref = _wrapper(project, tiny, use_graphs=False, identity_capacity=6)
    ref.enrol_identities(imgs, **kw(0, 5))                                     # chunks (0, 2), (2, 4), (4, 5)
    wg = _wrapper(project, tiny, use_graphs=True, identity_capacity=6)
    wg.enrol_identities(imgs[:4], **kw(0, 4))                                  # the same chunks, in two calls
    first = [i % 4 for i in range(16)]
    for _ in range(2):                                                         # eager call, then the capture
        out = _frames(wg, tiny, first)
    want = _frames(ref, tiny, first)
    assert all(_same(x, y) for x, y in zip(out, want))
    assert wg.enrol_identities(imgs[4:], **kw(4, 5)) == [4]
    plan = [(5 * i + 2) % 5 for i in range(16)]
    out, want = _frames(wg, tiny, plan), _frames(ref, tiny, plan)
    for i in range(16):
        assert _same(out[i], want[i]), i
    assert len(wg._graphed['driver_bank'].signatures()) == 1
