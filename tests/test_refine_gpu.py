"""Stage 2 inside the video path, on the GPU: emo_stage2_head_f32 (the stage-2 tail as one stream launch), Stage2.refine_frames
and InferenceWrapper.attach_stage2 / animate(refine=True) / animate_frames(refine=True).
  * the kernel against the three launches it replaces at the real shape: both outputs bit for bit (device tanhf is the same
    function in both kernels and contraction is off: a difference would be a finding about the build, not a tolerance);
  * refine_frames against the reference's golden and the oracle, with the inputs and bounds of tests/test_stage2_gpu.py;
  * the wrapper: in-path bytes == refine_frames applied by hand to stage 1's fp32 output, within 1 of the stage-2 wrapper's own
    forward(); graphs on == graphs off; paste_back; the identity bank; a stage-2 size that differs from stage 1's.
The wrapper tests use the toy embedders and the tiny project of tests/test_infer_gpu.py and two deterministic toy mask callables.
"""
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


def matting(img):
    """deterministic toy matte, per pixel (so independent of the batch a frame is in): exact 0, exact 1 and fractions"""
    return (img.mean(1, keepdim=True) * 1.6 - 0.3).clamp(0, 1)


def face_parsing(img):
    return (img[:, 1:2] > 0.35).float()


MASKS = {"matting": matting, "face_parsing": face_parsing}


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


@pytest.fixture(scope="module")
def tiny2(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_stage2.pt"), weights_only=False)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_face", [True, False])
def test_stage2_head_kernel_is_the_three_launch_chain_bit_for_bit_at_the_real_shape(with_face):
    from emoportraits_amd import hip, ops
    lib = hip.load()
    N, Cin, H = 2, 32, 512
    S = H * H
    g = torch.Generator().manual_seed(11)
    d = lambda t: t.to(DEV).contiguous()
    x = d(torch.randn(N, Cin, H, H, generator=g))
    w = d(torch.randn(3, Cin, generator=g) * 0.35)
    b = d(torch.randn(3, generator=g) * 0.3)
    scale, shift = d(torch.rand(N, Cin, generator=g) + 0.5), d(torch.randn(N, Cin, generator=g) * 0.3)
    img = torch.rand(N, 3, H, H, generator=g)
    img = d(torch.where(torch.rand(N, 3, H, H, generator=g) < 0.3, (img * 0.05).where(img < 0.5, 1 - img * 0.05), img))
    mask, face = d(matting(torch.rand(N, 3, H, H, generator=g))), d((torch.rand(N, 1, H, H, generator=g) > 0.3).float())
    st = hip.current_stream()
    add = torch.empty_like(img)
    hip.check(lib.emo_conv_head_f32(hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(scale), hip.ptr(shift), hip.ptr(add), N, Cin, 3, S, 1,
                                    hip.ACT["tanh"], st), "emo_conv_head_f32")
    want = ops.stage2_compose(img, add, mask, face if with_face else torch.ones_like(mask))
    want_u8 = ops.pack_rgb8(want)
    raw = img + add * (mask * (face if with_face else 1.0))
    assert bool((raw < 0).any()) and bool((raw > 1).any()) and bool((mask == 0).any()) and bool((mask == 1).any())
    for f32, u8 in ((True, True), (True, False), (False, True)):
        out = torch.full_like(img, float("nan")) if f32 else None
        out_u8 = torch.zeros((N, H, H, 3), device=DEV, dtype=torch.uint8) if u8 else None
        hip.check(lib.emo_stage2_head_f32(hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(scale), hip.ptr(shift), hip.ptr(img), hip.ptr(mask),
                                          hip.ptr(face) if with_face else None, hip.ptr(out), hip.ptr(out_u8), N, Cin, S, 1, st),
                  "emo_stage2_head_f32")
        if f32:
            assert _same(out, want)
        if u8:
            assert torch.equal(out_u8, want_u8)


# ---- Stage2.refine_frames against the reference -----------------------------------------------------------------------------
def test_refine_frames_batchnorm_default_flags_vs_reference_golden(tiny2):
    from emoportraits_amd import ops, stage2
    s2 = stage2.Stage2(tiny2["state_dict"], stage2.stage2_config(tiny2["cfg"]), DEV)
    d = lambda t: t.to(DEV)
    got = s2.refine_frames(d(tiny2["img"]), d(tiny2["mask"]), d(tiny2["face_mask"]), out="f32")
    chain = s2.refine(d(tiny2["img"]), d(tiny2["mask"]), d(tiny2["face_mask"]))
    e = (got.cpu() - tiny2["out"]).abs().max().item()
    e_chain = (chain.cpu() - tiny2["out"]).abs().max().item()
    print(f"PARITY stage2 refine_frames tiny golden (bn): out_abs {e:.2e} (refine, head on the MFMA kernel: {e_chain:.2e})")
    assert e <= 2e-4, (e, e_chain)
    u8 = s2.refine_frames(d(tiny2["img"]), d(tiny2["mask"]), d(tiny2["face_mask"]), out="u8")
    assert torch.equal(u8, ops.pack_rgb8(got))


@pytest.mark.parametrize("variant", ["gn_ws", "bn"])
def test_refine_frames_r256_vs_oracle(variant):
    import restate as O
    from emoportraits_amd import stage2
    over = dict(output_size_s2=256)
    if variant == "gn_ws":
        over.update(norm_layer_type="gn", use_ws=True)
    cfg = stage2.stage2_config(overrides=over)
    sd = stage2.random_state_dict(cfg, seed=3)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 256, 256, generator=g)
    mask = (torch.rand(2, 1, 256, 256, generator=g) > 0.1).float()
    face = (torch.rand(2, 1, 256, 256, generator=g) > 0.3).float()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        ref = O.stage2_forward(sd, cfg, img, mask, face)
    s2 = stage2.Stage2(sd, cfg, DEV)
    d = lambda t: t.to(DEV)
    got = s2.refine_frames(d(img), d(mask), d(face), out="f32")
    chain = s2.refine(d(img), d(mask), d(face))
    e = (got.cpu() - ref["out"]).abs().max().item()
    e_chain = (chain.cpu() - ref["out"]).abs().max().item()
    print(f"PARITY stage2 refine_frames R256 {variant}: out_abs {e:.2e} (refine, head on the MFMA kernel: {e_chain:.2e})")
    assert e <= 5e-4, (e, e_chain)


# ---- the wrapper ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def project(tmp_path_factory, tiny, tiny2):
    """the tiny stage-1 project of tests/test_infer_gpu.py plus logs_s2/exp2 with the tiny stage-2 model"""
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
    exp2 = root / "logs_s2" / "exp2"
    (exp2 / "checkpoints").mkdir(parents=True)
    with open(exp2 / "args.txt", "wt") as f:
        for k, v in tiny2["cfg"].items():
            f.write(f"{k}: {v}\n")
    torch.save(tiny2["state_dict"], exp2 / "checkpoints" / "m.pth")
    return root


def _stage1(project, tiny, source=True, **kw):
    from notebooks.infer import InferenceWrapper
    from test_infer_gpu import _toy_embedders
    w = InferenceWrapper(experiment_name="exp", model_file_name="model.pth", project_dir=str(project), folder="logs",
                         print_params=False, **kw)
    w.embedders.update(_toy_embedders(tiny, w.device))
    if source:
        S = tiny["cfg"]["image_size"]
        w.forward(source_image=tiny["img"], crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=tiny["idt_embed"],
                  custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=tiny["theta_src"])
    return w


def _stage2(project, **kw):
    from notebooks.infer_s2 import InferenceWrapper
    return InferenceWrapper(experiment_name="exp2", model_file_name="m.pth", project_dir=str(project), embedders=MASKS, **kw)


def _frames(N, Hf, Wf, seed=3):
    return torch.randint(0, 256, (N, Hf, Wf, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _collect(gen):
    out = {}
    for b0, t in gen:
        for j in range(t.shape[0]):
            out[b0 + j] = t[j].clone()
    return [out[i] for i in range(len(out))]


def test_in_path_bytes_are_refine_frames_on_stage_ones_output_and_within_one_of_the_stage2_wrapper(project, tiny):
    w, w2 = _stage1(project, tiny), _stage2(project)
    w.attach_stage2(w2)
    S = tiny["cfg"]["image_size"]
    N, bs = 14, 4
    frames = _frames(N, S, S)
    got = _collect(w.animate_frames(frames.pin_memory(), batch_size=bs, ring=2, refine=True))
    assert len(got) == N and all(f.dtype == torch.uint8 and tuple(f.shape) == (S, S, 3) and not f.is_cuda for f in got)
    s2 = w2.model_two
    for b0, img in w.animate_frames(frames, batch_size=bs, to_host=False, as_uint8=False):
        img = img.clone()
        by_hand = s2.refine_frames(img, matting(img).contiguous(), face_parsing(img).contiguous(), out="u8").cpu()
        third = w2.forward(img)[2].cpu()
        for j in range(img.shape[0]):
            assert torch.equal(got[b0 + j], by_hand[j]), b0 + j
            assert (got[b0 + j].int() - third[j].int()).abs().max().item() <= 1, b0 + j
    # masks from the caller instead of the wrapper's embedders; a bare Stage2
    w.attach_stage2(s2)
    again = _collect(w.animate_frames(frames, batch_size=bs, to_host=False, refine=True,
                                      refine_masks=lambda img: (matting(img), face_parsing(img))))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(again, got))
    # the fp32 image itself
    f32 = _collect(w.animate_frames(frames, batch_size=bs, to_host=False, as_uint8=False, refine=True,
                                    refine_masks=lambda img: (matting(img), face_parsing(img))))
    from emoportraits_amd import ops
    assert torch.equal(ops.pack_rgb8(torch.stack(f32)).cpu(), torch.stack(got))
    # cloth: the face mask is all ones
    w2c = _stage2(project, cloth=True)
    w.attach_stage2(w2c)
    cloth = _collect(w.animate_frames(frames[:bs], batch_size=bs, to_host=False, refine=True))
    img = next(w.animate_frames(frames[:bs], batch_size=bs, to_host=False, as_uint8=False))[1].clone()
    m = matting(img).contiguous()
    assert torch.equal(torch.stack(cloth), w2c.model_two.refine_frames(img, m, torch.ones_like(m), out="u8"))
    # without refine the attached model changes nothing
    plain = _collect(w.animate_frames(frames, batch_size=bs, to_host=False))
    w.attach_stage2(None)
    assert all(torch.equal(a, b) for a, b in zip(plain, _collect(w.animate_frames(frames, batch_size=bs, to_host=False))))
    with pytest.raises(ValueError, match="attach_stage2"):
        next(w.animate_frames(frames, refine=True))


def test_graphs_on_equals_graphs_off(project, tiny):
    """three batches of one shape (eager, capture, replay), a fourth, and a ragged last batch; twice, so that the second run
    replays every shape"""
    w2 = _stage2(project)
    S = tiny["cfg"]["image_size"]
    frames = _frames(18, S, S, seed=5)
    runs = {}
    for graphs in (True, False):
        w = _stage1(project, tiny, use_graphs=graphs)
        w.attach_stage2(w2)
        runs[graphs] = [_collect(w.animate_frames(frames, batch_size=4, to_host=False, refine=True)) for _ in range(2)]
        if graphs:
            assert len(w._graphed["stage2_u8"].signatures()) == 2 and w._graphed["stage2_f32"].signatures() == []
        else:
            assert "stage2_u8" not in w._graphed
    for run in runs[True] + runs[False][1:]:
        assert all(torch.equal(a, b) for a, b in zip(run, runs[False][0]))
    g = torch.Generator().manual_seed(17)
    pose = torch.randn(18, tiny["target_pose_embed"].shape[1], generator=g) * 0.5
    srt = (1 + 0.05 * torch.randn(18, 3, generator=g), 0.3 * torch.randn(18, 3, generator=g), 0.05 * torch.randn(18, 3, generator=g))
    out = {}
    for graphs in (True, False):
        w = _stage1(project, tiny, use_graphs=graphs)
        w.attach_stage2(w2)
        out[graphs] = _collect(w.animate(pose, srt, batch_size=4, refine=True))
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False]))


def test_refine_with_paste_back_is_paste_back_of_the_refined_image(project, tiny):
    w, w2 = _stage1(project, tiny), _stage2(project)
    w.attach_stage2(w2)
    S = tiny["cfg"]["image_size"]
    N, Hf, Wf = 10, S + S // 2 + 3, 2 * S + 5
    frames = _frames(N, Hf, Wf, seed=29)
    wins = []
    for n in range(N):
        s = S // 2 + ((Hf - S // 2) * n) // (N - 1)
        wins.append((min(Wf - s, 3 * n + 1), min(Hf - s, 2 * n), s))
    before = frames.clone()
    dev = frames.to(DEV)
    for src in (frames, dev):                                                  # a host chunk and a device-resident one
        full = torch.stack(_collect(w.animate_frames(src, batch_size=4, windows=wins, to_host=False, refine=True, paste_back=True)))
        refined = torch.stack(_collect(w.animate_frames(src, batch_size=4, windows=wins, to_host=False, refine=True, as_uint8=False)))
        for b0 in range(0, N, 4):
            want = w.paste_back(frames[b0:b0 + 4], refined[b0:b0 + 4], wins[b0:b0 + 4])
            assert torch.equal(full[b0:b0 + 4], want), b0
        assert torch.equal(frames, before) and torch.equal(dev.cpu(), before)       # the caller's frames stay as they were
        for i, (x0, y0, s) in enumerate(wins):
            outside = torch.ones(Hf, Wf, dtype=torch.bool)
            outside[y0:y0 + s, x0:x0 + s] = False
            assert torch.equal(full[i].cpu()[outside], frames[i][outside]) and not torch.equal(full[i].cpu(), frames[i]), i
    # the paste matte is computed on the REFINED image
    fn = lambda img: matting(img)
    full = torch.stack(_collect(w.animate_frames(frames[:4], batch_size=4, windows=wins[:4], to_host=False, refine=True, paste_back=True,
                                                 paste_matte=fn)))
    assert torch.equal(full, w.paste_back(frames[:4], refined[:4], wins[:4], matte=fn(refined[:4])))
    # and the frames differ from the unrefined paste
    plain = torch.stack(_collect(w.animate_frames(frames[:4], batch_size=4, windows=wins[:4], to_host=False, paste_back=True)))
    assert not torch.equal(plain, torch.stack(_collect(w.animate_frames(frames[:4], batch_size=4, windows=wins[:4], to_host=False,
                                                                        refine=True, paste_back=True))))


def test_refine_with_identities_equals_each_identitys_own_refined_pass(project, tiny):
    from test_identity_bank_gpu import _drivers, _enrol, _sources
    w = _stage1(project, tiny, source=False, identity_capacity=3)
    w.attach_stage2(_stage2(project))
    assert _enrol(w, tiny, _sources(tiny, 3)) == [0, 1, 2]
    N = 33
    pose, srt = _drivers(tiny, N)
    ids = torch.tensor([(5 * i + i // 7) % 3 for i in range(N)])
    per = []
    for k in range(3):
        w.load_identity(k)
        per.append(_collect(w.animate(pose, srt, batch_size=16, refine=True)))
    mixed = _collect(w.animate(pose, srt, batch_size=16, refine=True, identities=ids))
    for i in range(N):
        assert torch.equal(mixed[i], per[int(ids[i])][i]), i
    assert not torch.equal(per[0][0], per[1][0])


def test_a_stage2_size_other_than_stage_ones_resizes_first(project, tiny, tiny2):
    """stage 1 renders 64 x 64, stage 2 works at 128 x 128 (seeded random weights): bilinear resize, masks of the RESIZED image"""
    from emoportraits_amd import ops, stage2
    cfg = stage2.stage2_config(dict(tiny2["cfg"], output_size_s2=128))
    s2 = stage2.Stage2(stage2.random_state_dict(cfg, seed=2), cfg, DEV)
    w = _stage1(project, tiny)
    w.attach_stage2(s2)
    S = tiny["cfg"]["image_size"]
    assert S == 64
    frames = _frames(6, S, S, seed=7)
    masks = lambda img: (matting(img), face_parsing(img))
    got = _collect(w.animate_frames(frames, batch_size=4, refine=True, refine_masks=masks))
    assert all(tuple(f.shape) == (128, 128, 3) and f.dtype == torch.uint8 for f in got)
    for b0, img in w.animate_frames(frames, batch_size=4, to_host=False, as_uint8=False):
        big = ops.resize2d(img.clone(), (128, 128), "bilinear")
        want = s2.refine_frames(big, matting(big).contiguous(), face_parsing(big).contiguous(), out="u8").cpu()
        for j in range(img.shape[0]):
            assert torch.equal(got[b0 + j], want[j]), b0 + j
    # frames out: the refined 128 x 128 image pasted into windows of larger frames (sides 32 ... 128)
    big_frames = _frames(4, 150, 170, seed=8)
    wins = [(3, 5, 96), (40, 20, 128), (70, 50, 100), (0, 0, 32)]
    full = torch.stack(_collect(w.animate_frames(big_frames, batch_size=4, windows=wins, to_host=False, refine=True, paste_back=True,
                                                 refine_masks=masks)))
    refined = torch.stack(_collect(w.animate_frames(big_frames, batch_size=4, windows=wins, to_host=False, refine=True, as_uint8=False,
                                                    refine_masks=masks)))
    assert tuple(refined.shape) == (4, 3, 128, 128) and torch.equal(full, w.paste_back(big_frames, refined, wins))
    with pytest.raises(ValueError, match="quarter of the 128-pixel"):       # 31 < 128 / 4 (and >= 64 / 4: stage 1 alone takes it)
        next(w.animate_frames(big_frames, windows=[(0, 0, 31)] * 4, refine=True, paste_back=True, refine_masks=masks))
    assert len(_collect(w.animate_frames(big_frames, windows=[(0, 0, 31)] * 4, to_host=False, paste_back=True))) == 4
