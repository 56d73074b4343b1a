"""Stage 2 inside animate() / animate_frames() (InferenceWrapper.attach_stage2, refine=True) without a GPU: the package's host code on
CPU tensors, its library the host-compiled kernels (tests/emul/emulibs.install), the wrapper made without its constructor and
its driver pass a seeded image; the tiny stage-2 model of tests/golden/tiny_stage2.pt (64 x 64: no resize).
  * by default the stage-2 body is a recording stand-in (seconds): the checks of refine=True raise before any C-ABI call; the
    stand-in is handed stage 1's image and the callables' masks bit for bit, batch by batch, and what it returns is yielded; with
    the real tail on a seeded activation a batch is ONE emo_stage2_head_f32 and neither emo_stage2_compose_f32 nor emo_pack_rgb8;
    refine=False counts the calls it counted before the feature existed;
  * EMO_EMUL_FULL=1 (about a minute more): Stage2.refine_frames on the golden inputs of the real reference, the bound
    Stage2.refine is held to there (tests/test_hot_path_emul.py, tests/test_stage2_gpu.py).
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "emul"))
import emulibs  # noqa: E402

pytestmark = pytest.mark.skipif(not emulibs.available(), reason="needs ROCm clang++ and the built product library (weight packing asks it for tile sizes)")
FULL = os.environ.get("EMO_EMUL_FULL") == "1"
S = 64


def matting(img):
    """deterministic toy matte: exact 0, exact 1 and fractions"""
    return (img.mean(1, keepdim=True) * 1.6 - 0.3).clamp(0, 1)


def face_parsing(img):
    return (img[:, 1:2] > 0.35).float()


def stage1_image(k, b):
    """what the stubbed driver pass returns for its k-th call"""
    return torch.rand(b, 3, S, S, generator=torch.Generator().manual_seed(100 + k))


@pytest.fixture()
def rig(monkeypatch):
    """(stage-1 wrapper with a stubbed driver pass, tiny Stage2 on 'cpu', a stage2.InferenceWrapper around it, the counted library)"""
    lib = emulibs.install(monkeypatch.setattr)
    from emoportraits_amd import stage2
    from emoportraits_amd.infer import InferenceWrapper
    monkeypatch.delenv("EMO_CONV_PRECISION", raising=False)
    tiny = torch.load(os.path.join(HERE, "golden", "tiny_stage2.pt"), weights_only=False)
    s2 = stage2.Stage2(tiny["state_dict"], stage2.stage2_config(tiny["cfg"]), "cpu")
    w2 = object.__new__(stage2.InferenceWrapper)
    w2.model_two, w2.cfg, w2.cloth, w2.device = s2, s2.cfg, False, torch.device("cpu")
    w2.embedders = {"matting": matting, "face_parsing": face_parsing}
    w = object.__new__(InferenceWrapper)
    w.device, w.rank, w.world = torch.device("cpu"), 0, 1
    w.cfg = dict(image_size=S)
    w._init_state(use_graphs=False, pose_momentum=0.3)
    w.embedders = {}
    w._canonical_cl = torch.zeros(1)
    w.driven = []

    def drive(pose, theta):
        w.driven.append(stage1_image(len(w.driven), pose.shape[0]))
        return w.driven[-1].clone()
    w._drive = drive
    lib.calls.clear()
    return w, s2, w2, lib


def _drivers(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    pose = torch.randn(N, 5, generator=g)
    srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.3 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
    return pose, srt


def test_every_check_of_refine_raises_before_the_first_launch(rig):
    w, s2, w2, lib = rig
    pose, srt = _drivers(6)
    frames = torch.zeros(6, 96, 96, 3, dtype=torch.uint8)
    wins = [(8, 8, 64)] * 6

    def both(match, **kw):
        with pytest.raises(ValueError, match=match):
            next(w.animate(pose, srt, batch_size=4, refine=True, **kw))
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(frames, windows=wins, batch_size=4, refine=True, **kw))
    both("attach_stage2")                                              # nothing attached
    w.attach_stage2(w2)
    w.attach_stage2(None)
    both("attach_stage2")                                              # detached again
    with pytest.raises(TypeError):
        w.attach_stage2(object())
    w.attach_stage2(s2)                                                # a bare Stage2 has no mask callables
    both("matting")
    both("callable", refine_masks=3)                                   # refine_masks that is not callable
    w2.embedders = {"matting": matting}
    w.attach_stage2(w2)
    both("face_parsing")
    w2.embedders = {"face_parsing": face_parsing}
    both("matting")
    w2.cloth = True                                                    # cloth: all ones for the face mask, the matte still needed
    both("matting")
    w2.embedders = {"matting": matting, "face_parsing": face_parsing}
    real = s2.device
    s2.device = torch.device("meta")                                   # a stage-2 model on another device
    both("is on")
    s2.device = real
    with pytest.raises(ValueError, match="refine=True"):               # masks without refinement: a mistake, not a silent no-op
        next(w.animate(pose, srt, refine_masks=lambda img: None))
    assert lib.calls == {} and w.driven == []


def test_animate_frames_checks_its_arguments_with_refine_before_any_launch(rig):
    """the argument checks of animate_frames (tests/test_paste_back_emul.py) with refine=True; the quarter rule on output_size_s2"""
    w, s2, w2, lib = rig
    w.attach_stage2(w2)
    frames = torch.zeros(6, 96, 96, 3, dtype=torch.uint8)
    wins = [(8, 8, 64)] * 6
    with pytest.raises(ValueError, match="windows"):
        next(w.animate_frames(frames, paste_back=True, refine=True))
    with pytest.raises(ValueError, match="feather"):
        next(w.animate_frames(frames, windows=wins, paste_back=True, feather=0.75, refine=True))
    with pytest.raises(RuntimeError, match="matting"):
        next(w.animate_frames(frames, windows=wins, paste_back=True, paste_matte=True, refine=True))
    with pytest.raises(ValueError, match="paste_matte"):
        next(w.animate_frames(frames, windows=wins, paste_back=True, paste_matte=3, refine=True))
    with pytest.raises(ValueError, match="as_uint8"):
        next(w.animate_frames(frames, windows=wins, as_uint8=False, refine=True))
    with pytest.raises(ValueError, match="as_uint8"):
        next(w.animate_frames(frames, windows=wins, to_host=False, as_uint8=False, paste_back=True, refine=True))
    with pytest.raises(ValueError, match="quarter of the 64-pixel"):
        next(w.animate_frames(frames, windows=[(0, 0, 15)] * 6, paste_back=True, refine=True))
    w.cfg = dict(image_size=32)                                        # stage 1 at 32, stage 2 at 64: a side of 8 passes the
    with pytest.raises(ValueError, match="quarter of the 64-pixel"):   # stage-1 rule and fails the stage-2 one
        next(w.animate_frames(frames, windows=[(0, 0, 8)] * 6, paste_back=True, refine=True))
    assert lib.calls == {} and w.driven == []


@pytest.mark.parametrize("masks", ["embedders", "cloth", "refine_masks"])
def test_animate_hands_stage_two_the_rendered_image_and_the_masks_batch_by_batch(rig, masks):
    w, s2, w2, lib = rig
    w2.cloth = masks == "cloth"
    w.attach_stage2(w2 if masks != "refine_masks" else s2)
    seen = []

    def stand_in(img, mask, face, out="u8"):
        seen.append((img.clone(), mask.clone(), face.clone(), out))
        return torch.full((img.shape[0], S, S, 3), len(seen), dtype=torch.uint8) if out == "u8" else img * 0.5
    s2.refine_frames = stand_in
    pose, srt = _drivers(10)
    kw = dict(refine_masks=lambda img: (matting(img) * 0.5, face_parsing(img))) if masks == "refine_masks" else {}
    got = list(w.animate(pose, srt, batch_size=4, refine=True, **kw))
    assert [b0 for b0, _ in got] == [0, 4, 8] and [len(f) for _, f in got] == [4, 4, 2]          # a ragged last batch
    for k, (b0, frames) in enumerate(got):
        img, mask, face, out = seen[k]
        want = stage1_image(k, len(frames))
        assert out == "u8" and torch.equal(img, want)
        assert torch.equal(mask, matting(want) * (0.5 if masks == "refine_masks" else 1.0))
        assert torch.equal(face, torch.ones_like(mask) if masks == "cloth" else face_parsing(want))
        assert frames.dtype == torch.uint8 and bool((frames == k + 1).all())
    assert "emo_pack_rgb8" not in lib.calls and "emo_resize2d_f32" not in lib.calls             # 64 -> 64: no resize
    seen.clear()
    got = list(w.animate(pose[:4], srt_slice(srt, 4), batch_size=4, refine=True, as_uint8=False, **kw))
    assert seen[0][3] == "f32" and torch.equal(got[0][1], seen[0][0] * 0.5)


def srt_slice(srt, n):
    return tuple(t[:n] for t in srt)


def test_a_batch_ends_in_one_stage2_head_launch_and_is_the_three_launch_chain(rig):
    """the real tail (Stage2.refine_frames -> ops.stage2_head) behind a stand-in body: a seeded [2,32,64,64] activation"""
    from emoportraits_amd import ops
    w, s2, w2, lib = rig
    w.attach_stage2(w2)
    g = torch.Generator().manual_seed(9)
    act = torch.randn(2, 32, S, S, generator=g)
    scale, shift = torch.rand(2, 32, generator=g) + 0.5, torch.randn(2, 32, generator=g) * 0.3
    masked = []
    s2.encoder = lambda x: masked.append(x) or x
    s2.decoder.body = lambda lat: (act, (scale, shift))
    pose, srt = _drivers(6)
    got = list(w.animate(pose, srt, batch_size=2, refine=True))
    assert len(got) == 3
    assert lib.calls["emo_stage2_head_f32"] == 3 and lib.calls["emo_mul_mask_f32"] == 3
    assert "emo_stage2_compose_f32" not in lib.calls and "emo_pack_rgb8" not in lib.calls and "emo_conv_head_f32" not in lib.calls
    f32 = list(w.animate(pose[:2], srt_slice(srt, 2), batch_size=2, refine=True, as_uint8=False))[0][1]
    for k, (b0, u8) in enumerate(got):
        img = stage1_image(k, 2)
        m, f = matting(img), face_parsing(img)
        assert torch.equal(masked[k], img * m)                                                   # the encoder saw img * matte
        add = ops.conv_head(act, s2.decoder.head, scale, shift, relu_in=True, act="tanh")
        want = ops.stage2_compose(img, add, m, f)
        assert torch.equal(u8, ops.pack_rgb8(want))
        assert (want > 0).any() and (want < 1).any()
    # (the fp32 form of a batch: the driver stub's 4th image)
    img = stage1_image(3, 2)
    add = ops.conv_head(act, s2.decoder.head, scale, shift, relu_in=True, act="tanh")
    assert torch.equal(f32, ops.stage2_compose(img, add, matting(img), face_parsing(img)))
    # a launch form the stream kernel refuses runs the chain Stage2.refine runs
    lib.calls.clear()
    off = torch.empty(img.numel() + 1)[1:].view_as(img).copy_(img)                               # an image 4 bytes off a 16-byte line
    assert off.data_ptr() % 16 and off.is_contiguous()
    odd = ops.stage2_head(act, s2.decoder.head, scale, shift, off, matting(img), None, out="both")
    assert "emo_stage2_head_f32" not in lib.calls and lib.calls["emo_stage2_compose_f32"] == 1 and lib.calls["emo_pack_rgb8"] == 1
    add = ops.conv_igemm(act, s2.decoder.head, scale, shift, relu_in=True, act="tanh")            # (the head as refine() runs it)
    want = ops.stage2_compose(img, add, matting(img), torch.ones(2, 1, S, S))
    assert torch.equal(odd[0], want) and torch.equal(odd[1], ops.pack_rgb8(want))


def test_without_refine_animate_makes_the_calls_it_made_before(rig):
    """refine=False (the default), a model attached or not: per batch one emo_pose_theta_f32 and one emo_pack_rgb8 (none with
    as_uint8=False), the same frames, and nothing else"""
    w, s2, w2, lib = rig
    pose, srt = _drivers(10)
    plain = [(b0, f.clone()) for b0, f in w.animate(pose, srt, batch_size=4)]
    assert lib.calls == {"emo_pose_theta_f32": 3, "emo_pack_rgb8": 3}
    lib.calls.clear()
    w.driven.clear()
    w.attach_stage2(w2)
    again = list(w.animate(pose, srt, batch_size=4))
    assert lib.calls == {"emo_pose_theta_f32": 3, "emo_pack_rgb8": 3}
    assert all(a[0] == b[0] and torch.equal(a[1], b[1]) for a, b in zip(plain, again))
    lib.calls.clear()
    w.driven.clear()
    raw = list(w.animate(pose, srt, batch_size=4, as_uint8=False))
    assert lib.calls == {"emo_pose_theta_f32": 3} and all(torch.equal(f, stage1_image(k, len(f))) for k, (_, f) in enumerate(raw))


@pytest.mark.skipif(not FULL, reason="EMO_EMUL_FULL=1: the stage-2 refinement (about a minute)")
def test_refine_frames_through_the_emulated_kernels_matches_the_reference(rig):
    """Stage2.refine_frames on the golden img / mask / face_mask of the real reference: out_abs <= 2e-4, the bound refine() is
    held to on the same golden (tests/test_hot_path_emul.py), and the bytes within 1 of the golden image's.
    Measured on the emulated kernels: out_abs 4.47e-07, largest byte difference 0."""
    w, s2, w2, lib = rig
    tiny = torch.load(os.path.join(HERE, "golden", "tiny_stage2.pt"), weights_only=False)
    f32 = s2.refine_frames(tiny["img"], tiny["mask"], tiny["face_mask"], out="f32")
    assert lib.calls["emo_stage2_head_f32"] == 1 and "emo_stage2_compose_f32" not in lib.calls
    u8 = s2.refine_frames(tiny["img"], tiny["mask"], tiny["face_mask"], out="u8")
    out_abs = (f32 - tiny["out"]).abs().max().item()
    want = tiny["out"].clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1)
    byte_err = (u8.int() - want.int()).abs().max().item()
    print(f"PARITY emulated stage 2 refine_frames (tiny golden, bn): out_abs {out_abs:.2e}, largest byte difference {byte_err}")
    assert out_abs <= 2e-4 and byte_err <= 1
