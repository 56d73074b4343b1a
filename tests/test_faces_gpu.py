"""Several faces per frame on the GPU (ABI 18).  No tolerance anywhere: the crops are bit for bit the single-window ops on
frames[frame_of], a paste is bit for bit the faces pasted one after another with the single-window op (which
tests/test_paste_back_gpu.py and tests/test_nv12_gpu.py hold to the fp64 restatement).
  * the kernels on the shared small case of tests/faces_reference.py, RGB and NV12, and one production-shaped launch (4 frames of
    1080 x 1920 with 4 faces each, S = 512);
  * InferenceWrapper.animate_frames(faces=) on the tiny fixture with a 2-slot bank: a regular clip (6 frames x 2 faces) against
    the flattened windows= form of the parent path, whose batches are the same; an irregular clip (2, 0, 3, 1, 0, 2 faces)
    against paste_back(faces=) of its own renders -- host frames through the ring, device frames, RGB and NV12."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import faces_reference as R  # noqa: E402
import nv12_reference as NV  # noqa: E402
import paste_back_reference as PB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE = ("bt601", True)


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


def _paste(fmt, frames, img, matte, wins, feather, frame_of=None):
    """ops.paste_windows / paste_windows_nv12 on a device copy of host tensors -> host"""
    from emoportraits_amd import ops
    work, m = frames.to(DEV), None if matte is None else matte.to(DEV)
    if fmt == "rgb8":
        out = ops.paste_windows(work, img.to(DEV), _sq(wins), feather, m, frame_of=frame_of)
    else:
        out = ops.paste_windows_nv12(work, img.to(DEV), _sq(wins), feather, m, *MODE, frame_of=frame_of)
    assert out is work
    return out.cpu()


def _one(fmt, feather):
    return lambda frame, img, matte, w: _paste(fmt, frame, img, matte, [w], feather)


@pytest.fixture(scope="module")
def small():
    R.check_case()
    return {"rgb8": R.small_rgb(), "nv12": R.small_nv12()}


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def test_crops_are_the_window_crops_of_the_faces_frames(small):
    from emoportraits_amd import ops
    x = ops.unpack_rgb8(small["rgb8"]["noise"][0].to(DEV))
    got = ops.resize2d_windows(x, (R.S, R.S), _sq(R.WINDOWS), "bicubic", True, frame_of=R.FRAME_OF)
    assert torch.equal(got, ops.resize2d_windows(x[R.FRAME_OF].contiguous(), (R.S, R.S), _sq(R.WINDOWS), "bicubic", True))
    nv = small["nv12"]["noise"][0].to(DEV)
    got = ops.nv12_windows(nv, (R.S, R.S), _sq(R.WINDOWS), *MODE, frame_of=R.FRAME_OF)
    assert torch.equal(got, ops.nv12_windows(nv[R.FRAME_OF].contiguous(), (R.S, R.S), _sq(R.WINDOWS), *MODE))
    assert tuple(got.shape) == (6, 3, R.S, R.S) and bool(got.any())


@pytest.mark.parametrize("feather,use_matte", PB.CASES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_paste_is_the_faces_pasted_one_after_another(small, fmt, kind, feather, use_matte):
    frames, img, matte = small[fmt][kind]
    m = matte if use_matte else None
    want = R.sequential(_one(fmt, feather), frames, img, m, R.WINDOWS, R.FRAME_OF)
    got = _paste(fmt, frames, img, m, R.WINDOWS, feather, R.FRAME_OF)
    assert torch.equal(got, want) and not torch.equal(got, frames)
    touched = (R.rgb_mask if fmt == "rgb8" else R.nv12_mask)(len(R.FACES), R.WINDOWS, R.FRAME_OF)
    assert torch.equal(got[1], frames[1]) and torch.equal(got[~touched], frames[~touched])


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_order_one_face_per_frame_and_device_only_windows(small, fmt):
    from emoportraits_amd import ops
    frames, img, matte = small[fmt]["noise"]
    got = _paste(fmt, frames, img, matte, R.WINDOWS, 0.0625, R.FRAME_OF)
    # the two faces of frame 0 the other way round: other bytes inside their intersection, the same everywhere else
    order = [1, 0, 2, 3, 4, 5]
    swapped = _paste(fmt, frames, img[order], matte[order], [R.WINDOWS[i] for i in order], 0.0625, R.FRAME_OF)
    mask = R.rgb_mask if fmt == "rgb8" else R.nv12_mask
    both = mask(len(R.FACES), R.WINDOWS[:1], [0]) & mask(len(R.FACES), R.WINDOWS[1:2], [0])
    assert not torch.equal(got[both], swapped[both]) and torch.equal(got[~both], swapped[~both])
    # one face per frame is the batched op
    full, img6, matte6 = (PB.small_inputs() if fmt == "rgb8" else NV.small_inputs())["smooth"]
    assert torch.equal(_paste(fmt, full, img6, matte6, PB.WINDOWS, 0.0625, list(range(6))), _paste(fmt, full, img6, matte6, PB.WINDOWS, 0.0625))
    # windows the host never sees, the middle face of frame 2 invalid: the paste of the others
    want = R.sequential(_one(fmt, 0.0625), frames, img, matte, R.WINDOWS, R.FRAME_OF, skip=(3,))
    for bad in ((300, 100, 96, 95), (400, 100, 96, 96), (300, 100, 31, 31)):
        win = torch.tensor(_sq(R.WINDOWS[:3]) + [bad] + _sq(R.WINDOWS[4:]), dtype=torch.int32).to(DEV)
        work = frames.to(DEV)
        if fmt == "rgb8":
            ops.paste_windows(work, img.to(DEV), win, 0.0625, matte.to(DEV), frame_of=R.FRAME_OF)
        else:
            ops.paste_windows_nv12(work, img.to(DEV), win, 0.0625, matte.to(DEV), *MODE, frame_of=R.FRAME_OF)
        assert torch.equal(work.cpu(), want), bad


def test_paste_faces_production_size():
    """16 faces of S = 512 in 4 frames of 1080 x 1920, 4 each (paste_back_reference.production_inputs regrouped; sides 300 ... 900 at
    random places: most of them overlap), feather 1/16 and a matte; RGB, and the same faces on NV12 frames of random bytes"""
    frames, img, matte, wins = PB.production_inputs()
    frame_of = [m // 4 for m in range(16)]
    meet = lambda a, b: all(a[k] < b[k] + b[2] and b[k] < a[k] + a[2] for k in (0, 1))
    assert sum(meet(wins[a], wins[b]) for a in range(16) for b in range(a + 1, 16) if frame_of[a] == frame_of[b]) >= 8
    frames = frames[:4].contiguous()
    want = R.sequential(_one("rgb8", 0.0625), frames, img, matte, wins, frame_of)
    assert torch.equal(_paste("rgb8", frames, img, matte, wins, 0.0625, frame_of), want)
    nv = torch.randint(0, 256, (4, 1620, 1920), generator=torch.Generator().manual_seed(12), dtype=torch.uint8)
    want = R.sequential(_one("nv12", 0.0625), nv, img, matte, wins, frame_of)
    assert torch.equal(_paste("nv12", nv, img, matte, wins, 0.0625, frame_of), want)


# ---- the wrapper -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


@pytest.fixture(scope="module")
def wrapper(tmp_path_factory, tiny):
    from emoportraits_amd import config
    from test_identity_bank_gpu import _enrol, _sources, _wrapper
    root = tmp_path_factory.mktemp("proj")
    exp = root / "logs" / "exp"
    (exp / "checkpoints").mkdir(parents=True)
    cfg = config.hot_path_config(overrides=tiny["cfg"])
    with open(exp / "args.txt", "wt") as f:
        for k, v in cfg.items():
            f.write(f"{k}: {v}\n")
        f.write("experiment_name: exp\nuse_seg: True\n")
    torch.save(tiny["state_dict"], exp / "checkpoints" / "model.pth")
    w = _wrapper(root, tiny, use_graphs=False, identity_capacity=2)
    assert _enrol(w, tiny, _sources(tiny, 2)) == [0, 1]
    w.load_identity(0)
    return w


def faces_clip(S, counts, seed):
    """frames of (3S/2 + 2) x (2S + 6) random bytes and counts[i] faces in frame i: sides S/2 ... the frame's height, the faces
    of a frame near its top-left corner so that they overlap, odd and even origins"""
    Hf, Wf = S + S // 2 + 2, 2 * S + 6
    assert Hf % 2 == 0 and Wf % 2 == 0
    frames = torch.randint(0, 256, (len(counts), Hf, Wf, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    faces = []
    for i, c in enumerate(counts):
        of_frame = []
        for k in range(c):
            s = S // 2 + ((Hf - S // 2) * ((i + 2 * k) % 5)) // 4
            of_frame.append((min(Wf - s, 7 * k + 3 * i + 1), min(Hf - s, 5 * k + i), s))
        faces.append(of_frame)
    return frames, faces


def _collect(gen):
    out = {}
    for b0, t in gen:
        for j in range(t.shape[0]):
            out[b0 + j] = t[j].cpu().clone()
    return torch.stack([out[i] for i in range(len(out))])


def test_a_regular_clip_is_the_flattened_windows_path(wrapper, tiny):
    """6 frames x 2 faces, batch_size 4: the batches of the faces form are two frames = four faces, those of
    animate_frames(frames[frame_of], windows=flat) -- the same launches, so the fp32 renders are the same bits; the pasted frames
    are those renders pasted face after face with the single-window paste_back"""
    w = wrapper
    S = tiny["cfg"]["image_size"]
    frames, faces = faces_clip(S, [2] * 6, seed=31)
    flat = [f for of_frame in faces for f in of_frame]
    frame_of = [i for i, of_frame in enumerate(faces) for _ in of_frame]
    kw = dict(batch_size=4, identities=[0, 1] * 6, mix=True, smooth_pose=True, smooth_per_identity=True)
    w.reset_pose_state()
    parent = _collect(w.animate_frames(frames[frame_of], windows=flat, to_host=False, as_uint8=False, **kw))
    w.reset_pose_state()
    rendered = _collect(w.animate_frames(frames, faces=faces, to_host=False, as_uint8=False, **kw))
    assert tuple(rendered.shape) == (12, 3, S, S) and torch.equal(rendered, parent)
    want = frames.to(DEV)
    for m, f in enumerate(frame_of):
        want[f:f + 1] = w.paste_back(want[f:f + 1], rendered[m:m + 1], [flat[m]])
    w.reset_pose_state()
    got = _collect(w.animate_frames(frames, faces=faces, ring=2, paste_back=True, **kw))
    assert torch.equal(got, want.cpu()) and not torch.equal(got, frames)


@pytest.mark.parametrize("fmt", ["rgb8", "nv12"])
def test_an_irregular_clip_is_paste_back_of_its_own_renders(wrapper, tiny, fmt):
    """2, 0, 3, 1, 0, 2 faces, batch_size 4 (spans (0,2) (2,4) (4,6)): animate_frames(faces=, paste_back=True) = paste_back(frames,
    the fp32 renders of the same run without it, faces=); frames without a face come back as they went in; host frames through
    the ring and device frames give the same bytes; nothing of the caller's is modified"""
    from emoportraits_amd import ops
    w = wrapper
    S = tiny["cfg"]["image_size"]
    counts = [2, 0, 3, 1, 0, 2]
    rgb, faces = faces_clip(S, counts, seed=37)
    fkw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    frames = rgb if fmt == "rgb8" else ops.pack_nv12(ops.unpack_rgb8(rgb.to(DEV)), *MODE).cpu()
    kw = dict(batch_size=4, faces=faces, identities=[(3 * m + m // 3) % 2 for m in range(8)], mix=True, smooth_pose=True,
              smooth_per_identity=True, **fkw)
    matte = lambda img: img.mean(dim=1, keepdim=True).clamp(0, 1)
    w.reset_pose_state()
    rendered = _collect(w.animate_frames(frames, to_host=False, as_uint8=False, **kw))
    assert rendered.dtype == torch.float32 and tuple(rendered.shape) == (8, 3, S, S)
    before = frames.clone()
    want = w.paste_back(frames, rendered, faces=faces, matte=matte, **fkw)
    assert want.is_cuda and torch.equal(frames, before)
    want = want.cpu()
    assert torch.equal(want[1], frames[1]) and torch.equal(want[4], frames[4]) and not torch.equal(want[0], frames[0])
    paste = dict(paste_back=True, paste_matte=matte)
    w.reset_pose_state()
    host = _collect(w.animate_frames(frames, ring=2, **kw, **paste))
    assert torch.equal(host, want) and torch.equal(frames, before)
    dev_frames = frames.to(DEV)
    w.reset_pose_state()
    dev = _collect(w.animate_frames(dev_frames, to_host=False, **kw, **paste))
    assert torch.equal(dev, want) and torch.equal(dev_frames.cpu(), frames)
    # the uint8 crops of the faces, through the ring, indexed by face
    w.reset_pose_state()
    crops = _collect(w.animate_frames(frames, ring=2, **kw))
    packed = ops.pack_rgb8(rendered.to(DEV)) if fmt == "rgb8" else ops.pack_nv12(rendered.to(DEV), *MODE)
    assert torch.equal(crops, packed.cpu())
