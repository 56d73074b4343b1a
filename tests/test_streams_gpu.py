"""Frames of different sizes in one batch on the GPU (ABI 19).  No tolerance anywhere: every comparison is bit for bit against
the parent's own entry points on the canvas batch of tests/streams_reference.py (the premise of that comparison is asserted on
the CPU build, tests/test_streams_emul.py).
  * the kernels on the shared small case, rgb8 and NV12, and one production-shaped launch: 16 faces of S = 512 in four frames of
    480 x 640, 720 x 1280, 1080 x 1920 and 2160 x 3840, four each, against the 2160 x 3840 canvas;
  * InferenceWrapper.animate_streams on the tiny fixture with a 2-slot bank: three streams of equal length and three frame
    sizes with irregular face counts, identities over both slots, mix and smooth_pose, against animate_frames(canvas clip,
    faces=) -- fp32 renders, uint8 crops through the ring, paste_back with a matte for host frames through the ring and for
    device frames, rgb8 and NV12; streams of unequal length against paste_back(faces=) of the run's own renders, frame by frame;
    refine=True against the canvas path; the caller's tensors unchanged after every call."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import paste_back_reference as PB  # noqa: E402
import streams_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE = ("bt601", True)
FMTS = ["rgb8", "nv12"]


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


def _mode(fmt):
    return MODE if fmt == "nv12" else ()


def _canvas_crops(canvas, size, wins, frame_of, fmt):
    """the parent's crops of a uniform batch on the device"""
    from emoportraits_amd import ops
    if fmt == "nv12":
        return ops.nv12_windows(canvas, (size, size), _sq(wins), *MODE, frame_of=frame_of)
    return ops.resize2d_windows(ops.unpack_rgb8(canvas), (size, size), _sq(wins), "bicubic", True, frame_of=frame_of)


def _canvas_paste(canvas, img, matte, wins, frame_of, feather, fmt):
    from emoportraits_amd import ops
    if fmt == "nv12":
        return ops.paste_windows_nv12(canvas, img, _sq(wins), feather, matte, *MODE, frame_of=frame_of)
    return ops.paste_windows(canvas, img, _sq(wins), feather, matte, frame_of=frame_of)


# ---- the kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather,use_matte", PB.CASES)
@pytest.mark.parametrize("fmt", FMTS)
def test_the_small_case_is_the_canvas(fmt, feather, use_matte):
    from emoportraits_amd import ops
    R.check_case(fmt)
    frames, sizes, wins = R.random_frames(R.SIZES[fmt], fmt, 7), R.SIZES[fmt], R.windows(fmt)
    _, img, matte = PB.small_inputs()["noise"]
    img, matte = img.to(DEV), (matte.to(DEV) if use_matte else None)
    canvas = R.canvas(frames, fmt, 1).to(DEV)
    dev = [f.to(DEV) for f in frames]
    crops = ops.crop_faces_mixed(dev, R.S, _sq(wins), R.FRAME_OF, fmt, *_mode(fmt))
    assert torch.equal(crops, _canvas_crops(canvas, R.S, wins, R.FRAME_OF, fmt)) and bool(crops.any())
    assert all(torch.equal(d.cpu(), f) for d, f in zip(dev, frames))
    want = R.regions(_canvas_paste(canvas, img, matte, wins, R.FRAME_OF, feather, fmt).cpu(), sizes, fmt)
    assert ops.paste_faces_mixed(dev, img, _sq(wins), R.FRAME_OF, feather, matte, fmt, *_mode(fmt)) is dev
    assert all(torch.equal(d.cpu(), w) for d, w in zip(dev, want))
    assert torch.equal(want[1], frames[1]) and not torch.equal(want[0], frames[0])
    # windows the host never sees, one of them inside the canvas but outside ITS frame: the paste of the others, zeros for its crop
    keep = [0, 2, 3, 4, 5]
    bad = torch.tensor(_sq(wins[:1] + [R.OUTSIDE_ITS_FRAME] + wins[2:]), dtype=torch.int32).to(DEV)
    canvas = R.canvas(frames, fmt, 1).to(DEV)
    want = R.regions(_canvas_paste(canvas, img[keep], None if matte is None else matte[keep], [wins[i] for i in keep],
                                   [R.FRAME_OF[i] for i in keep], feather, fmt).cpu(), sizes, fmt)
    dev = [f.to(DEV) for f in frames]
    got = ops.crop_faces_mixed(dev, R.S, bad, R.FRAME_OF, fmt, *_mode(fmt))
    assert not bool(got[1].any()) and torch.equal(got[keep], crops[keep])
    ops.paste_faces_mixed(dev, img, bad, R.FRAME_OF, feather, matte, fmt, *_mode(fmt))
    assert all(torch.equal(d.cpu(), w) for d, w in zip(dev, want))


def test_a_production_shaped_launch_is_the_canvas():
    """16 faces of S = 512 in four frames of 480 x 640, 720 x 1280, 1080 x 1920 and 2160 x 3840, four each; sides and places as
    paste_back_reference.production_inputs draws them, clipped to each frame; feather 1/16 and a matte; rgb8, then NV12"""
    from emoportraits_amd import ops
    _, img, matte, drawn = PB.production_inputs()
    sizes = [(480, 640), (720, 1280), (1080, 1920), (2160, 3840)]
    frame_of = [m // 4 for m in range(16)]
    wins = []
    for (x0, y0, s), f in zip(drawn, frame_of):
        h, w = sizes[f]
        s = min(s, h, w)
        wins.append((min(x0, w - s), min(y0, h - s), s))
    assert all(4 * s >= 512 for _, _, s in wins)
    img, matte = img.to(DEV), matte.to(DEV)
    for fmt in FMTS:
        frames = R.random_frames(sizes, fmt, 13)
        canvas = R.canvas(frames, fmt, 14).to(DEV)
        dev = [f.to(DEV) for f in frames]
        crops = ops.crop_faces_mixed(dev, 512, _sq(wins), frame_of, fmt, *_mode(fmt))
        assert torch.equal(crops, _canvas_crops(canvas, 512, wins, frame_of, fmt))
        del crops
        want = _canvas_paste(canvas, img, matte, wins, frame_of, 0.0625, fmt)
        ops.paste_faces_mixed(dev, img, _sq(wins), frame_of, 0.0625, matte, fmt, *_mode(fmt))
        for d, f, w, hw in zip(dev, frames, want, sizes):
            assert torch.equal(d, R.region(w, hw, fmt)) and not torch.equal(d.cpu(), f)
        del want, canvas, dev


# ---- the wrapper -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


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


@pytest.fixture(scope="module")
def wrapper(project, tiny):
    from test_identity_bank_gpu import _enrol, _sources, _wrapper
    w = _wrapper(project, tiny, use_graphs=False, identity_capacity=2)
    assert _enrol(w, tiny, _sources(tiny, 2)) == [0, 1]
    w.load_identity(0)
    return w


def stream_sizes(S):
    """three frame sizes (H, W), all even, none a multiple of the others"""
    return [(S + S // 2 + 2, 2 * S + 6), (S + 6, S + 2), (2 * S, S + S // 2)]


def make_streams(S, counts, fmt, seed, device=None):
    """one stream per row of counts, stream k in size k (mod 3), counts[k][t] faces in its frame t: sides S / 2 ... the frame's
    smaller side, near the top-left corner so that the faces of a frame overlap, odd and even origins; identities over both slots"""
    from emoportraits_amd import ops
    g = torch.Generator().manual_seed(seed)
    streams = []
    for k, of_stream in enumerate(counts):
        H, W = stream_sizes(S)[k % 3]
        rgb = torch.randint(0, 256, (len(of_stream), H, W, 3), generator=g, dtype=torch.uint8)
        frames = rgb if fmt == "rgb8" else ops.pack_nv12(ops.unpack_rgb8(rgb.to(DEV)), *MODE).cpu()
        faces, side = [], min(H, W)
        for t, c in enumerate(of_stream):
            of_frame = []
            for j in range(c):
                s = S // 2 + ((side - S // 2) * ((t + 2 * j + k) % 5)) // 4
                of_frame.append((min(W - s, 7 * j + 3 * t + k + 1), min(H - s, 5 * j + t), s))
            faces.append(of_frame)
        n = sum(of_stream)
        streams.append(dict(frames=frames if device is None else frames.to(device), faces=faces,
                            identities=[(3 * m + m // 3 + k) % 2 for m in range(n)]))
    return streams


def canvas_clip(streams, fmt):
    """the streams' frames in tick order on a canvas -> (order, canvas clip on the host, faces per frame, identities per face)"""
    from emoportraits_amd import frames as F
    order = F.interleave([len(st["faces"]) for st in streams])
    first = [[0] for _ in streams]
    for f, st in zip(first, streams):
        for of_frame in st["faces"]:
            f.append(f[-1] + len(of_frame))
    clip = R.canvas([streams[s]["frames"][t] for s, t in order], fmt, 9)
    ids = [i for s, t in order for i in streams[s]["identities"][first[s][t]:first[s][t + 1]]]
    return order, clip, [streams[s]["faces"][t] for s, t in order], ids


def _rows(gen):
    out = {}
    for b0, t in gen:
        for j in range(t.shape[0]):
            out[b0 + j] = t[j].cpu().clone()
    return [out[i] for i in range(len(out))]


def _items(gen):
    return [(s, t, o.cpu().clone()) for batch in gen for s, t, o in batch]


COUNTS = [[1, 2, 0, 1], [1, 0, 1, 2], [2, 1, 1, 0]]                             # 12 faces; tick order: 1 1 2 | 2 0 1 | 0 1 1 | 1 2 0


@pytest.mark.parametrize("fmt", FMTS)
def test_three_streams_are_animate_frames_of_the_canvas_clip(wrapper, tiny, fmt):
    from emoportraits_amd import frames as F
    w, S = wrapper, tiny["cfg"]["image_size"]
    streams = make_streams(S, COUNTS, fmt, seed=41)
    order, clip, faces, ids = canvas_clip(streams, fmt)
    sizes = [R.frame_size(streams[s]["frames"][t], fmt) for s, t in order]
    counts = [len(f) for f in faces]
    assert counts == [1, 1, 2, 2, 0, 1, 0, 1, 1, 1, 2, 0] and F.face_spans(counts, 0, 12, 4) == [(0, 3), (3, 7), (7, 10), (10, 12)]
    before = [st["frames"].clone() for st in streams]
    fkw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    kw = dict(batch_size=4, mix=True, smooth_pose=True, **fkw)
    ckw = dict(faces=faces, identities=ids, smooth_per_identity=True, **kw)
    unchanged = lambda: all(torch.equal(st["frames"], b) for st, b in zip(streams, before))
    with_faces = [(s, t) for (s, t), c in zip(order, counts) if c]
    # fp32 renders
    w.reset_pose_state()
    want = torch.stack(_rows(w.animate_frames(clip, to_host=False, as_uint8=False, **ckw)))
    w.reset_pose_state()
    got = _items(w.animate_streams(streams, to_host=False, as_uint8=False, **kw))
    assert [(s, t) for s, t, _ in got] == with_faces and [o.shape[0] for _, _, o in got] == [c for c in counts if c]
    assert got[0][2].dtype == torch.float32 and torch.equal(torch.cat([o for _, _, o in got]), want) and unchanged()
    # uint8 crops through the ring
    w.reset_pose_state()
    want = torch.stack(_rows(w.animate_frames(clip, ring=2, **ckw)))
    w.reset_pose_state()
    got = _items(w.animate_streams(streams, ring=2, **kw))
    assert [(s, t) for s, t, _ in got] == with_faces and torch.equal(torch.cat([o for _, _, o in got]), want) and unchanged()
    # paste_back with a matte: host frames through the ring, device frames
    matte = lambda img: img.mean(dim=1, keepdim=True).clamp(0, 1)
    paste = dict(paste_back=True, paste_matte=matte)
    w.reset_pose_state()
    want = _rows(w.animate_frames(clip, ring=2, **ckw, **paste))
    w.reset_pose_state()
    host = _items(w.animate_streams(streams, ring=2, **kw, **paste))
    dev_streams = [dict(st, frames=st["frames"].to(DEV)) for st in streams]
    w.reset_pose_state()
    dev = _items(w.animate_streams(dev_streams, to_host=False, **kw, **paste))
    for got in (host, dev):
        assert [(s, t) for s, t, _ in got] == order
        for (s, t, o), full, hw in zip(got, want, sizes):
            assert torch.equal(o, R.region(full, hw, fmt)), (s, t)
    pasted = [not torch.equal(o, streams[s]["frames"][t]) for s, t, o in host]
    assert pasted == [c > 0 for c in counts] and unchanged()
    assert all(torch.equal(d["frames"].cpu(), b) for d, b in zip(dev_streams, before))


@pytest.mark.parametrize("fmt", FMTS)
def test_streams_of_unequal_length_are_paste_back_of_their_own_renders(wrapper, tiny, fmt):
    w, S = wrapper, tiny["cfg"]["image_size"]
    streams = make_streams(S, [[1, 2, 0, 1, 1], [2], [0, 1, 1]], fmt, seed=43)
    streams[2]["frames"] = [streams[2]["frames"][:1], streams[2]["frames"][1:]]      # (chunks)
    full = [st["frames"] if isinstance(st["frames"], torch.Tensor) else torch.cat(st["frames"]) for st in streams]
    before = [f.clone() for f in full]
    fkw = dict(frame_format="nv12", colorspace=MODE[0], full_range=MODE[1]) if fmt == "nv12" else {}
    kw = dict(batch_size=3, mix=True, smooth_pose=True, **fkw)
    w.reset_pose_state()
    renders = {(s, t): o for s, t, o in _items(w.animate_streams(streams, to_host=False, as_uint8=False, **kw))}
    w.reset_pose_state()
    got = _items(w.animate_streams(streams, ring=2, paste_back=True, feather=0.125, **kw))
    assert [(s, t) for s, t, _ in got] == [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2), (2, 2), (0, 3), (0, 4)]
    for s, t, o in got:
        frame, of_frame = full[s][t:t + 1], streams[s]["faces"][t]
        if not of_frame:
            assert (s, t) not in renders and torch.equal(o, frame[0])
            continue
        want = w.paste_back(frame, renders[(s, t)], faces=[of_frame], feather=0.125, **fkw)
        assert torch.equal(o, want[0].cpu()) and not torch.equal(o, frame[0]), (s, t)
    assert all(torch.equal(f, b) for f, b in zip(full, before))


def test_refine_in_the_streams_path_is_the_canvas_path(project, tiny, golden_dir):
    """stage 2 in the path (the tiny stage-2 fixture of tests/test_refine_gpu.py): refinement starts where the render returns,
    so the pasted frames are those of the canvas path"""
    import test_refine_gpu as T
    from emoportraits_amd import frames as F
    tiny2 = torch.load(os.path.join(golden_dir, "tiny_stage2.pt"), weights_only=False)
    exp2 = project / "logs_s2" / "exp2"
    (exp2 / "checkpoints").mkdir(parents=True)
    with open(exp2 / "args.txt", "wt") as f:
        for k, v in tiny2["cfg"].items():
            f.write(f"{k}: {v}\n")
    torch.save(tiny2["state_dict"], exp2 / "checkpoints" / "m.pth")
    w = T._stage1(project, tiny)
    w.attach_stage2(T._stage2(project))
    S = tiny["cfg"]["image_size"]
    streams = [{k: v for k, v in st.items() if k != "identities"} for st in make_streams(S, [[1, 2], [1, 0], [0, 1]], "rgb8", seed=47)]
    order = F.interleave([2, 2, 2])
    clip = R.canvas([streams[s]["frames"][t] for s, t in order], "rgb8", 9)
    faces = [streams[s]["faces"][t] for s, t in order]
    kw = dict(batch_size=4, ring=2, refine=True, paste_back=True)
    want = _rows(w.animate_frames(clip, faces=faces, **kw))
    got = _items(w.animate_streams(streams, **kw))
    assert [(s, t) for s, t, _ in got] == order
    for (s, t, o), full in zip(got, want):
        assert torch.equal(o, R.region(full, R.frame_size(streams[s]["frames"][t], "rgb8"), "rgb8")), (s, t)
    assert got[4][:2] == (1, 1) and not torch.equal(got[0][2], streams[0]["frames"][0]) and torch.equal(got[4][2], streams[1]["frames"][1])
