"""The five ABI 22 entry points (csrc/resample.hip: emo_yuv420_crop_f32, emo_pack_yuv420, emo_paste_yuv420, emo_yuv420_crop_ragged_f32,
emo_paste_ragged_yuv420) without a GPU: the kernels are compiled for the host from the product's own source (tests/emul/emulibs.py,
the sequential build) and run on host memory, every surface between guard bytes and with pitches larger than a row.  The checks
themselves are tests/yuv420_reference.py's, shared with tests/test_yuv420_gpu.py:
  * exact: layout 0 is the ten NV12 entry points; yuv420p is NV12 on the same samples; p010 and yuv420p10 agree on the same codes,
    ignore the unused bits on read and write them as zero; a 10-bit frame of codes 4 * byte decodes to the 8-bit crop (limited
    range); ABI 17's exact cases, the faces and the ragged forms on every new layout; the refusals, with nothing written;
  * the 10-bit layouts against the fp64 restatement: D within 1e-6, C within 1e-5, E and P every code within 1 and at most 2e-3
    of the touched samples different at all, torch's own fp32 evaluation held to the same caps as the premise;
  * ops.* and InferenceWrapper.animate_frames / paste_back / animate_streams / animate on CPU tensors in every new format, the
    package pointed at the host-compiled library inside the test only, calls counted.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
from counting_lib import CountingLib as _Lib  # noqa: E402
import emulibs  # noqa: E402
import yuv420_reference as Y  # noqa: E402

R = Y.R


@pytest.fixture(scope="module")
def lib():
    return emulibs.stream(False)


@pytest.fixture(scope="module")
def api(lib):
    from emoportraits_amd import hip
    return Y.Api(lib, Y.HostMemory(), hip.SIGNATURES)


@pytest.fixture(scope="module")
def inp():
    return Y.inputs()


def test_the_restatement_at_8_bits_is_nv12_reference(inp):
    Y.check_the_restatement_at_8_bits_is_nv12_reference(inp)


def test_layout_0_is_the_ten_nv12_entry_points(api, inp):
    Y.check_layout0_is_the_nv12_entry_points(api, inp)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_yuv420p_is_nv12_on_the_same_samples(api, inp, kind, which):
    Y.check_planar_8bit_is_nv12(api, inp, kind, which)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_p010_and_yuv420p10_agree_and_keep_the_unused_bits_clean(api, inp, kind, which):
    Y.check_the_two_10bit_layouts_agree(api, inp, kind, which)


@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_codes_4_times_the_byte_decode_to_the_8bit_crop_in_limited_range(api, inp, kind):
    Y.check_8bit_against_10bit_limited_range(api, inp, kind)


@pytest.mark.parametrize("fmt", Y.NEW)
def test_the_exact_cases_of_abi_17(api, inp, fmt):
    Y.check_exact_cases(api, inp, fmt)


@pytest.mark.parametrize("fmt", Y.NEW)
def test_faces_are_pasted_in_list_order_and_ragged_frames_are_uniform_frames(api, inp, fmt):
    Y.check_faces_and_ragged(api, inp, fmt)


def test_refusals_write_nothing(api, inp):
    Y.check_refusals(api, inp)


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("fmt", ["p010", "yuv420p10"])
def test_10bit_against_the_fp64_restatement(api, inp, fmt, kind):
    """Measured, worst over all cases (the CPU emulation of the product's kernels and the MI355X give the same figures): D
    1.65e-7, C 4.59e-7; E 5.60e-5 of the samples differ, P 6.98e-4 of the touched samples, never by more than 1; torch's fp32
    evaluation of the restatement: 1.65e-7, 3.87e-7, 5.60e-5, 6.85e-4"""
    Y.check_10bit_against_fp64(api, inp, fmt, kind, print)


def test_the_entry_points_are_in_the_abi_table():
    from emoportraits_amd import hip, _abi_version
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert _abi_version.EMO_ABI_VERSION >= 22 and "ABI 22." in hdr
    for name, n in (("emo_yuv420_crop_f32", 21), ("emo_pack_yuv420", 14), ("emo_paste_yuv420", 22), ("emo_yuv420_crop_ragged_f32", 15),
                    ("emo_paste_ragged_yuv420", 16)):
        assert f"int {name}(" in hdr and len(hip.SIGNATURES[name]) == n


# ---- host logic on CPU tensors ---------------------------------------------------------------------------------------------
def _image(k, b):
    return torch.rand(b, 3, Y.S, Y.S, generator=torch.Generator().manual_seed(40 + k)) * 1.2 - 0.1


@pytest.fixture()
def wrapper(monkeypatch, lib):
    """an InferenceWrapper on CPU tensors: the library the host-compiled one, the networks stand-ins (the driver pass a seeded
    image per call), the uploads plain copies"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import hip
    from emoportraits_amd.infer import InferenceWrapper
    facade = _Lib(lib)
    monkeypatch.setattr(hip, "load", lambda: facade)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    monkeypatch.setattr(frames_mod, "uploaded", lambda chunk, spans, device, stream: ((a, b, chunk[a:b].clone()) for a, b in spans))

    def uploaded_mixed(batches, device, stream, copy_all):
        for batch in batches:
            shapes = [tuple(f.shape) for f in batch]
            offsets, total = frames_mod.arena_layout(shapes, batch[0].element_size())
            arena = torch.zeros(total, dtype=torch.uint8)
            views = frames_mod.arena_views(arena, shapes, offsets, batch[0].dtype)
            for v, f in zip(views, batch):
                v.copy_(f)
            yield views, arena
    monkeypatch.setattr(frames_mod, "uploaded_mixed", uploaded_mixed)
    w = object.__new__(InferenceWrapper)
    w.device, w.rank, w.world = torch.device("cpu"), 0, 1
    w.cfg = dict(image_size=Y.S)
    w._init_state(use_graphs=False)
    w.embedders = {}
    w._canonical_cl = torch.zeros(1)
    w.lib = facade
    w.crops, w.driven = [], []

    def head_pose(crops):
        w.crops.append(crops.clone())
        return (torch.eye(4).expand(crops.shape[0], 4, 4).contiguous(),)

    def drive(pose, theta):
        w.driven.append(_image(len(w.driven), pose.shape[0]))
        return w.driven[-1].clone()
    w._head_pose = head_pose
    w._expression = lambda crops, theta, what: (torch.zeros(crops.shape[0], 4), None)
    w._drive = drive
    return w


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


def _frames(inp, fmt, kind="noise"):
    """(the clip in the format, the same samples as NV12 frames -- 10-bit: None, the codes)"""
    codes = inp[kind][0 if Y.BITS[fmt] == 8 else 1]
    return Y.tensor_of(codes, fmt), (Y.tensor_of(codes, "nv12") if Y.BITS[fmt] == 8 else None), codes


@pytest.mark.parametrize("fmt", Y.NEW)
def test_ops_on_cpu_tensors(wrapper, api, inp, fmt):
    from emoportraits_amd import ops
    frames, _, codes = _frames(inp, fmt, "smooth")
    img, matte = inp["smooth"][2], inp["smooth"][3]
    mode = ("bt601", True)
    assert frames.dtype == Y.TORCH_DTYPE[fmt] == ops.yuv420_dtype(fmt)
    rc, want = api.crop(fmt, codes, Y.WINDOWS_ODD, (Y.S, Y.S), mode)
    assert torch.equal(ops.yuv420_windows(frames, fmt, (Y.S, Y.S), _sq(Y.WINDOWS_ODD), *mode), want)
    rc, want = api.crop(fmt, codes, None, (Y.H, Y.W), mode)
    assert torch.equal(ops.yuv420_windows(frames, fmt, colorspace=mode[0], full_range=mode[1]), want)
    rc, want, _ = api.paste(fmt, codes, img, Y.WINDOWS_ODD, 0.0625, matte, mode)
    work = frames.clone()
    assert ops.paste_windows_yuv420(work, fmt, img, _sq(Y.WINDOWS_ODD), 0.0625, matte, *mode) is work
    assert torch.equal(Y.codes_of(work, fmt), want)
    rc, want, _ = api.pack(fmt, img, mode)
    got = ops.pack_yuv420(img, fmt, *mode)
    assert got.dtype == frames.dtype and tuple(got.shape) == (Y.N, 3 * Y.S // 2, Y.S) and torch.equal(Y.codes_of(got, fmt), want)
    if not Y.PLANAR[fmt]:                                                        # a [..., :W] view of a padded surface is taken as it is
        padded = torch.zeros((Y.N, frames.shape[1], Y.W + 32), dtype=frames.dtype)
        padded[:, :, :Y.W] = frames
        rc, want = api.crop(fmt, codes, Y.WINDOWS, (Y.S, Y.S), mode)
        assert torch.equal(ops.yuv420_windows(padded[:, :, :Y.W], fmt, (Y.S, Y.S), _sq(Y.WINDOWS), *mode), want)
    wrapper.lib.calls.clear()
    sq = _sq(Y.WINDOWS)
    other = torch.zeros(frames.shape, dtype=torch.uint16 if frames.dtype == torch.uint8 else torch.uint8)
    for bad, match in ((other, fmt), (frames[:, :404], "3H/2"), (frames[:, :, :479], "3H/2"), (frames[:, :, ::2], "stride"),
                       (frames[0], "3H/2")):
        with pytest.raises(ValueError, match=match):
            ops.yuv420_windows(bad, fmt, (Y.S, Y.S), sq)
        with pytest.raises(ValueError, match=match):
            ops.paste_windows_yuv420(bad, fmt, img, sq)
    if Y.PLANAR[fmt]:
        padded = torch.zeros((Y.N, frames.shape[1], Y.W + 32), dtype=frames.dtype)
        with pytest.raises(ValueError, match="dense rows"):
            ops.yuv420_windows(padded[:, :, :Y.W], fmt, (Y.S, Y.S), sq)
    with pytest.raises(ValueError, match="inside"):
        ops.yuv420_windows(frames, fmt, (Y.S, Y.S), sq[:5] + [(353, 142, 128, 128)])
    with pytest.raises(ValueError, match="colorspace"):
        ops.yuv420_windows(frames, fmt, (Y.S, Y.S), sq, colorspace="bt2020")
    with pytest.raises(ValueError, match="even"):
        ops.pack_yuv420(img[:, :, :127], fmt)
    with pytest.raises(ValueError, match="frame_format"):
        ops.pack_yuv420(img, "i420")
    assert wrapper.lib.calls == {}


@pytest.mark.parametrize("fmt", Y.NEW)
def test_wrapper_paste_back_and_animate_frames(wrapper, api, inp, fmt):
    """animate_frames in every new format: one crop launch per batch; the crops the networks see are those of the NV12 path on
    the same samples (8-bit) or ops.yuv420_windows' (10-bit); what is yielded is ops.pack_yuv420 of the driver pass' images, with
    paste_back=True paste_back() of them; yuv420p results are the NV12 path's re-laid out"""
    from emoportraits_amd import ops
    frames, nv12, codes = _frames(inp, fmt)
    matte = inp["smooth"][3]
    w, mode = wrapper, ("bt601", False)
    kw = dict(frame_format=fmt, colorspace=mode[0], full_range=mode[1])
    got = list(w.animate_frames(frames, batch_size=4, windows=Y.WINDOWS_ODD, to_host=False, **kw))
    assert [b0 for b0, _ in got] == [0, 4] and [t.shape[0] for _, t in got] == [4, 2]
    assert w.lib.calls == {"emo_yuv420_crop_f32": 2, "emo_pack_yuv420": 2}
    rc, crops = api.crop(fmt, codes, Y.WINDOWS_ODD, (Y.S, Y.S), mode)
    assert torch.equal(torch.cat(w.crops), crops)
    images = torch.cat(w.driven)
    out = torch.cat([t for _, t in got])
    assert out.dtype == frames.dtype and tuple(out.shape[1:]) == (3 * Y.S // 2, Y.S) and torch.equal(out, ops.pack_yuv420(images, fmt, *mode))
    if nv12 is not None:                                                         # the NV12 path on the same samples, re-laid out
        assert torch.equal(Y.codes_of(out, fmt), ops.pack_nv12(images, *mode).int())
        assert torch.equal(crops, ops.nv12_windows(nv12, (Y.S, Y.S), _sq(Y.WINDOWS_ODD), *mode))
    # rgb8 crops out of the same run, and the format out of rgb8 frames
    w.crops.clear(); w.driven.clear()
    rgb = torch.cat([t for _, t in w.animate_frames(frames, batch_size=4, windows=Y.WINDOWS_ODD, to_host=False, out_format="rgb8", **kw)])
    assert torch.equal(rgb, ops.pack_rgb8(torch.cat(w.driven)))
    # paste_back() and animate_frames(paste_back=True)
    w.crops.clear(); w.driven.clear(); w.lib.calls.clear()
    before = frames.clone()
    img = inp["smooth"][2]
    rc, want, _ = api.paste(fmt, codes, img, Y.WINDOWS, 0.0625, matte, mode)
    back = w.paste_back(frames, img, Y.WINDOWS, matte=matte, **kw)
    assert back.dtype == frames.dtype and torch.equal(Y.codes_of(back, fmt), want) and torch.equal(frames, before)
    assert w.lib.calls == {"emo_paste_yuv420": 1}
    if nv12 is not None:
        assert torch.equal(Y.codes_of(back, fmt), w.paste_back(nv12, img, Y.WINDOWS, matte=matte, frame_format="nv12", colorspace=mode[0],
                                                               full_range=mode[1]).int())
    w.lib.calls.clear()
    got = list(w.animate_frames(frames, batch_size=4, windows=Y.WINDOWS, to_host=False, paste_back=True, feather=0.25,
                                paste_matte=lambda im: matte[:im.shape[0]], **kw))
    assert w.lib.calls == {"emo_yuv420_crop_f32": 2, "emo_paste_yuv420": 2}
    images = torch.cat(w.driven)
    want = torch.cat([w.paste_back(frames[a:b], images[a:b], Y.WINDOWS[a:b], 0.25, matte[:b - a], **kw) for a, b in ((0, 4), (4, 6))])
    assert torch.equal(torch.cat([t for _, t in got]), want) and torch.equal(frames, before) and not torch.equal(want, frames)


@pytest.mark.parametrize("fmt", Y.NEW)
def test_wrapper_faces_and_streams(wrapper, api, inp, fmt):
    from emoportraits_amd import ops
    frames, nv12, codes = _frames(inp, fmt)
    w, mode = wrapper, ("bt709", True)
    kw = dict(frame_format=fmt, colorspace=mode[0], full_range=mode[1])
    faces = [[w_ for w_, f in zip(Y.FACES, Y.FACE_FRAME) if f == i] for i in range(Y.N)]
    got = list(w.animate_frames(frames, batch_size=8, faces=faces, to_host=False, paste_back=True, feather=0.0625, **kw))
    assert w.lib.calls == {"emo_yuv420_crop_f32": 1, "emo_paste_yuv420": 1}
    images = torch.cat(w.driven)
    rc, crops = api.crop(fmt, codes, Y.FACES, (Y.S, Y.S), mode, frame_of=Y.FACE_FRAME)
    assert torch.equal(torch.cat(w.crops), crops)
    rc, want, _ = api.paste(fmt, codes, images, Y.FACES, 0.0625, None, mode, frame_of=Y.FACE_FRAME)
    out = torch.cat([t for _, t in got])
    assert torch.equal(Y.codes_of(out, fmt), want)
    assert torch.equal(out, w.paste_back(frames, images, feather=0.0625, faces=faces, **kw))
    if nv12 is not None:
        assert torch.equal(want, w.paste_back(nv12, images, feather=0.0625, faces=faces, frame_format="nv12", colorspace=mode[0],
                                              full_range=mode[1]).int())
    # two streams of different sizes in one batch
    w.crops.clear(); w.driven.clear(); w.lib.calls.clear()
    small, wins_s, _ = Y.ragged_case(codes)
    a, b = frames[:2], Y.tensor_of(torch.cat([small[2], small[2].flip(2)]), fmt)
    wa, wb = [(10, 5, 70), (40, 30, 128)], [(141, 7, 170), (3, 1, 64)]
    streams = [dict(frames=a, windows=wa), dict(frames=b, windows=wb)]
    got = list(w.animate_streams(streams, batch_size=4, to_host=False, paste_back=True, **kw))
    assert w.lib.calls == {"emo_yuv420_crop_ragged_f32": 1, "emo_paste_ragged_yuv420": 1}
    images = torch.cat(w.driven)
    out = {(s, t): f.clone() for batch in got for s, t, f in batch}
    order = [(0, 0), (1, 0), (0, 1), (1, 1)]
    for row, (s, t) in enumerate(order):
        src, win = (a, wa) if s == 0 else (b, wb)
        want = w.paste_back(src[t:t + 1], images[row:row + 1], [win[t]], **kw)
        assert out[(s, t)].dtype == frames.dtype and torch.equal(out[(s, t)], want[0]), (s, t)
        assert torch.equal(w.crops[0][row], ops.yuv420_windows(src[t:t + 1], fmt, (Y.S, Y.S), _sq([win[t]]), *mode)[0])
    # crops out of the streams: ops.pack_yuv420 of the images
    w.crops.clear(); w.driven.clear()
    got = list(w.animate_streams(streams, batch_size=4, to_host=False, **kw))
    crops_out = torch.cat([f for batch in got for _, _, f in batch])
    assert torch.equal(crops_out, ops.pack_yuv420(torch.cat(w.driven), fmt, *mode))


def test_animate_out_format_is_the_pack_of_its_image(wrapper, monkeypatch):
    from emoportraits_amd import ops
    w = wrapper
    monkeypatch.setattr(w, "_preflight", lambda *a, **k: (None, None))
    monkeypatch.setattr(w, "_control_plans", lambda *a, **k: (None, None))
    monkeypatch.setattr(w, "_pose_controls", lambda theta, *a, **k: theta)
    monkeypatch.setattr(ops, "pose_theta", lambda s, r, t: torch.eye(4).expand(s.shape[0], 4, 4).contiguous())
    monkeypatch.setattr(w, "_render_theta", lambda theta, ident, tt: theta)
    for fmt in Y.NEW:
        w.driven.clear()
        got = torch.cat([t for _, t in w.animate(torch.zeros(5, 4), [torch.zeros(5, 3)] * 3, batch_size=4, out_format=fmt, colorspace="bt601")])
        assert got.dtype == Y.TORCH_DTYPE[fmt] and torch.equal(got, ops.pack_yuv420(torch.cat(w.driven), fmt, "bt601"))


@pytest.mark.parametrize("fmt", Y.NEW)
def test_the_argument_checks_launch_nothing(wrapper, inp, fmt):
    frames, _, _ = _frames(inp, fmt)
    w = wrapper
    rgb = torch.zeros(Y.N, Y.H, Y.W, 3, dtype=torch.uint8)
    other = torch.zeros(frames.shape, dtype=torch.uint16 if frames.dtype == torch.uint8 else torch.uint8)
    nv = dict(frame_format=fmt, windows=Y.WINDOWS)
    cases = [("3H/2", frames[:, :404], nv), ("3H/2", frames[:, :, :479], nv), ("3H/2", rgb, nv), (fmt, other, nv),
             ("stride", frames[:, :, ::2], nv),
             ("paste_back", frames, dict(nv, paste_back=True, out_format="rgb8")),
             ("paste_back", frames, dict(nv, paste_back=True, out_format="nv12")),
             ("paste_back", rgb, dict(windows=Y.WINDOWS, paste_back=True, out_format=fmt)),
             ("out_format", frames, dict(nv, to_host=False, as_uint8=False, out_format=fmt)),
             ("frame_format", frames, dict(windows=Y.WINDOWS, frame_format="i420")),
             ("out_format", frames, dict(nv, out_format="yuv")),
             ("colorspace", frames, dict(nv, colorspace="bt2020"))]
    if frames.dtype == torch.uint16:
        cases.append((r"\[N,H,W,3\]|uint8", frames, dict(windows=Y.WINDOWS)))
    for match, fr, kw in cases:
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(fr, **kw))
    with pytest.raises(ValueError, match="3H/2"):
        w.paste_back(frames[:, :404], inp["noise"][2], Y.WINDOWS, frame_format=fmt)
    with pytest.raises(ValueError, match="3H/2"):
        next(w.animate_streams([dict(frames=frames[:, :404], windows=Y.WINDOWS)], frame_format=fmt))
    w.cfg["image_size"] = Y.S - 1
    with pytest.raises(ValueError, match="even image_size"):
        next(w.animate_frames(frames, **nv))
    with pytest.raises(ValueError, match="even image_size"):
        next(w.animate_frames(rgb, windows=Y.WINDOWS, out_format=fmt))
    with pytest.raises(ValueError, match="even image_size"):
        next(w.animate(torch.zeros(2, 4), [torch.zeros(2, 3)] * 3, out_format=fmt))
    w.cfg["image_size"] = Y.S
    with pytest.raises(ValueError, match="out_format"):
        next(w.animate(torch.zeros(2, 4), [torch.zeros(2, 3)] * 3, out_format=fmt, as_uint8=False))
    assert w.lib.calls == {} and w.driven == []


def test_the_video_tool_reads_raw_files_of_every_format(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("animate_video", os.path.join(ROOT, "tools", "animate_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    codes = torch.randint(0, 1024, (5, 12, 16), generator=torch.Generator().manual_seed(0), dtype=torch.int32)
    for fmt in Y.NEW:
        clip = Y.tensor_of(codes >> (10 - Y.BITS[fmt]), fmt)
        path = str(tmp_path / f"clip_{fmt}.yuv")
        clip.numpy().tofile(path)
        assert os.path.getsize(path) == 5 * 12 * 16 * clip.element_size()
        chunks = list(tool.load_nv12(path, 16, 8, 2, fmt))
        assert [c.shape[0] for c in chunks] == [2, 2, 1] and chunks[0].dtype == clip.dtype and torch.equal(torch.cat(chunks), clip)
        with open(path, "ab") as f:
            f.write(b"\0" * 7)
        with pytest.raises(SystemExit, match="whole number"):
            next(tool.load_nv12(path, 16, 8, 2, fmt))
