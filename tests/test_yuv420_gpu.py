"""Planar and 10-bit YUV 4:2:0 frames on the GPU (ABI 22): the checks of tests/yuv420_reference.py that tests/test_yuv420_emul.py
runs on the host-compiled kernels, here on the library built for gfx950 with every surface in device memory between guard bytes
-- layout 0 against the ten NV12 entry points, yuv420p against NV12, the two 10-bit layouts against each other and against the
fp64 restatement (D 1e-6, C 1e-5, E and P within one code and 2e-3 of the touched samples), ABI 17's exact cases, faces, ragged
frames, the refusals -- and InferenceWrapper.animate_frames / paste_back / animate_streams / enrol_identities / animate in every
new format on the tiny fixture with toy embedders."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import yuv420_reference as Y  # noqa: E402

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def api():
    import ctypes
    from emoportraits_amd import hip
    hip.load()
    return Y.Api(ctypes.CDLL(hip.LIB_PATH), Y.DeviceMemory(), hip.SIGNATURES)


@pytest.fixture(scope="module")
def inp():
    return Y.inputs()


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
    Y.check_10bit_against_fp64(api, inp, fmt, kind, print)


# ---- the wrapper on the tiny fixture (the small wrapper tests/test_nv12_gpu.py builds) -----------------------------------------
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


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


def _clip(S, N, Hf, Wf, seed, bits):
    """N frames as codes and one window per frame: sides S / 2 ... min(Hf, Wf), odd and even origins, the first and last on the borders"""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 1 << bits, (N, 3 * Hf // 2, Wf), generator=g, dtype=torch.int32)
    top = min(Hf, Wf)
    wins = []
    for n in range(N):
        s = S // 2 + ((top - S // 2) * n) // max(N - 1, 1)
        x0 = 0 if n == 0 else (Wf - s if n == N - 1 else min(Wf - s, 5 * n + 1))
        y0 = 0 if n == 0 else (Hf - s if n == N - 1 else min(Hf - s, 3 * n))
        wins.append((x0, y0, s))
    return codes, wins


def _collect(gen):
    out = {}
    for b0, t in gen:
        for j in range(t.shape[0]):
            out[b0 + j] = t[j].cpu().clone()
    return torch.stack([out[i] for i in range(len(out))])


MODE = dict(colorspace="bt601", full_range=True)


@pytest.mark.parametrize("fmt", Y.NEW)
def test_animate_frames_and_paste_back_in_every_new_format(wrapper, tiny, fmt):
    """the fp32 images are the render of ops.yuv420_windows' crops; the format out is ops.pack_yuv420 of them, paste_back=True is
    paste_back() of them -- host frames through the pinned ring and device frames alike; yuv420p gives the NV12 path's samples"""
    from emoportraits_amd import ops
    w = wrapper
    S = tiny["cfg"]["image_size"]
    N, B = 10, 4
    codes, wins = _clip(S, N, S + S // 2 + 2, 2 * S + 6, 5, Y.BITS[fmt])          # (H / 2 odd: the planar V plane starts mid-row)
    frames = Y.tensor_of(codes, fmt)
    kw = dict(batch_size=B, windows=wins, frame_format=fmt, **MODE)
    w.reset_pose_state()
    rendered = _collect(w.animate_frames(frames, to_host=False, as_uint8=False, **kw))
    assert rendered.dtype == torch.float32 and tuple(rendered.shape) == (N, 3, S, S)
    crops = ops.yuv420_windows(frames[:B].to(DEV), fmt, (S, S), _sq(wins[:B]), "bt601", True)
    theta = w._head_pose(crops)[0]
    pose, _ = w._expression(crops, theta, "test")
    assert torch.equal(w._render(pose, theta, None, True, None, "f32").cpu(), rendered[:B])
    want = ops.pack_yuv420(rendered.to(DEV), fmt, "bt601", True).cpu()
    host = _collect(w.animate_frames(frames, ring=2, **kw))
    assert host.dtype == frames.dtype and tuple(host.shape) == (N, 3 * S // 2, S) and torch.equal(host, want)
    assert torch.equal(_collect(w.animate_frames(frames.to(DEV), to_host=False, out_format=fmt, **kw)), want)
    rgb = _collect(w.animate_frames(frames, ring=2, out_format="rgb8", **kw))
    assert torch.equal(rgb, ops.pack_rgb8(rendered.to(DEV)).cpu())
    if Y.BITS[fmt] == 8:                                                         # the NV12 path on the same samples
        nv12 = Y.tensor_of(codes, "nv12")
        r12 = _collect(w.animate_frames(nv12, to_host=False, as_uint8=False, **dict(kw, frame_format="nv12")))
        assert torch.equal(r12, rendered)
        assert torch.equal(Y.codes_of(want, fmt), ops.pack_nv12(rendered.to(DEV), "bt601", True).cpu().int())
    # paste_back
    before = frames.clone()
    full = w.paste_back(frames, rendered, wins, frame_format=fmt, **MODE)
    assert full.is_cuda and full.dtype == frames.dtype and tuple(full.shape) == tuple(frames.shape) and torch.equal(frames, before)
    full = full.cpu()
    touched = Y.R.touched_mask(codes.shape, wins)
    got_codes = Y.codes_of(full, fmt)
    assert torch.equal(got_codes[~touched], codes[~touched]) and not torch.equal(got_codes, codes)
    if Y.BITS[fmt] == 8:
        assert torch.equal(got_codes, w.paste_back(nv12, rendered, wins, frame_format="nv12", **MODE).cpu().int())
    host = _collect(w.animate_frames(frames, ring=2, paste_back=True, **kw))
    assert torch.equal(host, full)
    dev_frames = frames.to(DEV)
    dev = _collect(w.animate_frames(dev_frames, to_host=False, paste_back=True, **kw))
    assert torch.equal(dev, full) and torch.equal(dev_frames.cpu(), frames)
    # animate(out_format=) packs animate()'s fp32 images
    from test_identity_bank_gpu import _drivers
    pose, srt = _drivers(tiny, 6)
    f32 = _collect(w.animate(pose, srt, batch_size=4, as_uint8=False))
    assert torch.equal(_collect(w.animate(pose, srt, batch_size=4, out_format=fmt, **MODE)), ops.pack_yuv420(f32.to(DEV), fmt, "bt601", True).cpu())


@pytest.mark.parametrize("fmt", Y.NEW)
def test_faces_and_streams_in_every_new_format(wrapper, tiny, fmt):
    from emoportraits_amd import ops
    w = wrapper
    S = tiny["cfg"]["image_size"]
    bits = Y.BITS[fmt]
    ca, wa = _clip(S, 4, S + 10, S + 30, 7, bits)
    cb, wb = _clip(S, 3, 2 * S + 2, S + 2, 8, bits)
    a, b = Y.tensor_of(ca, fmt), Y.tensor_of(cb, fmt)
    kw = dict(frame_format=fmt, **MODE)
    # several faces per frame: one launch is paste_back(faces=) of the images of the same run
    faces = [[wa[0], wa[1]], [], [wa[2]], [wa[3], wa[1], wa[0]]]
    ids = [0, 1, 0, 1, 0, 1]
    w.reset_pose_state()
    rendered = _collect(w.animate_frames(a, batch_size=4, faces=faces, identities=ids, to_host=False, as_uint8=False, **kw))
    assert tuple(rendered.shape) == (6, 3, S, S)
    got = _collect(w.animate_frames(a, batch_size=4, faces=faces, identities=ids, ring=2, paste_back=True, **kw))
    want = w.paste_back(a, rendered, faces=faces, frame_format=fmt, **MODE).cpu()
    assert got.dtype == a.dtype and torch.equal(got, want) and torch.equal(got[1], a[1]) and not torch.equal(got[0], a[0])
    # two streams of different sizes in one batch, through the pinned arena ring and on the device
    streams = [dict(frames=a, windows=wa, identities=0), dict(frames=b, windows=wb, identities=1)]
    crops = {}
    for batch in w.animate_streams(streams, batch_size=4, to_host=False, as_uint8=False, **kw):
        for s, t, f in batch:
            crops[(s, t)] = f.clone()
    for to_host in (True, False):
        n = 0
        for batch in w.animate_streams(streams, batch_size=4, to_host=to_host, ring=2, paste_back=True, **kw):
            for s, t, f in batch:
                src, win = (a, wa) if s == 0 else (b, wb)
                want = w.paste_back(src[t:t + 1], crops[(s, t)], [win[t]], frame_format=fmt, **MODE)
                assert f.dtype == a.dtype and torch.equal(f.cpu(), want[0].cpu()), (s, t)
                n += 1
        assert n == 7
    out = [f for batch in w.animate_streams(streams, batch_size=4, to_host=False, **kw) for _, _, f in batch]
    order = [(s, t) for t in range(4) for s in (0, 1) if t < (4, 3)[s]]
    want = ops.pack_yuv420(torch.cat([crops[k] for k in order]), fmt, "bt601", True)
    assert torch.equal(torch.cat(out), want)


@pytest.mark.parametrize("fmt", Y.NEW)
def test_enrol_identities_from_frames_is_enrolment_from_their_crops(project, tiny, fmt):
    from emoportraits_amd import ops
    from test_identity_bank_gpu import _wrapper
    S = tiny["cfg"]["image_size"]
    codes, wins = _clip(S, 3, S + 10, S + 30, 11, Y.BITS[fmt])
    frames = Y.tensor_of(codes, fmt)
    masks = torch.ones(3, 1, S, S)
    custom = dict(custome_idt_embed=tiny["idt_embed"].expand(3, *tiny["idt_embed"].shape[1:]).contiguous(),
                  custome_source_pose_embed=tiny["source_pose_embed"].expand(3, -1).contiguous(),
                  custome_source_theta_embed=tiny["theta_src"].reshape(1, 4, 4).expand(3, 4, 4).contiguous())
    banks = []
    for from_frames in (True, False):
        w = _wrapper(project, tiny, use_graphs=False, identity_capacity=3)
        if from_frames:
            slots = w.enrol_identities(frames, source_masks=masks, windows=wins, frame_format=fmt, **MODE, **custom)
        else:
            crops = ops.yuv420_windows(frames.to(DEV), fmt, (S, S), _sq(wins), "bt601", True)
            slots = w.enrol_identities(crops.cpu(), source_masks=masks, **custom)
        assert slots == [0, 1, 2]
        banks.append(w._bank_cl.clone())
    assert torch.equal(banks[0], banks[1]) and bool(banks[0].any())
    with pytest.raises(ValueError, match="3H/2"):
        w.enrol_identities(frames[:, :, :-1], source_masks=masks, windows=wins, frame_format=fmt, **custom)


def test_every_value_error_is_raised_before_the_first_launch(wrapper, tiny, guarded_outputs):
    guarded_outputs.may_serve_nothing("only argument errors are provoked, each before anything is allocated or launched")
    w = wrapper
    S = tiny["cfg"]["image_size"]
    for fmt in Y.NEW:
        codes, wins = _clip(S, 4, S + 10, S + 30, 3, Y.BITS[fmt])
        frames = Y.tensor_of(codes, fmt)
        other = torch.zeros(frames.shape, dtype=torch.uint16 if frames.dtype == torch.uint8 else torch.uint8)
        nv = dict(frame_format=fmt, windows=wins)
        for match, fr, kw in (("3H/2", frames[:, :-1], nv), ("3H/2", frames[:, :, :-1], nv), (fmt, other, nv), ("stride", frames[:, :, :4 * (frames.shape[2] // 4):2], nv),
                              ("paste_back", frames, dict(nv, paste_back=True, out_format="rgb8")),
                              ("out_format", frames, dict(nv, to_host=False, as_uint8=False, out_format=fmt)),
                              ("frame_format", frames, dict(windows=wins, frame_format="i420")),
                              ("out_format", frames, dict(nv, out_format="yuv")),
                              ("colorspace", frames, dict(nv, colorspace="bt2020"))):
            with pytest.raises(ValueError, match=match):
                next(w.animate_frames(fr, **kw))
        size = w.cfg["image_size"]
        w.cfg["image_size"] = size - 1
        try:
            with pytest.raises(ValueError, match="even image_size"):
                next(w.animate_frames(frames, **nv))
        finally:
            w.cfg["image_size"] = size
