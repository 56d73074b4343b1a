"""NV12 frames in and out on the GPU (ABI 17): ops.nv12_windows, ops.pack_nv12 and ops.paste_windows_nv12 on the cases of
tests/test_nv12_emul.py -- against the definitions restated in torch and evaluated in fp64 on the CPU (tests/nv12_reference.py: D
within 1e-6, C within 1e-5, E and P every byte within 1 and at most 2e-3 of the touched bytes different at all), the exact cases,
guard bytes around padded surfaces, the refusals -- and InferenceWrapper.animate_frames / animate / paste_back / enrol_identities
with frame_format / out_format 'nv12' on the tiny fixture with toy embedders: the fp32 images are the render of
ops.nv12_windows' crops, NV12 out is ops.pack_nv12 of them, paste_back=True is paste_back() of them, and the rgb8 path of the same
run still yields ops.pack_rgb8 of the same images."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import nv12_reference as R  # noqa: E402
import yuv420_reference as Y  # noqa: E402

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"
FILL = Y.FILL
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def small():
    return R.small_inputs()


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


class Surface(Y.Surface):
    """N NV12 frames on the device between GUARD bytes, rows `pitch` apart, all padding = FILL (yuv420_reference.Surface, layout
    nv12, device memory); .view is the [N, rows, W] view the ops take"""

    def __init__(self, n, rows, w, pitch=None, frames=None):
        super().__init__(Y.DeviceMemory(), "nv12", n, rows // 3 * 2, w, pad=(pitch or w) - w, arr=None if frames is None else frames.numpy())
        self.view = self.dev[Y.GUARD:Y.GUARD + n * self.fstride].view(n, rows, self.pitch_y)[:, :, :w]

    def padding_intact(self):
        return self.read()[1]


def _crop(nv12, wins, size, mode, pitch=None, device_table=False):
    from emoportraits_amd import ops
    s = Surface(*nv12.shape, pitch, nv12)
    w = None if wins is None else (torch.tensor(_sq(wins), dtype=torch.int32, device=DEV) if device_table else _sq(wins))
    out = ops.nv12_windows(s.view, size, w, *mode).cpu()
    assert s.padding_intact() and torch.equal(s.view.cpu(), nv12)
    return out


def _pack(img, mode, pitch=None):
    from emoportraits_amd import ops
    n, _, h, w = img.shape
    s = Surface(n, 3 * h // 2, w, pitch)
    assert ops.pack_nv12(img.to(DEV), *mode, out=s.view) is s.view
    assert s.padding_intact()
    return s.view.cpu()


def _paste(nv12, img, wins, feather=0.0, matte=None, mode=R.MODES[0], pitch=None, device_table=False):
    from emoportraits_amd import ops
    s = Surface(*nv12.shape, pitch, nv12)
    w = torch.tensor(_sq(wins), dtype=torch.int32, device=DEV) if device_table else _sq(wins)
    assert ops.paste_windows_nv12(s.view, img.to(DEV), w, feather, None if matte is None else matte.to(DEV), *mode) is s.view
    assert s.padding_intact()
    return s.view.cpu()


def _untouched_equal(got, nv12, wins):
    keep = ~R.touched_mask(nv12.shape, wins)
    return torch.equal(got[keep], nv12[keep])


# ---- the kernels against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_decode_against_the_fp64_restatement(small, kind, mode):
    nv12 = small[kind][0]
    got = _crop(nv12, None, None, mode, pitch=R.W + 32 if kind == "noise" else None)
    ref = R.decode(nv12, *mode, F64)
    err, err32 = (got.double() - ref).abs().max().item(), (R.decode(nv12, *mode, F32).double() - ref).abs().max().item()
    print(f"PARITY nv12 D {kind} {mode[0]} full_range {mode[1]}: max abs err {err:.2e} (torch fp32 against fp64: {err32:.2e})")
    assert err32 <= R.D_TOL
    assert err <= R.D_TOL
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_crop_against_the_fp64_restatement(small, kind, which):
    nv12 = small[kind][0]
    wins = (R.WINDOWS, R.WINDOWS_ODD)[which]
    for mode in R.MODES[which::2]:
        got = _crop(nv12, wins, (R.S, R.S), mode)
        ref = R.crop(nv12, wins, R.S, *mode, F64)
        err, err32 = (got.double() - ref).abs().max().item(), (R.crop(nv12, wins, R.S, *mode, F32).double() - ref).abs().max().item()
        print(f"PARITY nv12 C {kind} windows {which} {mode[0]} full_range {mode[1]}: max abs err {err:.2e} "
              f"(torch fp32 against fp64: {err32:.2e})")
        assert err32 <= R.C_TOL
        assert err <= R.C_TOL


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_pack_against_the_fp64_restatement(small, kind, mode):
    img = small[kind][1]
    for im, pitch in ((img, None), (img[:2, :, :6, :10].contiguous(), 13), (img[:, :, 1:127, :126].contiguous(), 200)):
        got = _pack(im, mode, pitch)
        worst, share, share32 = R.compare_bytes(got, R.encode(im.double(), *mode, F64), R.encode(im, *mode, F32), got.numel())
        print(f"PARITY nv12 E {kind} {tuple(im.shape[-2:])} {mode[0]} full_range {mode[1]}: max byte diff {worst}, share of bytes "
              f"that differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
        assert share32 <= R.MAX_SHARE
        assert worst <= R.MAX_BYTE_DIFF
        assert share <= R.MAX_SHARE


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("case", range(len(R.CASES)))
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_paste_against_the_fp64_restatement(small, kind, case, which):
    nv12, img, matte = small[kind]
    feather, use_matte = R.CASES[case]
    wins = (R.WINDOWS, R.WINDOWS_ODD)[which]
    mode = R.MODES[(case + which) % 4]
    m = matte if use_matte else None
    got = _paste(nv12, img, wins, feather, m, mode)
    worst, share, share32 = R.compare_paste(got, nv12, img, wins, feather, m, *mode)
    print(f"PARITY nv12 P {kind} windows {which} feather {feather} matte {use_matte} {mode[0]} full_range {mode[1]}: max byte diff "
          f"{worst}, share of touched bytes that differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
    assert share32 <= R.MAX_SHARE
    assert worst <= R.MAX_BYTE_DIFF
    assert share <= R.MAX_SHARE
    assert _untouched_equal(got, nv12, wins)


# ---- exact cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_the_fused_crop_is_conversion_then_resize_windows_bit_for_bit(small, which):
    from emoportraits_amd import ops
    nv12 = small["noise"][0]
    wins = (R.WINDOWS, R.WINDOWS_ODD)[which]
    mode = R.MODES[which + 1]
    rgb = ops.nv12_windows(nv12.to(DEV), None, None, *mode)
    want = ops.resize2d_windows(rgb, (R.S, R.S), _sq(wins), "bicubic", clamp01=True).cpu()
    assert torch.equal(_crop(nv12, wins, (R.S, R.S), mode), want)
    # the window table on the device only; a padded surface; every frame on its own
    assert torch.equal(_crop(nv12, wins, (R.S, R.S), mode, pitch=R.W + 2, device_table=True), want)
    for n in range(R.N):
        assert torch.equal(_crop(nv12[n:n + 1], wins[n:n + 1], (R.S, R.S), mode)[0], want[n]), n
    # a non-square output and window, and the whole frame resized (no table)
    rect = [(x0, y0, s, max(2, s // 2)) for x0, y0, s in wins]
    want = ops.resize2d_windows(rgb, (40, 72), rect, "bicubic", clamp01=True)
    assert torch.equal(ops.nv12_windows(nv12.to(DEV), (40, 72), rect, *mode), want)
    want = ops.resize2d(rgb, (40, 72), "bicubic", clamp01=True)
    assert torch.equal(ops.nv12_windows(nv12.to(DEV), (40, 72), None, *mode), want)
    # a device-side window that leaves the frame: zeros for its frame
    bad = torch.tensor(_sq([wins[0], (411, 5, 70), (0, 0, 271), (300, 100, 0), (-1, 1, 180), (352, 143, 128)]), dtype=torch.int32, device=DEV)
    got = ops.nv12_windows(nv12.to(DEV), (R.S, R.S), bad, *mode).cpu()
    assert torch.equal(got[0], _crop(nv12, wins, (R.S, R.S), mode)[0]) and not got[1:].any()


@pytest.mark.parametrize("mode", R.MODES)
def test_achromatic_frames_survive_decode_and_pack(mode):
    from emoportraits_amd import ops
    nv12 = R.achromatic(mode[1])
    rgb = ops.nv12_windows(nv12.to(DEV), None, None, *mode)
    assert torch.equal(rgb[:, 0], rgb[:, 1]) and torch.equal(rgb[:, 0], rgb[:, 2])
    assert torch.equal(ops.pack_nv12(rgb, *mode).cpu(), nv12)


@pytest.mark.parametrize("mode", R.MODES)
def test_paste_exact_cases(small, mode):
    nv12, img, matte = small["noise"]
    # side == S on an even origin without feather: emo_pack_nv12's bytes
    wins = [(0, 0, R.S), (2, 142, R.S), (352, 0, R.S), (350, 142, R.S), (100, 70, R.S), (352, 142, R.S)]
    want = _pack(img, mode)
    for device_table in (False, True):
        got = _paste(nv12, img, wins, 0.0, None, mode, pitch=R.W + 6, device_table=device_table)
        for n, (x0, y0, s) in enumerate(wins):
            assert torch.equal(got[n, y0:y0 + s, x0:x0 + s], want[n, :s]), n
            assert torch.equal(got[n, R.H + y0 // 2:R.H + (y0 + s) // 2, x0:x0 + s], want[n, s:]), n
        assert _untouched_equal(got, nv12, wins)
    # a matte of zeros changes nothing, a matte of ones is no matte
    for wins in (R.WINDOWS, R.WINDOWS_ODD):
        for feather in (0.0, 0.0625):
            assert torch.equal(_paste(nv12, img, wins, feather, torch.zeros(R.N, 1, R.S, R.S), mode), nv12)
            none = _paste(nv12, img, wins, feather, None, mode)
            assert torch.equal(_paste(nv12, img, wins, feather, torch.ones(R.N, 1, R.S, R.S), mode), none) and not torch.equal(none, nv12)


@pytest.mark.parametrize("feather,use_matte", R.CASES)
def test_no_byte_outside_the_touched_rectangles_changes(small, feather, use_matte):
    nv12, img, matte = small["noise"]
    edge = [(0, 0, 33), (R.W - 34, 0, 34), (0, R.H - 35, 35), (R.W - 36, R.H - 36, 36), (1, 1, 129), (2, 3, 131)]
    for i, wins in enumerate((R.WINDOWS, R.WINDOWS_ODD, edge)):
        got = _paste(nv12, img, wins, feather, matte if use_matte else None, R.MODES[i], pitch=R.W + 10 * i)
        assert _untouched_equal(got, nv12, wins)
        touched = R.touched_mask(nv12.shape, wins)
        assert int((got != nv12)[touched].sum()) > 0.5 * int(touched.sum()) * (0.2 if use_matte else 1.0)


def test_a_pasted_frame_does_not_depend_on_its_batch_and_bad_device_windows_are_skipped(small):
    from emoportraits_amd import ops
    nv12, img, matte = small["smooth"]
    mode = R.MODES[2]
    for wins in (R.WINDOWS, R.WINDOWS_ODD):
        whole = _paste(nv12, img, wins, 0.0625, matte, mode)
        for n in range(R.N):
            assert torch.equal(_paste(nv12[n:n + 1], img[n:n + 1], wins[n:n + 1], 0.0625, matte[n:n + 1], mode)[0], whole[n]), n
        assert torch.equal(_paste(nv12, img, wins, 0.0625, matte, mode, device_table=True), whole)
    whole = _paste(nv12, img, R.WINDOWS, 0.0625, matte, mode)
    bad = torch.tensor([(10, 5, 70, 71), (411, 5, 70, 70), (0, 0, 270, 270), (300, 100, 31, 31), (-1, 1, 180, 180), (352, 143, 128, 128)],
                       dtype=torch.int32, device=DEV)
    got = ops.paste_windows_nv12(nv12.to(DEV), img.to(DEV), bad, 0.0625, matte.to(DEV), *mode).cpu()
    for n in range(R.N):
        assert torch.equal(got[n], whole[n] if n == 2 else nv12[n]), n


def test_refusals_write_nothing(small):
    from emoportraits_amd import ops
    nv12, img, _ = small["noise"]
    work, im = nv12.to(DEV), img.to(DEV)
    sq = _sq(R.WINDOWS)
    for bad, msg in ((sq[:5], "windows for"), (sq[:5] + [(352, 142, 128, 127)], "square"), (sq[:5] + [(353, 142, 128, 128)], "inside"),
                     (sq[:5] + [(352, 142, 31, 31)], "quarter")):
        with pytest.raises(ValueError, match=msg):
            ops.paste_windows_nv12(work, im, bad)
    with pytest.raises(ValueError, match="feather"):
        ops.paste_windows_nv12(work, im, sq, feather=0.6)
    with pytest.raises(ValueError, match="colorspace"):
        ops.paste_windows_nv12(work, im, sq, colorspace="bt2020")
    with pytest.raises(ValueError, match="inside"):
        ops.nv12_windows(work, (R.S, R.S), sq[:5] + [(353, 142, 128, 128)])
    with pytest.raises(ValueError, match="even"):
        ops.pack_nv12(im[:, :, :127].contiguous())
    with pytest.raises(ValueError, match="even"):
        ops.nv12_windows(work[:, :, :479], (R.S, R.S), sq)
    with pytest.raises(ValueError, match="3H/2"):
        ops.nv12_windows(work[:, :404], (R.S, R.S), sq)
    with pytest.raises(ValueError, match="pitch"):
        ops.nv12_windows(work[:, :, ::2], (R.S, R.S), sq)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.nv12_windows(nv12, (R.S, R.S), sq)
    with pytest.raises(RuntimeError, match="device"):
        ops.paste_windows_nv12(nv12, im, sq)
    assert torch.equal(work.cpu(), nv12)
    # the C ABI itself: codes, nothing written
    import ctypes
    from emoportraits_amd import hip
    lib = hip.load()
    out = torch.full((R.N, 3, R.S, R.S), -7.0, device=DEV)
    win = torch.tensor(sq, dtype=torch.int32)
    wd = win.to(DEV)
    y, uv = ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(work.data_ptr() + R.H * R.W)
    fs = 3 * R.H * R.W // 2
    st = hip.current_stream()
    ok = [y, uv, R.W, fs, R.H, R.W, hip.ptr(wd), hip.ptr(win), hip.ptr(out), R.N, R.S, R.S, 0, 0, st]
    for k, v in {0: None, 1: None, 2: R.W - 2, 4: R.H - 1, 5: R.W - 1, 8: None, 9: 0, 12: 2}.items():
        a = list(ok)
        a[k] = v
        assert lib.emo_nv12_windows_f32(*a) == -1, k
    ok = [hip.ptr(im), None, hip.ptr(wd), hip.ptr(win), y, uv, R.W, fs, R.N, R.S, R.H, R.W, 0.0, 0, 0, st]
    for k, v in {0: None, 2: None, 4: None, 5: None, 6: R.W - 2, 10: R.H - 1, 11: R.W - 1, 12: 0.75, 13: -1}.items():
        a = list(ok)
        a[k] = v
        assert lib.emo_paste_windows_nv12(*a) == -1, k
    ok = [hip.ptr(im), y, uv, R.W, fs, R.N, R.S, R.S, 0, 0, st]
    for k, v in {0: None, 1: None, 2: None, 3: R.S - 2, 6: R.S - 1, 7: R.S - 1, 8: 7}.items():
        a = list(ok)
        a[k] = v
        assert lib.emo_pack_nv12(*a) == -1, k
    torch.cuda.synchronize()
    assert torch.equal(work.cpu(), nv12) and bool((out == -7.0).all())


# ---- the wrapper -----------------------------------------------------------------------------------------------------------
def matting(img):
    """deterministic toy matte, per pixel: exact 0, exact 1 and fractions"""
    return (img.mean(1, keepdim=True) * 1.6 - 0.3).clamp(0, 1)


def face_parsing(img):
    return (img[:, 1:2] > 0.35).float()


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


@pytest.fixture(scope="module")
def project(tmp_path_factory, tiny, golden_dir):
    """the tiny stage-1 project of tests/test_paste_back_gpu.py plus logs_s2/exp2 with the tiny stage-2 model"""
    from emoportraits_amd import config
    tiny2 = torch.load(os.path.join(golden_dir, "tiny_stage2.pt"), weights_only=False)
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


@pytest.fixture(scope="module")
def wrapper(project, tiny):
    from test_identity_bank_gpu import _enrol, _sources, _wrapper
    w = _wrapper(project, tiny, use_graphs=False, identity_capacity=2)
    assert _enrol(w, tiny, _sources(tiny, 2)) == [0, 1]
    w.load_identity(0)
    return w


def _clip(S, N, Hf, Wf, seed):
    """N NV12 frames and one window per frame: sides S / 2 ... min(Hf, Wf), odd and even origins, the first and last on the borders"""
    g = torch.Generator().manual_seed(seed)
    nv12 = torch.randint(0, 256, (N, 3 * Hf // 2, Wf), generator=g, dtype=torch.uint8)
    top = min(Hf, Wf)
    wins = []
    for n in range(N):
        s = S // 2 + ((top - S // 2) * n) // max(N - 1, 1)
        x0 = 0 if n == 0 else (Wf - s if n == N - 1 else min(Wf - s, 5 * n + 1))
        y0 = 0 if n == 0 else (Hf - s if n == N - 1 else min(Hf - s, 3 * n))
        wins.append((x0, y0, s))
    return nv12, wins


def _collect(gen):
    out = {}
    for b0, t in gen:
        for j in range(t.shape[0]):
            out[b0 + j] = t[j].cpu().clone()
    return torch.stack([out[i] for i in range(len(out))])


MODE = dict(colorspace="bt601", full_range=True)


def test_the_fp32_images_are_the_render_of_nv12_windows_crops_and_both_outputs_pack_them(wrapper, tiny):
    from emoportraits_amd import ops
    w = wrapper
    S = tiny["cfg"]["image_size"]
    N, B = 10, 4
    nv12, wins = _clip(S, N, S + S // 2 + 4, 2 * S + 6, seed=5)
    kw = dict(batch_size=B, windows=wins, frame_format="nv12", **MODE)
    rendered = _collect(w.animate_frames(nv12, to_host=False, as_uint8=False, **kw))
    assert rendered.dtype == torch.float32 and tuple(rendered.shape) == (N, 3, S, S)
    # by hand: the crops of ops.nv12_windows through the same networks
    for b0 in range(0, N, B):
        crops = ops.nv12_windows(nv12[b0:b0 + B].to(DEV), (S, S), _sq(wins[b0:b0 + B]), "bt601", True)
        theta = w._head_pose(crops)[0]
        pose, _ = w._expression(crops, theta, "test")
        img = w._render(pose, theta, None, True, None, "f32")
        assert torch.equal(img.cpu(), rendered[b0:b0 + B]), b0
    # NV12 out (the default for NV12 in) through the pinned ring with a short last batch, and on the device
    want = ops.pack_nv12(rendered.to(DEV), "bt601", True).cpu()
    host = _collect(w.animate_frames(nv12, ring=2, **kw))
    assert host.dtype == torch.uint8 and tuple(host.shape) == (N, 3 * S // 2, S) and torch.equal(host, want)
    assert torch.equal(_collect(w.animate_frames(nv12.to(DEV), to_host=False, out_format="nv12", **kw)), want)
    # a padded device surface is taken as it is
    padded = torch.full((N, nv12.shape[1], nv12.shape[2] + 26), FILL, dtype=torch.uint8, device=DEV)
    padded[:, :, :nv12.shape[2]] = nv12.to(DEV)
    assert torch.equal(_collect(w.animate_frames(padded[:, :, :nv12.shape[2]], to_host=False, **kw)), want)
    # the rgb8 output of the same run is ops.pack_rgb8 of the same images
    rgb = _collect(w.animate_frames(nv12, ring=2, out_format="rgb8", **kw))
    assert tuple(rgb.shape) == (N, S, S, 3) and torch.equal(rgb, ops.pack_rgb8(rendered.to(DEV)).cpu())
    # rgb8 frames in, NV12 crops out: ops.pack_nv12 of that run's images; and the rgb8 path itself is what it was
    frames = torch.randint(0, 256, (N, S + 9, S + 31, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    kw8 = dict(batch_size=B, windows=[(x // 2, y // 2, s // 2 + 8) for x, y, s in wins])
    r8 = _collect(w.animate_frames(frames, to_host=False, as_uint8=False, **kw8))
    assert torch.equal(_collect(w.animate_frames(frames, ring=2, out_format="nv12", **kw8)), ops.pack_nv12(r8.to(DEV)).cpu())
    assert torch.equal(_collect(w.animate_frames(frames, ring=2, **kw8)), ops.pack_rgb8(r8.to(DEV)).cpu())
    # animate(out_format='nv12') packs animate()'s fp32 images
    from test_identity_bank_gpu import _drivers
    pose, srt = _drivers(tiny, 6)
    f32 = _collect(w.animate(pose, srt, batch_size=4, as_uint8=False))
    assert torch.equal(_collect(w.animate(pose, srt, batch_size=4, out_format="nv12", **MODE)), ops.pack_nv12(f32.to(DEV), "bt601", True).cpu())


@pytest.mark.parametrize("mode", ["plain", "smooth_pose", "identities", "matte"])
def test_animate_frames_nv12_paste_back_equals_paste_back_of_the_rendered_images(wrapper, tiny, mode):
    """animate_frames(frame_format='nv12', paste_back=True) = paste_back(frames, the fp32 images of the same run without it,
    windows, frame_format='nv12'), bit for bit; host frames through the pinned ring (ring=2, a short last batch) and
    device-resident frames give the same bytes, and the caller's tensors are not modified"""
    w = wrapper
    S = tiny["cfg"]["image_size"]
    N, B = 10, 4
    nv12, wins = _clip(S, N, S + S // 2 + 4, 2 * S + 6, seed=5)
    kw = dict(frame_format="nv12", **MODE)
    matte = None
    if mode == "smooth_pose":
        kw.update(smooth_pose=True)
    elif mode == "identities":
        kw.update(identities=[(3 * i + i // 4) % 2 for i in range(N)], smooth_pose=True, smooth_per_identity=True, mix=True)
    elif mode == "matte":
        matte = lambda img: img.mean(dim=1, keepdim=True).clamp(0, 1)
    w.reset_pose_state()
    rendered = _collect(w.animate_frames(nv12, batch_size=B, windows=wins, to_host=False, as_uint8=False, **kw))
    before = nv12.clone()
    want = w.paste_back(nv12, rendered, wins, matte=matte, frame_format="nv12", **MODE)
    assert want.is_cuda and want.dtype == torch.uint8 and tuple(want.shape) == tuple(nv12.shape) and torch.equal(nv12, before)
    want = want.cpu()
    assert _untouched_equal(want, nv12, wins) and not torch.equal(want, nv12)
    paste = dict(paste_back=True, paste_matte=matte)
    w.reset_pose_state()
    host = _collect(w.animate_frames(nv12, batch_size=B, windows=wins, ring=2, **kw, **paste))
    assert torch.equal(host, want)
    dev_frames = nv12.to(DEV)
    w.reset_pose_state()
    dev = _collect(w.animate_frames(dev_frames, batch_size=B, windows=wins, to_host=False, **kw, **paste))
    assert torch.equal(dev, want) and torch.equal(dev_frames.cpu(), nv12)
    w.reset_pose_state()
    dev_ring = _collect(w.animate_frames(dev_frames, batch_size=B, windows=wins, ring=2, **kw, **paste))
    assert torch.equal(dev_ring, want) and torch.equal(dev_frames.cpu(), nv12)
    again = w.paste_back(dev_frames, rendered.to(DEV), wins, matte=matte, frame_format="nv12", **MODE)
    assert torch.equal(again.cpu(), want) and torch.equal(dev_frames.cpu(), nv12)


def test_chunks_of_two_frame_sizes_get_a_new_ring(wrapper, tiny):
    w = wrapper
    S = tiny["cfg"]["image_size"]
    a, wa = _clip(S, 5, S + 10, S + 30, seed=7)
    b, wb = _clip(S, 6, 2 * S, S + 2, seed=8)
    kw = dict(batch_size=4, windows=wa + wb, frame_format="nv12")
    w.reset_pose_state()
    rendered = _collect(w.animate_frames([a, b], to_host=False, as_uint8=False, **kw))
    got = {}
    for b0, full in w.animate_frames([a, b], ring=2, paste_back=True, feather=0.25, **kw):
        got[b0] = full.clone()
    assert sorted(got) == [0, 4, 5, 9]
    assert torch.equal(torch.cat([got[0], got[4]]), w.paste_back(a, rendered[:5], wa, feather=0.25, frame_format="nv12").cpu())
    assert torch.equal(torch.cat([got[5], got[9]]), w.paste_back(b, rendered[5:], wb, feather=0.25, frame_format="nv12").cpu())


def test_refine_packs_and_pastes_the_refined_image(project, tiny):
    from emoportraits_amd import ops
    from notebooks.infer_s2 import InferenceWrapper as Stage2Wrapper
    from test_identity_bank_gpu import _wrapper
    w = _wrapper(project, tiny, use_graphs=True)
    S = tiny["cfg"]["image_size"]
    w.forward(source_image=tiny["img"], crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=tiny["idt_embed"],
              custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=tiny["theta_src"])
    w.attach_stage2(Stage2Wrapper(experiment_name="exp2", model_file_name="m.pth", project_dir=str(project),
                                  embedders={"matting": matting, "face_parsing": face_parsing}))
    N, B = 6, 4
    nv12, wins = _clip(S, N, S + S // 2 + 4, 2 * S + 6, seed=9)
    kw = dict(batch_size=B, windows=wins, to_host=False, refine=True, frame_format="nv12")
    refined = _collect(w.animate_frames(nv12, as_uint8=False, **kw))
    plain = _collect(w.animate_frames(nv12, batch_size=B, windows=wins, to_host=False, as_uint8=False, frame_format="nv12"))
    assert not torch.equal(refined, plain)
    assert torch.equal(_collect(w.animate_frames(nv12, **kw)), ops.pack_nv12(refined.to(DEV)).cpu())
    full = _collect(w.animate_frames(nv12, paste_back=True, **kw))
    assert torch.equal(full, w.paste_back(nv12, refined, wins, frame_format="nv12").cpu())


def test_enrol_identities_from_nv12_frames_is_enrolment_from_their_crops(project, tiny):
    from emoportraits_amd import ops
    from test_identity_bank_gpu import _wrapper
    S = tiny["cfg"]["image_size"]
    nv12, wins = _clip(S, 3, S + 10, S + 30, seed=11)
    masks = torch.ones(3, 1, S, S)
    custom = dict(custome_idt_embed=tiny["idt_embed"].expand(3, *tiny["idt_embed"].shape[1:]).contiguous(),
                  custome_source_pose_embed=tiny["source_pose_embed"].expand(3, -1).contiguous(),
                  custome_source_theta_embed=tiny["theta_src"].reshape(1, 4, 4).expand(3, 4, 4).contiguous())
    banks = []
    for from_frames in (True, False):
        w = _wrapper(project, tiny, use_graphs=False, identity_capacity=3)
        if from_frames:
            slots = w.enrol_identities(nv12, source_masks=masks, windows=wins, frame_format="nv12", **MODE, **custom)
        else:
            crops = ops.nv12_windows(nv12.to(DEV), (S, S), _sq(wins), "bt601", True)
            slots = w.enrol_identities(crops.cpu(), source_masks=masks, **custom)
        assert slots == [0, 1, 2]
        banks.append(w._bank_cl.clone())
    assert torch.equal(banks[0], banks[1]) and bool(banks[0].any())
    with pytest.raises(ValueError, match="3H/2"):
        w.enrol_identities(nv12[:, :, :-1], source_masks=masks, windows=wins, frame_format="nv12", **custom)


def test_every_value_error_is_raised_before_the_first_launch(wrapper, tiny, guarded_outputs):
    guarded_outputs.may_serve_nothing("only argument errors are provoked, each before anything is allocated or launched")
    w = wrapper
    S = tiny["cfg"]["image_size"]
    nv12, wins = _clip(S, 4, S + 10, S + 30, seed=3)
    rgb = torch.zeros(4, S + 10, S + 30, 3, dtype=torch.uint8)
    nv = dict(frame_format="nv12", windows=wins)
    for match, frames, kw in (("3H/2", nv12[:, :-1], nv), ("3H/2", nv12[:, :, :-1], nv), ("3H/2", rgb, nv),
                              (r"\[N,H,W,3\]", nv12, dict(windows=wins)),
                              ("paste_back", nv12, dict(nv, paste_back=True, out_format="rgb8")),
                              ("paste_back", rgb, dict(windows=wins, paste_back=True, out_format="nv12")),
                              ("out_format", nv12, dict(nv, to_host=False, as_uint8=False, out_format="nv12")),
                              ("frame_format", nv12, dict(windows=wins, frame_format="i420")),
                              ("out_format", nv12, dict(nv, out_format="yuv")),
                              ("colorspace", nv12, dict(nv, colorspace="bt2020"))):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(frames, **kw))
    size = w.cfg["image_size"]
    w.cfg["image_size"] = size - 1
    try:
        with pytest.raises(ValueError, match="even image_size"):
            next(w.animate_frames(nv12, **nv))
        with pytest.raises(ValueError, match="even image_size"):
            next(w.animate_frames(rgb, windows=wins, out_format="nv12"))
    finally:
        w.cfg["image_size"] = size
