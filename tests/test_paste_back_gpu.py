"""Rendered crops pasted back into the full driver frames, on the GPU: ops.paste_windows (emo_paste_windows_rgb8, ABI 15) against
the definition restated in torch and evaluated in fp64 on the CPU (tests/paste_back_reference.py: every byte within 1, at most
2e-3 of the window bytes different at all) on the inputs of the CPU test and on one production-sized batch (16 frames of
1080 x 1920, S = 512, sides 300 ... 900); the exact cases of tests/test_paste_back_emul.py; and
InferenceWrapper.animate_frames(paste_back=True) against paste_back() of the same run's fp32 images -- host and device frames,
a short last batch, ring=2, smooth_pose, identities, a matte, chunks of two frame sizes.  Tiny fixture, toy embedders."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import paste_back_reference as R  # noqa: E402

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def small():
    return R.small_inputs()


def _sq(wins):
    return [(x, y, s, s) for x, y, s in wins]


def _paste(frames, img, wins, feather=0.0, matte=None):
    from emoportraits_amd import ops
    work = ops.torch.empty_like(frames, device=DEV).copy_(frames)       # (ops.torch: pasted into between the guards of this module's tests)
    out = ops.paste_windows(work, img.to(DEV), _sq(wins), feather, None if matte is None else matte.to(DEV))
    assert out is work
    return out.cpu()


def _outside_equal(got, frames, wins):
    mask = torch.ones(frames.shape[:3], dtype=torch.bool)
    for n, w in enumerate(wins):
        mask[n, w[1]:w[1] + w[2], w[0]:w[0] + w[2]] = False
    return torch.equal(got[mask], frames[mask])


def _check(got, frames, img, wins, feather, matte, what):
    worst, share, share32 = R.compare(got, frames, img, wins, feather, matte)
    print(f"PARITY paste {what} feather {feather} matte {matte is not None}: max byte diff {worst}, share of window bytes that "
          f"differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
    assert worst <= R.MAX_BYTE_DIFF
    assert share <= R.MAX_SHARE
    assert _outside_equal(got, frames, wins)
    return share32


# ---- the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather,use_matte", R.CASES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_paste_windows_against_the_fp64_restatement(small, kind, feather, use_matte):
    frames, img, matte = small[kind]
    m = matte if use_matte else None
    share32 = _check(_paste(frames, img, R.WINDOWS, feather, m), frames, img, R.WINDOWS, feather, m, kind)
    assert share32 <= R.MAX_SHARE


def test_paste_windows_production_size():
    """16 frames of 1080 x 1920, S = 512, sides 300 ... 900 (a third of them downscale: antialiased), feather 1/16 and a matte.
    torch's own fp32 noise on this case must stay under a quarter of the cap, so that the kernel keeps its headroom."""
    frames, img, matte, wins = R.production_inputs()
    assert min(w[2] for w in wins) == 300 and max(w[2] for w in wins) == 900
    share32 = _check(_paste(frames, img, wins, 0.0625, matte), frames, img, wins, 0.0625, matte, "1080p")
    assert share32 <= 5e-4


def test_exact_cases(small):
    from emoportraits_amd import ops
    frames, img, matte = small["noise"]
    S = img.shape[-1]
    Hf, Wf = frames.shape[1:3]
    # side == S without feather: emo_pack_rgb8's bytes; x0 % 4 = 0 .. 3 and all four borders, frames at every byte alignment
    wins = [(0, 0, S), (1, 142, S), (2, 7, S), (3, 100, S), (352, 0, S), (351, 142, S)]
    want = ops.pack_rgb8(img.to(DEV)).cpu()
    for offset in range(4):
        raw = torch.zeros(frames.numel() + 4, dtype=torch.uint8, device=DEV)
        work = raw[offset:offset + frames.numel()].view(frames.shape)
        work.copy_(frames)
        ops.paste_windows(work, img.to(DEV), _sq(wins))
        got = work.cpu()
        for n, (x0, y0, s) in enumerate(wins):
            assert torch.equal(got[n, y0:y0 + s, x0:x0 + s], want[n]), (offset, n)
        assert _outside_equal(got, frames, wins)
        assert int(raw[:offset].sum()) == 0 and int(raw[offset + frames.numel():].sum()) == 0
    # no byte outside a window changes: up- and downscaling windows on every border and corner
    for wins in ([(0, 0, 33), (Wf - 34, 0, 34), (0, Hf - 35, 35), (Wf - 36, Hf - 36, 36), (1, 1, 129), (2, 3, 131)],
                 [(3, 0, 270), (209, 0, 270), (210, 0, 270), (0, 1, 269), (5, 17, 32), (6, 18, 201)]):
        for feather, use_matte in R.CASES:
            got = _paste(frames, img, wins, feather, matte if use_matte else None)
            assert _outside_equal(got, frames, wins) and not torch.equal(got, frames)
    # a matte of zeros changes nothing, a matte of ones is no matte
    for feather in (0.0, 0.0625):
        assert torch.equal(_paste(frames, img, R.WINDOWS, feather, torch.zeros(6, 1, S, S)), frames)
        assert torch.equal(_paste(frames, img, R.WINDOWS, feather, torch.ones(6, 1, S, S)), _paste(frames, img, R.WINDOWS, feather))
    # a frame does not depend on its batch
    whole = _paste(frames, img, R.WINDOWS, 0.0625, matte)
    for n in range(6):
        assert torch.equal(_paste(frames[n:n + 1], img[n:n + 1], R.WINDOWS[n:n + 1], 0.0625, matte[n:n + 1])[0], whole[n]), n


def test_device_windows_equal_the_host_list_and_bad_ones_are_refused(small):
    from emoportraits_amd import ops
    frames, img, matte = small["smooth"]
    want = _paste(frames, img, R.WINDOWS, 0.0625, matte)
    work = frames.to(DEV)
    dev_wins = torch.tensor(_sq(R.WINDOWS), dtype=torch.int32, device=DEV)
    assert torch.equal(ops.paste_windows(work, img.to(DEV), dev_wins, 0.0625, matte.to(DEV)).cpu(), want)
    # device-side windows that are not square, leave the frame or shrink by more than 4: those frames stay as they were
    bad = torch.tensor([(10, 5, 70, 71), (411, 5, 70, 70), (0, 0, 270, 270), (300, 100, 31, 31), (-1, 1, 180, 180), (352, 143, 128, 128)],
                       dtype=torch.int32, device=DEV)
    got = ops.paste_windows(frames.to(DEV), img.to(DEV), bad, 0.0625, matte.to(DEV)).cpu()
    for n in range(6):
        assert torch.equal(got[n], want[n] if n == 2 else frames[n]), n
    work = frames.to(DEV)
    for wins, msg in ((_sq(R.WINDOWS)[:5], "windows for"), (_sq(R.WINDOWS)[:5] + [(352, 142, 128, 127)], "square"),
                      (_sq(R.WINDOWS)[:5] + [(353, 142, 128, 128)], "inside"), (_sq(R.WINDOWS)[:5] + [(352, 142, 31, 31)], "quarter")):
        with pytest.raises(ValueError, match=msg):
            ops.paste_windows(work, img.to(DEV), wins)
    with pytest.raises(RuntimeError, match="device"):
        ops.paste_windows(frames, img.to(DEV), _sq(R.WINDOWS))
    assert torch.equal(work.cpu(), frames)


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


def _clip(S, N, Hf, Wf, seed):
    """N frames and one window per frame: sides S / 2 ... min(Hf, Wf), every x0 % 4, the first and last touching the borders"""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (N, Hf, Wf, 3), generator=g, dtype=torch.uint8)
    top = min(Hf, Wf)
    wins = []
    for n in range(N):
        s = S // 2 + ((top - S // 2) * n) // max(N - 1, 1)
        x0 = 0 if n == 0 else (Wf - s if n == N - 1 else min(Wf - s, 5 * n + 1))
        y0 = 0 if n == 0 else (Hf - s if n == N - 1 else min(Hf - s, 3 * n))
        wins.append((x0, y0, s))
    return frames, wins


def _collect(gen):
    out = {}
    for b0, t in gen:
        for j in range(t.shape[0]):
            out[b0 + j] = t[j].cpu().clone()
    return torch.stack([out[i] for i in range(len(out))])


@pytest.mark.parametrize("mode", ["plain", "smooth_pose", "identities", "matte"])
def test_animate_frames_paste_back_equals_paste_back_of_the_rendered_images(wrapper, tiny, mode):
    """animate_frames(paste_back=True) = paste_back(frames, the fp32 images of the same run without it, windows), bit for bit,
    and the input frames outside the windows; host frames through the pinned ring (ring=2, a short last batch) and
    device-resident frames with to_host=False give the same bytes, and the caller's device tensor is not modified"""
    w = wrapper
    S = tiny["cfg"]["image_size"]
    N, B = 10, 4
    frames, wins = _clip(S, N, S + S // 2 + 3, 2 * S + 5, seed=5)
    kw = {}
    matte = None
    if mode == "smooth_pose":
        kw = dict(smooth_pose=True)
    elif mode == "identities":
        kw = dict(identities=[(3 * i + i // 4) % 2 for i in range(N)], smooth_pose=True, smooth_per_identity=True, mix=True)
    elif mode == "matte":
        matte = lambda img: img.mean(dim=1, keepdim=True).clamp(0, 1)
    w.reset_pose_state()
    rendered = _collect(w.animate_frames(frames, batch_size=B, windows=wins, to_host=False, as_uint8=False, **kw))
    assert rendered.dtype == torch.float32 and tuple(rendered.shape) == (N, 3, S, S)
    before = frames.clone()
    want = w.paste_back(frames, rendered, wins, matte=matte)
    assert want.is_cuda and want.dtype == torch.uint8 and torch.equal(frames, before)
    want = want.cpu()
    assert _outside_equal(want, frames, wins) and not torch.equal(want, frames)
    paste = dict(paste_back=True, paste_matte=matte)
    w.reset_pose_state()
    host = _collect(w.animate_frames(frames, batch_size=B, windows=wins, ring=2, **kw, **paste))
    assert torch.equal(host, want)
    dev_frames = frames.to(DEV)
    w.reset_pose_state()
    dev = _collect(w.animate_frames(dev_frames, batch_size=B, windows=wins, to_host=False, **kw, **paste))
    assert torch.equal(dev, want)
    assert torch.equal(dev_frames.cpu(), frames)                        # the caller's device-resident frames are untouched
    w.reset_pose_state()
    dev_ring = _collect(w.animate_frames(dev_frames, batch_size=B, windows=wins, ring=2, **kw, **paste))
    assert torch.equal(dev_ring, want) and torch.equal(dev_frames.cpu(), frames)
    # paste_back() of a device tensor clones it
    again = w.paste_back(dev_frames, rendered.to(DEV), wins, matte=matte)
    assert torch.equal(again.cpu(), want) and torch.equal(dev_frames.cpu(), frames)


def test_chunks_of_two_frame_sizes_get_a_new_ring_and_the_crop_path_is_unchanged(wrapper, tiny):
    w = wrapper
    S = tiny["cfg"]["image_size"]
    a, wa = _clip(S, 5, S + 9, S + 30, seed=7)
    b, wb = _clip(S, 6, 2 * S, S + 1, seed=8)
    w.reset_pose_state()
    crops = [t.cpu().clone() for _, t in w.animate_frames([a, b], batch_size=4, windows=wa + wb, ring=2)]
    assert all(tuple(c.shape[1:]) == (S, S, 3) for c in crops)
    rendered = _collect(w.animate_frames([a, b], batch_size=4, windows=wa + wb, to_host=False, as_uint8=False))
    from emoportraits_amd import ops
    assert torch.equal(torch.cat(crops), ops.pack_rgb8(rendered.to(DEV)).cpu())
    got = {}
    for b0, full in w.animate_frames([a, b], batch_size=4, windows=wa + wb, ring=2, paste_back=True, feather=0.25):
        got[b0] = full.clone()
    assert sorted(got) == [0, 4, 5, 9]
    assert torch.equal(torch.cat([got[0], got[4]]), w.paste_back(a, rendered[:5], wa, feather=0.25).cpu())
    assert torch.equal(torch.cat([got[5], got[9]]), w.paste_back(b, rendered[5:], wb, feather=0.25).cpu())
    with pytest.raises(ValueError, match="windows"):
        next(w.animate_frames(a, paste_back=True))
    with pytest.raises(RuntimeError, match="matting"):
        next(w.animate_frames(a, windows=wa, paste_back=True, paste_matte=True))
