"""TEST INFRASTRUCTURE ONLY -- the definition of emo_paste_windows_rgb8 (include/emo_hip.h, ABI 15) restated in torch, and the
inputs the CPU and the GPU test of it share.  The restatement is evaluated in fp64 (the arbiter) and in fp32 (torch's own
rounding noise on the same expression: the premise of the bound on the share of differing bytes)."""
import torch
import torch.nn.functional as F

# the two bounds of every comparison with the fp64 restatement
MAX_BYTE_DIFF = 1        # every byte within 1 of the fp64 result: a truncation flips where rounding noise straddles an integer
MAX_SHARE = 2e-3         # ... and at most this share of the window bytes differs at all

WINDOWS = [(10, 5, 70), (100, 20, 250), (0, 0, 270), (300, 100, 96), (211, 1, 180), (352, 142, 128)]   # (x0, y0, side); S = 128
CASES = [(0.0, False), (0.0625, False), (0.0625, True), (0.25, True)]                                    # (feather, matte?)


def smooth(g, shape, k):
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    x = F.avg_pool2d(F.pad(x, (k, k, k, k), mode="replicate"), 2 * k + 1, 1)
    lo, hi = x.amin(), x.amax()
    return (x - lo) / (hi - lo) * 1.2 - 0.1


def paste(frames_u8, img, wins, feather, matte, dt):
    """frames_u8 [N,Hf,Wf,3] uint8, img [N,3,S,S], matte [N,1,S,S] or None, wins (x0, y0, s) per frame; evaluated in dtype dt"""
    out = frames_u8.clone()
    for n, (x0, y0, s) in enumerate(wins):
        r = F.interpolate(img[n:n + 1].to(dt), size=(s, s), mode="bicubic", align_corners=False,
                          antialias=bool(s < img.shape[-1]))[0].clamp(0, 1) * 255
        c = torch.arange(s, dtype=dt) + 0.5
        d = torch.minimum(c, s - c)
        a = (torch.minimum(d[:, None], d[None, :]) / (feather * s)).clamp(0, 1) if feather > 0 else torch.ones(s, s, dtype=dt)
        if matte is not None:
            a = a * F.interpolate(matte[n:n + 1].to(dt), size=(s, s), mode="bilinear", align_corners=False)[0, 0]
        fb = frames_u8[n, y0:y0 + s, x0:x0 + s].permute(2, 0, 1).to(dt)
        v = (1 - a) * fb + a * r
        out[n, y0:y0 + s, x0:x0 + s] = v.to(torch.uint8).permute(1, 2, 0)
    return out


def small_inputs():
    """{'smooth' | 'noise': (frames uint8 [6,270,480,3], img fp32 [6,3,128,128], matte fp32 [6,1,128,128])}, seed 3, drawn in this
    order from one generator"""
    g = torch.Generator().manual_seed(3)
    N, H, W, S = 6, 270, 480, 128
    out = {}
    frames = (smooth(g, (N, 3, H, W), 4).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    img = smooth(g, (N, 3, S, S), 3).float()
    matte = smooth(g, (N, 1, S, S), 6).clamp(0, 1).float()
    out["smooth"] = (frames, img, matte)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    img = torch.rand(N, 3, S, S, generator=g) * 1.2 - 0.1
    matte = torch.rand(N, 1, S, S, generator=g)
    out["noise"] = (frames, img, matte)
    return out


def production_inputs(seed=11):
    """one production-sized batch: N = 16 frames of 1080 x 1920, S = 512, window sides spread over 300 ... 900, smooth content (a
    rendered head and a decoded frame are smooth at the pixel scale)"""
    g = torch.Generator().manual_seed(seed)
    N, H, W, S = 16, 1080, 1920, 512
    frames = torch.cat([(smooth(g, (1, 3, H, W), 4).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1) for _ in range(N)]).contiguous()
    img = smooth(g, (N, 3, S, S), 3).float()
    matte = smooth(g, (N, 1, S, S), 6).clamp(0, 1).float()
    wins = []
    for n in range(N):
        s = 300 + (600 * n) // (N - 1)
        x0 = int(torch.randint(0, W - s + 1, (1,), generator=g))
        y0 = int(torch.randint(0, H - s + 1, (1,), generator=g))
        wins.append((x0, y0, s))
    return frames, img, matte, wins


def window_bytes(wins):
    return sum(s * s * 3 for _, _, s in wins)


def compare(got, frames, img, wins, feather, matte):
    """-> (max byte difference of `got` to the fp64 restatement, share of the window bytes that differ, the same share for torch's
    fp32 evaluation of the restatement).  `got` uint8 [N,Hf,Wf,3] on the host."""
    ref64 = paste(frames, img.double(), wins, feather, None if matte is None else matte.double(), torch.float64)
    ref32 = paste(frames, img, wins, feather, matte, torch.float32)
    diff = (got.int() - ref64.int()).abs()
    n = window_bytes(wins)
    return diff.max().item(), diff.ne(0).sum().item() / n, (ref32.int() - ref64.int()).ne(0).sum().item() / n
