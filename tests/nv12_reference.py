"""TEST INFRASTRUCTURE ONLY -- the NV12 definitions of include/emo_hip.h (ABI 17: D bytes -> RGB, E RGB -> bytes, C the crop
emo_nv12_windows_f32 computes, P the paste emo_paste_windows_nv12 computes) restated in torch, and the inputs the CPU and the GPU
test of them share.  Every restatement is evaluated in fp64 (the arbiter) and in fp32 (torch's own rounding noise on the same
expression: the premise of the caps below)."""
import torch
import torch.nn.functional as F

import paste_back_reference as PB

# the bounds of the comparisons with the fp64 restatement
D_TOL = 1e-6             # D: at most 5 roundings (two quotients, a product, up to two sums) of magnitudes <= 2.2: 5 * 2.2 * 2^-24 = 6.6e-7
C_TOL = 1e-5             # C: the bound the project's crop resize carries
MAX_BYTE_DIFF = PB.MAX_BYTE_DIFF      # E, P: every byte within 1 of the fp64 result ...
MAX_SHARE = PB.MAX_SHARE              # ... and at most this share of the touched bytes different at all

N, H, W, S = 6, 270, 480, 128
WINDOWS = PB.WINDOWS                                                                     # (x0, y0, side)
WINDOWS_ODD = [(1, 1, 129), (3, 0, 270), (209, 0, 270), (0, 1, 269), (5, 17, 33), (7, 19, 201)]   # odd origins / sides, all borders
CASES = PB.CASES                                                                         # (feather, matte?)
MODES = [("bt709", False), ("bt601", True), ("bt709", True), ("bt601", False)]           # (colorspace, full_range)
MATRIX_ID = {"bt709": 0, "bt601": 1}


def coef(colorspace, full_range):
    """every constant of the definitions, in fp64 (Python floats)"""
    Kr, Kb = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}[colorspace]
    Kg = 1.0 - Kr - Kb
    oy, sy, sc = (0.0, 255.0, 255.0) if full_range else (16.0, 219.0, 224.0)
    return dict(Kr=Kr, Kg=Kg, Kb=Kb, oy=oy, sy=sy, sc=sc, rv=2 * (1 - Kr), bu=2 * (1 - Kb), gv=2 * Kr * (1 - Kr) / Kg,
                gu=2 * Kb * (1 - Kb) / Kg, cbs=sc / (2 * (1 - Kb)), crs=sc / (2 * (1 - Kr)))


def planes(nv12):
    """uint8 [N, 3H/2, W] -> (Y [N,H,W], U [N,H/2,W/2], V [N,H/2,W/2]) views"""
    h = nv12.shape[1] // 3 * 2
    uv = nv12[:, h:].reshape(nv12.shape[0], h // 2, nv12.shape[2] // 2, 2)
    return nv12[:, :h], uv[..., 0], uv[..., 1]


def decode(nv12, colorspace, full_range, dt):
    """D: uint8 [N, 3H/2, W] -> [N,3,H,W] in dtype dt"""
    k = coef(colorspace, full_range)
    Y, U, V = planes(nv12)
    up = lambda c: c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    yp = (Y.to(dt) - k["oy"]) / k["sy"]
    cb, cr = (up(U).to(dt) - 128) / k["sc"], (up(V).to(dt) - 128) / k["sc"]
    r, b = yp + k["rv"] * cr, yp + k["bu"] * cb
    g = (yp - k["gv"] * cr) - k["gu"] * cb
    return torch.stack([r, g, b], dim=1).clamp(0, 1)


def codes(img, k):
    """[..., 3, h, w] clamped image -> (Yc, Cbc, Crc) of E before the rounding"""
    x = img.clamp(0, 1)
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    yp = (k["Kr"] * r + k["Kg"] * g) + k["Kb"] * b
    return k["oy"] + k["sy"] * yp, 128 + k["cbs"] * (b - yp), 128 + k["crs"] * (r - yp)


def _quad(t):
    """[..., 2h, 2w] -> the four members of every 2 x 2 block, in the order 00, 01, 10, 11"""
    return t[..., 0::2, 0::2], t[..., 0::2, 1::2], t[..., 1::2, 0::2], t[..., 1::2, 1::2]


def _byte(v):
    return torch.floor(v).clamp(0, 255).to(torch.uint8)


def encode(img, colorspace, full_range, dt):
    """E: [N,3,H,W] -> uint8 [N, 3H/2, W], evaluated in dtype dt"""
    k = coef(colorspace, full_range)
    yc, cbc, crc = codes(img.to(dt), k)
    n, h, w = yc.shape
    out = torch.empty((n, 3 * h // 2, w), dtype=torch.uint8)
    out[:, :h] = _byte(yc + 0.5)
    uv = out[:, h:].view(n, h // 2, w // 2, 2)
    for j, c in enumerate((cbc, crc)):
        a, b, c2, d = _quad(c)
        uv[..., j] = _byte((((a + b) + c2) + d) * 0.25 + 0.5)
    return out


def crop(nv12, wins, size, colorspace, full_range, dt):
    """C: crop n = clamp01(bicubic resize of D(frame n)[:, y0:y0+s, x0:x0+s] to size x size)"""
    rgb = decode(nv12, colorspace, full_range, dt)
    return torch.cat([F.interpolate(rgb[n:n + 1, :, y0:y0 + s, x0:x0 + s], size=(size, size), mode="bicubic",
                                    align_corners=False).clamp(0, 1) for n, (x0, y0, s) in enumerate(wins)])


def chroma_rect(x0, y0, s):
    """the chroma samples that cover the luma window: (cx0, cy0, cx1, cy1), ends exclusive"""
    return x0 >> 1, y0 >> 1, ((x0 + s - 1) >> 1) + 1, ((y0 + s - 1) >> 1) + 1


def paste(nv12, img, wins, feather, matte, colorspace, full_range, dt):
    """P: nv12 uint8 [N, 3Hf/2, Wf], img [N,3,S,S], matte [N,1,S,S] or None, wins (x0, y0, s) per frame; evaluated in dtype dt"""
    k = coef(colorspace, full_range)
    out = nv12.clone()
    Y, U, V = planes(out)
    for n, (x0, y0, s) in enumerate(wins):
        r = F.interpolate(img[n:n + 1].to(dt), size=(s, s), mode="bicubic", align_corners=False,
                          antialias=bool(s < img.shape[-1]))[0].clamp(0, 1)
        c = torch.arange(s, dtype=dt) + 0.5
        d = torch.minimum(c, s - c)
        a = (torch.minimum(d[:, None], d[None, :]) / (feather * s)).clamp(0, 1) if feather > 0 else torch.ones(s, s, dtype=dt)
        if matte is not None:
            a = (a * F.interpolate(matte[n:n + 1].to(dt), size=(s, s), mode="bilinear", align_corners=False)[0, 0]).clamp(0, 1)
        yc, cbc, crc = codes(r, k)
        Y[n, y0:y0 + s, x0:x0 + s] = _byte(((1 - a) * Y[n, y0:y0 + s, x0:x0 + s].to(dt) + a * yc) + 0.5)
        # a and a * C on the covering chroma rectangle's luma pixels, zero outside the window
        pad = (x0 & 1, (x0 + s) & 1, y0 & 1, (y0 + s) & 1)
        a4 = _quad(F.pad(a, pad))
        am = (((a4[0] + a4[1]) + a4[2]) + a4[3]) * 0.25
        cx0, cy0, cx1, cy1 = chroma_rect(x0, y0, s)
        for plane, code in ((U, cbc), (V, crc)):
            t = _quad(F.pad(a * code, pad))
            mean = (((t[0] + t[1]) + t[2]) + t[3]) * 0.25
            plane[n, cy0:cy1, cx0:cx1] = _byte(((1 - am) * plane[n, cy0:cy1, cx0:cx1].to(dt) + mean) + 0.5)
    return out


def touched_mask(shape, wins):
    """bool [N, 3H/2, W]: the luma rectangle of every frame's window and the byte pairs of its covering chroma rectangle"""
    n, rows, w = shape
    h = rows // 3 * 2
    mask = torch.zeros(shape, dtype=torch.bool)
    for i, (x0, y0, s) in enumerate(wins):
        mask[i, y0:y0 + s, x0:x0 + s] = True
        cx0, cy0, cx1, cy1 = chroma_rect(x0, y0, s)
        mask[i, h + cy0:h + cy1, 2 * cx0:2 * cx1] = True
    return mask


def compare_bytes(got, ref64, ref32, touched):
    """-> (max byte difference of `got` to the fp64 restatement, share of the `touched` bytes that differ, the same share for
    torch's fp32 evaluation of the restatement)"""
    diff = (got.int() - ref64.int()).abs()
    return diff.max().item(), diff.ne(0).sum().item() / touched, (ref32.int() - ref64.int()).ne(0).sum().item() / touched


def compare_paste(got, nv12, img, wins, feather, matte, colorspace, full_range):
    ref64 = paste(nv12, img.double(), wins, feather, None if matte is None else matte.double(), colorspace, full_range, torch.float64)
    ref32 = paste(nv12, img, wins, feather, matte, colorspace, full_range, torch.float32)
    return compare_bytes(got, ref64, ref32, int(touched_mask(nv12.shape, wins).sum()))


def small_inputs():
    """{'smooth' | 'noise': (nv12 uint8 [6,405,480], img fp32 [6,3,128,128], matte fp32 [6,1,128,128])}, seed 5, drawn in this
    order from one generator.  Smooth frames are the fp64 encoding (bt709, limited range) of a smooth RGB picture."""
    g = torch.Generator().manual_seed(5)
    out = {}
    rgb = PB.smooth(g, (N, 3, H, W), 4).clamp(0, 1)
    img = PB.smooth(g, (N, 3, S, S), 3).float()
    matte = PB.smooth(g, (N, 1, S, S), 6).clamp(0, 1).float()
    out["smooth"] = (encode(rgb, "bt709", False, torch.float64), img, matte)
    nv12 = torch.randint(0, 256, (N, 3 * H // 2, W), generator=g, dtype=torch.uint8)
    img = torch.rand(N, 3, S, S, generator=g) * 1.2 - 0.1
    matte = torch.rand(N, 1, S, S, generator=g)
    out["noise"] = (nv12, img, matte)
    return out


def achromatic(full_range):
    """one frame, U = V = 128, Y over the whole legal range (16 ... 235, or 0 ... 255), every value in every block position"""
    lo, hi = (0, 255) if full_range else (16, 235)
    h, w = 16, 2 * (hi - lo + 1)
    y = torch.arange(lo, hi + 1, dtype=torch.uint8).repeat_interleave(2)[None, :].repeat(h, 1)
    y[1::2] = y[1::2].flip(1)
    return torch.cat([y, torch.full((h // 2, w), 128, dtype=torch.uint8)])[None].contiguous()
