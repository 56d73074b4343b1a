"""TEST INFRASTRUCTURE ONLY -- the YUV 4:2:0 definitions of include/emo_hip.h (ABI 22) restated in torch on CODES, generalising
tests/nv12_reference.py (8-bit) to 10-bit codes, the four sample layouts as arrays, guarded surfaces in host or device memory, and
the checks the CPU emulation test and the GPU test of the five ABI 22 entry points share (they differ only in where the memory
lies).  Frames travel through the checks as `codes`: int32 [N, 3H/2, W] in NV12's arrangement (H rows of Y, H/2 rows of
interleaved U, V), whatever layout they are laid out in for a call."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import nv12_reference as R
import paste_back_reference as PB

FORMATS = ("nv12", "yuv420p", "p010", "yuv420p10")
LAYOUT = {f: i for i, f in enumerate(FORMATS)}
NEW = FORMATS[1:]
BITS = {"nv12": 8, "yuv420p": 8, "p010": 10, "yuv420p10": 10}
SHIFT = {"nv12": 0, "yuv420p": 0, "p010": 6, "yuv420p10": 0}
PLANAR = {"nv12": False, "yuv420p": True, "p010": False, "yuv420p10": True}
NP_DTYPE = {"nv12": np.uint8, "yuv420p": np.uint8, "p010": np.uint16, "yuv420p10": np.uint16}
IGNORED = {"p010": 0x003F, "yuv420p10": 0xFC00}             # the bits of a word outside its code
GUARD, FILL = 64, 0xA5
F64, F32 = torch.float64, torch.float32
N, H, W, S = R.N, R.H, R.W, R.S
MODES, CASES, WINDOWS, WINDOWS_ODD, MATRIX_ID = R.MODES, R.CASES, R.WINDOWS, R.WINDOWS_ODD, R.MATRIX_ID
D_TOL, C_TOL, MAX_CODE_DIFF, MAX_SHARE = R.D_TOL, R.C_TOL, R.MAX_BYTE_DIFF, R.MAX_SHARE
SEED = 7


# ---- the definitions on codes -----------------------------------------------------------------------------------------------
def coef(colorspace, full_range, bits):
    """nv12_reference.coef with the range constants of the code width (10 bits: 64 / 876 / 896, or 0 / 1023 / 1023)"""
    k = dict(R.coef(colorspace, full_range))
    if bits == 10:
        k["oy"], k["sy"], k["sc"] = (0.0, 1023.0, 1023.0) if full_range else (64.0, 876.0, 896.0)
        k["cbs"], k["crs"] = k["sc"] / (2 * (1 - k["Kb"])), k["sc"] / (2 * (1 - k["Kr"]))
    k["mid"], k["top"] = float(1 << (bits - 1)), float((1 << bits) - 1)
    return k


def decode(codes, colorspace, full_range, bits, dt):
    k = coef(colorspace, full_range, bits)
    Y, U, V = R.planes(codes)
    up = lambda c: c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    yp = (Y.to(dt) - k["oy"]) / k["sy"]
    cb, cr = (up(U).to(dt) - k["mid"]) / k["sc"], (up(V).to(dt) - k["mid"]) / k["sc"]
    r, b = yp + k["rv"] * cr, yp + k["bu"] * cb
    g = (yp - k["gv"] * cr) - k["gu"] * cb
    return torch.stack([r, g, b], dim=1).clamp(0, 1)


def _pre(img, k):
    x = img.clamp(0, 1)
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    yp = (k["Kr"] * r + k["Kg"] * g) + k["Kb"] * b
    return k["oy"] + k["sy"] * yp, k["mid"] + k["cbs"] * (b - yp), k["mid"] + k["crs"] * (r - yp)


def _code(v, k):
    return torch.floor(v).clamp(0, k["top"]).to(torch.int32)


def encode(img, colorspace, full_range, bits, dt):
    k = coef(colorspace, full_range, bits)
    yc, cbc, crc = _pre(img.to(dt), k)
    n, h, w = yc.shape
    out = torch.empty((n, 3 * h // 2, w), dtype=torch.int32)
    out[:, :h] = _code(yc + 0.5, k)
    uv = out[:, h:].view(n, h // 2, w // 2, 2)
    for j, c in enumerate((cbc, crc)):
        a, b, c2, d = R._quad(c)
        uv[..., j] = _code((((a + b) + c2) + d) * 0.25 + 0.5, k)
    return out


def crop(codes, wins, size, colorspace, full_range, bits, dt):
    rgb = decode(codes, colorspace, full_range, bits, dt)
    return torch.cat([F.interpolate(rgb[n:n + 1, :, y0:y0 + s, x0:x0 + s], size=(size, size), mode="bicubic",
                                    align_corners=False).clamp(0, 1) for n, (x0, y0, s) in enumerate(wins)])


def paste(codes, img, wins, feather, matte, colorspace, full_range, bits, dt):
    """nv12_reference.paste on codes of `bits` bits"""
    k = coef(colorspace, full_range, bits)
    out = codes.clone()
    Y, U, V = R.planes(out)
    for n, (x0, y0, s) in enumerate(wins):
        r = F.interpolate(img[n:n + 1].to(dt), size=(s, s), mode="bicubic", align_corners=False,
                          antialias=bool(s < img.shape[-1]))[0].clamp(0, 1)
        c = torch.arange(s, dtype=dt) + 0.5
        d = torch.minimum(c, s - c)
        a = (torch.minimum(d[:, None], d[None, :]) / (feather * s)).clamp(0, 1) if feather > 0 else torch.ones(s, s, dtype=dt)
        if matte is not None:
            a = (a * F.interpolate(matte[n:n + 1].to(dt), size=(s, s), mode="bilinear", align_corners=False)[0, 0]).clamp(0, 1)
        yc, cbc, crc = _pre(r, k)
        Y[n, y0:y0 + s, x0:x0 + s] = _code(((1 - a) * Y[n, y0:y0 + s, x0:x0 + s].to(dt) + a * yc) + 0.5, k)
        pad = (x0 & 1, (x0 + s) & 1, y0 & 1, (y0 + s) & 1)
        a4 = R._quad(F.pad(a, pad))
        am = (((a4[0] + a4[1]) + a4[2]) + a4[3]) * 0.25
        cx0, cy0, cx1, cy1 = R.chroma_rect(x0, y0, s)
        for plane, code in ((U, cbc), (V, crc)):
            t = R._quad(F.pad(a * code, pad))
            mean = (((t[0] + t[1]) + t[2]) + t[3]) * 0.25
            plane[n, cy0:cy1, cx0:cx1] = _code(((1 - am) * plane[n, cy0:cy1, cx0:cx1].to(dt) + mean) + 0.5, k)
    return out


def compare_codes(got, ref64, ref32, touched):
    """nv12_reference.compare_bytes on codes"""
    return R.compare_bytes(got, ref64, ref32, touched)


def inputs():
    """{'smooth' | 'noise': (codes8 int32 [6,405,480], codes10, img fp32 [6,3,128,128], matte fp32 [6,1,128,128])}, seed 7"""
    g = torch.Generator().manual_seed(SEED)
    out = {}
    rgb = PB.smooth(g, (N, 3, H, W), 4).clamp(0, 1)
    img = PB.smooth(g, (N, 3, S, S), 3).float()
    matte = PB.smooth(g, (N, 1, S, S), 6).clamp(0, 1).float()
    out["smooth"] = (encode(rgb, "bt709", False, 8, F64), encode(rgb, "bt709", False, 10, F64), img, matte)
    c8 = torch.randint(0, 256, (N, 3 * H // 2, W), generator=g, dtype=torch.int32)
    c10 = torch.randint(0, 1024, (N, 3 * H // 2, W), generator=g, dtype=torch.int32)
    out["noise"] = (c8, c10, torch.rand(N, 3, S, S, generator=g) * 1.2 - 0.1, torch.rand(N, 1, S, S, generator=g))
    return out


def achromatic(full_range, bits):
    """one frame, chroma at the mid-point, Y over the whole legal range, every value in every block position (codes)"""
    lo, hi = (0, (1 << bits) - 1) if full_range else (16 << (bits - 8), 235 << (bits - 8))
    h, w = 16, 2 * (hi - lo + 1)
    y = torch.arange(lo, hi + 1, dtype=torch.int32).repeat_interleave(2)[None, :].repeat(h, 1)
    y[1::2] = y[1::2].flip(1)
    return torch.cat([y, torch.full((h // 2, w), 1 << (bits - 1), dtype=torch.int32)])[None].contiguous()


# ---- codes <-> the arrays of a layout -----------------------------------------------------------------------------------------
def junk_like(codes, fmt, seed=3):
    """random values for the ignored bits of every word (zeros for the 8-bit layouts)"""
    if fmt not in IGNORED:
        return torch.zeros_like(codes)
    return torch.randint(0, 1 << 16, codes.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32) & IGNORED[fmt]


def to_layout(codes, fmt, junk=None):
    """codes int32 [N, 3H/2, W] (NV12's arrangement) -> the frames as an array [N, 3H/2, W] of the layout's dtype, dense: planar
    layouts hold the U plane and then the V plane straight after Y (ffmpeg's rawvideo frame)"""
    n, rows, w = codes.shape
    h = rows // 3 * 2
    words = (codes << SHIFT[fmt]) | (0 if junk is None else junk)
    if PLANAR[fmt]:
        uv = words[:, h:].reshape(n, h // 2, w // 2, 2)
        words = torch.cat([words[:, :h].reshape(n, -1), uv[..., 0].reshape(n, -1), uv[..., 1].reshape(n, -1)], dim=1).reshape(n, rows, w)
    return words.numpy().astype(NP_DTYPE[fmt])


def from_layout(arr, fmt):
    """the inverse of to_layout -> (codes int32 in NV12's arrangement, the ignored bits of every word in the same arrangement)"""
    words = torch.from_numpy(np.ascontiguousarray(arr).astype(np.int32))
    n, rows, w = words.shape
    h = rows // 3 * 2
    if PLANAR[fmt]:
        flat = words.reshape(n, -1)
        u = flat[:, h * w:h * w + h * w // 4].reshape(n, h // 2, w // 2)
        v = flat[:, h * w + h * w // 4:].reshape(n, h // 2, w // 2)
        words = torch.cat([flat[:, :h * w].reshape(n, h, w), torch.stack([u, v], dim=-1).reshape(n, h // 2, w)], dim=1)
    return (words >> SHIFT[fmt]) & ((1 << BITS[fmt]) - 1), words & IGNORED.get(fmt, 0)


# ---- memory: where the arrays of a call lie -----------------------------------------------------------------------------------
class HostMemory:
    """numpy arrays as they are (the CPU emulation)"""

    def put(self, arr):
        return arr

    @staticmethod
    def ptr(h):
        return None if h is None else ctypes.c_void_p(h.ctypes.data)

    @staticmethod
    def get(h):
        return h


class DeviceMemory:
    """a copy on the GPU, read back after the call"""

    def put(self, arr):
        # (ops.torch: where a test has the guarded_outputs fixture the copy lies between that allocator's guards as well)
        from emoportraits_amd import ops
        t = torch.from_numpy(arr)
        return ops.torch.empty(tuple(t.shape), dtype=t.dtype, device="cuda").copy_(t)

    @staticmethod
    def ptr(h):
        return None if h is None else ctypes.c_void_p(h.data_ptr())

    @staticmethod
    def get(h):
        torch.cuda.synchronize()
        return h.cpu().numpy()


def _hp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def w4(wins):
    return np.ascontiguousarray([(w[0], w[1], w[2], w[3] if len(w) > 3 else w[2]) for w in wins], dtype=np.int32).reshape(-1, 4)


class Surface:
    """N frames of a layout in one byte buffer between GUARD bytes: per frame the Y plane (H rows, `pad` extra samples a row),
    then the chroma -- H/2 interleaved rows of the luma pitch, or a U and a V plane of H/2 rows with `pad_c` extra samples a row
    -- and `gap` bytes to the next frame; everything that is no sample = FILL.  `arr` [N, 3H/2, W] as to_layout makes it."""

    def __init__(self, mem, fmt, n, h, w, pad=0, pad_c=0, gap=0, arr=None):
        self.mem, self.fmt, self.n, self.h, self.w = mem, fmt, n, h, w
        self.B = B = np.dtype(NP_DTYPE[fmt]).itemsize
        self.pitch_y = (w + pad) * B
        self.pitch_c = (w // 2 + pad_c) * B if PLANAR[fmt] else self.pitch_y
        crows = h if PLANAR[fmt] else h // 2                                      # chroma rows of pitch_c in a frame
        self.off_u = h * self.pitch_y
        self.off_v = self.off_u + (h // 2) * self.pitch_c
        self.fstride = self.off_u + crows * self.pitch_c + gap
        self.raw = np.full(2 * GUARD + n * self.fstride, FILL, np.uint8)
        self.data = np.zeros(self.raw.shape, bool)
        for f in range(n):
            for view in self._planes(self.data, f, as_bytes=True):
                view[...] = True
        if arr is not None:
            self.write(arr)
        self.before = self.raw.copy()
        self.dev = mem.put(self.raw)

    def _planes(self, raw, f, as_bytes=False):
        """the Y and the chroma plane(s) of frame f as strided views of the buffer"""
        dt, B = (raw.dtype, 1) if as_bytes else (np.dtype(NP_DTYPE[self.fmt]), self.B)
        k = self.B if as_bytes else 1
        base = GUARD + f * self.fstride
        mk = lambda off, rows, cols, pitch: np.ndarray((rows, cols * k), dt, raw.data, base + off, (pitch, B))
        if PLANAR[self.fmt]:
            return [mk(0, self.h, self.w, self.pitch_y), mk(self.off_u, self.h // 2, self.w // 2, self.pitch_c),
                    mk(self.off_v, self.h // 2, self.w // 2, self.pitch_c)]
        return [mk(0, self.h, self.w, self.pitch_y), mk(self.off_u, self.h // 2, self.w, self.pitch_c)]

    def write(self, arr):
        for f in range(self.n):
            flat, at = arr[f].reshape(-1), 0
            for view in self._planes(self.raw, f):
                view[...] = flat[at:at + view.size].reshape(view.shape)
                at += view.size

    def args(self):
        base = self.mem.ptr(self.dev).value + GUARD
        v = ctypes.c_void_p(base + self.off_v) if PLANAR[self.fmt] else None
        return ctypes.c_void_p(base), ctypes.c_void_p(base + self.off_u), v, self.pitch_y, self.pitch_c, self.fstride

    def read(self):
        """-> (the frames as an array [N, 3H/2, W] of the layout, did everything that is no sample keep its FILL)"""
        raw = np.array(self.mem.get(self.dev))
        arr = np.stack([np.concatenate([v.reshape(-1) for v in self._planes(raw, f)]).reshape(3 * self.h // 2, self.w) for f in range(self.n)])
        return arr, bool((raw[~self.data] == FILL).all())

    def table_row(self, f):
        """frame f as a row of the frame table -- dense planar frames only (pad_c == pad / 2)"""
        return (self.mem.ptr(self.dev).value + GUARD + f * self.fstride, self.pitch_y, self.h, self.w)


class Api:
    """the five ABI 22 entry points (and the ten NV12 ones) of `lib` on codes, every frame on a guarded Surface of `mem`"""

    def __init__(self, lib, mem, signatures):
        self.lib, self.mem = lib, mem
        for name, sig in signatures.items():
            if name.startswith(("emo_yuv420", "emo_pack_yuv420", "emo_paste_yuv420", "emo_paste_ragged_yuv420", "emo_nv12", "emo_pack_nv12",
                                "emo_paste_windows_nv12", "emo_paste_faces_nv12", "emo_paste_faces_ragged_nv12", "emo_resize2d_windows_f32")):
                assert hasattr(lib, name), f"the library does not export {name}"
                getattr(lib, name).argtypes = sig
                getattr(lib, name).restype = ctypes.c_int

    def _put(self, a):
        return None if a is None else self.mem.put(np.ascontiguousarray(a))

    def surface(self, fmt, codes, junk=None, **geom):
        n, rows, w = codes.shape
        return Surface(self.mem, fmt, n, rows // 3 * 2, w, arr=to_layout(codes, fmt, junk), **geom)

    def crop(self, fmt, codes, wins, size, mode, host_windows=True, frame_of=None, junk=None, old=False, **geom):
        """emo_yuv420_crop_f32 (old: emo_nv12_windows_f32 / emo_nv12_faces_f32) -> (return code, fp32 [M,3,Ho,Wo]); the frames and
        everything around them are checked to be unchanged"""
        s = self.surface(fmt, codes, junk, **geom)
        win = None if wins is None else w4(wins)
        m = codes.shape[0] if frame_of is None else len(frame_of)
        out = self._put(np.full((m, 3) + tuple(size), np.float32(-7.0)))
        fof = None if frame_of is None else np.ascontiguousarray(frame_of, dtype=np.int32)
        dwin, dfof = self._put(win), self._put(fof)
        y, u, v, py, pc, fs = s.args()
        p, mt = self.mem.ptr, (MATRIX_ID[mode[0]], int(mode[1]), None)
        if not old:
            rc = self.lib.emo_yuv420_crop_f32(LAYOUT[fmt], y, u, v, py, pc, fs, s.h, s.w, p(dwin), _hp(win) if host_windows else None, p(dfof),
                                              _hp(fof), p(out), m, s.n, size[0], size[1], *mt)
        elif frame_of is None:
            rc = self.lib.emo_nv12_windows_f32(y, u, py, fs, s.h, s.w, p(dwin), _hp(win) if host_windows else None, p(out), m, size[0], size[1], *mt)
        else:
            rc = self.lib.emo_nv12_faces_f32(y, u, py, fs, s.h, s.w, p(dwin), _hp(win) if host_windows else None, p(dfof), _hp(fof), p(out), m,
                                             s.n, size[0], size[1], *mt)
        got = torch.from_numpy(np.array(self.mem.get(out)))
        assert np.array_equal(np.array(self.mem.get(s.dev)), s.before), "a crop wrote into its frames"
        return rc, got

    def pack(self, fmt, img, mode, old=False, **geom):
        """emo_pack_yuv420 (old: emo_pack_nv12) -> (return code, codes, the ignored bits of every word)"""
        n, _, h, w = img.shape
        s = Surface(self.mem, fmt, n, h, w, **geom)
        im = self._put(img.numpy())
        y, u, v, py, pc, fs = s.args()
        mt = (MATRIX_ID[mode[0]], int(mode[1]), None)
        if old:
            rc = self.lib.emo_pack_nv12(self.mem.ptr(im), y, u, py, fs, n, h, w, *mt)
        else:
            rc = self.lib.emo_pack_yuv420(LAYOUT[fmt], self.mem.ptr(im), y, u, v, py, pc, fs, n, h, w, *mt)
        arr, intact = s.read()
        assert intact, "pack wrote outside its samples"
        return (rc,) + from_layout(arr, fmt)

    def paste(self, fmt, codes, img, wins, feather=0.0, matte=None, mode=MODES[0], host_windows=True, frame_of=None, junk=None, old=False,
              **geom):
        """emo_paste_yuv420 (old: emo_paste_windows_nv12 / emo_paste_faces_nv12) on a copy -> (return code, codes, ignored bits)"""
        s = self.surface(fmt, codes, junk, **geom)
        win = w4(wins)
        fof = None if frame_of is None else np.ascontiguousarray(frame_of, dtype=np.int32)
        im, mt_, dwin, dfof = self._put(img.numpy()), self._put(None if matte is None else matte.numpy()), self._put(win), self._put(fof)
        m = img.shape[0]
        y, u, v, py, pc, fs = s.args()
        p, mt = self.mem.ptr, (float(feather), MATRIX_ID[mode[0]], int(mode[1]), None)
        hw = _hp(win) if host_windows else None
        if not old:
            rc = self.lib.emo_paste_yuv420(LAYOUT[fmt], p(im), p(mt_), p(dwin), hw, p(dfof), _hp(fof), y, u, v, py, pc, fs, m, s.n, img.shape[-1],
                                           s.h, s.w, *mt)
        elif frame_of is None:
            rc = self.lib.emo_paste_windows_nv12(p(im), p(mt_), p(dwin), hw, y, u, py, fs, m, img.shape[-1], s.h, s.w, *mt)
        else:
            rc = self.lib.emo_paste_faces_nv12(p(im), p(mt_), p(dwin), hw, p(dfof), _hp(fof), y, u, py, fs, m, s.n, img.shape[-1], s.h, s.w, *mt)
        arr, intact = s.read()
        assert intact, "paste wrote outside its samples"
        return (rc,) + from_layout(arr, fmt)

    def ragged(self, fmt, frames, wins, frame_of, mode, size=None, img=None, matte=None, feather=0.0, host_windows=True, old=False,
               table_edit=None):
        """emo_yuv420_crop_ragged_f32 (img None) / emo_paste_ragged_yuv420 (old: the NV12 ragged entry points) on a list of frames
        (codes [1, 3H/2, W]) of different sizes, each a dense guarded surface of its own -> (return code, crops | list of codes)"""
        surf = [self.surface(fmt, c) for c in frames]
        table = np.array([s.table_row(0) for s in surf], dtype=np.int64).reshape(-1, 4)
        if table_edit is not None:
            table_edit(table)
        win, fof = w4(wins), np.ascontiguousarray(frame_of, dtype=np.int32)
        dtab, dwin, dfof = self._put(table), self._put(win), self._put(fof)
        p, m, hw = self.mem.ptr, len(frame_of), _hp(win) if host_windows else None
        mt = (MATRIX_ID[mode[0]], int(mode[1]), None)
        lay = () if old else (LAYOUT[fmt],)
        if img is None:
            out = self._put(np.full((m, 3) + tuple(size), np.float32(-7.0)))
            fn = self.lib.emo_nv12_faces_ragged_f32 if old else self.lib.emo_yuv420_crop_ragged_f32
            rc = fn(*lay, p(dtab), _hp(table), p(dwin), hw, p(dfof), _hp(fof), p(out), m, len(surf), size[0], size[1], *mt)
            res = torch.from_numpy(np.array(self.mem.get(out)))
        else:
            im, mt_ = self._put(img.numpy()), self._put(None if matte is None else matte.numpy())
            fn = self.lib.emo_paste_faces_ragged_nv12 if old else self.lib.emo_paste_ragged_yuv420
            rc = fn(*lay, p(im), p(mt_), p(dtab), _hp(table), p(dwin), hw, p(dfof), _hp(fof), m, len(surf), img.shape[-1], float(feather), *mt)
            res = None
        back = []
        for s in surf:
            arr, intact = s.read()
            assert intact, "a ragged call wrote outside its samples"
            back.append(from_layout(arr, fmt)[0])
        return rc, (back if res is None else res)

    def resize_windows(self, rgb, wins, size):
        """emo_resize2d_windows_f32(bicubic, clamp01) of fp32 frames [N,3,H,W]"""
        n, _, h, w = rgb.shape
        x, win = self._put(rgb.numpy()), self._put(w4(wins))
        out = self._put(np.zeros((n, 3) + tuple(size), np.float32))
        assert self.lib.emo_resize2d_windows_f32(self.mem.ptr(x), h * w, w, self.mem.ptr(win), self.mem.ptr(out), n, 3, size[0], size[1], 1, 1, None) == 0
        return torch.from_numpy(np.array(self.mem.get(out)))


def touched_mask(shape, wins, frame_of=None):
    """nv12_reference.touched_mask with several faces per frame"""
    if frame_of is None:
        return R.touched_mask(shape, wins)
    mask = torch.zeros(shape, dtype=torch.bool)
    for w, f in zip(wins, frame_of):
        mask[f] |= R.touched_mask((1,) + tuple(shape[1:]), [w])[0]
    return mask


def codes10_of_bytes(codes8):
    """the 10-bit codes 4 * byte: what a p010 word byte << 8 holds"""
    return codes8 << 2


# ---- the checks both tests run (api: an Api on host or device memory) ---------------------------------------------------------
GEOM = {"nv12": dict(pad=6, gap=10), "p010": dict(pad=6, gap=12), "yuv420p": dict(pad=10, pad_c=3, gap=7), "yuv420p10": dict(pad=4, pad_c=5, gap=6)}
FACES = [(10, 5, 70), (40, 30, 128), (300, 100, 96), (211, 1, 180), (352, 142, 128), (1, 1, 129), (0, 0, 270), (100, 100, 64)]
FACE_FRAME = [0, 0, 1, 3, 3, 3, 4, 4]                          # frames 2 and 5 have no face; faces of a frame overlap
FACES_SQ = [(x, y, s, s) for x, y, s in FACES]


def check_layout0_is_the_nv12_entry_points(api, inp):
    c8, _, img, matte = inp["noise"]
    mode = MODES[1]
    for wins in (None, WINDOWS, WINDOWS_ODD):
        size = (H, W) if wins is None else (S, S)
        for hw in (True, False):
            a, b = api.crop("nv12", c8, wins, size, mode, hw, old=True, **GEOM["nv12"]), api.crop("nv12", c8, wins, size, mode, hw, **GEOM["nv12"])
            assert a[0] == b[0] == 0 and torch.equal(a[1], b[1])
    a, b = api.crop("nv12", c8, FACES, (S, S), mode, frame_of=FACE_FRAME, old=True), api.crop("nv12", c8, FACES, (S, S), mode, frame_of=FACE_FRAME)
    assert a[0] == b[0] == 0 and torch.equal(a[1], b[1])
    a, b = api.pack("nv12", img, mode, old=True, **GEOM["nv12"]), api.pack("nv12", img, mode, **GEOM["nv12"])
    assert a[0] == b[0] == 0 and torch.equal(a[1], b[1])
    for i, (feather, use_matte) in enumerate(CASES):
        wins, m = (WINDOWS, WINDOWS_ODD)[i % 2], matte if use_matte else None
        a = api.paste("nv12", c8, img, wins, feather, m, MODES[i], old=True, **GEOM["nv12"])
        b = api.paste("nv12", c8, img, wins, feather, m, MODES[i], **GEOM["nv12"])
        assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]) and not torch.equal(b[1], c8)
    fi = torch.cat([img, img[:2]])
    a = api.paste("nv12", c8, fi, FACES, 0.0625, None, mode, frame_of=FACE_FRAME, old=True)
    b = api.paste("nv12", c8, fi, FACES, 0.0625, None, mode, frame_of=FACE_FRAME)
    assert a[0] == b[0] == 0 and torch.equal(a[1], b[1])
    frames, wins, fof = ragged_case(c8)
    a, b = api.ragged("nv12", frames, wins, fof, mode, (S, S), old=True), api.ragged("nv12", frames, wins, fof, mode, (S, S))
    assert a[0] == b[0] == 0 and torch.equal(a[1], b[1])
    a = api.ragged("nv12", frames, wins, fof, mode, img=img[:len(fof)], feather=0.0625, old=True)
    b = api.ragged("nv12", frames, wins, fof, mode, img=img[:len(fof)], feather=0.0625)
    assert a[0] == b[0] == 0 and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def ragged_case(codes):
    """three frames of different sizes cut out of `codes` (each the top-left corner of a uniform frame), faces and their frames"""
    def cut(f, h, w):
        y, uv = codes[f:f + 1, :h, :w], codes[f:f + 1, H:H + h // 2, :w]
        return torch.cat([y, uv], dim=1).contiguous()
    frames = [cut(0, 270, 480), cut(1, 96, 128), cut(2, 180, 322)]
    wins = [(10, 5, 70), (40, 30, 128), (0, 0, 96), (3, 1, 64), (141, 7, 170)]
    return frames, wins, [0, 0, 1, 1, 2]


def check_planar_8bit_is_nv12(api, inp, kind, which):
    """yuv420p on de-interleaved planes gives NV12's results on the same samples: every mode and case"""
    c8, _, img, matte = inp[kind]
    wins = (WINDOWS, WINDOWS_ODD)[which]
    for mode in MODES:
        a, b = api.crop("nv12", c8, wins, (S, S), mode), api.crop("yuv420p", c8, wins, (S, S), mode, **GEOM["yuv420p"])
        assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]), mode
        a, b = api.pack("nv12", img, mode), api.pack("yuv420p", img, mode, **GEOM["yuv420p"])
        assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]), mode
        for feather, use_matte in CASES:
            m = matte if use_matte else None
            a = api.paste("nv12", c8, img, wins, feather, m, mode)
            b = api.paste("yuv420p", c8, img, wins, feather, m, mode, **GEOM["yuv420p"])
            assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]) and not torch.equal(b[1], c8), (mode, feather, use_matte)
    a, b = api.crop("nv12", c8, None, (H, W), MODES[0]), api.crop("yuv420p", c8, None, (H, W), MODES[0])
    assert a[0] == b[0] == 0 and torch.equal(a[1], b[1])


def check_the_two_10bit_layouts_agree(api, inp, kind, which):
    _, c10, img, matte = inp[kind]
    wins = (WINDOWS, WINDOWS_ODD)[which]
    jp, jq = junk_like(c10, "p010"), junk_like(c10, "yuv420p10", 4)
    for mode in MODES:
        a = api.crop("p010", c10, wins, (S, S), mode, **GEOM["p010"])
        b = api.crop("yuv420p10", c10, wins, (S, S), mode, **GEOM["yuv420p10"])
        assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]), mode
        # junk in the ignored bits of the input does not change a crop
        aj, bj = api.crop("p010", c10, wins, (S, S), mode, junk=jp), api.crop("yuv420p10", c10, wins, (S, S), mode, junk=jq)
        assert torch.equal(aj[1], a[1]) and torch.equal(bj[1], a[1]), mode
        a, b = api.pack("p010", img, mode, **GEOM["p010"]), api.pack("yuv420p10", img, mode, **GEOM["yuv420p10"])
        assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]) and not a[2].any() and not b[2].any(), mode
        for feather, use_matte in CASES:
            m = matte if use_matte else None
            a = api.paste("p010", c10, img, wins, feather, m, mode, junk=jp, **GEOM["p010"])
            b = api.paste("yuv420p10", c10, img, wins, feather, m, mode, junk=jq, **GEOM["yuv420p10"])
            assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]) and not torch.equal(a[1], c10), (mode, feather, use_matte)
            touched = touched_mask(c10.shape, wins)
            for (_, codes, ignored), junk in ((a, jp), (b, jq)):
                assert not ignored[touched].any()                                # a touched sample comes out clean
                assert torch.equal(ignored[~touched], junk[~touched])            # an untouched one keeps all 16 bits
                assert torch.equal(codes[~touched], c10[~touched])


def check_8bit_against_10bit_limited_range(api, inp, kind):
    """a p010 frame of words byte << 8 (codes 4 * byte) gives the NV12 crop of those bytes, limited range only"""
    c8 = inp[kind][0]
    for wins, size in ((WINDOWS, (S, S)), (WINDOWS_ODD, (S, S)), (None, (H, W))):
        for mode in (m for m in MODES if not m[1]):
            a = api.crop("nv12", c8, wins, size, mode)
            for fmt in ("p010", "yuv420p10"):
                b = api.crop(fmt, codes10_of_bytes(c8), wins, size, mode)
                assert a[0] == b[0] == 0 and torch.equal(a[1], b[1]), (fmt, mode)
    arr = to_layout(codes10_of_bytes(c8), "p010")
    assert np.array_equal(arr, to_layout(c8, "nv12").astype(np.uint16) << 8)


def check_exact_cases(api, inp, fmt):
    """ABI 17's exact cases on one layout"""
    bits, g = BITS[fmt], GEOM[fmt]
    codes, img, matte = inp["noise"][0 if bits == 8 else 1], inp["noise"][2], inp["noise"][3]
    for which, wins in enumerate((WINDOWS, WINDOWS_ODD)):
        mode = MODES[which + 1]
        rc, rgb = api.crop(fmt, codes, None, (H, W), mode)
        assert rc == 0
        want = api.resize_windows(rgb, wins, (S, S))
        rc, got = api.crop(fmt, codes, wins, (S, S), mode)
        assert rc == 0 and torch.equal(got, want)                                # the fused crop is D, then the window resize
        rc, dev = api.crop(fmt, codes, wins, (S, S), mode, host_windows=False, **g)
        assert rc == 0 and torch.equal(dev, want)                                # device and host window tables agree
        for n in (0, N - 1):
            rc, one = api.crop(fmt, codes[n:n + 1], wins[n:n + 1], (S, S), mode)
            assert rc == 0 and torch.equal(one[0], want[n]), n                   # a frame does not depend on its batch
    for mode in MODES:
        ach = achromatic(mode[1], bits)
        h, w = ach.shape[1] // 3 * 2, ach.shape[2]
        rc, rgb = api.crop(fmt, ach, None, (h, w), mode)
        assert rc == 0 and torch.equal(rgb[:, 0], rgb[:, 1]) and torch.equal(rgb[:, 0], rgb[:, 2])
        rc, back, ignored = api.pack(fmt, rgb, mode)
        assert rc == 0 and torch.equal(back, ach) and not ignored.any()
    even = [(0, 0, S), (2, 142, S), (352, 0, S), (350, 142, S), (100, 70, S), (352, 142, S)]
    for hw, mode in ((True, MODES[0]), (False, MODES[3])):
        rc, got, _ = api.paste(fmt, codes, img, even, 0.0, None, mode, hw, **g)
        rc2, want, _ = api.pack(fmt, img, mode)
        assert rc == 0 and rc2 == 0
        for n, (x0, y0, s) in enumerate(even):                                   # side == S, even origin, no feather: pack's samples
            assert torch.equal(got[n, y0:y0 + s, x0:x0 + s], want[n, :s]), n
            assert torch.equal(got[n, H + y0 // 2:H + (y0 + s) // 2, x0:x0 + s], want[n, s:]), n
        keep = ~R.touched_mask(codes.shape, even)
        assert torch.equal(got[keep], codes[keep])
    edge = [(0, 0, 33), (W - 34, 0, 34), (0, H - 35, 35), (W - 36, H - 36, 36), (1, 1, 129), (2, 3, 131)]
    for i, wins in enumerate((WINDOWS, WINDOWS_ODD, edge)):
        feather, use_matte = CASES[i + 1]
        rc, got, _ = api.paste(fmt, codes, img, wins, feather, matte if use_matte else None, MODES[i], **g)
        touched = R.touched_mask(codes.shape, wins)
        assert rc == 0 and torch.equal(got[~touched], codes[~touched])           # nothing outside the touched rectangles changes
        assert int((got != codes)[touched].sum()) > 0.1 * int(touched.sum())     # (and they were written)
    for wins, mode in ((WINDOWS, MODES[1]), (WINDOWS_ODD, MODES[3])):
        rc, got, _ = api.paste(fmt, codes, img, wins, 0.0625, torch.zeros(N, 1, S, S), mode)
        assert rc == 0 and torch.equal(got, codes)                               # a zero matte changes nothing
        rc1, ones, _ = api.paste(fmt, codes, img, wins, 0.0625, torch.ones(N, 1, S, S), mode)
        rc2, none, _ = api.paste(fmt, codes, img, wins, 0.0625, None, mode)
        assert rc1 == 0 and rc2 == 0 and torch.equal(ones, none) and not torch.equal(none, codes)
        rc, whole, _ = api.paste(fmt, codes, img, wins, 0.0625, matte, mode)
        for n in (1, N - 1):
            rc, one, _ = api.paste(fmt, codes[n:n + 1], img[n:n + 1], wins[n:n + 1], 0.0625, matte[n:n + 1], mode)
            assert rc == 0 and torch.equal(one[0], whole[n]), n


def check_faces_and_ragged(api, inp, fmt):
    bits = BITS[fmt]
    codes, img, matte = inp["noise"][0 if bits == 8 else 1], inp["noise"][2], inp["noise"][3]
    fi, fm = torch.cat([img, img[:2].flip(0)]), torch.cat([matte, matte[:2]])
    mode = MODES[2]
    # crops: row m is the windows form's crop of frame frame_of[m]
    rc, got = api.crop(fmt, codes, FACES, (S, S), mode, frame_of=FACE_FRAME, **GEOM[fmt])
    rc2, want = api.crop(fmt, codes[FACE_FRAME], FACES, (S, S), mode)
    assert rc == 0 and rc2 == 0 and torch.equal(got, want)
    # paste: one launch is the faces pasted one after another in list order
    for feather, m in ((0.0, None), (0.0625, fm)):
        rc, got, _ = api.paste(fmt, codes, fi, FACES, feather, m, mode, frame_of=FACE_FRAME, **GEOM[fmt])
        assert rc == 0
        want = codes.clone()
        for j, (w, f) in enumerate(zip(FACES, FACE_FRAME)):
            rc, one, _ = api.paste(fmt, want[f:f + 1], fi[j:j + 1], [w], feather, None if m is None else m[j:j + 1], mode)
            assert rc == 0
            want[f] = one[0]
        assert torch.equal(got, want)
        touched = touched_mask(codes.shape, FACES, FACE_FRAME)
        assert torch.equal(got[~touched], codes[~touched])
    # ragged: the uniform entry point on frames held in the top-left corner
    frames, wins, fof = ragged_case(codes)
    rc, got = api.ragged(fmt, frames, wins, fof, mode, (S, S))
    held = torch.zeros((3,) + tuple(codes.shape[1:]), dtype=torch.int32)
    for f, c in enumerate(frames):
        h, w = c.shape[1] // 3 * 2, c.shape[2]
        held[f, :h, :w], held[f, H:H + h // 2, :w] = c[0, :h], c[0, h:]
    rc2, want = api.crop(fmt, held, wins, (S, S), mode, frame_of=fof, host_windows=False)
    assert rc == 0 and rc2 == 0 and torch.equal(got, want)
    rc, back = api.ragged(fmt, frames, wins, fof, mode, img=img[:5], matte=matte[:5], feather=0.0625)
    rc2, want, _ = api.paste(fmt, held, img[:5], wins, 0.0625, matte[:5], mode, host_windows=False, frame_of=fof)
    assert rc == 0 and rc2 == 0
    for f, c in enumerate(back):
        h, w = c.shape[1] // 3 * 2, c.shape[2]
        assert torch.equal(c[0, :h], want[f, :h, :w]) and torch.equal(c[0, h:], want[f, H:H + h // 2, :w]), f
        assert not torch.equal(c, frames[f])


def check_refusals(api, inp):
    """every refusal of ABI 22 beyond ABI 17 / 18 / 19's, and those on every layout, with nothing written"""
    lib, mem = api.lib, api.mem
    img1 = inp["noise"][2][:1]
    for fmt in FORMATS:
        codes = inp["noise"][0 if BITS[fmt] == 8 else 1][:1]
        B = 1 if BITS[fmt] == 8 else 2
        # what ABI 17 refuses, through the new entry points: windows (codes and precedence), feather
        for wins, code in (([(10, 5, 70, 71)], -2), ([(10, 5, 31)], -2), ([(411, 5, 70)], -1), ([(10, 201, 70)], -1), ([(-1, 5, 70)], -1),
                           ([(10, 5, 0)], -1), ([(0, 0, 271)], -1)):
            rc, got, _ = api.paste(fmt, codes, img1, wins)
            assert rc == code and torch.equal(got, codes), (fmt, wins, rc)
            rc, got, _ = api.paste(fmt, codes, img1, wins, host_windows=False)   # only the device sees them: the kernel skips the frame
            assert rc == 0 and torch.equal(got, codes), (fmt, wins, rc)
            if code == -1:
                rc, out = api.crop(fmt, codes, wins, (S, S), MODES[0])
                assert rc == -1 and bool((out == -7.0).all())
        for feather in (-0.01, 0.51, float("nan")):
            rc, got, _ = api.paste(fmt, codes, img1, [(10, 5, 70)], feather)
            assert rc == -1 and torch.equal(got, codes)
        # argument by argument on a tiny frame; the buffers keep their fill
        s = Surface(mem, fmt, 1, 8, 8)
        y, u, v, py, pc, fs = s.args()
        win = w4([(0, 0, 4, 4)])
        dwin, out, im = mem.put(win), mem.put(np.full((1, 3, 4, 4), np.float32(-7))), mem.put(np.full((1, 3, 8, 8), np.float32(0.5)))
        im4 = mem.put(np.full((1, 3, 4, 4), np.float32(0.5)))
        p, L = mem.ptr, LAYOUT[fmt]
        odd = lambda q: ctypes.c_void_p(q.value + 1)
        crop_ok = [L, y, u, v, py, pc, fs, 8, 8, p(dwin), _hp(win), None, None, p(out), 1, 1, 4, 4, 0, 0, None]
        pack_ok = [L, p(im), y, u, v, py, pc, fs, 1, 8, 8, 0, 0, None]
        paste_ok = [L, p(im4), None, p(dwin), _hp(win), None, None, y, u, v, py, pc, fs, 1, 1, 4, 8, 8, 0.0, 0, 0, None]
        short_c = (4 if PLANAR[fmt] else 8) * B - B
        crop_bad = {0: [4, -1], 1: [None], 2: [None], 4: [8 * B - B], 5: [short_c], 6: [-2], 7: [7, 0], 8: [7, 0], 9: [None], 13: [None],
                    14: [0], 16: [0], 17: [-1], 18: [2, -1]}
        pack_bad = {0: [4, -1], 1: [None], 2: [None], 3: [None], 5: [8 * B - B], 6: [short_c], 7: [-2], 8: [0], 9: [7, 0], 10: [7, 0], 11: [2, -1]}
        paste_bad = {0: [4, -1], 1: [None], 3: [None], 7: [None], 8: [None], 10: [8 * B - B], 11: [short_c], 12: [-2], 13: [0], 15: [0], 16: [7, 0],
                     17: [7, 0], 18: [0.6], 19: [2, -1]}
        if PLANAR[fmt]:
            crop_bad[3], pack_bad[4], paste_bad[9] = [None], [None], [None]
        if B == 2:                                                               # 16-bit layouts: an odd address, pitch or stride
            crop_bad[1].append(odd(y)); crop_bad[2].append(odd(u)); crop_bad[4].append(py + 1); crop_bad[5].append(pc + 1); crop_bad[6].append(fs + 1)
            pack_bad[2].append(odd(y)); pack_bad[3].append(odd(u)); pack_bad[5].append(py + 1); pack_bad[6].append(pc + 1); pack_bad[7].append(fs + 1)
            paste_bad[7].append(odd(y)); paste_bad[8].append(odd(u)); paste_bad[10].append(py + 1); paste_bad[11].append(pc + 1); paste_bad[12].append(fs + 1)
            if PLANAR[fmt]:
                crop_bad[3].append(odd(v)); pack_bad[4].append(odd(v)); paste_bad[9].append(odd(v))
        for fn, ok, bad in ((lib.emo_yuv420_crop_f32, crop_ok, crop_bad), (lib.emo_pack_yuv420, pack_ok, pack_bad),
                            (lib.emo_paste_yuv420, paste_ok, paste_bad)):
            for k, values in bad.items():
                for val in values:
                    a = list(ok)
                    a[k] = val
                    assert fn(*a) == -1, (fmt, fn.__name__, k, val)
        # the windows form takes no frame_of_host; the faces form of the paste needs one
        fof = np.zeros(1, np.int32)
        a = list(crop_ok); a[12] = _hp(fof)
        assert lib.emo_yuv420_crop_f32(*a) == -1
        a = list(paste_ok); a[5] = p(mem.put(fof))
        assert lib.emo_paste_yuv420(*a) == -1
        a = list(paste_ok); a[5], a[6] = p(mem.put(fof)), _hp(np.ones(1, np.int32))
        assert lib.emo_paste_yuv420(*a) == -1
        assert np.array_equal(np.array(mem.get(s.dev)), s.before) and bool((np.array(mem.get(out)) == -7).all())
        assert lib.emo_yuv420_crop_f32(*crop_ok) == 0 and lib.emo_paste_yuv420(*paste_ok) == 0 and lib.emo_pack_yuv420(*pack_ok) == 0
        assert not bool((np.array(mem.get(out)) == -7).any())
        # the frame table
        frames, wins, fof_l = ragged_case(codes.repeat(3, 1, 1))
        def bad_row(col, val):
            def edit(t):
                t[1, col] = val(t[1, col]) if callable(val) else val
            return edit
        edits = [bad_row(0, 0), bad_row(2, 0), bad_row(3, -2), bad_row(2, 95), bad_row(3, 127), bad_row(1, 128 * B - B)]
        if B == 2:
            edits += [bad_row(0, lambda a: a + 1), bad_row(1, lambda a: a + 1)]
        if PLANAR[fmt]:
            edits += [bad_row(1, lambda a: a + B)]                               # a pitch that does not halve into whole samples
        for e in edits:
            rc, out_r = api.ragged(fmt, frames, wins, fof_l, MODES[0], (S, S), table_edit=e)
            assert rc == -1 and bool((out_r == -7.0).all())
            rc, back = api.ragged(fmt, frames, wins, fof_l, MODES[0], img=inp["noise"][2][:5], table_edit=e)
            assert rc == -1 and all(torch.equal(x, y) for x, y in zip(back, frames))
        rc, back = api.ragged(fmt, frames, wins[:4] + [(141, 7, 31)], fof_l, MODES[0], img=inp["noise"][2][:5])
        assert rc == -2 and all(torch.equal(x, y) for x, y in zip(back, frames))
        rc, out_r = api.ragged(fmt, frames, wins, [0, 1, 0, 1, 2], MODES[0], (S, S))
        assert rc == -1 and bool((out_r == -7.0).all())
    s = Surface(mem, "nv12", 1, 8, 8)
    y, u, v, py, pc, fs = s.args()
    for layout in (-1, 4, 17):
        assert lib.emo_yuv420_crop_ragged_f32(layout, None, None, None, None, None, None, None, 0, 1, 4, 4, 0, 0, None) == -1
        assert lib.emo_paste_ragged_yuv420(layout, None, None, None, None, None, None, None, None, 0, 1, 4, 0.0, 0, 0, None) == -1


def check_10bit_against_fp64(api, inp, fmt, kind, report):
    """D within 1e-6, C within 1e-5; E and P: every code within 1 of the fp64 restatement and at most MAX_SHARE of the touched
    samples different at all, on inputs where torch's fp32 evaluation of the restatement stays under the same caps"""
    _, c10, img, matte = inp[kind]
    for mode in MODES:
        rc, got = api.crop(fmt, c10, None, (H, W), mode, **GEOM[fmt])
        ref = decode(c10, *mode, 10, F64)
        err, err32 = (got.double() - ref).abs().max().item(), (decode(c10, *mode, 10, F32).double() - ref).abs().max().item()
        report(f"PARITY {fmt} D {kind} {mode[0]} full_range {mode[1]}: max abs err {err:.2e} (torch fp32 against fp64: {err32:.2e})")
        assert rc == 0 and err32 <= D_TOL
        assert err <= D_TOL and got.min() >= 0 and got.max() <= 1
        for im, geom in ((img, GEOM[fmt]), (img[:, :, 1:127, :126].contiguous(), {})):
            rc, got, _ = api.pack(fmt, im, mode, **geom)
            worst, share, share32 = compare_codes(got, encode(im.double(), *mode, 10, F64), encode(im, *mode, 10, F32), got.numel())
            report(f"PARITY {fmt} E {kind} {tuple(im.shape[-2:])} {mode[0]} full_range {mode[1]}: max code diff {worst}, share of samples "
                   f"that differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
            assert rc == 0 and share32 <= MAX_SHARE
            assert worst <= MAX_CODE_DIFF and share <= MAX_SHARE
    for which, wins in enumerate((WINDOWS, WINDOWS_ODD)):
        for mode in MODES[which::2]:
            rc, got = api.crop(fmt, c10, wins, (S, S), mode)
            ref = crop(c10, wins, S, *mode, 10, F64)
            err, err32 = (got.double() - ref).abs().max().item(), (crop(c10, wins, S, *mode, 10, F32).double() - ref).abs().max().item()
            report(f"PARITY {fmt} C {kind} windows {which} {mode[0]} full_range {mode[1]}: max abs err {err:.2e} (torch fp32 against "
                   f"fp64: {err32:.2e})")
            assert rc == 0 and err32 <= C_TOL
            assert err <= C_TOL
        for case, (feather, use_matte) in enumerate(CASES):
            mode, m = MODES[(case + which) % 4], matte if use_matte else None
            rc, got, _ = api.paste(fmt, c10, img, wins, feather, m, mode)
            ref64 = paste(c10, img.double(), wins, feather, None if m is None else m.double(), *mode, 10, F64)
            ref32 = paste(c10, img, wins, feather, m, *mode, 10, F32)
            touched = R.touched_mask(c10.shape, wins)
            worst, share, share32 = compare_codes(got, ref64, ref32, int(touched.sum()))
            report(f"PARITY {fmt} P {kind} windows {which} feather {feather} matte {use_matte} {mode[0]} full_range {mode[1]}: max code "
                   f"diff {worst}, share of touched samples that differ {share:.2e} (torch fp32 against fp64: {share32:.2e})")
            assert rc == 0 and share32 <= MAX_SHARE
            assert worst <= MAX_CODE_DIFF and share <= MAX_SHARE
            assert torch.equal(got[~touched], c10[~touched])


def check_the_restatement_at_8_bits_is_nv12_reference(inp):
    c8, _, img, matte = inp["noise"]
    u8 = c8.to(torch.uint8)
    for mode in MODES:
        assert torch.equal(decode(c8, *mode, 8, F64), R.decode(u8, *mode, F64))
        assert torch.equal(encode(img, *mode, 8, F32), R.encode(img, *mode, F32).int())
        assert torch.equal(paste(c8, img, WINDOWS_ODD, 0.0625, matte, *mode, 8, F32), R.paste(u8, img, WINDOWS_ODD, 0.0625, matte, *mode, F32).int())


# ---- tensors of a format for the Python layers ---------------------------------------------------------------------------------
TORCH_DTYPE = {"nv12": torch.uint8, "yuv420p": torch.uint8, "p010": torch.uint16, "yuv420p10": torch.uint16}


def tensor_of(codes, fmt, junk=None):
    """codes -> the frames as a torch tensor [N, 3H/2, W] of the format's dtype"""
    return torch.from_numpy(to_layout(codes, fmt, junk))


def codes_of(t, fmt):
    return from_layout(t.cpu().numpy(), fmt)[0]
