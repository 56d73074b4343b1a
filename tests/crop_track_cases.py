"""TEST INFRASTRUCTURE ONLY -- the seeded cases that tests/test_crop_track_emul.py (the host-compiled kernel) and
tests/test_crop_track_gpu.py (the device) both hold to hostglue.crop_track: boxes of every kind the contract names, over frames
of four sizes and K interleaved tracker streams."""
import numpy as np

FRAMES = [(1920, 1080), (97, 61), (2, 2), (1, 1)]                     # (W, H)
BIG = float(1 << 30)


def _ordinary(rng, W, H):
    """a box whose window fits: centre well inside the frame, extent 20 % ... 60 % of the shorter edge"""
    s = min(W, H)
    cx, cy = rng.uniform(0.35, 0.65) * W, rng.uniform(0.35, 0.65) * H
    hw, hh = rng.uniform(0.1, 0.3) * s, rng.uniform(0.1, 0.3) * s
    return [cx - hw, cy - hh, cx + hw, cy + hh]


def _special(W, H):
    """the boxes the contract names, for a W x H frame (pixels)"""
    nan, inf = float("nan"), float("inf")
    q = min(W, H) / 4
    return [[-q, H / 2 - q, q, H / 2 + q], [W / 2 - q, -q, W / 2 + q, q],                   # over the left and the top edge
            [W - q, H / 2 - q, W + q, H / 2 + q], [W / 2 - q, H - q, W / 2 + q, H + q],     # over the right and the bottom edge
            [-W, -H, 2 * W, 2 * H], [-5e8, -5e8, 5e8 + W, 5e8 + H],                         # larger than the frame
            [W + 10, H / 2, W + 60, H / 2 + 40], [-90.0, -80.0, -10.0, -20.0],              # the centre outside the frame
            [W / 2, H / 2, W / 2, H / 2], [W / 2 + 20, H / 2 + 20, W / 2 - 20, H / 2 - 20],  # zero and negative extent
            [nan, 0, 10, 10], [0, 0, inf, 10], [0, -inf, 10, 10], [1e300, 0, 10, 10], [0, 0, BIG, 10], [0, 0, 10, -BIG],
            [-(BIG - 1), H / 2 - q, BIG - 1 + W, H / 2 + q]]                                 # just inside the range, about the frame


class Case:
    """one seeded call: M rows over K interleaved tracker streams (two rows outside [0, K) where M allows).  A stream is a video: its
    rows share a frame size, 97 x 61 for every fourth stream (drawn less often) and 1920 x 1080 for the others; every eleventh row
    sits in a 2 x 2 or 1 x 1 frame instead, every seventh is one of the special boxes, and a stream's first row is an ordinary box
    (a `fixed` tracker keeps it)"""

    def __init__(self, M, K, seed, momentum=0.5, smooth=True, fixed=False, scale=1.0, box_format="xyxy", missing="skip", min_side=2,
                 null_streams=False, one_size=None, special0=None):
        rng = np.random.default_rng(seed)
        self.M, self.K = M, K
        self.kw = dict(momentum=momentum, smooth=smooth, fixed=fixed, scale=scale, box_format=box_format, missing=missing, min_side=min_side)
        small = np.array([k % 4 == 1 for k in range(K)])
        weight = np.where(small, 0.4, 1.0)
        so = rng.choice(K, M, p=weight / weight.sum()).astype(np.int32)
        if null_streams:
            so[:] = 0
        self.sizes = np.zeros((M, 2), np.int32)
        boxes = np.zeros((M, 4))
        specials, begun = 0, set()
        for i in range(M):
            k = int(so[i])
            W, H = one_size or FRAMES[1 if small[k] else 0]
            if k in begun and one_size is None and i % 11 == 10:
                W, H = FRAMES[2 + (i // 11) % 2]
                boxes[i] = [0, 0, 2, 2] if (i // 11) % 4 < 2 else [0, 0, 1, 1]
            elif k in begun and i % 7 == 3:
                sp = _special(W, H)
                boxes[i] = sp[(specials + (seed if special0 is None else special0)) % len(sp)]
                specials += 1
            else:
                boxes[i] = _ordinary(rng, W, H)
            begun.add(k)
            self.sizes[i] = (W, H)
        if box_format == "relative":                          # (the same boxes about as relative ones; the 1.2 and 0.9 move them)
            W, H = self.sizes[:, 0].astype(np.float64), self.sizes[:, 1].astype(np.float64)
            boxes = np.stack([boxes[:, 0] / W, boxes[:, 1] / H, (boxes[:, 2] - boxes[:, 0]) / W, (boxes[:, 3] - boxes[:, 1]) / H], 1)
        self.boxes = np.ascontiguousarray(boxes)
        self.so = None if null_streams else so
        if self.so is not None and M >= 12:
            self.so[7], self.so[11] = -1, K
        self.one_size = one_size

    def states(self):
        return np.full((self.K, 3), np.nan), np.zeros(self.K, np.int32), np.zeros((self.K, 4), np.int32)

    def size_arg(self, rows=slice(None)):
        return self.one_size if self.one_size else np.ascontiguousarray(self.sizes[rows])

    def restated(self, st, rows=slice(None), why=None):
        from emoportraits_amd import hostglue
        so = None if self.so is None else self.so[rows]
        return hostglue.crop_track(self.boxes[rows], so, self.size_arg(rows), *st, K=self.K, why=why, **self.kw)


def sweep(M, K):
    """the cases of one (M, K): momentum 0.01, 0.5, 1.0; fixed; scale 1.0 and 1.3; both formats; skip and hold; min_side 2 and 128;
    without smoothing; one frame size for all rows"""
    base = 1000 * K + M
    return [Case(M, K, base + 0, momentum=0.01), Case(M, K, base + 1, momentum=0.5, scale=1.3, missing="hold"),
            Case(M, K, base + 2, momentum=1.0, min_side=128), Case(M, K, base + 3, fixed=True, missing="hold", min_side=128),
            Case(M, K, base + 4, box_format="relative", scale=1.3), Case(M, K, base + 5, box_format="relative", missing="hold", momentum=0.01),
            Case(M, K, base + 6, smooth=False, special0=8), Case(M, K, base + 7, smooth=False, missing="hold", one_size=(1920, 1080)),
            Case(M, K, base + 8, one_size=(97, 61), scale=1.3, missing="hold")]


def hostglue_crop_track(boxes, size, **kw):
    """hostglue.crop_track of rows that share one frame size and one stateless stream"""
    from emoportraits_amd import hostglue
    return hostglue.crop_track(boxes, None, size, None, None, None, **kw)
