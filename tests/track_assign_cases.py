"""TEST INFRASTRUCTURE ONLY -- the cases that tests/test_track_assign_emul.py (the host-compiled kernel) and
tests/test_track_assign_gpu.py (the device) both hold to hostglue.track_assign, and a plain-loop reference of the association
written from the text of include/emo_hip.h (ABI 25) alone: Python floats (doubles, every operation rounded on its own), no numpy
arithmetic, nothing imported from emoportraits_amd."""
import math

import numpy as np

QNAN = np.uint64(0x7ff8000000000000)
BIG = float(1 << 30)


def _box(det, box_format):
    d = [float(v) for v in det]
    return d if box_format == 0 else [d[0], d[1], d[0] + d[2], d[1] + d[3]]


def _usable(b):
    return all(math.isfinite(v) and abs(v) < BIG for v in b) and b[2] > b[0] and b[3] > b[1]


def _iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / (((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter)


def reference(dets, stream_of, ref, age, min_iou, max_missed, box_format):
    """the header's text as loops -> (boxes [F,P,4], restart [F,P], track_of [F,D]); ref [K,P,4] and age [K,P] updated in place"""
    dets = np.ascontiguousarray(dets, np.float64)
    F, D = dets.shape[:2]
    K, P = age.shape
    boxes = np.empty((F, P, 4), np.float64)
    boxes.view(np.uint64)[:] = QNAN
    restart, track_of = np.zeros((F, P), np.int32), np.full((F, D), -1, np.int32)
    for f in range(F):
        k = 0 if stream_of is None else int(stream_of[f])
        if k < 0 or k >= K:
            continue
        box = [_box(dets[f, d], box_format) for d in range(D)]
        usable = [_usable(b) for b in box]
        matched = [False] * P
        while True:                                                              # 1. match
            best_iou, best_p, best_d = -1.0, -1, -1
            for p in range(P):
                if age[k, p] < 0 or matched[p]:
                    continue
                for d in range(D):
                    if not usable[d] or track_of[f, d] >= 0:
                        continue
                    v = _iou([float(x) for x in ref[k, p]], box[d])
                    if v > best_iou:                                             # (strictly: the smaller p, then the smaller d, stays)
                        best_iou, best_p, best_d = v, p, d
            if best_p < 0 or best_iou < min_iou:
                break
            ref[k, best_p] = box[best_d]
            age[k, best_p] = 0
            matched[best_p] = True
            boxes.view(np.uint64)[f, best_p] = dets.view(np.uint64)[f, best_d]
            track_of[f, best_d] = best_p
        for p in range(P):                                                       # 2. age
            if age[k, p] >= 0 and not matched[p]:
                age[k, p] += 1
                if age[k, p] > max_missed:
                    age[k, p] = -1
                    restart[f, p] = 1
        for d in range(D):                                                       # 3. births
            if not usable[d] or track_of[f, d] >= 0:
                continue
            free = [p for p in range(P) if age[k, p] < 0]
            if not free:
                continue
            p = free[0]
            ref[k, p] = box[d]
            age[k, p] = 0
            boxes.view(np.uint64)[f, p] = dets.view(np.uint64)[f, d]
            restart[f, p] = 1
            track_of[f, d] = p
    return boxes, restart, track_of                                              # 4. the rest is as it was filled


class Case:
    def __init__(self, name, dets, P, K=1, stream_of=None, min_iou=0.3, max_missed=2, box_format=0, ref=None, age=None):
        self.name, self.P, self.K = name, P, K
        self.dets = np.ascontiguousarray(dets, np.float64)
        self.F, self.D = self.dets.shape[:2]
        self.so = None if stream_of is None else np.ascontiguousarray(stream_of, np.int32)
        self.kw = dict(min_iou=float(min_iou), max_missed=int(max_missed), box_format=int(box_format))
        self._ref, self._age = ref, age

    def states(self):
        """(ref [K,P,4], age [K,P]) as the case begins: every slot free unless the case brings live tracks"""
        ref = np.full((self.K, self.P, 4), np.nan) if self._ref is None else np.array(self._ref, np.float64).reshape(self.K, self.P, 4)
        age = np.full((self.K, self.P), -1, np.int32) if self._age is None else np.array(self._age, np.int32).reshape(self.K, self.P)
        return ref.copy(), age.copy()

    def rows(self, rows):
        return self.dets[rows], None if self.so is None else np.ascontiguousarray(self.so[rows])

    def reference(self, st, rows=slice(None)):
        dets, so = self.rows(rows)
        return reference(dets, so, st[0], st[1], **self.kw)

    def restated(self, st, rows=slice(None)):
        from emoportraits_amd import hostglue
        dets, so = self.rows(rows)
        kw = dict(self.kw, box_format=("xyxy", "relative")[self.kw["box_format"]])
        return hostglue.track_assign(dets, so, st[0], st[1], **kw)


NAN4 = [np.nan] * 4


def permuted(boxes, D=4, seed=7):
    """ordered boxes [N,P,4] as a detector hands them out: the P faces of a frame at a random P of D rows, the other rows NaN; frame 0
    in order -> (dets [N,D,4], at [N,P] = the row of every face)"""
    N, P = boxes.shape[:2]
    rng = np.random.default_rng(seed)
    dets, at = np.full((N, D, 4), np.nan), np.zeros((N, P), np.int64)
    for t in range(N):
        at[t] = np.arange(P) if t == 0 else rng.permutation(D)[:P]
        dets[t, at[t]] = boxes[t]
    return dets, at


def _sq(cx, cy, h):
    return [cx - h, cy - h, cx + h, cy + h]


def cases():
    rng = np.random.default_rng(25)
    out = []
    # two faces whose order in the list swaps every frame (a NaN row of padding between them on odd frames)
    a = [_sq(30 + t, 40, 10) for t in range(8)]
    b = [_sq(90 - t, 44, 12) for t in range(8)]
    out.append(Case("swap", [[a[t], NAN4, b[t]] if t % 2 == 0 else [b[t], a[t], NAN4] for t in range(8)], P=2))
    # a face missing for max_missed frames comes back to its slot; for max_missed + 1 it dies and is born again
    for gap, name in ((2, "gap_max_missed"), (3, "gap_one_more")):
        d = [[a[t] if not 2 <= t < 2 + gap else NAN4, b[t]] for t in range(8)]
        out.append(Case(name, d, P=2, max_missed=2))
    # ... and dies in the very frame in which a new face appears elsewhere: the freed slot is taken in that frame
    c = _sq(150, 20, 8)
    out.append(Case("death_and_birth_in_one_frame", [[a[t] if t < 2 else NAN4, b[t], c if t >= 3 else NAN4] for t in range(8)], P=2,
                    max_missed=1))
    # max_missed 0: a track dies in its first frame without a detection
    out.append(Case("max_missed_0", [[a[t] if t != 3 else NAN4, b[t]] for t in range(6)], P=3, max_missed=0))
    # more usable detections than free slots
    far = [_sq(20 + 60 * j, 30, 10) for j in range(4)]
    out.append(Case("more_faces_than_slots", [[far[(j + t) % 4] for j in range(4)] for t in range(5)], P=2))
    # two bit-identical detections (tie on d), two live tracks with the same ref (tie on p)
    out.append(Case("tie_on_d", [[a[0], b[0], NAN4], [a[1], a[1], b[1]], [a[2], b[2], a[2]]], P=3))
    out.append(Case("tie_on_p", [[a[0], NAN4], [a[1], a[1]], [NAN4, a[2]]], P=3, ref=[a[0], a[0], NAN4], age=[0, 1, -1]))
    # IoU exactly min_iou (1 x 1 in 2 x 1: 1 / 2) and min_iou one ulp above that IoU
    unit, wide = [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 2.0, 1.0]
    out.append(Case("iou_at_min_iou", [[unit], [wide], [unit]], P=2, min_iou=0.5))
    out.append(Case("iou_one_ulp_below", [[unit], [wide], [unit]], P=2, min_iou=np.nextafter(0.5, 1.0)))
    third = [[0.0, 0.0, 3.0, 1.0]], [[0.0, 0.0, 1.0, 1.0]]                       # 1 / 3, rounded, against min_iou = that double
    out.append(Case("iou_at_a_rounded_third", third, P=2, min_iou=1.0 / 3.0))
    out.append(Case("min_iou_1", [[a[0]], [a[0]], [a[1]]], P=2, min_iou=1.0))
    # what is not a detection: NaN, infinities, x1 <= x0, y1 <= y0, 2^30 and beyond; and the largest values that are
    odd = [[[10, 10, 30, 30.0], NAN4, [0, 0, np.inf, 10], [50, 50, 50, 70.0]],
           [[11, 10, 31, 30.0], [60, 60, 80, 60.0], [0, 0, BIG, 10], [-BIG, 0, 10, 10]],
           [[12, 10, 32, 30.0], [90, 20, 80, 40.0], [np.nan, 0, 10, 10], [0, 0, BIG - 1, 10]],
           [[13, 10, 33, 30.0], [0, -np.inf, 10, 10], [1e300, 0, 2e300, 10], [-(BIG - 1), 0, BIG - 1, 12]]]
    out.append(Case("unusable", odd, P=3))
    # relative (xmin, ymin, width, height): the same two faces, swapped, and a width of zero
    rel = lambda q: [q[0] / 128, q[1] / 96, (q[2] - q[0]) / 128, (q[3] - q[1]) / 96]
    out.append(Case("relative", [[rel(a[t]), rel(b[t]), [0.5, 0.5, 0.0, 0.1]] if t % 2 else [rel(b[t]), [0.1, 0.1, -0.1, 0.2], rel(a[t])]
                                 for t in range(6)], P=2, box_format=1))
    # three streams interleaved, stream 1 without a frame, one frame of a stream outside [0, K) on either side
    so = [0, 2, 0, 2, -1, 2, 0, 3, 0, 2, 2, 0]
    d = [[a[t % 8], b[t % 8]] if (t + s) % 2 else [b[t % 8], a[t % 8]] for t, s in enumerate(so)]
    out.append(Case("streams", d, P=2, K=3, stream_of=so))
    # every lane's share: 16 faces on a grid, each frame jittered and permuted among 32 rows
    grid = np.array([_sq(40 + 70 * (j % 4), 40 + 70 * (j // 4), 20) for j in range(16)])
    d = np.full((6, 32, 4), np.nan)
    for t in range(6):
        d[t, rng.permutation(32)[:16]] = grid + rng.uniform(-3, 3, (16, 4))
    out.append(Case("full_16_by_32", d, P=16, max_missed=1))
    # the same with faces that come and go, more faces than slots and coincident boxes: deaths, births and ties in volume
    d = np.full((12, 32, 4), np.nan)
    for t in range(12):
        on = rng.random(16) < 0.7
        rows = rng.permutation(32)
        d[t, rows[:16][on]] = (grid + np.round(rng.uniform(-6, 6, (16, 4))))[on]
        d[t, rows[16:20]] = grid[rng.integers(0, 16, 4)]
    out.append(Case("crowd_12_by_32", d, P=12, max_missed=1, min_iou=0.25))
    return out
