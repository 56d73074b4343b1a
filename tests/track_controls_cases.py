"""Cases of the control streams that follow face tracks (include/emo_hip.h, ABI 26: emo_theta_ema_scan_tracks_f32,
emo_expr_controls_tracks_f32, emo_head_pose_controls_tracks_f32) -- no tests here; tests/test_track_controls_emul.py runs them on
the host builds of the kernels, tests/test_track_controls_gpu.py on the device.

A case is the inputs of one call with its two row masks, and three statements of what the call computes:
    restated  the masked restatement in emoportraits_amd.hostglue, which the kernels are held to bit for bit;
    plain     an independent plain loop that only ever calls the UNMASKED hostglue functions: every stream's rows are cut at its
              restarts, within a segment the absent rows are dropped and the unmasked function runs over the rest (state fresh
              after a restart, carried in front of the first), and an absent row is the unmasked function on that single row from
              a copy of the state in front of it.  It is what holds the restatement to the header's text;
    unmasked  the function without masks.
Rows: 37 over K = 3 streams plus two rows of stream -1 and two of stream K (41 in all); for the head-pose kernel also 150 rows
over K = 2, so that a thread of its 64-thread block takes several rows and segments straddle the stride.  restart is random at
p = 0.25 and present at p = 0.7, and then, so that they are there whatever the seed:
    stream 0's first row is absent (and no restart: a carried state stays, a fresh stream begins at its first present row);
    stream 1's last row is a restart on an absent row: its flags end at 0 even where they came in as 1;
    stream 2's first row, and its first row behind the cut, are restarts (K = 3): the second call restarts a stream that carries state.
Every case is run in one call and in two that carry the state, cut in the middle (CUT)."""
import itertools

import numpy as np

from emoportraits_amd import hostglue


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def streams_and_masks(n, K, seed, strays=2):
    """-> (stream_of [n + 2 * strays] int32, restart, present int32): n rows over K streams, `strays` rows of stream -1 and of
    stream K spread among them, the masks as the module's text says"""
    rng = np.random.default_rng(seed)
    while True:                                                  # (every stream has rows on both sides of the cut)
        so = rng.integers(0, K, n).astype(np.int32)
        for j, at in enumerate(sorted(rng.choice(n, 2 * strays, replace=False))):
            so = np.insert(so, at + j, -1 if j % 2 == 0 else K)
        so = so.astype(np.int32)
        N = so.shape[0]
        if all((so[:N // 2] == k).sum() >= 2 and (so[N // 2:] == k).sum() >= 2 for k in range(K)):
            break
    restart = (rng.random(N) < 0.25).astype(np.int32)
    present = (rng.random(N) < 0.7).astype(np.int32)
    rows = lambda k, lo=0: [i for i in range(lo, N) if so[i] == k]
    first0 = rows(0)[0]
    restart[first0], present[first0] = 0, 0
    last1 = rows(1 % K)[-1]
    restart[last1], present[last1] = 1, 0
    if K > 2:
        restart[rows(2)[0]] = 1
        restart[rows(2, N // 2)[0]] = 1
    return so, restart, present


class _Case:
    """what the three kinds share: the rows' streams and masks, the cut, and the plain-loop statement over `unmasked`"""

    def _init(self, n, K, seed, masked=True):
        self.K = K
        self.so, self.restart, self.present = streams_and_masks(n, K, seed)
        self.n = self.so.shape[0]
        self.cut = self.n // 2
        if not masked:
            self.restart = self.present = None

    def halves(self):
        return slice(0, self.cut), slice(self.cut, self.n)

    def live(self, rows=slice(None)):
        so = self.so[rows]
        return (so >= 0) & (so < self.K)

    def masks(self, rows=slice(None)):
        return tuple(None if m is None else np.ascontiguousarray(m[rows]) for m in (self.restart, self.present))

    def plain(self, st, rows=slice(None)):
        """the independent statement (the module's text): only self.unmasked is ever called, on rows of one stream"""
        lo, hi, _ = rows.indices(self.n)
        outs = self.blank(hi - lo)
        restart = np.zeros(self.n, np.int32) if self.restart is None else self.restart
        present = np.ones(self.n, np.int32) if self.present is None else self.present

        def put(idx, vals):
            for o, v in zip(outs, vals):
                o[[i - lo for i in idx]] = v
        for k in range(self.K):
            idx = [i for i in range(lo, hi) if self.so[i] == k]
            segments, seg, begins = [], [], False                # a segment: (its rows, whether it begins with a restart)
            for i in idx:
                if restart[i]:
                    if seg or begins:
                        segments.append((seg, begins))
                    seg, begins = [], True
                seg.append(i)
            if seg or begins:
                segments.append((seg, begins))
            for seg, begins in segments:
                if begins:
                    self.clear(st, k)
                front = [a.copy() for a in st]
                here = [i for i in seg if present[i]]
                for i in seg:
                    if not present[i]:
                        copy = [a.copy() for a in front]
                        before = [j for j in here if j < i]
                        if before:
                            self.unmasked(before, copy)
                        put([i], self.unmasked([i], copy))
                if here:
                    put(here, self.unmasked(here, st))
        return outs


class ScanCase(_Case):
    """emo_theta_ema_scan_tracks_f32: values [n,16], state (state [K,16], has [K])"""
    kind = "scan"

    def __init__(self, n=37, K=3, seed=0, masked=True):
        self._init(n, K, seed, masked)
        rng = np.random.default_rng(1000 + seed)
        self.values = _f32(rng.standard_normal((self.n, 16)))
        self.momentum = float(rng.choice([0.5, 0.3, 0.01]))

    def states(self, carried=False):
        rng = np.random.default_rng(7)
        if carried:
            return [_f32(rng.standard_normal((self.K, 16))), np.ones(self.K, np.int32)]
        return [np.full((self.K, 16), np.nan, np.float32), np.zeros(self.K, np.int32)]

    flags = (1,)

    def blank(self, m):
        return [np.full((m, 16), np.nan, np.float32)]

    def clear(self, st, k):
        st[1][k] = 0

    def unmasked(self, idx, st):
        k = int(self.so[idx[0]])
        out, cur = hostglue.ema_scan(self.values[idx], st[0][k] if st[1][k] else None, self.momentum)
        st[0][k], st[1][k] = cur, 1
        return [out]

    def restated(self, st, rows=slice(None)):
        return [hostglue.ema_scan_tracks(self.values[rows], self.so[rows], st[0], st[1], self.momentum, *self.masks(rows))]


# every combination of (neutral, gain, offset, relative, smooth) the expression entry point admits: gain and relative need the neutral
EXPR_COMBOS = [c for c in itertools.product([False, True], repeat=5) if c[0] or not (c[1] or c[3])]


class ExprCase(_Case):
    """emo_expr_controls_tracks_f32: values [n,E], state (anchor [K,E], has_anchor [K], ema [K,E], has_ema [K])"""
    kind = "expr"

    def __init__(self, E, combo, n=37, K=3, seed=0, masked=True):
        self._init(n, K, seed, masked)
        rng = np.random.default_rng(2000 + seed)
        neutral, gain, offset, self.relative, self.smooth = combo
        self.E, self.combo = E, combo
        self.values = _f32(rng.standard_normal((self.n, E)))
        self.neutral = _f32(rng.standard_normal((K, E))) if neutral else None
        self.gain = _f32(rng.uniform(0.0, 2.0, self.n)) if gain else None
        self.offset = _f32(0.3 * rng.standard_normal((self.n, E))) if offset else None
        self.momentum = float(rng.choice([0.5, 0.3, 0.01])) if self.smooth else None

    def states(self, carried=False):
        rng = np.random.default_rng(8)
        if carried:
            return [_f32(rng.standard_normal((self.K, self.E))), np.ones(self.K, np.int32),
                    _f32(rng.standard_normal((self.K, self.E))), np.ones(self.K, np.int32)]
        return [np.full((self.K, self.E), np.nan, np.float32), np.zeros(self.K, np.int32),
                np.full((self.K, self.E), np.nan, np.float32), np.zeros(self.K, np.int32)]

    @property
    def flags(self):
        """the positions of the flags in the state that the call reads and writes"""
        return tuple(i for i, on in ((1, self.relative), (3, self.smooth)) if on)

    def blank(self, m):
        return [np.full((m, self.E), np.nan, np.float32)]

    def clear(self, st, k):
        for i in self.flags:
            st[i][k] = 0

    def _sl(self, a, rows):
        return None if a is None else a[rows]

    def unmasked(self, idx, st):
        return [hostglue.expression_controls(self.values[idx], self.so[idx], self.neutral, self._sl(self.gain, idx), self._sl(self.offset, idx),
                                             *st, self.relative, self.momentum)]

    def restated(self, st, rows=slice(None)):
        restart, present = self.masks(rows)
        return [hostglue.expression_controls(self.values[rows], self.so[rows], self.neutral, self._sl(self.gain, rows),
                                             self._sl(self.offset, rows), *st, self.relative, self.momentum, restart=restart, present=present)]


# (source, gain, rot_off, trans_off, zoom, relative, frontal): everything on, every control alone, gain absent against present
_ON = dict(source=True, gain=True, rot_off=True, trans_off=True, zoom=True, relative=True, frontal=False)
_OFF = dict(source=False, gain=False, rot_off=False, trans_off=False, zoom=False, relative=False, frontal=False)
POSE_COMBOS = [_ON, dict(_ON, relative=False, frontal=True), dict(_ON, gain=False), dict(_OFF, source=True, relative=True),
               dict(_OFF, source=True, gain=True), dict(_OFF, rot_off=True), dict(_OFF, trans_off=True), dict(_OFF, zoom=True),
               dict(_OFF, frontal=True), dict(_OFF, source=True, gain=True, relative=True), _OFF]


class PoseCase(_Case):
    """emo_head_pose_controls_tracks_f32: scale [n,cols], rotation, translation [n,3], state (anchor [K,9], has_anchor [K]); the
    outputs are the edited rows [n,9] (theta is emo_pose_theta_f32 of them: the tests form it with the library at hand)"""
    kind = "pose"

    def __init__(self, combo, cols=3, n=37, K=3, seed=0, masked=True):
        self._init(n, K, seed, masked)
        rng = np.random.default_rng(3000 + seed)
        n = self.n
        self.combo, self.relative, self.frontal = combo, combo["relative"], combo["frontal"]
        self.scale = _f32(1 + 0.1 * rng.standard_normal((n, cols)))
        self.rotation = _f32(1.5 * rng.standard_normal((n, 3)))                            # beyond -pi/2 and beyond pi
        self.translation = _f32(0.1 * rng.standard_normal((n, 3)))
        self.source = None
        if combo["source"]:
            self.source = _f32(np.concatenate([1 + 0.1 * rng.standard_normal((K, 3)), 1.2 * rng.standard_normal((K, 3)),
                                               0.1 * rng.standard_normal((K, 3))], axis=1))
        self.gain = _f32(rng.uniform(0.0, 2.0, n)) if combo["gain"] else None
        self.rot_off = _f32(0.3 * rng.standard_normal((n, 3))) if combo["rot_off"] else None
        self.trans_off = _f32(0.05 * rng.standard_normal((n, 3))) if combo["trans_off"] else None
        self.zoom = _f32(rng.uniform(0.5, 2.0, n)) if combo["zoom"] else None

    def states(self, carried=False):
        rng = np.random.default_rng(9)
        if carried:
            anchor = np.concatenate([1 + 0.1 * rng.standard_normal((self.K, 3)), 0.8 * rng.standard_normal((self.K, 3)),
                                     0.1 * rng.standard_normal((self.K, 3))], axis=1)
            return [_f32(anchor), np.ones(self.K, np.int32)]
        return [np.full((self.K, 9), np.nan, np.float32), np.zeros(self.K, np.int32)]

    @property
    def flags(self):
        return (1,) if self.relative else ()

    def blank(self, m):
        return [np.full((m, 9), np.nan, np.float32)]

    def clear(self, st, k):
        if self.relative:
            st[1][k] = 0

    def args(self, rows):
        sl = lambda a: None if a is None else np.ascontiguousarray(a[rows])
        return [sl(a) for a in (self.scale, self.rotation, self.translation, self.so)] + [self.source] + \
               [sl(a) for a in (self.gain, self.rot_off, self.trans_off, self.zoom)]

    def _state(self, st):
        return st if self.relative else (None, None)

    def unmasked(self, idx, st):
        return [hostglue.head_pose_controls(*self.args(idx), *self._state(st), self.relative, self.frontal, K=self.K)[0]]

    def restated(self, st, rows=slice(None)):
        restart, present = self.masks(rows)
        return [hostglue.head_pose_controls(*self.args(rows), *self._state(st), self.relative, self.frontal, K=self.K, restart=restart,
                                            present=present)[0]]


def scan_cases():
    return [ScanCase(seed=s) for s in (0, 1)]


def expr_cases():
    return [ExprCase(E, combo, seed=10 * s + E) for s, combo in enumerate(EXPR_COMBOS) for E in (5, 130)]


def pose_cases():
    out = [PoseCase(combo, cols, seed=20 * s + cols) for s, combo in enumerate(POSE_COMBOS) for cols in (1, 3)]
    # more rows in a stream than the block has threads: a thread takes several rows, segments straddle its stride
    return out + [PoseCase(combo, 3, n=150, K=2, seed=500 + s) for s, combo in enumerate((POSE_COMBOS[0], POSE_COMBOS[3]))]


def same_bits(a, b):
    return np.array_equal(_f32(a).view(np.uint32), _f32(b).view(np.uint32))


def same_states(case, a, b):
    """flags equal; the state values of the streams whose flag is set equal bit for bit (the others mean nothing)"""
    for i in case.flags:
        if not np.array_equal(a[i], b[i]) or not same_bits(a[i - 1][a[i] != 0], b[i - 1][b[i] != 0]):
            return False
    return True
