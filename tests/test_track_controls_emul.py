"""The control streams that follow face tracks, without a GPU: emo_theta_ema_scan_tracks_f32, emo_expr_controls_tracks_f32 and
emo_head_pose_controls_tracks_f32 (csrc/smallops.hip), compiled for the host from the product's own source (tests/emul/emulibs.stream,
the sequential and the threaded build), on the cases of tests/track_controls_cases.py: against the masked restatements of
emoportraits_amd.hostglue bit for bit; with both masks NULL against the entry points without masks; and the restatements against
an independent plain loop over the unmasked hostglue functions.  Then ops' checks and InferenceWrapper.animate_frames(tracking=
dict(follow_tracks=True)) on the bare-wrapper rig with the counting library: the masks are the tracker's own, the launches are the
new entry points', the rows driven are the restatement's, and one, two and three ranks drive the same rows.  No tolerances."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import track_controls_cases as C  # noqa: E402
from bare_wrapper import bare_wrapper, host_uploads  # noqa: E402
from counting_lib import CountingLib  # noqa: E402

V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
OLD = {"scan": "emo_theta_ema_scan_f32", "expr": "emo_expr_controls_f32", "pose": "emo_head_pose_controls_f32"}
NEW = {"scan": "emo_theta_ema_scan_tracks_f32", "expr": "emo_expr_controls_tracks_f32", "pose": "emo_head_pose_controls_tracks_f32"}
# the argument types in front of the masks, and behind them
FRONT = {"scan": [V] * 4 + [I, I, F, F], "expr": [V] * 9 + [I] * 5 + [F, F], "pose": [V, I] + [V] * 10 + [I] * 4}
BACK = {"scan": [V, V], "expr": [V, V], "pose": [V, V, V]}
ARGTYPES = {NEW[k]: FRONT[k] + [V, V] + BACK[k] for k in NEW}
ARGTYPES.update({OLD[k]: FRONT[k] + BACK[k] for k in OLD})


@pytest.fixture(scope="module", params=[False, True], ids=["loop", "threads"])
def stream(request):
    import emulibs
    return emulibs.stream(request.param)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _m(momentum):
    return (0.0, 0.0) if momentum is None else (float(np.float32(momentum)), float(np.float32(1 - momentum)))


def front_args(c, st, rows):
    """the arguments of a case's entry point in front of the masks, for the rows `rows`, and the number of rows"""
    sl = lambda a: None if a is None else np.ascontiguousarray(a[rows])
    so = sl(c.so)
    n = so.shape[0]
    if c.kind == "scan":
        return [sl(c.values), so, st[0], st[1], n, c.K, *_m(c.momentum)], n
    if c.kind == "expr":
        an, ha = (st[0], st[1]) if c.relative else (None, None)
        em, he = (st[2], st[3]) if c.smooth else (None, None)
        return [sl(c.values), so, c.neutral, sl(c.gain), sl(c.offset), an, ha, em, he, n, c.K, c.E, int(c.relative), int(c.smooth),
                *_m(c.momentum)], n
    an, ha = (st[0], st[1]) if c.relative else (None, None)
    scale = sl(c.scale)
    return [scale, scale.shape[1], sl(c.rotation), sl(c.translation), so, c.source, sl(c.gain), sl(c.rot_off), sl(c.trans_off), sl(c.zoom),
            an, ha, n, c.K, int(c.relative), int(c.frontal)], n


def launch(lib, c, st, rows=slice(None), entry="new", rc=0):
    """one call of the case's entry point on numpy arrays (entry 'new': with the case's masks; 'old': the entry point without
    masks), the outputs pre-filled with NaN -> [the output rows, theta for the head pose]"""
    args, n = front_args(c, st, rows)
    name = (NEW if entry == "new" else OLD)[c.kind]
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = ARGTYPES[name], ctypes.c_int
    outs = c.blank(n) + ([np.full((n, 16), np.nan, np.float32)] if c.kind == "pose" else [])
    keep = [a for a in args if isinstance(a, np.ndarray)]                     # (alive across the call)
    masks = list(c.masks(rows)) if entry == "new" else []
    assert fn(*[_p(a) if isinstance(a, np.ndarray) or a is None else a for a in args], *[_p(a) for a in masks], *[_p(o) for o in outs],
              None) == rc, (name, len(keep))
    return outs


def pose_theta(lib, rows):
    fn = lib.emo_pose_theta_f32
    fn.argtypes, fn.restype = [V, I, V, V, V, I, V], ctypes.c_int
    s, r, t = (np.ascontiguousarray(rows[:, i:i + 3], np.float32) for i in (0, 3, 6))
    out = np.full((rows.shape[0], 16), np.nan, np.float32)
    assert fn(_p(s), 3, _p(r), _p(t), _p(out), rows.shape[0], None) == 0
    return out


ALL = C.scan_cases() + C.expr_cases() + C.pose_cases()
_id = lambda c: f"{c.kind}-{getattr(c, 'E', '')}{getattr(c, 'combo', '')}-n{c.n}"


# ---- 1. the cases, and the restatement against the plain loop -----------------------------------------------------------------------
def test_the_cases_hold_what_they_are_there_for():
    assert len(C.EXPR_COMBOS) == 20 and len(C.POSE_COMBOS) == 11 and len(ALL) == 2 + 40 + 24
    for c in ALL:
        K, rows = c.K, lambda k, lo=0: [i for i in range(lo, c.n) if c.so[i] == k]
        assert c.n == (41 if K == 3 else 154) and (c.so == -1).sum() == 2 and (c.so == K).sum() == 2
        assert c.present[rows(0)[0]] == 0 and c.restart[rows(0)[0]] == 0
        assert c.restart[rows(1)[-1]] == 1 and c.present[rows(1)[-1]] == 0
        assert K == 2 or c.restart[rows(2)[0]] == 1 == c.restart[rows(2, c.cut)[0]]
        assert 0 < c.cut < c.n and all(rows(k, c.cut) and rows(k)[0] < c.cut for k in range(K))
        assert c.restart.sum() >= 4 and 8 <= c.present.sum() <= c.n - 4
    big = [c for c in ALL if c.n == 154]
    assert len(big) == 2 and all(min((c.so == k).sum() for k in range(2)) > 64 for c in big)
    # a flag that came in as 1 leaves as 0
    c = ALL[0]
    for statement in (c.plain, c.restated):
        st = c.states(carried=True)
        statement(st)
        assert st[1][1] == 0


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_the_restatement_is_the_plain_loop_over_the_unmasked_functions(c):
    """outputs of every row (the absent ones included), flags and the state under a set flag: fresh and carried states, one call
    and two; the rows of no stream stay unwritten"""
    for carried in (False, True):
        a, b = c.states(carried), c.states(carried)
        want, got = c.plain(a), c.restated(b)
        assert C.same_bits(got[0], want[0]) and C.same_states(c, a, b), carried
        live = c.live()
        assert np.isnan(got[0][~live]).all() and not np.isnan(got[0][live]).any()
        two, plain_two = c.states(carried), c.states(carried)
        parts = [c.restated(two, r)[0] for r in c.halves()]
        assert C.same_bits(np.concatenate(parts), want[0]) and C.same_states(c, two, a)
        parts = [c.plain(plain_two, r)[0] for r in c.halves()]
        assert C.same_bits(np.concatenate(parts), want[0]) and C.same_states(c, plain_two, a)


def test_the_masks_change_something_and_only_where_there_is_state():
    changed = {}
    for c in ALL:
        with_masks = c.restated(c.states())[0]
        restart, present = c.restart, c.present
        c.restart = c.present = None
        try:
            without = c.restated(c.states())[0]
        finally:
            c.restart, c.present = restart, present
        changed.setdefault((c.kind, bool(c.flags)), []).append(not C.same_bits(with_masks, without))
    assert all(changed[("scan", True)]) and all(changed[("expr", True)]) and all(changed[("pose", True)])
    assert not any(changed[("expr", False)]) and not any(changed[("pose", False)])


# ---- 2. the kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=_id)
def test_kernel_is_the_restatement(stream, c):
    for carried in (False, True):
        host, dev, two = c.states(carried), c.states(carried), c.states(carried)
        want = c.restated(host)[0]
        got = launch(stream, c, dev)
        assert C.same_bits(got[0], want) and C.same_states(c, dev, host), carried
        parts = [launch(stream, c, two, r) for r in c.halves()]
        assert C.same_bits(np.concatenate([p[0] for p in parts]), want) and C.same_states(c, two, host), carried
        live = c.live()
        assert np.isnan(got[0][~live]).all() and np.isfinite(got[0][live]).all()
        if c.kind == "pose":
            assert np.isnan(got[1][~live]).all() and C.same_bits(got[1][live], pose_theta(stream, got[0][live]))


def test_out_may_be_values_for_the_expression_controls(stream):
    for c in C.expr_cases()[-4:]:
        host, dev = c.states(True), c.states(True)
        want = c.restated(host)[0]
        args, n = front_args(c, dev, slice(None))
        fn = getattr(stream, NEW["expr"])
        fn.argtypes, fn.restype = ARGTYPES[NEW["expr"]], ctypes.c_int
        inplace = args[0]
        assert fn(*[_p(a) if isinstance(a, np.ndarray) or a is None else a for a in args], _p(c.restart), _p(c.present), _p(inplace), None) == 0
        live = c.live()
        assert C.same_bits(inplace[live], want[live]) and C.same_states(c, dev, host)


@pytest.mark.parametrize("c", ALL[::3], ids=_id)
def test_null_masks_are_the_entry_point_without_masks(stream, c):
    """both masks NULL: outputs and state bit for bit the existing entry point and the unmasked restatement; one mask alone is the
    other at its default"""
    restart, present = c.restart, c.present
    try:
        c.restart = c.present = None
        for carried in (False, True):
            null, old, host = c.states(carried), c.states(carried), c.states(carried)
            want = c.restated(host)[0]
            got, was = launch(stream, c, null), launch(stream, c, old, entry="old")
            assert all(C.same_bits(g, w) for g, w in zip(got, was)) and C.same_bits(got[0], want)
            assert C.same_states(c, null, old) and C.same_states(c, null, host)
            plain = c.states(carried)
            for k in range(c.K):                                                # the unmasked function, stream by stream
                idx = [i for i in range(c.n) if c.so[i] == k]
                assert C.same_bits(c.unmasked(idx, plain)[0], want[idx])
            assert C.same_states(c, plain, host)
        c.restart, c.present = restart, None
        every = np.ones(c.n, np.int32)
        a, b = c.states(True), c.states(True)
        one = launch(stream, c, a)[0]
        c.present = every
        assert C.same_bits(one, launch(stream, c, b)[0]) and C.same_states(c, a, b)
        c.restart, c.present = None, present
        a, b = c.states(True), c.states(True)
        one = launch(stream, c, a)[0]
        c.restart = np.zeros(c.n, np.int32)
        assert C.same_bits(one, launch(stream, c, b)[0]) and C.same_states(c, a, b)
    finally:
        c.restart, c.present = restart, present


def test_the_refusals_are_the_siblings(stream):
    """what the entry points without masks refuse, the new ones refuse, before anything is written"""
    scan, expr, pose = C.ScanCase(seed=3), C.ExprCase(5, (True,) * 5, seed=3), C.PoseCase(C.POSE_COMBOS[0], seed=3)

    def refused(c, change):
        st = c.states()
        args, n = front_args(c, st, slice(None))
        outs = c.blank(n) + ([np.full((n, 16), np.nan, np.float32)] if c.kind == "pose" else [])
        args = [_p(a) if isinstance(a, np.ndarray) or a is None else a for a in args] + [_p(c.restart), _p(c.present)] + [_p(o) for o in outs]
        for at, v in change.items():
            args[at] = v
        fn = getattr(stream, NEW[c.kind])
        fn.argtypes, fn.restype = ARGTYPES[NEW[c.kind]], ctypes.c_int
        rc = fn(*args, None)
        assert all(np.isnan(o).all() for o in outs) and not any(st[i].any() for i in c.flags)
        return rc
    for change in ({0: None}, {2: None}, {3: None}, {10: None}, {4: 0}, {5: 0}, {4: -1}):
        assert refused(scan, change) == -1, change
    for change in ({0: None}, {18: None}, {9: 0}, {10: 0}, {11: 0}, {2: None}, {5: None}, {6: None}, {7: None}, {8: None}):
        assert refused(expr, change) == -1, change
    for change in ({0: None}, {2: None}, {3: None}, {18: None}, {19: None}, {12: 0}, {13: 0}, {1: 2}, {5: None}, {10: None}, {11: None},
                   {15: 1}):
        assert refused(pose, change) == -1, change


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_in_the_header_and_the_abi_table():
    from emoportraits_amd import _abi_version, hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "ABI 26." in hdr and all(f"int {name}(" in hdr for name in NEW.values())
    assert _abi_version.EMO_ABI_VERSION >= 26 and "#define EMO_ABI_VERSION %d" % _abi_version.EMO_ABI_VERSION in hdr
    for name, types in ARGTYPES.items():
        assert list(hip.SIGNATURES[name]) == types, name


# ---- 4. ops and the wrapper on the bare-wrapper rig ----------------------------------------------------------------------------------
ASSIGN, RESTARTS = "emo_track_assign_f64", "emo_crop_track_restarts_f64"
E5 = 5


class _BothBuilds:
    """the association from the threaded build (its argmax is a wave exchange), every other entry point from the loop build"""

    def __init__(self, loop, threads):
        self._loop, self._threads = loop, threads

    def __getattr__(self, name):
        return getattr(self._threads if name == ASSIGN else self._loop, name)


@pytest.fixture()
def rig(monkeypatch):
    """a wrapper on CPU tensors with a 3-slot bank whose identities have a source expression and a source pose; the crops through
    the host-compiled kernels, the head pose and the expression fixed functions of the crop (recorded), the driver pass a recorder;
    every call of the three control ops is written down with its masks"""
    import emulibs
    from emoportraits_amd import ops
    host_uploads(monkeypatch)
    w = bare_wrapper(monkeypatch, CountingLib(_BothBuilds(emulibs.stream(False), emulibs.stream(True))), 3)
    g = torch.Generator().manual_seed(70)
    w.sources = torch.cat([1 + 0.1 * torch.randn(3, 3, generator=g), 0.4 * torch.randn(3, 3, generator=g), 0.05 * torch.randn(3, 3, generator=g)], 1)
    w.neutrals = torch.randn(3, E5, generator=g)
    for k in range(3):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4), w.neutrals[k], w.sources[k])
    w._canonical_cl = torch.zeros(1, 2, 2, 2, 4)
    w.regressed, w.embedded, w.seen = [], [], {"scan": [], "expr": [], "pose": []}

    def head_pose(crops):
        f = crops.flatten(1)[:, 3::17][:, :9] - 0.5
        srt = (1 + 0.2 * f[:, 0:3]).contiguous(), (4.0 * f[:, 3:6]).contiguous(), (0.2 * f[:, 6:9]).contiguous()
        w.regressed.append(torch.cat(srt, 1))
        return (ops.pose_theta(*srt),) + srt

    def expression(crops, theta, what):
        e = (crops.flatten(1)[:, 5::31][:, :E5] * 4 - 2).contiguous()
        w.embedded.append(e.clone())
        return e, None
    w._head_pose, w._expression = head_pose, expression

    def spy(kind, name, first):
        real = getattr(ops, name)

        def call(*args, **kw):
            rows = args[0] if first is None else torch.cat(args[:3], 1)
            w.seen[kind].append((rows.clone(), kw.get("restart"), kw.get("present")))
            return real(*args, **kw)
        monkeypatch.setattr(ops, name, call)
    spy("scan", "theta_ema_scan", None), spy("expr", "expression_controls", None), spy("pose", "head_pose_controls", 3)
    return w


def _clip(n, hw, seed):
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _box(cx, cy, half):
    return [cx - half, cy - half, cx + half, cy + half]


def birth_clip(N=12, W=128, H=96):
    """face A in frames 0 ... 3 (detection row 1), nobody in frames 4 ... 6, face C from frame 7 (row 2) -- with max_missed = 2 A's
    track dies in frame 6 and C is born into its slot; a second face B all along (row 0 or 3), which the detector drops in frames 2
    and 3.  -> dets [N,4,4]"""
    dets = np.full((N, 4, 4), np.nan)
    for t in range(N):
        if t < 4:
            dets[t, 1] = _box(40 + t, 44 - t, 14)
        if t >= 7:
            dets[t, 2] = _box(44 - t, 50 + t % 3, 16)
        if t not in (2, 3):
            dets[t, 0 if t % 2 else 3] = _box(96 - t, 40 + t, 12)
    return dets


CONTROLS = dict(smooth_pose=True, smooth_per_identity=True, expression=dict(relative=True, smooth=True, momentum=0.4, gain=1.5),
                head_pose=dict(relative=True, gain=0.8))
TRACKING = dict(tracks=2, min_iou=0.2, max_missed=2, smooth=True, momentum=0.5)


def _drive(w, frames, dets, **kw):
    """-> the rows the driver pass was handed, in order: (pose [rows,E], theta [rows,16]) as numpy"""
    w.recorded.clear(), w.regressed.clear(), w.embedded.clear()
    for v in w.seen.values():
        v.clear()
    w.lib.calls.clear()
    for _ in w.animate_frames(frames, detections=dets, to_host=False, as_uint8=False, **kw):
        pass
    return torch.cat([r[0] for r in w.recorded]).numpy(), torch.cat([r[1] for r in w.recorded]).numpy().reshape(-1, 16)


def _reset(w):
    w.reset_crop_state(), w.reset_pose_state(), w.reset_expression_state()


def _tracker(dets, W, H):
    """hostglue's account of the chunk: restart [rows], present [rows] as the wrapper must form them"""
    from emoportraits_amd import hostglue
    N = dets.shape[0]
    ref, age = np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32)
    boxes, restart, _ = hostglue.track_assign(dets, None, ref, age, min_iou=0.2, max_missed=2)
    st = np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros((2, 4), np.int32)
    _, paste, _ = hostglue.crop_track(boxes.reshape(-1, 4), np.tile(np.int32([0, 1]), N), (W, H), *st, restart=restart.reshape(-1),
                                      smooth=True, momentum=0.5)
    return restart.reshape(-1).astype(np.int32), (paste[:, 2] > 0).astype(np.int32)


def test_follow_tracks_hands_the_trackers_masks_to_the_new_entry_points(rig):
    """the birth clip in batches of two frames: `present` is the tracker's paste window having a side, `restart` track_assign's;
    one launch per batch of the masked head-pose and expression entry points and one per chunk of the masked scan (smooth_pose
    scans a chunk in one launch), none of the entry points without masks; the rows driven are the masked restatements of what the
    embedders returned; batch size and chunking do not matter; without the field the launches are the old ones"""
    from emoportraits_amd import hostglue
    w, N, (H, W) = rig, 12, (96, 128)
    clip, dets = _clip(N, (H, W), 31), birth_clip()
    restart, present = _tracker(dets, W, H)
    assert restart.reshape(N, 2)[:, 0].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0] and restart.reshape(N, 2)[:, 1].tolist() == [1] + [0] * 11
    assert present.reshape(N, 2)[:, 0].tolist() == [1] * 4 + [0] * 3 + [1] * 5 and present.reshape(N, 2)[:, 1].tolist() == [1, 1, 0, 0] + [1] * 8
    ids, td = [0, 2] * N, torch.from_numpy(dets)
    _reset(w)
    pose, theta = _drive(w, clip, td, tracking=dict(TRACKING, follow_tracks=True), identities=ids, batch_size=4, **CONTROLS)
    calls = dict(w.lib.calls)
    assert calls[NEW["pose"]] == 6 and calls[NEW["expr"]] == 6 and calls[NEW["scan"]] == 1 and not any(name in calls for name in OLD.values())
    assert calls[ASSIGN] == 1 and calls[RESTARTS] == 1
    for kind in ("scan", "expr", "pose"):
        assert torch.cat([s[1] for s in w.seen[kind]]).tolist() == restart.tolist(), kind
        assert torch.cat([s[2] for s in w.seen[kind]]).tolist() == present.tolist(), kind
    assert w.tracked_present[0].tolist() == present.tolist() and w.tracked_present[1] == 0 and w.tracked_present[0].dtype == torch.int32
    assert w.tracked_assignment[1].reshape(-1).tolist() == restart.tolist()
    # the rows driven: the masked restatements of what the embedders returned, every identity its own stream
    srt, emb, so = torch.cat(w.regressed).numpy(), torch.cat(w.embedded).numpy(), np.int32(ids)
    n = 2 * N
    rows, _ = hostglue.head_pose_controls(srt[:, 0:3], srt[:, 3:6], srt[:, 6:9], so, w.sources.numpy(), np.full(n, 0.8, np.float32), None, None, None,
                                          np.zeros((3, 9), np.float32), np.zeros(3, np.int32), True, False, restart=restart, present=present)
    edited = pose_theta(w.lib._lib, rows)
    want_theta = hostglue.ema_scan_tracks(edited, so, np.zeros((3, 16), np.float32), np.zeros(3, np.int32), 0.3, restart, present)
    want_pose = hostglue.expression_controls(emb, so, w.neutrals.numpy(), np.full(n, 1.5, np.float32), None, np.zeros((3, E5), np.float32),
                                             np.zeros(3, np.int32), np.zeros((3, E5), np.float32), np.zeros(3, np.int32), True, 0.4,
                                             restart=restart, present=present)
    assert C.same_bits(theta, want_theta) and C.same_bits(pose, want_pose)
    assert w._bank_streams.theta_has.tolist() == [1, 0, 1] and w._bank_streams.pose_anchor_has.tolist() == [1, 0, 1]
    for kw in (dict(frames=clip, detections=td, batch_size=2), dict(frames=clip, detections=td, batch_size=16),
               dict(frames=iter([clip[:5], clip[5:7], clip[7:]]), detections=td, batch_size=4),
               dict(frames=iter([clip[:7], clip[7:]]), detections=iter([td[:7], td[7:]]), batch_size=6)):
        _reset(w)
        got = _drive(w, kw.pop("frames"), kw.pop("detections"), tracking=dict(TRACKING, follow_tracks=True), identities=ids, **kw, **CONTROLS)
        assert C.same_bits(got[0], pose) and C.same_bits(got[1], theta), kw
    # the field absent or False: the launches of the entry points without masks, the same in both, and other rows
    runs = []
    for tracking in (TRACKING, dict(TRACKING, follow_tracks=False)):
        _reset(w)
        w.tracked_present = None
        runs.append(_drive(w, clip, td, tracking=tracking, identities=ids, batch_size=4, **CONTROLS))
        runs.append(dict(w.lib.calls))
        assert w.lib.calls[OLD["pose"]] == 6 and w.lib.calls[OLD["expr"]] == 6 and w.lib.calls[OLD["scan"]] == 1
        assert not any(name in w.lib.calls for name in NEW.values()) and w.tracked_present is None
        assert all(s[1] is None and s[2] is None for v in w.seen.values() for s in v)
    assert runs[1] == runs[3] and C.same_bits(runs[0][0], runs[2][0]) and C.same_bits(runs[0][1], runs[2][1])
    assert {OLD[k]: v for k, v in ((k, calls[NEW[k]]) for k in NEW)} == {name: runs[1][name] for name in OLD.values()}
    assert {k: v for k, v in calls.items() if k not in NEW.values()} == {k: v for k, v in runs[1].items() if k not in OLD.values()}
    assert not C.same_bits(runs[0][0], pose) and not C.same_bits(runs[0][1], theta)


def test_nothing_more_is_launched_without_a_control_that_carries_state(rig):
    w, N, (H, W) = rig, 6, (96, 128)
    clip, td = _clip(N, (H, W), 32), torch.from_numpy(birth_clip()[:N])
    kw = dict(identities=[0, 2] * N, batch_size=4, expression=dict(gain=1.5, offset=torch.ones(E5)), head_pose=dict(frontal=True, zoom=1.1), mix=True)
    _reset(w)
    plain = _drive(w, clip, td, tracking=TRACKING, **kw)
    before = dict(w.lib.calls)
    _reset(w)
    got = _drive(w, clip, td, tracking=dict(TRACKING, follow_tracks=True), **kw)
    assert dict(w.lib.calls) == before and not any(name in before for name in NEW.values())
    assert C.same_bits(got[0], plain[0]) and C.same_bits(got[1], plain[1])
    # ordered boxes have no births: present alone
    boxes = torch.from_numpy(np.stack([np.array(_box(40 + t, 44, 14)) if t != 2 else np.full(4, np.nan) for t in range(N)]))
    w.pred_source_srt, w.pred_source_pose_embed = w.sources[1][None], w.neutrals[1][None]
    w.recorded.clear()
    for v in w.seen.values():
        v.clear()
    _reset(w)
    for _ in w.animate_frames(clip, boxes=boxes, tracking=dict(follow_tracks=True), batch_size=4, to_host=False, as_uint8=False, smooth_pose=True,
                              head_pose=dict(relative=True)):
        pass
    for kind in ("scan", "pose"):
        assert all(s[1] is None for s in w.seen[kind]) and torch.cat([s[2] for s in w.seen[kind]]).tolist() == [1, 1, 0, 1, 1, 1]


def test_errors_come_before_any_launch(rig):
    from emoportraits_amd import ops
    w, N, (H, W) = rig, 4, (96, 128)
    clip = _clip(N, (H, W), 33)
    w.lib.calls.clear()
    boxes = torch.tensor([_box(40.0, 44.0, 14.0)] * N, dtype=torch.float64)
    with pytest.raises(ValueError, match="follow_tracks"):
        next(w.animate_streams([dict(frames=clip, boxes=boxes)], tracking=dict(follow_tracks=True)))
    with pytest.raises(ValueError, match="boxes= is missing"):
        next(w.animate_frames(clip, tracking=dict(follow_tracks=True)))
    with pytest.raises(ValueError, match="no field"):
        next(w.animate_frames(clip, boxes=boxes, tracking=dict(follow_track=True)))
    n, K = 6, 2
    values, state, has = torch.zeros(n, 4, 4), torch.zeros(K, 4, 4), torch.zeros(K, dtype=torch.int32)
    ok = torch.ones(n, dtype=torch.int32)
    bad = [(ok.long(), "int32"), (ok[:5], "contiguous"), (torch.ones(2 * n, dtype=torch.int32)[::2], "contiguous"), (ok.reshape(n, 1), "contiguous"),
           ([1] * n, "int32")]
    for which in ("restart", "present"):
        for mask, match in bad:
            with pytest.raises(ValueError, match=f"{which}.*{match}|{match}.*{which}"):
                ops.theta_ema_scan(values, None, state, has, 0.3, **{which: mask})
            with pytest.raises(ValueError, match=which):
                ops.expression_controls(torch.zeros(n, E5), None, ema=torch.zeros(1, E5), has_ema=has[:1], momentum=0.5, **{which: mask})
            with pytest.raises(ValueError, match=which):
                ops.head_pose_controls(torch.ones(n, 3), torch.zeros(n, 3), torch.zeros(n, 3), **{which: mask})
    assert not w.lib.calls
    ops.theta_ema_scan(values, None, state, has, 0.3, restart=ok)
    ops.head_pose_controls(torch.ones(n, 3), torch.zeros(n, 3), torch.zeros(n, 3), present=ok)
    assert dict(w.lib.calls) == {NEW["scan"]: 1, NEW["pose"]: 1}


def test_one_two_and_three_ranks_drive_the_same_rows(rig, monkeypatch):
    """the birth clip (a birth, a death and a dropout in one chunk) on 1, 2 and 3 ranks: every rank tracks the whole chunk and runs
    the three controls over all its rows, so the rows a rank drives are the one-rank run's, bit for bit.  The gather of the other
    ranks' rows is a stand-in that hands out the one-rank run's rows after checking the rank's own share against them."""
    from emoportraits_amd import parallel
    w, N, (H, W) = rig, 12, (96, 128)
    clip, td, ids = _clip(N, (H, W), 31), torch.from_numpy(birth_clip()), [0, 2] * N
    kw = dict(tracking=dict(TRACKING, follow_tracks=True), identities=ids, batch_size=4, **CONTROLS)
    _reset(w)
    pose, theta = _drive(w, clip, td, **kw)
    whole = {(9,): torch.cat([s[0] for s in w.seen["pose"]]), (4, 4): w.seen["scan"][0][0].clone(), (E5,): torch.cat([s[0] for s in w.seen["expr"]])}
    state = [t.clone() for t in (w._bank_streams.theta, w._bank_streams.theta_has, w._bank_streams.pose_anchor, w._bank_streams.pose_anchor_has,
                                 w._bank_streams.expr_anchor, w._bank_streams.expr_anchor_has, w._bank_streams.expr_ema, w._bank_streams.expr_ema_has)]
    gathers = []

    def gather_rows(local, counts, rank, world):
        full = whole[tuple(local.shape[1:])]
        lo = sum(counts[:rank])
        assert full.shape[0] == sum(counts) and torch.equal(local.view(torch.int32), full[lo:lo + counts[rank]].view(torch.int32))
        gathers.append(tuple(local.shape[1:]))
        return full.clone()
    monkeypatch.setattr(parallel, "gather_rows", gather_rows)
    for world in (2, 3):
        parts = []
        for rank in range(world):
            _reset(w)
            gathers.clear()
            w.rank, w.world = rank, world
            try:
                parts.append(_drive(w, clip, td, **kw))
            finally:
                w.rank, w.world = 0, 1
            assert sorted(gathers) == [(4, 4), (5,), (9,)]
            assert w.lib.calls[NEW["pose"]] == 1 == w.lib.calls[NEW["expr"]] == w.lib.calls[NEW["scan"]] and not any(n in w.lib.calls for n in OLD.values())
            for kind in ("scan", "expr", "pose"):
                assert w.seen[kind][0][1].shape[0] == 2 * N == w.seen[kind][0][2].shape[0]
            now = (w._bank_streams.theta, w._bank_streams.theta_has, w._bank_streams.pose_anchor, w._bank_streams.pose_anchor_has,
                   w._bank_streams.expr_anchor, w._bank_streams.expr_anchor_has, w._bank_streams.expr_ema, w._bank_streams.expr_ema_has)
            for i in (1, 3, 5, 7):
                on = state[i] != 0
                assert torch.equal(now[i], state[i]) and torch.equal(now[i - 1][on].view(torch.int32), state[i - 1][on].view(torch.int32))
        assert C.same_bits(np.concatenate([p[0] for p in parts]), pose) and C.same_bits(np.concatenate([p[1] for p in parts]), theta), world
