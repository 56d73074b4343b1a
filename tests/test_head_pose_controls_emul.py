"""The head-pose controls of the batched entry points without a GPU: emo_head_pose_controls_f32 (csrc/smallops.hip), compiled for
the host from the product's own source (tests/emul/emulibs.stream, the sequential and the threaded build), against the host code
it restates (hostglue.head_pose_controls), bit for bit; its theta bit for bit emo_pose_theta_f32 of the edited rows and within
1e-5 of an fp64 S R T formed here (the bound of test_pose_theta_against_the_reference_golden); InferenceWrapper.animate /
animate_frames / animate_streams(head_pose=) on the recorder rigs of tests/test_expression_controls_emul.py.
"""
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
from bare_wrapper import bare_wrapper as _bare_wrapper, host_uploads  # noqa: E402
from counting_lib import CountingLib as _Lib  # noqa: E402


@pytest.fixture(scope="module", params=[False, True], ids=["loop", "threads"])
def stream(request):
    import emulibs
    return emulibs.stream(request.param)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _bits(a):
    return _f32(a).view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


V, I = ctypes.c_void_p, ctypes.c_int
ARGTYPES = [V, I] + [V] * 10 + [I] * 4 + [V] * 3


def raw(lib, scale, rotation, translation, so, source, gain, rot_off, trans_off, zoom, anchor, has_a, n, K, relative, frontal, out_srt,
        out_theta, cols=None):
    fn = lib.emo_head_pose_controls_f32
    fn.argtypes, fn.restype = ARGTYPES, ctypes.c_int
    cols = (3 if scale is None else scale.shape[1]) if cols is None else cols
    return fn(_p(scale), cols, _p(rotation), _p(translation), _p(so), _p(source), _p(gain), _p(rot_off), _p(trans_off), _p(zoom),
              _p(anchor), _p(has_a), n, K, int(relative), int(frontal), _p(out_srt), _p(out_theta), None)


def pose_theta(lib, rows):
    """emo_pose_theta_f32 of [n,9] rows from the same library"""
    fn = lib.emo_pose_theta_f32
    fn.argtypes, fn.restype = [V, I, V, V, V, I, V], ctypes.c_int
    s, r, t = (_f32(rows[:, i:i + 3]) for i in (0, 3, 6))
    out = np.full((rows.shape[0], 16), np.nan, np.float32)
    assert fn(_p(s), 3, _p(r), _p(t), _p(out), rows.shape[0], None) == 0
    return out


def srt64(rows):
    """S R T of [n,9] rows in float64, the rotation clamped to [-pi/2, pi] (utils/point_transforms.py:188-242)"""
    out = np.zeros((len(rows), 16))
    for i, p in enumerate(np.asarray(rows, np.float64)):
        y, x, z = np.clip(p[3:6], -np.pi / 2, np.pi)
        Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
        Ry = np.array([[np.cos(x), 0, np.sin(x)], [0, 1, 0], [-np.sin(x), 0, np.cos(x)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(z), -np.sin(z)], [0, np.sin(z), np.cos(z)]])
        S, R, T = np.eye(4), np.eye(4), np.eye(4)
        S[:3, :3] = np.diag(p[0:3])
        R[:3, :3] = Rz @ Ry @ Rx
        T[:3, 3] = p[6:9]
        out[i] = (S @ R @ T).reshape(16)
    return out


class Case:
    """seeded inputs of one call: rotations on both sides of the clamp, scales about one, K interleaved streams"""

    def __init__(self, n, K, cols=3, source=True, gain=True, rot_off=True, trans_off=True, zoom=True, relative=True, frontal=False,
                 seed=0, null_streams=False):
        rng = np.random.default_rng(seed)
        self.n, self.K, self.relative, self.frontal = n, K, relative, frontal
        self.scale = _f32(1 + 0.1 * rng.standard_normal((n, cols)))
        self.rotation = _f32(1.5 * rng.standard_normal((n, 3)))                          # beyond -pi/2 and beyond pi
        self.rotation[rng.integers(0, n), 0], self.rotation[rng.integers(0, n), 2] = -2.5, 3.5
        self.translation = _f32(0.1 * rng.standard_normal((n, 3)))
        self.so = None if null_streams else rng.integers(0, K, n).astype(np.int32)
        self.source = None
        if source:
            self.source = _f32(np.concatenate([1 + 0.1 * rng.standard_normal((K, 3)), 1.2 * rng.standard_normal((K, 3)),
                                               0.1 * rng.standard_normal((K, 3))], axis=1))
        self.gain = _f32(rng.uniform(0.0, 2.0, n)) if gain else None
        self.rot_off = _f32(0.3 * rng.standard_normal((n, 3))) if rot_off else None
        self.trans_off = _f32(0.05 * rng.standard_normal((n, 3))) if trans_off else None
        self.zoom = _f32(rng.uniform(0.5, 2.0, n)) if zoom else None

    def states(self):
        return np.full((self.K, 9), np.nan, np.float32), np.zeros(self.K, np.int32)

    def _args(self, rows):
        sl = lambda a: None if a is None else np.ascontiguousarray(a[rows])
        return [sl(a) for a in (self.scale, self.rotation, self.translation, self.so)] + [self.source] + \
               [sl(a) for a in (self.gain, self.rot_off, self.trans_off, self.zoom)]

    def kernel(self, lib, st, rows=slice(None)):
        args = self._args(rows)
        m = args[0].shape[0]
        out, theta = np.full((m, 9), np.nan, np.float32), np.full((m, 16), np.nan, np.float32)
        st = st if self.relative else (None, None)
        assert raw(lib, *args, *st, m, self.K, self.relative, self.frontal, out, theta) == 0
        return out, theta

    def restated(self, st, rows=slice(None)):
        from emoportraits_amd import hostglue
        st = st if self.relative else (None, None)
        return hostglue.head_pose_controls(*self._args(rows), *st, self.relative, self.frontal, K=self.K)


def _same_states(a, b):
    """flags equal; the anchor rows of the streams that have begun equal bit for bit (the others were never written)"""
    return np.array_equal(a[1], b[1]) and _same(a[0][a[1] != 0], b[0][b[1] != 0])


def _check(lib, c, rows=slice(None), a=None, b=None):
    """one call of the kernel and of the restatement from equal states: rows, states, theta"""
    a, b = a or c.states(), b or c.states()
    got, theta = c.kernel(lib, a, rows)
    want, _ = c.restated(b, rows)
    assert _same(got, want) and _same_states(a, b)
    so = None if c.so is None else c.so[rows]
    live = np.ones(len(got), bool) if so is None else (so >= 0) & (so < c.K)
    assert np.isnan(got[~live]).all() and np.isnan(theta[~live]).all() and not np.isnan(got[live]).any()
    if live.any():
        assert _same(theta[live], pose_theta(lib, got[live]))
        assert np.abs(theta[live] - srt64(got[live])).max() <= 1e-5
    return got, theta, a, b


# (source, gain, rot_off, trans_off, zoom, relative, frontal): everything on, every control alone, gain absent against present
ON = dict(source=True, gain=True, rot_off=True, trans_off=True, zoom=True, relative=True, frontal=False)
OFF = dict(source=False, gain=False, rot_off=False, trans_off=False, zoom=False, relative=False, frontal=False)
COMBOS = [ON, dict(ON, relative=False, frontal=True), dict(ON, gain=False), dict(OFF, source=True, relative=True),
          dict(OFF, source=True, gain=True), dict(OFF, rot_off=True), dict(OFF, trans_off=True), dict(OFF, zoom=True),
          dict(OFF, frontal=True), dict(OFF, source=True, gain=True, relative=True), OFF]


@pytest.mark.parametrize("cols", [1, 3])
def test_kernel_is_the_restatement(stream, cols):
    """n = 1; 200 rows over three interleaved streams (more rows than the block has threads); one stream; every control on,
    each alone, gain absent against present; scale in one column and in three"""
    for seed, combo in enumerate(COMBOS):
        _check(stream, Case(200, 3, cols, seed=seed, **combo))
        _check(stream, Case(1, 3, cols, seed=50 + seed, **combo))
        _check(stream, Case(9, 1, cols, seed=100 + seed, null_streams=True, **combo))           # stream_of NULL, K = 1


def test_no_control_is_the_clamped_row_and_its_theta(stream):
    c = Case(40, 1, 3, seed=7, null_streams=True, **OFF)
    got, theta, _, _ = _check(stream, c)
    want = np.concatenate([c.scale, np.clip(c.rotation, np.float32(-np.float32(np.pi) / 2), np.float32(np.pi)), c.translation], axis=1)
    assert _same(got, want)
    raw_rows = np.concatenate([c.scale, c.rotation, c.translation], axis=1)
    assert _same(theta, pose_theta(stream, raw_rows))                                          # (theta clamps once more: the same)


def test_a_stream_without_a_row_and_rows_of_no_stream(stream):
    n, K = 9, 3
    c = Case(n, K, seed=300, **ON)
    c.so = np.int32([0, -1, 2, K, 0, K, -1, 2, 0])
    got, theta, a, b = _check(stream, c)
    assert list(a[1]) == [1, 0, 1] and np.isnan(a[0][1]).all()
    first0 = np.concatenate([c.scale[0], np.clip(c.rotation[0], np.float32(-np.float32(np.pi) / 2), np.float32(np.pi)), c.translation[0]])
    assert _same(a[0][0], first0)                                                               # the anchor: the first row after step 0
    # stream 1 begins in a later call; 0 and 2 keep their anchors and flags
    before = a[0].copy()
    c2 = Case(n, K, seed=301, **ON)
    c2.so = np.int32([1, 1, 0, 2, -1, 1, 0, K, 2])
    _check(stream, c2, a=a, b=b)
    assert list(a[1]) == [1, 1, 1] and _same(a[0][[0, 2]], before[[0, 2]])
    only_off = Case(2, K, seed=302, **ON)
    only_off.so = np.int32([-1, K])
    st = only_off.states()
    got, theta = only_off.kernel(stream, st)
    assert np.isnan(got).all() and np.isnan(theta).all() and not st[1].any() and np.isnan(st[0]).all()


def test_the_anchor_is_carried_across_a_split_at_every_position(stream):
    for K, null in ((1, True), (2, False)):
        c = Case(7, K, seed=400 + K, null_streams=null, **ON)
        whole = c.states()
        want, want_theta = c.kernel(stream, whole)
        for cut in range(1, 7):
            two, host = c.states(), c.states()
            parts = [_check(stream, c, rows, a=two, b=host) for rows in (slice(0, cut), slice(cut, 7))]
            assert _same(np.concatenate([p[0] for p in parts]), want) and _same(np.concatenate([p[1] for p in parts]), want_theta)
            assert _same_states(two, whole)


def test_frontal_zeroes_yaw_pitch_and_translation_exactly(stream):
    c = Case(40, 3, seed=500, **dict(OFF, frontal=True))
    got, _, _, _ = _check(stream, c)
    assert not _bits(got[:, [3, 4, 6, 7, 8]]).any()                                            # +0.0, every bit
    assert _same(got[:, 0:3], c.scale) and _same(got[:, 5], np.clip(c.rotation[:, 2], np.float32(-np.float32(np.pi) / 2), np.float32(np.pi)))
    # with offsets: frontal first, then the deltas (ExpressionEmbed.forward_image: normalize, then delta_yaw / delta_pitch)
    c = Case(40, 3, seed=501, **dict(OFF, frontal=True, rot_off=True))
    got, _, _, _ = _check(stream, c)
    assert _same(got[:, 3:5], c.rot_off[:, 0:2])


def test_refusals_return_bad_arg_and_write_nothing(stream):
    n, K = 4, 2
    c = Case(n, K, seed=600, **ON)
    an, ha = c.states()
    out, theta = np.full((n, 9), np.nan, np.float32), np.full((n, 16), np.nan, np.float32)
    ok = dict(scale=c.scale, rotation=c.rotation, translation=c.translation, so=c.so, source=c.source, gain=c.gain, rot_off=c.rot_off,
              trans_off=c.trans_off, zoom=c.zoom, anchor=an, has_a=ha, n=n, K=K, relative=1, frontal=0, out_srt=out, out_theta=theta)
    bad = [dict(scale=None), dict(rotation=None), dict(translation=None), dict(out_srt=None), dict(out_theta=None), dict(n=0), dict(K=0),
           dict(n=-1), dict(cols=2), dict(cols=0), dict(source=None), dict(source=None, relative=0), dict(anchor=None), dict(has_a=None),
           dict(frontal=1)]
    for change in bad:
        assert raw(stream, **{**ok, **change}) == -1, change
        assert np.isnan(out).all() and np.isnan(theta).all() and np.isnan(an).all() and not ha.any(), change
    assert raw(stream, **ok) == 0 and not np.isnan(out).any()
    assert raw(stream, **{**ok, "relative": 0, "anchor": None, "has_a": None}) == 0
    assert raw(stream, **{**ok, "relative": 0, "source": None, "gain": None, "anchor": None, "has_a": None, "frontal": 1}) == 0


def test_the_entry_point_is_in_the_abi_table():
    from emoportraits_amd import _abi_version, hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "int emo_head_pose_controls_f32(" in hdr and _abi_version.EMO_ABI_VERSION >= 21
    assert len(hip.SIGNATURES["emo_head_pose_controls_f32"]) == len(ARGTYPES)


# ---- ops and the wrapper on the recorder rig of tests/test_expression_controls_emul.py ---------------------------------------------
NAME = "emo_head_pose_controls_f32"
E5 = 5


def _sources(K, seed=70):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([1 + 0.1 * torch.randn(K, 3, generator=g), 0.4 * torch.randn(K, 3, generator=g), 0.05 * torch.randn(K, 3, generator=g)], 1)


def _fill(w, K):
    w.sources = _sources(K)
    for k in range(K):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4), torch.zeros(E5), w.sources[k])
    w._canonical_cl = torch.zeros(1, 2, 2, 2, 4)


@pytest.fixture()
def wrapper(monkeypatch):
    """an InferenceWrapper with a 3-slot bank and everything but the driver pass: that records (pose, theta, identity)"""
    import emulibs
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(True)), 3)
    _fill(w, 3)
    return w


def _drivers(N, seed):
    g = torch.Generator().manual_seed(seed)
    pose = torch.randn(N, E5, generator=g)
    srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.9 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
    return pose, srt


def _run(w, pose, srt, batch_size=4, **kw):
    w.recorded.clear()
    for _ in w.animate(pose, srt, batch_size=batch_size, as_uint8=False, **kw):
        pass
    return torch.cat([r[1] for r in w.recorded]).numpy().reshape(-1, 16), torch.cat([r[0] for r in w.recorded]).numpy()


class HostState:
    """the anchors of K streams for the restatement, carried from call to call as the wrapper's are; -> (rows, the theta the
    package's own emo_pose_theta_f32 forms of them)"""

    def __init__(self, K, lib):
        self.st, self.lib = (np.zeros((K, 9), np.float32), np.zeros(K, np.int32)), lib

    def __call__(self, srt, ids, source=None, gain=None, rot_off=None, trans_off=None, zoom=None, relative=False, frontal=False):
        from emoportraits_amd import hostglue
        n = len(srt[0])
        per_row = lambda v: None if v is None else np.broadcast_to(_f32(v), (n,))
        rows3 = lambda v: None if v is None else np.broadcast_to(_f32(v), (n, 3))
        rows, _ = hostglue.head_pose_controls(*[_f32(t) for t in srt], ids, None if source is None else _f32(source), per_row(gain),
                                              rows3(rot_off), rows3(trans_off), per_row(zoom), *(self.st if relative else (None, None)),
                                              relative, frontal)
        return rows, pose_theta(self.lib._lib, rows)

    def reset(self, k):
        self.st[1][k] = 0


def test_ops_broadcast_scalars_and_three_wide_offsets_to_the_rows(wrapper):
    from emoportraits_amd import ops
    c = Case(40, 3, seed=700, **ON)
    t = lambda a: None if a is None else torch.from_numpy(a)
    anchor, has = torch.zeros(3, 9), torch.zeros(3, dtype=torch.int32)
    rows, theta = ops.head_pose_controls(t(c.scale), t(c.rotation), t(c.translation), t(c.so), t(c.source), 0.5, t(c.rot_off[0]),
                                         t(c.trans_off[0]), 1.25, anchor, has, True, False)
    c.gain, c.zoom = np.full(40, 0.5, np.float32), np.full(40, 1.25, np.float32)
    c.rot_off, c.trans_off = np.tile(c.rot_off[:1], (40, 1)), np.tile(c.trans_off[:1], (40, 1))
    st = c.states()
    want, _ = c.restated(st)
    assert _same(rows.numpy(), want) and theta.shape == (40, 4, 4) and _same(anchor.numpy(), st[0]) and has.tolist() == [1, 1, 1]
    per_row, _ = ops.head_pose_controls(t(c.scale), t(c.rotation), t(c.translation), t(c.so), t(c.source), t(c.gain), t(c.rot_off),
                                        t(c.trans_off), t(c.zoom), torch.zeros(3, 9), torch.zeros(3, dtype=torch.int32), True, False)
    assert _same(per_row.numpy(), want)
    for kw, match in ((dict(zoom=torch.ones(3)), "entries"), (dict(rotation_offset=torch.zeros(4)), r"\[3\]"),
                      (dict(translation_offset=torch.zeros(5, 3)), r"\[3\]"), (dict(relative=True), "source"), (dict(gain=0.5), "source"),
                      (dict(source=t(c.source), relative=True), "anchor"), (dict(frontal=True, relative=True), "frontal")):
        with pytest.raises(ValueError, match=match):
            ops.head_pose_controls(t(c.scale), t(c.rotation), t(c.translation), **kw)
    with pytest.raises(ValueError, match="scale"):
        ops.head_pose_controls(torch.ones(4, 2), torch.zeros(4, 3), torch.zeros(4, 3))


def test_animate_hands_the_restated_thetas_to_the_driver_pass(wrapper):
    """13 frames in batches of 4 over three identities: relative + per-row gain, offsets and zoom, each row about its own slot's
    source pose and within its own slot's stream; a second call carries every slot's anchor on; no dependence on batch_size; a new
    identity in a slot, drop_identity and reset_pose_state restart streams, load_identity restores the source pose"""
    from emoportraits_amd import HeadPoseControls
    w, N = wrapper, 13
    pose, srt = _drivers(N, 3)
    pose2, srt2 = _drivers(N, 4)
    ids = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]
    ids2 = [1, 1, 0, 2, 0, 2, 2, 1, 0, 0, 0, 2, 1]
    g = torch.Generator().manual_seed(9)
    gain, zoom = torch.rand(N, generator=g) * 2, 0.5 + torch.rand(N, generator=g)
    rot, trans = 0.2 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g)
    host = HostState(3, w.lib)
    hp = HeadPoseControls(relative=True, gain=gain, rotation_offset=rot, translation_offset=trans, zoom=zoom)
    want_rows, want = host(srt, ids, w.sources, gain, rot, trans, zoom, True)
    got, poses = _run(w, pose, srt, identities=ids, head_pose=hp)
    assert _same(got, want) and np.array_equal(poses, pose.numpy())
    assert w.lib.calls[NAME] == 1                                               # the whole stream in one launch
    assert _same(torch.cat(w.pred_target_srt, 1).numpy(), want_rows)            # what was rendered with
    # the second call continues each slot's stream (a mapping serves as well as the class; a scalar gain, [3] offsets)
    _, want2 = host(srt2, ids2, w.sources, 0.5, rot[0], None, None, True)
    got2, _ = _run(w, pose2, srt2, identities=ids2, head_pose=dict(relative=True, gain=0.5, rotation_offset=rot[0]))
    assert _same(got2, want2)
    # batch sizes: the same thetas from the same starting state; mix and smooth_pose work on the edited thetas
    saved = w._bank_streams.pose_anchor.clone(), w._bank_streams.pose_anchor_has.clone()
    rows = []
    for bs in (4, 5, 16):
        w._bank_streams.pose_anchor.copy_(saved[0]), w._bank_streams.pose_anchor_has.copy_(saved[1])
        rows.append(_run(w, pose, srt, batch_size=bs, identities=ids, head_pose=hp)[0])
    assert _same(rows[0], rows[1]) and _same(rows[0], rows[2])
    _, edited = host(srt, ids, w.sources, gain, rot, trans, zoom, True)
    assert _same(rows[0], edited)
    from emoportraits_amd import hostglue
    w._bank_streams.pose_anchor.copy_(saved[0]), w._bank_streams.pose_anchor_has.copy_(saved[1])
    w._bank_streams.theta_has.zero_()
    smoothed, _ = _run(w, pose, srt, identities=ids, head_pose=hp, smooth_pose=True, smooth_per_identity=True)
    want_s = np.empty_like(edited)
    for k in range(3):
        sel = [i for i, v in enumerate(ids) if v == k]
        want_s[sel] = hostglue.ema_scan(edited[sel].reshape(-1, 4, 4), None, 0.3)[0].reshape(-1, 16)
    assert _same(smoothed, want_s)
    # a new identity in slot 1, drop + store of slot 2: those streams restart, slot 0 carries on
    w.idt_embed, w.pred_source_theta, w.pred_source_pose_embed = torch.zeros(1, 4, 1, 1), torch.eye(4)[None], None
    w.pred_source_srt = w.sources[1][None] + 0.1
    assert w.store_identity(1) == 1
    w.drop_identity(2)
    assert w._bank_srt_has == [True, True, False]
    w.pred_source_srt = w.sources[2][None]
    assert w.store_identity(2) == 2
    sources = w.sources.clone()
    sources[1] += 0.1
    host.reset(1), host.reset(2)
    got, _ = _run(w, pose2, srt2, identities=ids2, head_pose=hp)
    assert _same(got, host(srt2, ids2, sources, gain, rot, trans, zoom, True)[1])
    w.reset_pose_state([0])
    host.reset(0)
    got, _ = _run(w, pose, srt, identities=ids, head_pose=hp)
    assert _same(got, host(srt, ids, sources, gain, rot, trans, zoom, True)[1])
    w.reset_pose_state()
    assert w._bank_streams.pose_anchor_has.tolist() == [0, 0, 0]
    import emoportraits_amd.ops as ops
    vol = ops.volume_to_channels_first
    try:
        ops.volume_to_channels_first = lambda cl: cl
        w.load_identity(1)
    finally:
        ops.volume_to_channels_first = vol
    assert torch.equal(w.pred_source_srt, sources[1][None])


def test_animate_single_identity_anchor_is_carried_on_the_wrapper(wrapper):
    w, N = wrapper, 13
    w.pred_source_theta = torch.eye(4)[None]
    w.pred_source_srt = w.sources[1][None]
    pose, srt = _drivers(N, 5)
    srt = (srt[0][:, :1].contiguous(), srt[1], srt[2])                          # a one-column scale
    host = HostState(1, w.lib)
    hp = dict(relative=True, gain=1.5, zoom=1.1)
    got, _ = _run(w, pose, srt, head_pose=hp)
    assert _same(got, host(srt, None, w.sources[1:2], 1.5, None, None, 1.1, True)[1])
    got, _ = _run(w, pose[:7], [t[:7] for t in srt], batch_size=5, head_pose=hp)                 # (the anchor of the first call)
    assert _same(got, host([t[:7] for t in srt], None, w.sources[1:2], 1.5, None, None, 1.1, True)[1])
    assert _same(w._stream.pose_anchor[0].numpy(), host.st[0][0])
    w.reset_pose_state()
    assert w._stream.pose_anchor_has.tolist() == [0]
    # offsets, zoom and frontal need neither a source pose nor a state
    w.pred_source_srt = None
    got, _ = _run(w, pose, srt, head_pose=dict(rotation_offset=[0.2, -0.1, 0.0], frontal=True))
    assert _same(got, HostState(1, w.lib)(srt, None, None, None, [0.2, -0.1, 0.0], None, None, False, True)[1]) and w._stream.pose_anchor_has.tolist() == [0]


def test_defaults_launch_nothing_and_change_nothing(wrapper):
    from emoportraits_amd import HeadPoseControls
    w = wrapper
    pose, srt = _drivers(13, 6)
    ids = [0, 1, 2] * 4 + [0]
    kw = dict(identities=ids, mix=True, smooth_pose=True, smooth_per_identity=True)
    runs = []
    for head_pose in ("absent", None, HeadPoseControls(), {}, dict(gain=1.0, zoom=1.0, rotation_offset=None)):
        w.reset_pose_state()
        w.lib.calls.clear()
        runs.append(_run(w, pose, srt, **kw, **({} if head_pose == "absent" else dict(head_pose=head_pose))))
        assert w.lib.calls.get(NAME, 0) == 0 and w._bank_streams.pose_anchor_has.tolist() == [0, 0, 0] and w._stream.pose_anchor_has.tolist() == [0]
    for got in runs[1:]:
        assert np.array_equal(got[0], runs[0][0]) and np.array_equal(got[1], runs[0][1])


def test_errors_come_before_any_launch(wrapper):
    w = wrapper
    pose, srt = _drivers(4, 8)
    w.pred_source_theta = torch.eye(4)[None]
    w._bank_write(1, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4))       # a slot without a source triple
    w.lib.calls.clear()
    w.recorded.clear()
    ids = [0, 1, 0, 2]
    for hp in (dict(relative=True), dict(gain=0.5), dict(gain=[1.0, 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match="slot 1 has none"):
            next(w.animate(pose, srt, identities=ids, head_pose=hp))
        with pytest.raises(ValueError, match="source"):                          # the current identity has none either
            next(w.animate(pose, srt, head_pose=hp))
    ok = [0, 0, 2, 2]
    for hp, match in ((dict(frontal=True, relative=True), "frontal"), (dict(gain=[1.0, 2.0]), "rows"), (dict(zoom=[1.0, 2.0]), "rows"),
                      (dict(rotation_offset=torch.zeros(3, 3)), "rows"), (dict(translation_offset=torch.zeros(2, 3)), "rows"),
                      (dict(rotation_offset=torch.zeros(4)), r"\[3\]"), (dict(translation_offset=torch.zeros(4, 2)), r"\[3\]"),
                      (dict(gain=torch.ones(2, 2)), "per row"), (dict(gian=2.0), "no field"), (3.0, "mapping")):
        with pytest.raises(ValueError, match=match):
            next(w.animate(pose, srt, identities=ok, head_pose=hp))
    with pytest.raises(ValueError, match="target_theta=False"):
        next(w.animate(pose, srt, identities=ok, target_theta=False, head_pose=dict(zoom=1.1)))
    next(w.animate(pose, srt, identities=ok, target_theta=False, as_uint8=False, head_pose={}))   # (no active edit: fine)
    assert NAME not in w.lib.calls and len(w.recorded) == 1
    # the slot without a source triple still serves what needs none
    w.lib.calls.clear()
    for _ in w.animate(pose, srt, identities=ids, as_uint8=False, head_pose=dict(frontal=True, zoom=0.9)):
        pass
    assert w.lib.calls == {NAME: 1}


# ---- animate_frames / animate_streams on toy embedders ----------------------------------------------------------------------------
E6 = 6


@pytest.fixture()
def video(monkeypatch):
    """a wrapper on CPU tensors with a 3-slot bank: the crops through the host-compiled kernels, the head pose a fixed function of
    the crop through emo_pose_theta_f32 (its output recorded), the expression embedder and the driver pass recorders"""
    import emulibs
    from emoportraits_amd import ops
    host_uploads(monkeypatch)
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(False)), 3)
    _fill(w, 3)
    w.regressed, w.aligned_by = [], []

    def head_pose(crops):
        f = crops.flatten(1)[:, 3::17][:, :9] - 0.5
        srt = (1 + 0.2 * f[:, 0:3]).contiguous(), (4.0 * f[:, 3:6]).contiguous(), (0.2 * f[:, 6:9]).contiguous()
        theta = ops.pose_theta(*srt)
        w.regressed.append((theta.clone(),) + srt)
        return (theta,) + srt

    def expression(crops, theta, what):
        w.aligned_by.append(theta.clone())
        return (crops.flatten(1)[:, 5::31][:, :E6] * 4 - 2).contiguous(), None
    w._head_pose = head_pose
    w._expression = expression
    return w


def _clip(n, hw, seed):
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _frames_run(w, frames, **kw):
    w.recorded.clear(), w.regressed.clear(), w.aligned_by.clear()
    for _ in w.animate_frames(frames, to_host=False, as_uint8=False, **kw):
        pass
    return torch.cat([r[1] for r in w.recorded]).numpy().reshape(-1, 16)


def _regressed(w):
    return [torch.cat([r[i] for r in w.regressed]) for i in range(4)]


def test_animate_frames_thetas_are_the_restatement_whatever_the_batches_and_chunks(video):
    w, N = video, 13
    clip = _clip(N, (16, 16), 80)
    ids = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]
    g = torch.Generator().manual_seed(81)
    gain, rot = torch.rand(N, generator=g) * 2, 0.2 * torch.randn(N, 3, generator=g)
    hp = dict(relative=True, gain=gain, rotation_offset=rot, zoom=1.2)
    plain = _frames_run(w, clip, batch_size=4, identities=ids)
    own, *srt = _regressed(w)
    assert np.array_equal(plain, own.numpy().reshape(-1, 16)) and w.lib.calls.get(NAME, 0) == 0
    assert torch.equal(torch.cat(w.aligned_by), own)
    host = HostState(3, w.lib)
    _, want = host(srt, ids, w.sources, gain, rot, None, 1.2, True)
    got = _frames_run(w, clip, batch_size=4, identities=ids, head_pose=hp)
    assert _same(got, want) and w.lib.calls[NAME] == 4                          # one launch per batch, the anchors in the bank
    assert not np.array_equal(got, plain)
    assert torch.equal(torch.cat(w.aligned_by), own)                            # the embedder aligns by the regressor's own theta
    assert _same(w.pred_target_theta.numpy().reshape(-1, 16), want[12:])
    for k, kw in enumerate((dict(frames=clip, batch_size=5), dict(frames=clip, batch_size=16), dict(frames=iter([clip[:7], clip[7:]]), batch_size=4),
                            dict(frames=iter([clip[:3], clip[3:4], clip[4:]]), batch_size=3))):
        w.reset_pose_state()
        frames = kw.pop("frames")
        assert _same(_frames_run(w, frames, identities=ids, head_pose=hp, **kw), want), k
    # two calls carry the anchors: 7 frames, then 6
    w.reset_pose_state()
    first = _frames_run(w, clip[:7], batch_size=4, identities=ids[:7], head_pose=dict(hp, gain=gain[:7], rotation_offset=rot[:7]))
    second = _frames_run(w, clip[7:], batch_size=4, identities=ids[7:], head_pose=dict(hp, gain=gain[7:], rotation_offset=rot[7:]))
    assert _same(np.concatenate([first, second]), want)
    # mix and smooth_pose (the two-pass path) work on the edited thetas; the embedder still aligns by the regressor's own
    from emoportraits_amd import hostglue
    w.reset_pose_state()
    got = _frames_run(w, clip, batch_size=4, identities=ids, head_pose=hp, smooth_pose=True, smooth_per_identity=True)
    want_s = np.empty_like(want)
    for k in range(3):
        sel = [i for i, v in enumerate(ids) if v == k]
        want_s[sel] = hostglue.ema_scan(want[sel].reshape(-1, 4, 4), None, 0.3)[0].reshape(-1, 16)
    assert _same(got, want_s) and torch.equal(torch.cat(w.aligned_by), own)
    # without identities: the one stream on the wrapper, about the current identity's source pose
    w.reset_pose_state()
    w.pred_source_srt = w.sources[2][None]
    host1 = HostState(1, w.lib)
    got = _frames_run(w, iter([clip[:6], clip[6:]]), batch_size=4, head_pose=dict(relative=True, gain=0.5))
    assert _same(got, host1(srt, None, w.sources[2:3], 0.5, None, None, None, True)[1])
    for kw, match in ((dict(faces=[[(0, 0, 16)]] * N, head_pose=dict(relative=True)), "identities"),
                      (dict(identities=ids, target_theta=False, head_pose=dict(frontal=True)), "target_theta=False"),
                      (dict(identities=ids, head_pose=dict(gain=gain[:5])), "rows")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_frames(clip, **kw))


def test_animate_streams_per_stream_values_reach_their_rows(video):
    w = video
    g = torch.Generator().manual_seed(84)
    rot_call, rot_rows = 0.2 * torch.randn(3, generator=g), 0.2 * torch.randn(3, 3, generator=g)

    def streams(chunked=False):
        a, b = _clip(3, (16, 16), 85), _clip(2, (20, 24), 86)
        return [dict(frames=iter([a[:1], a[1:]]) if chunked else a, windows=[(0, 0, 16), (0, 0, 12), (2, 1, 14)], identities=0,
                     head_pose=dict(gain=0.5)),
                dict(frames=iter([b[:1], b[1:]]) if chunked else b, faces=[[(0, 0, 16), (3, 2, 16)], [(1, 1, 18)]], identities=[1, 2, 1],
                     head_pose=dict(gain=[2.0, 1.0, 0.25], rotation_offset=rot_rows, zoom=[1.0, 1.5, 0.8]))]
    # tick order: (0,0) (1,0) (0,1) (1,1) (0,2); rows: s0 | s1 face 0, face 1 | s0 | s1 | s0
    ids = [0, 1, 2, 0, 1, 0]
    gain = [0.5, 2.0, 1.0, 0.5, 0.25, 0.5]
    zoom = [1.1, 1.0, 1.5, 1.1, 0.8, 1.1]
    rot = torch.stack([rot_call, rot_rows[0], rot_rows[1], rot_call, rot_rows[2], rot_call])
    hp = dict(relative=True, rotation_offset=rot_call, gain=3.0, zoom=1.1)

    def run(st, **kw):
        w.recorded.clear(), w.regressed.clear(), w.aligned_by.clear()
        w.reset_pose_state()
        for _ in w.animate_streams(st, to_host=False, as_uint8=False, **kw):
            pass
        return torch.cat([r[1] for r in w.recorded]).numpy().reshape(-1, 16), torch.cat([r[2] for r in w.recorded]).tolist()
    got, idents = run(streams(), batch_size=4, head_pose=hp)
    own, *srt = _regressed(w)
    assert idents == ids and own.shape[0] == 6
    _, want = HostState(3, w.lib)(srt, ids, w.sources, np.float32(gain), rot, None, np.float32(zoom), True)
    assert _same(got, want) and w.lib.calls[NAME] == 2 and torch.equal(torch.cat(w.aligned_by), own)
    for bs, chunked in ((2, False), (16, False), (4, True)):
        assert _same(run(streams(chunked), batch_size=bs, head_pose=hp)[0], want), (bs, chunked)
    # the call's own scalar gain / zoom and [3] offset where no stream brings its own
    bare = lambda: [{k: v for k, v in st.items() if k != "head_pose"} for st in streams()]
    got, _ = run(bare(), batch_size=4, head_pose=hp)
    assert _same(got, HostState(3, w.lib)(srt, ids, w.sources, 3.0, rot_call, None, 1.1, True)[1])
    # defaults: nothing launched, the regressor's own thetas
    w.lib.calls.clear()
    got, _ = run(bare(), batch_size=4, head_pose={})
    assert np.array_equal(got, own.numpy().reshape(-1, 16)) and w.lib.calls.get(NAME, 0) == 0
    for bad, match in ((dict(gain=[1.0] * 6), "one float"), (dict(zoom=[1.0] * 6), "one float"),
                       (dict(rotation_offset=torch.zeros(6, 3)), r"one \[3\] row"), (dict(frontal=True, relative=True), "frontal")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_streams(streams(), head_pose=bad))
    no_ids = [{k: v for k, v in st.items() if k != "identities"} for st in streams()]
    with pytest.raises(ValueError, match="identities"):
        next(w.animate_streams(no_ids, head_pose=dict(relative=True)))
    with pytest.raises(ValueError, match="one per face"):
        next(w.animate_streams([dict(streams()[0], head_pose=dict(gain=[1.0, 2.0]))], head_pose=hp))
    with pytest.raises(ValueError, match="not 'relative'"):
        next(w.animate_streams([dict(streams()[0], head_pose=dict(relative=True))], head_pose=hp))


def test_forward_keeps_the_source_triple_and_a_matrix_source_has_none(wrapper):
    """_theta_from: the triple is kept beside the theta; a 4x4 source theta leaves the identity without a source pose"""
    w = wrapper
    srt = tuple(t[:1] for t in _drivers(2, 11)[1])
    theta, kept = w._theta_from(srt)
    assert _same(w._srt9(kept).numpy(), torch.cat(srt, 1).numpy()) and theta.shape == (1, 4, 4)
    one_col = (srt[0][:, :1], srt[1], srt[2])
    assert _same(w._srt9(one_col).numpy()[0, :3], srt[0][0, :1].expand(3).numpy())
    assert w._theta_from(torch.eye(4)[None])[1] is None
