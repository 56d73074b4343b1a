"""The expression controls of the batched entry points without a GPU: emo_expr_controls_f32 (csrc/smallops.hip), compiled for the
host from the product's own source (tests/emul/emulibs.stream, the sequential and the threaded build), against the host code it
restates (hostglue.expression_controls), bit for bit; InferenceWrapper.animate(expression=) on the recorder rig of
tests/test_pose_controls_emul.py; animate_frames / animate_streams(expression=) on toy embedders, after the rig of
tests/test_streams_emul.py.  Nothing here has a tolerance.
"""
import ctypes
import itertools
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


ARGTYPES = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]


def raw(lib, values, so, neutral, gain, offset, anchor, has_a, ema, has_e, n, K, E, relative, smooth, momentum, out):
    fn = lib.emo_expr_controls_f32
    fn.argtypes, fn.restype = ARGTYPES, ctypes.c_int
    return fn(_p(values), _p(so), _p(neutral), _p(gain), _p(offset), _p(anchor), _p(has_a), _p(ema), _p(has_e), n, K, E,
              int(relative), int(smooth), float(np.float32(momentum)), float(np.float32(1 - momentum)), _p(out), None)


class Case:
    """seeded inputs of one call and fresh states (NaN values, clear flags) for the kernel and for the restatement"""

    def __init__(self, E, n, K, neutral, gain, offset, relative, smooth, seed, null_streams=False):
        rng = np.random.default_rng(seed)
        self.E, self.n, self.K, self.relative, self.smooth = E, n, K, relative, smooth
        self.values = _f32(rng.standard_normal((n, E)))
        self.so = None if null_streams else rng.integers(0, K, n).astype(np.int32)            # interleaved streams
        self.neutral = _f32(rng.standard_normal((K, E))) if neutral else None
        self.gain = _f32(rng.uniform(0.0, 2.0, n)) if gain else None
        self.offset = _f32(0.3 * rng.standard_normal((n, E))) if offset else None
        self.momentum = float(rng.choice([0.5, 0.3, 0.01, 1.0]))

    def states(self):
        return (np.full((self.K, self.E), np.nan, np.float32), np.zeros(self.K, np.int32),
                np.full((self.K, self.E), np.nan, np.float32), np.zeros(self.K, np.int32))

    def kernel(self, lib, st, rows=slice(None), out=None):
        v = self.values[rows] if out is None else out
        sl = lambda a: None if a is None else np.ascontiguousarray(a[rows])
        if out is None:
            out = np.full_like(v, np.nan)
        assert raw(lib, v, sl(self.so), self.neutral, sl(self.gain), sl(self.offset), *st, v.shape[0], self.K, self.E, self.relative,
                   self.smooth, self.momentum, out) == 0
        return out

    def restated(self, st, rows=slice(None)):
        from emoportraits_amd import hostglue
        sl = lambda a: None if a is None else a[rows]
        return hostglue.expression_controls(self.values[rows], sl(self.so), self.neutral, sl(self.gain), sl(self.offset), *st,
                                            self.relative, self.momentum if self.smooth else None)


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _same_states(a, b):
    """flags equal; the rows of the streams that have begun equal bit for bit (the others were never written)"""
    return all(np.array_equal(a[i + 1], b[i + 1]) and _same(a[i][a[i + 1] != 0], b[i][b[i + 1] != 0]) for i in (0, 2))


# every combination of (neutral, gain, offset, relative, smooth) the entry point admits: gain and relative need the neutral
COMBOS = [c for c in itertools.product([False, True], repeat=5) if c[0] or not (c[1] or c[3])]
SHAPES = list(itertools.product([1, 65, 128, 200], [1, 7, 40], [1, 3, 70]))


def test_the_corpus_is_what_the_kernel_admits():
    assert len(COMBOS) == 20 and len(SHAPES) == 36


def test_kernel_is_the_restatement_over_the_shapes(stream):
    """E below a wave, one past a wave, the released width and more than one stride of the block; one row to forty; one stream
    to seventy (most of them without a row); everything on, offset + smooth without a neutral, and relative transfer alone, each
    over every E, n and K"""
    combos = [(True, True, True, True, True), (False, False, True, False, True), (True, False, False, True, False)]
    for i, (E, n, K) in enumerate(SHAPES):
        combo = combos[(i + i // 3 + i // 9) % 3]
        c = Case(E, n, K, *combo, seed=i)
        a, b = c.states(), c.states()
        assert _same(c.kernel(stream, a), c.restated(b)), (E, n, K)
        assert _same_states(a, b), (E, n, K)


@pytest.mark.parametrize("shape", [(65, 7, 3), (200, 40, 3), (128, 40, 1)])
def test_kernel_is_the_restatement_over_the_combinations(stream, shape):
    for seed, combo in enumerate(COMBOS):
        c = Case(*shape, *combo, seed=100 + seed, null_streams=shape[2] == 1)
        a, b = c.states(), c.states()
        want = c.restated(b)
        assert _same(c.kernel(stream, a), want), combo
        assert _same_states(a, b), combo
        # `out` may be `values`
        a, inplace = c.states(), c.values.copy()
        assert _same(c.kernel(stream, a, out=inplace), want) and _same_states(a, b), combo


def test_state_is_carried_from_call_to_call_and_the_anchor_is_the_first_row(stream):
    for seed, (E, K) in enumerate([(65, 3), (128, 1), (200, 3)]):
        c = Case(E, 40, K, True, True, True, True, True, seed=200 + seed)
        whole, two, host = c.states(), c.states(), c.states()
        want = c.kernel(stream, whole)
        got = np.concatenate([c.kernel(stream, two, slice(0, 17)), c.kernel(stream, two, slice(17, 40))])
        assert _same(got, want) and _same_states(two, whole)
        assert _same(np.concatenate([c.restated(host, slice(0, 17)), c.restated(host, slice(17, 40))]), want)
        assert _same_states(host, whole)
        anchor_after_first = two[0].copy()
        for k in range(K):
            sel = np.nonzero(c.so == k)[0]
            assert whole[1][k] == (len(sel) > 0)
            if len(sel):
                assert _same(whole[0][k], c.values[sel[0]])                    # the stream's first row ...
        c.kernel(stream, two, slice(3, 29))                                       # ... and later rows leave it alone
        assert _same(two[0][two[1] != 0], anchor_after_first[two[1] != 0])


def test_rows_of_no_stream_stay_unwritten_and_touch_no_state(stream):
    E, n, K = 65, 9, 3
    c = Case(E, n, K, True, True, True, True, True, seed=300)
    c.so = np.int32([0, -1, 2, K, 0, K, -1, 2, 0])
    a, b = c.states(), c.states()
    got = c.kernel(stream, a)
    off = (c.so < 0) | (c.so >= K)
    assert np.isnan(got[off]).all() and not np.isnan(got[~off]).any()
    keep = np.nonzero(~off)[0]
    inside = Case(E, len(keep), K, True, True, True, True, True, seed=300)
    inside.values, inside.so, inside.neutral = c.values[keep], c.so[keep], c.neutral
    inside.gain, inside.offset, inside.momentum = c.gain[keep], c.offset[keep], c.momentum
    assert _same(got[keep], inside.restated(b)) and _same_states(a, b)
    assert list(a[1]) == [1, 0, 1] and list(a[3]) == [1, 0, 1] and np.isnan(a[0][1]).all() and np.isnan(a[2][1]).all()
    only_off = Case(E, 2, K, True, True, True, True, True, seed=301)
    only_off.so = np.int32([-1, K])
    st = only_off.states()
    assert np.isnan(only_off.kernel(stream, st)).all()
    assert not st[1].any() and not st[3].any() and np.isnan(st[0]).all() and np.isnan(st[2]).all()


def test_refusals_return_bad_arg_and_write_nothing(stream):
    n, K, E = 4, 2, 65
    c = Case(E, n, K, True, True, True, True, True, seed=400)
    an, ha, em, he = c.states()
    out = np.full((n, E), np.nan, np.float32)
    ok = dict(values=c.values, so=c.so, neutral=c.neutral, gain=c.gain, offset=c.offset, anchor=an, has_a=ha, ema=em, has_e=he,
              n=n, K=K, E=E, relative=1, smooth=1, momentum=0.5, out=out)
    bad = [dict(values=None), dict(out=None), dict(n=0), dict(K=0), dict(E=0), dict(n=-1), dict(K=-3), dict(E=-1),
           dict(neutral=None), dict(neutral=None, gain=None), dict(neutral=None, relative=0), dict(anchor=None), dict(has_a=None),
           dict(ema=None), dict(has_e=None)]
    for change in bad:
        assert raw(stream, **{**ok, **change}) == -1, change
        assert np.isnan(out).all() and np.isnan(an).all() and np.isnan(em).all() and not ha.any() and not he.any(), change
    assert raw(stream, **ok) == 0 and not np.isnan(out).any()
    # what a control does not need may be absent
    assert raw(stream, **{**ok, "relative": 0, "anchor": None, "has_a": None}) == 0
    assert raw(stream, **{**ok, "smooth": 0, "ema": None, "has_e": None}) == 0
    assert raw(stream, **{**ok, "neutral": None, "gain": None, "relative": 0, "anchor": None, "has_a": None}) == 0


def test_the_entry_point_is_in_the_abi_table():
    from emoportraits_amd import _abi_version, hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "int emo_expr_controls_f32(" in hdr and _abi_version.EMO_ABI_VERSION >= 20
    assert len(hip.SIGNATURES["emo_expr_controls_f32"]) == 18


# ---- animate(expression=) on the recorder rig of tests/test_pose_controls_emul.py ------------------------------------------------
E5 = 5            # the width of the recorder rig's `pose` rows


def _neutrals(K, E, seed=70):
    return torch.randn(K, E, generator=torch.Generator().manual_seed(seed))


@pytest.fixture()
def wrapper(monkeypatch):
    """an InferenceWrapper with a 3-slot bank and everything but the driver pass: that records (pose, theta, identity)"""
    import emulibs
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(True)), 3)
    w.neutrals = _neutrals(3, E5)
    for k in range(3):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4), w.neutrals[k])
    return w


def _drivers(N, seed):
    g = torch.Generator().manual_seed(seed)
    pose = torch.randn(N, E5, generator=g)
    srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.3 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
    return pose, srt


def _run(w, pose, srt, batch_size=4, **kw):
    w.recorded.clear()
    for _ in w.animate(pose, srt, batch_size=batch_size, as_uint8=False, **kw):
        pass
    return torch.cat([r[0] for r in w.recorded]).numpy(), torch.cat([r[1] for r in w.recorded]).numpy()


class HostState:
    """the states of K streams for the restatement, carried from call to call as the wrapper's are"""

    def __init__(self, K, E):
        self.st = (np.zeros((K, E), np.float32), np.zeros(K, np.int32), np.zeros((K, E), np.float32), np.zeros(K, np.int32))

    def __call__(self, values, ids, neutral, gain, offset, relative, momentum):
        from emoportraits_amd import hostglue
        n = len(values)
        gain = None if gain is None else np.broadcast_to(_f32(gain), (n,))
        offset = None if offset is None else np.broadcast_to(_f32(offset), np.shape(values))
        return hostglue.expression_controls(_f32(values), ids, None if neutral is None else _f32(neutral), gain, offset, *self.st, relative,
                                            momentum)

    def reset(self, k):
        self.st[1][k] = self.st[3][k] = 0


def test_animate_hands_the_restated_rows_to_the_driver_pass(wrapper):
    """13 frames in batches of 4 over three identities: relative + per-row gain + per-row offset + smooth, each row about its own
    slot's source expression and within its own slot's stream; a second call carries every slot's anchor and EMA on; the rows do
    not depend on batch_size; a new identity in a slot, drop_identity, reset_expression_state and forward(reset_tracking=True)
    restart streams"""
    from emoportraits_amd import ExpressionControls
    w, N = wrapper, 13
    pose, srt = _drivers(N, 3)
    pose2, srt2 = _drivers(N, 4)
    ids = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]
    ids2 = [1, 1, 0, 2, 0, 2, 2, 1, 0, 0, 0, 2, 1]
    g = torch.Generator().manual_seed(9)
    gain, offset = torch.rand(N, generator=g) * 2, 0.2 * torch.randn(N, E5, generator=g)
    host = HostState(3, E5)
    ex = ExpressionControls(relative=True, gain=gain, offset=offset, smooth=True, momentum=0.3)
    want = host(pose, ids, w.neutrals, gain, offset, True, 0.3)
    got, thetas = _run(w, pose, srt, identities=ids, expression=ex)
    plain_pose, plain_thetas = _run(w, pose, srt, identities=ids)
    assert _same(got, want) and np.array_equal(thetas, plain_thetas) and np.array_equal(plain_pose, pose.numpy())
    assert w.lib.calls["emo_expr_controls_f32"] == 1                            # the whole stream in one launch
    # the second call continues each slot's stream (a mapping serves as well as the class)
    want2 = host(pose2, ids2, w.neutrals, 0.5, offset[0], True, 0.3)
    got2, _ = _run(w, pose2, srt2, identities=ids2, expression=dict(relative=True, gain=0.5, offset=offset[0], smooth=True, momentum=0.3))
    assert _same(got2, want2)
    # batch sizes: the same rows from the same starting state
    saved = [t.clone() for t in (w._bank_streams.expr_anchor, w._bank_streams.expr_anchor_has, w._bank_streams.expr_ema, w._bank_streams.expr_ema_has)]
    rows = []
    for bs in (4, 5, 16):
        for t, s in zip((w._bank_streams.expr_anchor, w._bank_streams.expr_anchor_has, w._bank_streams.expr_ema, w._bank_streams.expr_ema_has), saved):
            t.copy_(s)
        rows.append(_run(w, pose, srt, batch_size=bs, identities=ids, expression=ex)[0])
    assert _same(rows[0], rows[1]) and _same(rows[0], rows[2])
    assert _same(rows[0], host(pose, ids, w.neutrals, gain, offset, True, 0.3))
    # a new identity in slot 1, drop + store of slot 2: those streams restart, slot 0 carries on
    w._canonical_cl, w.idt_embed, w.pred_source_theta = torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4)[None]
    w.pred_source_pose_embed = w.neutrals[1][None] + 1
    assert w.store_identity(1) == 1
    w.drop_identity(2)
    w.pred_source_pose_embed = w.neutrals[2][None]
    assert w.store_identity(2) == 2
    neutrals = w.neutrals.clone()
    neutrals[1] += 1
    host.reset(1), host.reset(2)
    got, _ = _run(w, pose2, srt2, identities=ids2, expression=ex)
    assert _same(got, host(pose2, ids2, neutrals, gain, offset, True, 0.3))
    w.reset_expression_state([0])
    host.reset(0)
    got, _ = _run(w, pose, srt, identities=ids, expression=ex)
    assert _same(got, host(pose, ids, neutrals, gain, offset, True, 0.3))
    assert w.forward(reset_tracking=True) is None
    assert w._bank_streams.expr_anchor_has.tolist() == [0, 0, 0] and w._bank_streams.expr_ema_has.tolist() == [0, 0, 0]
    # load_identity restores the slot's source expression as the current identity's
    w.hot_path = None
    import emoportraits_amd.ops as ops
    vol = ops.volume_to_channels_first
    try:
        ops.volume_to_channels_first = lambda cl: cl
        w.load_identity(1)
    finally:
        ops.volume_to_channels_first = vol
    assert torch.equal(w.pred_source_pose_embed, neutrals[1][None])


def test_animate_single_identity_stream_is_carried_on_the_wrapper(wrapper):
    w, N = wrapper, 13
    w._canonical_cl, w.pred_source_theta = torch.zeros(1, 2, 2, 2, 4), torch.eye(4)[None]
    w.pred_source_pose_embed = w.neutrals[1][None]
    pose, srt = _drivers(N, 5)
    host = HostState(1, E5)
    ex = dict(relative=True, gain=1.5, smooth=True, momentum=0.3)
    got, _ = _run(w, pose, srt, expression=ex)
    assert _same(got, host(pose, None, w.neutrals[1:2], 1.5, None, True, 0.3))
    got, _ = _run(w, pose[:7], srt, batch_size=5, expression=ex)                # (state from the first call)
    assert _same(got, host(pose[:7], None, w.neutrals[1:2], 1.5, None, True, 0.3))
    assert _same(w._stream.expr_anchor[0].numpy(), pose[0].numpy()) and _same(w._stream.expr_ema[0].numpy(), host.st[2][0])
    w.reset_expression_state()
    assert w._stream.expr_anchor_has.tolist() == [0] and w._stream.expr_ema_has.tolist() == [0]
    # offset alone needs neither a neutral nor a state
    w.pred_source_pose_embed = None
    got, _ = _run(w, pose, srt, expression=dict(offset=torch.ones(E5)))
    assert _same(got, (pose + 1).numpy()) and w._stream.expr_anchor_has.tolist() == [0] and w._stream.expr_ema_has.tolist() == [0]


def test_defaults_launch_nothing_and_change_nothing(wrapper):
    from emoportraits_amd import ExpressionControls
    w = wrapper
    pose, srt = _drivers(13, 6)
    ids = [0, 1, 2] * 4 + [0]
    kw = dict(identities=ids, mix=True, smooth_pose=True, smooth_per_identity=True)
    runs = []
    for expression in ("absent", None, ExpressionControls(), {}, dict(gain=1.0, momentum=0.9)):
        w.reset_pose_state()
        w.lib.calls.clear()
        runs.append(_run(w, pose, srt, **kw, **({} if expression == "absent" else dict(expression=expression))))
        assert w.lib.calls.get("emo_expr_controls_f32", 0) == 0
        assert w._bank_streams.expr_anchor_has.tolist() == [0, 0, 0] and w._bank_streams.expr_ema_has.tolist() == [0, 0, 0]
    for got in runs[1:]:
        assert np.array_equal(got[0], runs[0][0]) and np.array_equal(got[1], runs[0][1])
    assert np.array_equal(runs[0][0], pose.numpy())


def test_relative_transfer_of_a_still_clip_is_the_neutral_exactly(wrapper):
    w = wrapper
    pose, srt = _drivers(13, 7)
    still = pose[:1].expand(13, E5).contiguous()
    ids = [2, 0, 0, 1, 2, 2, 0, 1, 1, 0, 2, 1, 0]
    got, _ = _run(w, still, srt, identities=ids, expression=dict(relative=True, gain=1.0))
    assert _same(got, w.neutrals[ids].numpy())


def test_errors_come_before_any_launch(wrapper):
    w = wrapper
    pose, srt = _drivers(4, 8)
    w._canonical_cl, w.pred_source_theta = torch.zeros(1, 2, 2, 2, 4), torch.eye(4)[None]
    # _bank_write with three tensors still works: the slot has no neutral, and refuses the controls that need one
    w._bank_write(1, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4))
    w.lib.calls.clear()
    w.recorded.clear()
    ids = [0, 1, 0, 2]
    for ex in (dict(relative=True), dict(gain=0.5), dict(gain=[1.0, 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match="slot 1 has none"):
            next(w.animate(pose, srt, identities=ids, expression=ex))
        with pytest.raises(ValueError, match="source expression"):              # the current identity has none either
            next(w.animate(pose, srt, expression=ex))
    with pytest.raises(ValueError, match="override"):
        next(w.animate(pose, srt, identities=ids, expression=dict(override=pose)))
    for m in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            next(w.animate(pose, srt, identities=ids, expression=dict(smooth=True, momentum=m)))
    for ex, match in ((dict(gain=[1.0, 2.0]), "rows"), (dict(offset=torch.zeros(3, E5)), "rows"), (dict(offset=torch.zeros(2, 2, 2)), "dimensions"),
                      (dict(offset=torch.zeros(E5 + 1), gain=0.5), "widths"), (dict(gian=2.0), "no field"), (3.0, "mapping")):
        with pytest.raises(ValueError, match=match):
            next(w.animate(pose, srt, identities=[0, 0, 2, 2], expression=ex))
    assert w.lib.calls == {} and w.recorded == []
    # the slot without a neutral still serves what needs none
    for _ in w.animate(pose, srt, identities=ids, as_uint8=False, expression=dict(smooth=True, offset=torch.ones(E5))):
        pass
    assert w.lib.calls == {"emo_pose_theta_f32": 1, "emo_expr_controls_f32": 1} and len(w.recorded) == 1


# ---- animate_frames / animate_streams on toy embedders (after the rig of tests/test_streams_emul.py) ---------------------------
E6 = 6


@pytest.fixture()
def video(monkeypatch):
    """a wrapper on CPU tensors with a 3-slot bank: the crops through the host-compiled kernels, the head pose the identity, the
    expression a fixed function of the crop (recorded), the driver pass a recorder"""
    import emulibs
    host_uploads(monkeypatch)
    w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(False)), 3)
    w.neutrals = _neutrals(3, E6, 71)
    for k in range(3):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), torch.eye(4), w.neutrals[k])
    w._canonical_cl = torch.zeros(1, 2, 2, 2, 4)
    w.embedded = []

    def expression(crops, theta, what):
        w.embedded.append((crops.flatten(1)[:, 5::31][:, :E6] * 4 - 2).contiguous())
        return w.embedded[-1].clone(), None
    w._head_pose = lambda crops: (torch.eye(4).expand(crops.shape[0], 4, 4).contiguous(),)
    w._expression = expression
    return w


def _clip(n, hw, seed):
    return torch.randint(0, 256, (n, hw[0], hw[1], 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _frames_run(w, frames, **kw):
    w.recorded.clear()
    w.embedded.clear()
    for _ in w.animate_frames(frames, to_host=False, as_uint8=False, **kw):
        pass
    return torch.cat([r[0] for r in w.recorded]).numpy()


def test_animate_frames_rows_are_the_restatement_whatever_the_batches_and_chunks(video):
    w, N = video, 13
    clip = _clip(N, (16, 16), 80)
    ids = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]
    g = torch.Generator().manual_seed(81)
    gain, offset = torch.rand(N, generator=g) * 2, 0.2 * torch.randn(N, E6, generator=g)
    ex = dict(relative=True, gain=gain, offset=offset, smooth=True, momentum=0.3)
    plain = _frames_run(w, clip, batch_size=4, identities=ids)
    embedded = torch.cat(w.embedded).numpy()
    assert np.array_equal(plain, embedded) and w.lib.calls.get("emo_expr_controls_f32", 0) == 0
    host = HostState(3, E6)
    want = host(embedded, ids, w.neutrals, gain, offset, True, 0.3)
    got = _frames_run(w, clip, batch_size=4, identities=ids, expression=ex)
    assert _same(got, want) and w.lib.calls["emo_expr_controls_f32"] == 4       # one launch per batch, state in the bank
    for k, kw in enumerate((dict(frames=clip, batch_size=5), dict(frames=clip, batch_size=16), dict(frames=iter([clip[:7], clip[7:]]), batch_size=4),
                            dict(frames=iter([clip[:3], clip[3:4], clip[4:]]), batch_size=3))):
        w.reset_expression_state()
        frames = kw.pop("frames")
        assert _same(_frames_run(w, frames, identities=ids, expression=ex, **kw), want), k
    # two calls carry the state: 7 frames, then 6
    w.reset_expression_state()
    first = _frames_run(w, clip[:7], batch_size=4, identities=ids[:7], expression=dict(ex, gain=gain[:7], offset=offset[:7]))
    second = _frames_run(w, clip[7:], batch_size=4, identities=ids[7:], expression=dict(ex, gain=gain[7:], offset=offset[7:]))
    assert _same(np.concatenate([first, second]), want)
    # without identities: the one stream on the wrapper, about the current identity's source expression
    w.pred_source_pose_embed = w.neutrals[2][None]
    host1 = HostState(1, E6)
    got = _frames_run(w, iter([clip[:6], clip[6:]]), batch_size=4, expression=dict(relative=True, gain=0.5, smooth=True))
    assert _same(got, host1(embedded, None, w.neutrals[2:3], 0.5, None, True, 0.5))


def test_override_replaces_the_embedder_which_is_not_run(video):
    w, N = video, 9
    clip = _clip(N, (16, 16), 82)
    ids = [0, 1, 2] * 3
    table = torch.randn(N, E6, generator=torch.Generator().manual_seed(83))
    w._expression = lambda *a: pytest.fail("the expression embedder ran")
    got = _frames_run(w, clip, batch_size=4, identities=ids, expression=dict(override=table))
    assert np.array_equal(got, table.numpy()) and w.lib.calls.get("emo_expr_controls_f32", 0) == 0
    host = HostState(3, E6)
    got = _frames_run(w, iter([clip[:5], clip[5:]]), batch_size=4, identities=ids, expression=dict(override=table, relative=True, gain=2.0, smooth=True))
    assert _same(got, host(table, ids, w.neutrals, 2.0, None, True, 0.5))
    with pytest.raises(ValueError, match="rows"):
        next(w.animate_frames(clip, identities=ids, expression=dict(override=table[:5])))
    with pytest.raises(ValueError, match="identities"):                          # faces= without identities: no stream to follow
        next(w.animate_frames(clip, faces=[[(0, 0, 16)]] * N, expression=dict(smooth=True)))
    with pytest.raises(ValueError, match="identities"):
        next(w.animate_frames(clip, faces=[[(0, 0, 16)]] * N, expression=dict(relative=True)))


def test_animate_streams_per_stream_gain_and_offset_reach_their_rows(video):
    w = video
    g = torch.Generator().manual_seed(84)
    off_call, off_rows = 0.2 * torch.randn(E6, generator=g), 0.2 * torch.randn(3, E6, generator=g)

    def streams(chunked=False):
        a, b = _clip(3, (16, 16), 85), _clip(2, (20, 24), 86)
        return [dict(frames=iter([a[:1], a[1:]]) if chunked else a, windows=[(0, 0, 16), (0, 0, 12), (2, 1, 14)], identities=0,
                     expression=dict(gain=0.5)),
                dict(frames=iter([b[:1], b[1:]]) if chunked else b, faces=[[(0, 0, 16), (3, 2, 16)], [(1, 1, 18)]], identities=[1, 2, 1],
                     expression=dict(gain=[2.0, 1.0, 0.25], offset=off_rows))]
    # tick order: (0,0) (1,0) (0,1) (1,1) (0,2); rows: s0 | s1 face 0, face 1 | s0 | s1 | s0
    ids = [0, 1, 2, 0, 1, 0]
    gain = [0.5, 2.0, 1.0, 0.5, 0.25, 0.5]
    offset = torch.stack([off_call, off_rows[0], off_rows[1], off_call, off_rows[2], off_call])
    ex = dict(relative=True, smooth=True, momentum=0.3, offset=off_call, gain=3.0)

    def run(st, **kw):
        w.recorded.clear()
        w.embedded.clear()
        w.reset_expression_state()
        for _ in w.animate_streams(st, to_host=False, as_uint8=False, **kw):
            pass
        return torch.cat([r[0] for r in w.recorded]).numpy(), torch.cat([r[2] for r in w.recorded]).tolist()
    got, idents = run(streams(), batch_size=4, expression=ex)
    embedded = torch.cat(w.embedded).numpy()
    assert idents == ids and embedded.shape == (6, E6)
    host = HostState(3, E6)
    want = host(embedded, ids, w.neutrals, np.float32(gain), offset, True, 0.3)
    assert _same(got, want) and w.lib.calls["emo_expr_controls_f32"] == 2
    for bs, chunked in ((2, False), (16, False), (4, True)):
        assert _same(run(streams(chunked), batch_size=bs, expression=ex)[0], want), (bs, chunked)
    # the call's own scalar gain and [E] offset where no stream brings its own
    bare = [{k: v for k, v in st.items() if k != "expression"} for st in streams()]
    got, _ = run(bare, batch_size=4, expression=ex)
    assert _same(got, HostState(3, E6)(embedded, ids, w.neutrals, 3.0, off_call, True, 0.3))
    # defaults: nothing launched
    w.lib.calls.clear()
    got, _ = run([{k: v for k, v in st.items() if k != "expression"} for st in streams()], batch_size=4, expression={})
    assert np.array_equal(got, embedded) and w.lib.calls.get("emo_expr_controls_f32", 0) == 0
    for bad, match in ((dict(override=torch.zeros(6, E6)), "override"), (dict(gain=[1.0] * 6), "one float"),
                       (dict(offset=torch.zeros(6, E6)), r"one \[E\] row")):
        with pytest.raises(ValueError, match=match):
            next(w.animate_streams(streams(), expression=bad))
    no_ids = [{k: v for k, v in st.items() if k != "identities"} for st in streams()]
    with pytest.raises(ValueError, match="identities"):
        next(w.animate_streams(no_ids, expression=dict(smooth=True)))
    with pytest.raises(ValueError, match="one per face"):
        next(w.animate_streams([dict(streams()[0], expression=dict(gain=[1.0, 2.0]))], expression=ex))
