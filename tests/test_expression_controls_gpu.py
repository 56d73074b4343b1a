"""The expression controls on the GPU: ops.expression_controls against hostglue.expression_controls bit for bit;
animate_frames(expression=) against animate() fed with the expressions computed by hand (the embedder's rows through the host
restatement, the same batches); the state carried across calls; the source expression through store_identity / load_identity; a new
identity in a slot; the defaults.  Tiny fixture, toy embedders (the expression embedder row by row, so that a row does not depend
on the batch it is computed in).  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_hotpath.pt"), weights_only=False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (a, b))
    return np.array_equal(_bits(a), _bits(b))


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [65, 128])
def test_ops_expression_controls_is_the_restatement_bit_for_bit(E):
    """n = 40 rows over K = 3 interleaved streams (and rows of no stream), two calls that carry the state; everything on, and the
    combinations that leave a pointer out"""
    from emoportraits_amd import hostglue, ops
    n, K = 40, 3
    rng = np.random.default_rng(E)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    values, neutral = f32(rng.standard_normal((n, E))), f32(rng.standard_normal((K, E)))
    gain, offset = f32(rng.uniform(0, 2, n)), f32(0.3 * rng.standard_normal((n, E)))
    so = rng.integers(0, K, n).astype(np.int32)
    so[[5, 31]] = [-1, K]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    inside = (so >= 0) & (so < K)
    for use_neutral, use_gain, use_offset, relative, momentum in ((True, True, True, True, 0.3), (True, False, False, True, None),
                                                                  (True, True, False, False, 0.5), (False, False, True, False, 0.01),
                                                                  (True, False, True, False, None), (False, False, False, False, 1.0)):
        host = (np.zeros((K, E), np.float32), np.zeros(K, np.int32), np.zeros((K, E), np.float32), np.zeros(K, np.int32))
        state = [dev(a) for a in host]
        for lo, hi in ((0, 23), (23, n)):
            sl = lambda a, on=True: a[lo:hi] if on else None
            want = hostglue.expression_controls(values[lo:hi], so[lo:hi], neutral if use_neutral else None, sl(gain, use_gain),
                                                sl(offset, use_offset), *host, relative, momentum)
            out = ops.torch.empty((hi - lo, E), device=DEV, dtype=torch.float32).fill_(float("nan"))    # (ops.torch: between guards)
            got = ops.expression_controls(dev(values[lo:hi]), dev(so[lo:hi]), dev(neutral) if use_neutral else None,
                                          dev(sl(gain, use_gain)), dev(sl(offset, use_offset)), *state, relative, momentum, out=out)
            assert got is out and _same(got.cpu().numpy()[inside[lo:hi]], want[inside[lo:hi]])
            assert torch.isnan(got[~torch.from_numpy(inside[lo:hi])]).all()          # rows of no stream: unwritten
        for a, b in zip(state, host):
            assert _same(a, b) if b.dtype == np.float32 else a.cpu().tolist() == b.tolist()
    # a scalar gain and an [E] offset are broadcast to the rows; `out` may be `values`
    host = (np.zeros((1, E), np.float32), np.zeros(1, np.int32), np.zeros((1, E), np.float32), np.zeros(1, np.int32))
    state = [dev(a) for a in host]
    want = hostglue.expression_controls(values, None, neutral[:1], np.full(n, 0.25, np.float32), np.tile(offset[:1], (n, 1)), *host, True, 0.3)
    v = dev(values)
    assert ops.expression_controls(v, None, dev(neutral[:1]), 0.25, dev(offset[0]), *state, True, 0.3, out=v) is v and _same(v, want)


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def project(tmp_path_factory, tiny):
    from emoportraits_amd import config
    root = tmp_path_factory.mktemp("proj")
    exp = root / "logs" / "exp"
    (exp / "checkpoints").mkdir(parents=True)
    cfg = config.hot_path_config(overrides=tiny["cfg"])
    with open(exp / "args.txt", "wt") as f:
        for k, v in cfg.items():
            f.write(f"{k}: {v}\n")
        f.write("experiment_name: exp\nuse_seg: True\n")
    torch.save(tiny["state_dict"], exp / "checkpoints" / "model.pth")
    return root


def rowwise(fn):
    """the toy expression embedder one row at a time: a row's bits do not depend on the batch it arrives in"""
    def expression(crop, theta):
        outs = [fn(crop[i:i + 1], theta[i:i + 1]) for i in range(crop.shape[0])]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    return expression


def neutral_of(tiny, k):
    g = torch.Generator().manual_seed(50 + k)
    return (tiny["source_pose_embed"] + 0.3 * torch.randn(tiny["source_pose_embed"].shape, generator=g)).contiguous()


def make_wrapper(project, tiny, K=3, **kw):
    """a wrapper with K enrolled identities whose source expressions differ"""
    from test_identity_bank_gpu import _sources, _wrapper
    w = _wrapper(project, tiny, identity_capacity=K, **kw)
    w.embedders["expression_embedder"] = rowwise(w.embedders["expression_embedder"])
    S = tiny["cfg"]["image_size"]
    for k, (img, idt, th) in enumerate(_sources(tiny, K)):
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=neutral_of(tiny, k), custome_source_theta_embed=th)
        assert w.store_identity() == k
    return w


def _frames(tiny, N, seed=3):
    S = tiny["cfg"]["image_size"]
    return (torch.rand(N, S, S, 3, generator=torch.Generator().manual_seed(seed)) * 255).to(torch.uint8)


class Recorder:
    """what the embedders return and what the driver pass is handed and returns, batch by batch"""

    def __init__(self, w):
        self.w, self.embedded, self.srt, self.pose, self.img = w, [], [], [], []
        drive_bank, drive, expression, head_pose = w._drive_bank, w._drive, w._expression, w._head_pose

        def bank(pose, theta, ident):
            img = drive_bank(pose, theta, ident)
            self.pose.append(pose.clone()), self.img.append(img.clone())
            return img

        def single(pose, theta):
            img = drive(pose, theta)
            self.pose.append(pose.clone()), self.img.append(img.clone())
            return img

        def expr(crops, theta, what):
            out = expression(crops, theta, what)
            self.embedded.append(out[0].clone())
            return out

        def head(crops):
            out = head_pose(crops)
            self.srt.append([t.clone() for t in out[1:]])
            return out
        w._drive_bank, w._drive, w._expression, w._head_pose = bank, single, expr, head

    def clear(self):
        for rows in (self.embedded, self.srt, self.pose, self.img):
            rows.clear()

    def remove(self):
        for name in ("_drive_bank", "_drive", "_expression", "_head_pose"):
            self.w.__dict__.pop(name, None)


def _run_frames(w, rec, frames, **kw):
    rec.clear()
    for _ in w.animate_frames(frames, to_host=False, as_uint8=False, **kw):
        pass
    return torch.cat(rec.pose), torch.cat(rec.img)


def _host_state(K, E):
    return (np.zeros((K, E), np.float32), np.zeros(K, np.int32), np.zeros((K, E), np.float32), np.zeros(K, np.int32))


def _restate(values, ids, neutrals, gain, offset, state, relative, momentum):
    from emoportraits_amd import hostglue
    f32 = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
    return hostglue.expression_controls(f32(values), ids, f32(neutrals), f32(gain), f32(offset), *state, relative, momentum)


N, B = 13, 4
IDS = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]


def _controls(E):
    g = torch.Generator().manual_seed(77)
    return torch.rand(N, generator=g) * 2, 0.2 * torch.randn(N, E, generator=g)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_animate_frames_is_animate_fed_with_the_expressions_computed_by_hand(project, tiny, use_graphs):
    w = make_wrapper(project, tiny, use_graphs=use_graphs)
    E = tiny["cfg"]["lpe_output_channels_expression"]
    neutrals = torch.cat([neutral_of(tiny, k) for k in range(3)])
    assert _same(w._bank_expr, neutrals) and w._bank_expr_has == [True] * 3
    gain, offset = _controls(E)
    ex = dict(relative=True, gain=gain, offset=offset, smooth=True, momentum=0.3)
    frames = _frames(tiny, N)
    rec = Recorder(w)
    for _ in range(3 if use_graphs else 1):                                      # graphs: eager, capture, replay
        w.reset_expression_state()
        pose, img = _run_frames(w, rec, frames, batch_size=B, identities=IDS, expression=ex)
    embedded = torch.cat(rec.embedded)
    srt = [torch.cat([s[j] for s in rec.srt]) for j in range(3)]
    by_hand = _restate(embedded, IDS, neutrals, gain, offset, _host_state(3, E), True, 0.3)
    assert _same(pose, by_hand) and not _same(pose, embedded)
    rec.clear()
    for _ in w.animate(torch.from_numpy(by_hand), srt, batch_size=B, as_uint8=False, identities=IDS):
        pass
    assert _same(torch.cat(rec.pose), by_hand) and _same(torch.cat(rec.img), img)


def test_state_is_carried_across_calls(project, tiny):
    """7 frames, then 6 = 13 at once (batch_size 7: the same batches), with identities and without"""
    w = make_wrapper(project, tiny, use_graphs=False)
    E = tiny["cfg"]["lpe_output_channels_expression"]
    gain, offset = _controls(E)
    frames = _frames(tiny, N, seed=5)
    rec = Recorder(w)
    for ids in (IDS, None):
        kw = lambda a, b: dict(batch_size=7, expression=dict(relative=True, gain=gain[a:b], offset=offset[a:b], smooth=True),
                               **({} if ids is None else dict(identities=ids[a:b])))
        if ids is None:
            w.load_identity(1)
        w.reset_expression_state()
        pose, img = _run_frames(w, rec, frames, **kw(0, N))
        w.reset_expression_state()
        first = _run_frames(w, rec, frames[:7], **kw(0, 7))
        second = _run_frames(w, rec, frames[7:], **kw(7, N))
        assert _same(torch.cat([first[0], second[0]]), pose) and _same(torch.cat([first[1], second[1]]), img)
        w.reset_expression_state()
        restarted = _run_frames(w, rec, frames[7:], **kw(7, N))                  # (the state did matter)
        assert not _same(restarted[0], second[0])


def test_store_and_load_keep_the_source_expression_and_a_new_identity_restarts_its_slot(project, tiny):
    from test_identity_bank_gpu import _sources
    w = make_wrapper(project, tiny, use_graphs=False)
    E = tiny["cfg"]["lpe_output_channels_expression"]
    S = tiny["cfg"]["image_size"]
    for k in (2, 0, 1):
        w.load_identity(k)
        assert _same(w.pred_source_pose_embed, neutral_of(tiny, k))
    # relative + smooth on slot 0 and slot 1, then a new identity into slot 0: its stream restarts, slot 1's carries on
    frames = _frames(tiny, 8, seed=6)
    ids = [0, 1, 0, 0, 1, 1, 0, 1]
    ex = dict(relative=True, gain=1.5, smooth=True, momentum=0.3)
    rec = Recorder(w)
    neutrals = torch.cat([neutral_of(tiny, k) for k in range(3)])
    state = _host_state(3, E)
    pose, _ = _run_frames(w, rec, frames, batch_size=B, identities=ids, expression=ex)
    embedded = torch.cat(rec.embedded)
    assert _same(pose, _restate(embedded, ids, neutrals, np.full(8, 1.5), None, state, True, 0.3))
    assert w._bank_streams.expr_anchor_has.tolist() == [1, 1, 0] and w._bank_streams.expr_ema_has.tolist() == [1, 1, 0]
    img, idt, th = _sources(tiny, 1)[0]
    w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
              custome_source_pose_embed=neutral_of(tiny, 9), custome_source_theta_embed=th)
    assert w.store_identity(0) == 0
    assert w._bank_streams.expr_anchor_has.tolist() == [0, 1, 0] and w._bank_streams.expr_ema_has.tolist() == [0, 1, 0]
    neutrals[0] = neutral_of(tiny, 9)[0]
    state[1][0] = state[3][0] = 0
    pose, _ = _run_frames(w, rec, frames, batch_size=B, identities=ids, expression=ex)
    assert _same(pose, _restate(embedded, ids, neutrals, np.full(8, 1.5), None, state, True, 0.3))
    w.drop_identity(1)
    assert w._bank_streams.expr_anchor_has.tolist() == [1, 0, 0] and w._bank_expr_has == [True, False, True]


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_defaults_are_bit_identical_to_a_call_without_the_keyword(project, tiny, use_graphs):
    from emoportraits_amd import ExpressionControls
    w = make_wrapper(project, tiny, use_graphs=use_graphs)
    frames = _frames(tiny, N, seed=7)
    rec = Recorder(w)
    kw = dict(batch_size=B, identities=IDS, mix=True, smooth_pose=True, smooth_per_identity=True)
    runs = []
    for expression in ("absent", None, ExpressionControls(), {}):
        w.reset_pose_state()
        runs.append(_run_frames(w, rec, frames, **kw, **({} if expression == "absent" else dict(expression=expression))))
    for pose, img in runs[1:]:
        assert _same(pose, runs[0][0]) and _same(img, runs[0][1])
    assert _same(runs[0][0], torch.cat(rec.embedded))
    assert w._bank_streams.expr_anchor_has.tolist() == [0, 0, 0] and w._bank_streams.expr_ema_has.tolist() == [0, 0, 0]
