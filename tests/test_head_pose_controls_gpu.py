"""The head-pose controls on the GPU: ops.head_pose_controls against hostglue.head_pose_controls bit for bit, its theta bit for
bit ops.pose_theta of the edited rows and within 2e-6 of an fp64 S R T (test_pose_theta_and_pack's bound);
animate_frames(head_pose=) against animate() fed with the rows edited by hand (the regressor's rows through the host
restatement, the same batches), image and theta bit for bit; the defaults; batch sizes and chunks; animate_streams against the
faces path on the canvas clip.  Tiny fixture, toy embedders."""
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
@pytest.mark.parametrize("cols", [1, 3])
def test_ops_head_pose_controls_is_the_restatement_bit_for_bit(cols):
    """the cases of tests/test_head_pose_controls_emul.py at n = 40 rows over K = 3 interleaved streams (and rows of no stream),
    in two calls that carry the anchors"""
    from emoportraits_amd import hostglue, ops
    from test_head_pose_controls_emul import COMBOS, Case, srt64
    n, K = 40, 3
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    worst = 0.0
    for seed, combo in enumerate(COMBOS):
        c = Case(n, K, cols, seed=900 + seed, **combo)
        c.so[[5, 31]] = [-1, K]
        inside = (c.so >= 0) & (c.so < K)
        host = (np.zeros((K, 9), np.float32), np.zeros(K, np.int32))
        state = [dev(a) for a in host]
        for lo, hi in ((0, 23), (23, n)):
            args = c._args(slice(lo, hi))
            st = host if c.relative else (None, None)
            want, _ = hostglue.head_pose_controls(*args, *st, c.relative, c.frontal, K=K)
            if c.source is None and not c.relative:
                # (ops takes the number of streams from source / anchor: without either there is one stream, as in the wrapper)
                keep = np.nonzero(inside[lo:hi])[0]
                args = [None if a is None else (a if a is c.source else np.ascontiguousarray(a[keep])) for a in args]
                args[3], want = None, want[keep]
                got, theta = ops.head_pose_controls(*[dev(a) for a in args], None, None, False, c.frontal)
                live = torch.ones(len(keep), dtype=torch.bool)
            else:
                got, theta = ops.head_pose_controls(*[dev(a) for a in args], *(state if c.relative else (None, None)), c.relative,
                                                    c.frontal)
                live = torch.from_numpy(inside[lo:hi])
                want = want[inside[lo:hi]]
            got, theta = got.cpu(), theta.cpu()
            assert _same(got[live], want), combo
            edited = got[live].to(DEV)
            again = ops.pose_theta(*[edited[:, i:i + 3].contiguous() for i in (0, 3, 6)]).cpu()
            assert _same(theta[live], again), combo
            err = np.abs(theta[live].numpy().reshape(-1, 16).astype(np.float64) - srt64(got[live].numpy())).max()
            worst = max(worst, err)
            print(f"cols {cols} combo {seed} rows [{lo}, {hi}): theta against fp64 S R T, max abs error {err:.3e}")
            assert err <= 2e-6, combo
        if c.relative:
            assert state[1].cpu().tolist() == host[1].tolist() and _same(state[0].cpu()[host[1] != 0], host[0][host[1] != 0]), combo
    print(f"worst {worst:.3e}")


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


def source_of(k):
    """identity k's source (scale, rotation, translation)"""
    g = torch.Generator().manual_seed(60 + k)
    return 1 + 0.05 * torch.randn(1, 3, generator=g), 0.3 * torch.randn(1, 3, generator=g), 0.05 * torch.randn(1, 3, generator=g)


def make_wrapper(project, tiny, K=3, **kw):
    """a wrapper with K enrolled identities whose source poses, given as triples, differ"""
    from test_expression_controls_gpu import rowwise
    from test_identity_bank_gpu import _sources, _wrapper
    w = _wrapper(project, tiny, identity_capacity=K, **kw)
    w.embedders["expression_embedder"] = rowwise(w.embedders["expression_embedder"])
    S = tiny["cfg"]["image_size"]
    for k, (img, idt, _) in enumerate(_sources(tiny, K)):
        w.forward(source_image=img, crop=False, source_mask=torch.ones(1, 1, S, S), custome_idt_embed=idt,
                  custome_source_pose_embed=tiny["source_pose_embed"], custome_source_theta_embed=source_of(k))
        assert _same(w.pred_source_srt, torch.cat(source_of(k), 1))
        assert w.store_identity() == k
    return w


def _frames(tiny, N, seed=3):
    S = tiny["cfg"]["image_size"]
    return (torch.rand(N, S, S, 3, generator=torch.Generator().manual_seed(seed)) * 255).to(torch.uint8)


class Recorder:
    """what the embedders return and are handed, and what the driver pass is handed and returns, batch by batch"""

    def __init__(self, w):
        self.w, self.embedded, self.aligned_by, self.own, self.srt, self.theta, self.pose, self.img = w, [], [], [], [], [], [], []
        drive_bank, drive, expression, head_pose = w._drive_bank, w._drive, w._expression, w._head_pose

        def bank(pose, theta, ident):
            img = drive_bank(pose, theta, ident)
            self.pose.append(pose.clone()), self.theta.append(theta.clone()), self.img.append(img.clone())
            return img

        def single(pose, theta):
            img = drive(pose, theta)
            self.pose.append(pose.clone()), self.theta.append(theta.clone()), self.img.append(img.clone())
            return img

        def expr(crops, theta, what):
            out = expression(crops, theta, what)
            self.embedded.append(out[0].clone()), self.aligned_by.append(theta.clone())
            return out

        def head(crops):
            out = head_pose(crops)
            self.own.append(out[0].clone()), self.srt.append([t.clone() for t in out[1:]])
            return out
        w._drive_bank, w._drive, w._expression, w._head_pose = bank, single, expr, head

    def clear(self):
        for rows in (self.embedded, self.aligned_by, self.own, self.srt, self.theta, self.pose, self.img):
            rows.clear()

    def regressed(self):
        return [torch.cat([s[j] for s in self.srt]) for j in range(3)]


def _run_frames(w, rec, frames, **kw):
    rec.clear()
    for _ in w.animate_frames(frames, to_host=False, as_uint8=False, **kw):
        pass
    return torch.cat(rec.theta), torch.cat(rec.img)


def _restate(srt, ids, sources, gain, rot, trans, zoom, state, relative, frontal=False):
    from emoportraits_amd import hostglue
    f32 = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
    n = srt[0].shape[0]
    per_row = lambda v: None if v is None else np.broadcast_to(f32(v), (n,))
    rows3 = lambda v: None if v is None else np.broadcast_to(f32(v), (n, 3))
    return hostglue.head_pose_controls(*[f32(t) for t in srt], ids, f32(sources), per_row(gain), rows3(rot), rows3(trans), per_row(zoom),
                                       *(state if relative else (None, None)), relative, frontal)[0]


N, B = 13, 4
IDS = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1, 1, 0]
SOURCES = torch.cat([torch.cat(source_of(k), 1) for k in range(3)])


def _controls():
    g = torch.Generator().manual_seed(77)
    return torch.rand(N, generator=g) * 2, 0.2 * torch.randn(N, 3, generator=g)


def _host_state(K):
    return np.zeros((K, 9), np.float32), np.zeros(K, np.int32)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_animate_frames_is_animate_fed_with_the_rows_edited_by_hand(project, tiny, use_graphs):
    w = make_wrapper(project, tiny, use_graphs=use_graphs)
    assert _same(w._bank_srt, SOURCES) and w._bank_srt_has == [True] * 3
    gain, rot = _controls()
    hp = dict(relative=True, gain=gain, rotation_offset=rot, zoom=1.1)
    frames = _frames(tiny, N)
    rec = Recorder(w)
    for _ in range(3 if use_graphs else 1):                                      # graphs: eager, capture, replay
        w.reset_pose_state()
        theta, img = _run_frames(w, rec, frames, batch_size=B, identities=IDS, head_pose=hp)
    own, embedded, srt = torch.cat(rec.own), torch.cat(rec.embedded), rec.regressed()
    assert _same(torch.cat(rec.aligned_by), own)                                 # the embedder aligns by the regressor's own theta
    by_hand = _restate(srt, IDS, SOURCES, gain, rot, None, 1.1, _host_state(3), True)
    assert _same(torch.cat(w.pred_target_srt, 1), by_hand[12:]) and _same(w.pred_target_theta, theta[12:])
    assert not _same(theta, own)
    rec.clear()
    rows = torch.from_numpy(by_hand)
    for _ in w.animate(embedded, [rows[:, i:i + 3].contiguous() for i in (0, 3, 6)], batch_size=B, as_uint8=False, identities=IDS):
        pass
    assert _same(torch.cat(rec.theta), theta) and _same(torch.cat(rec.img), img)
    # animate(head_pose=) on the regressor's own rows: the same thetas and images
    rec.clear()
    w.reset_pose_state()
    for _ in w.animate(embedded, srt, batch_size=B, as_uint8=False, identities=IDS, head_pose=hp):
        pass
    assert _same(torch.cat(rec.theta), theta) and _same(torch.cat(rec.img), img)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_defaults_are_bit_identical_to_a_call_without_the_keyword(project, tiny, use_graphs):
    from emoportraits_amd import HeadPoseControls
    w = make_wrapper(project, tiny, use_graphs=use_graphs)
    frames = _frames(tiny, N, seed=7)
    rec = Recorder(w)
    kw = dict(batch_size=B, identities=IDS, mix=True, smooth_pose=True, smooth_per_identity=True)
    runs = []
    for head_pose in ("absent", None, HeadPoseControls(), {}):
        w.reset_pose_state()
        runs.append(_run_frames(w, rec, frames, **kw, **({} if head_pose == "absent" else dict(head_pose=head_pose))))
        assert w._bank_streams.pose_anchor_has.tolist() == [0, 0, 0] and w._stream.pose_anchor_has.tolist() == [0]
    for theta, img in runs[1:]:
        assert _same(theta, runs[0][0]) and _same(img, runs[0][1])


def test_thetas_do_not_depend_on_batch_size_or_chunking_and_the_anchor_is_carried(project, tiny):
    """batch_size 7 against 16; two chunks; 7 frames then 6 = 13 at once (batch_size 7: the same batches, so the images too);
    with identities and without"""
    w = make_wrapper(project, tiny, use_graphs=False)
    gain, rot = _controls()
    frames = _frames(tiny, N, seed=5)
    rec = Recorder(w)
    for ids in (IDS, None):
        kw = lambda a, b: dict(head_pose=dict(relative=True, gain=gain[a:b], rotation_offset=rot[a:b], translation_offset=[0.01, 0.0, -0.02]),
                               **({} if ids is None else dict(identities=ids[a:b])))
        if ids is None:
            w.load_identity(1)
        w.reset_pose_state()
        theta, img = _run_frames(w, rec, frames, batch_size=7, **kw(0, N))
        srt = rec.regressed()
        state = _host_state(3 if ids is not None else 1)
        want = _restate(srt, ids, SOURCES if ids is not None else SOURCES[1:2], gain, rot, [0.01, 0.0, -0.02], None, state, True)
        rows = torch.from_numpy(want).to(DEV)
        from emoportraits_amd import ops
        assert _same(theta, ops.pose_theta(*[rows[:, i:i + 3].contiguous() for i in (0, 3, 6)]))
        w.reset_pose_state()
        assert _same(_run_frames(w, rec, frames, batch_size=16, **kw(0, N))[0], theta)
        w.reset_pose_state()
        chunked = _run_frames(w, rec, iter([frames[:7], frames[7:]]), batch_size=7, **kw(0, N))
        assert _same(chunked[0], theta) and _same(chunked[1], img)
        w.reset_pose_state()
        first = _run_frames(w, rec, frames[:7], batch_size=7, **kw(0, 7))
        second = _run_frames(w, rec, frames[7:], batch_size=7, **kw(7, N))
        assert _same(torch.cat([first[0], second[0]]), theta) and _same(torch.cat([first[1], second[1]]), img)
        w.reset_pose_state()
        restarted = _run_frames(w, rec, frames[7:], batch_size=7, **kw(7, N))    # (the anchor did matter)
        assert not _same(restarted[0], second[0])


def test_two_streams_of_different_frame_sizes_are_the_faces_path_on_the_canvas_clip(project, tiny):
    import test_streams_gpu as TS
    w, S = make_wrapper(project, tiny, K=2, use_graphs=False), tiny["cfg"]["image_size"]
    counts = TS.COUNTS[:2]
    streams = TS.make_streams(S, counts, "rgb8", seed=43)
    g = torch.Generator().manual_seed(44)
    own = [dict(gain=0.5, rotation_offset=0.2 * torch.randn(sum(counts[0]), 3, generator=g)),
           dict(gain=(2 * torch.rand(sum(counts[1]), generator=g)).tolist(), zoom=1.2)]
    call = dict(relative=True, gain=3.0, zoom=0.9, rotation_offset=[0.1, -0.1, 0.05])
    order, clip, faces, ids = TS.canvas_clip(streams, "rgb8")
    first = [np.concatenate([[0], np.cumsum(c)]) for c in counts]
    rows = [(s, m) for s, t in order for m in range(first[s][t], first[s][t + 1])]           # (stream, face of the stream) of every row
    gain = torch.tensor([0.5 if s == 0 else own[1]["gain"][m] for s, m in rows])
    zoom = torch.tensor([0.9 if s == 0 else 1.2 for s, m in rows])
    rot = torch.stack([own[0]["rotation_offset"][m] if s == 0 else torch.tensor(call["rotation_offset"]) for s, m in rows])
    kw = dict(batch_size=4, mix=True, smooth_pose=True)
    w.reset_pose_state()
    want = torch.stack(TS._rows(w.animate_frames(clip, to_host=False, as_uint8=False, faces=faces, identities=ids, smooth_per_identity=True,
                                                 head_pose=dict(relative=True, gain=gain, zoom=zoom, rotation_offset=rot), **kw)))
    w.reset_pose_state()
    plain = torch.stack(TS._rows(w.animate_frames(clip, to_host=False, as_uint8=False, faces=faces, identities=ids, smooth_per_identity=True, **kw)))
    w.reset_pose_state()
    got = TS._items(w.animate_streams([dict(st, head_pose=o) for st, o in zip(streams, own)], to_host=False, as_uint8=False, head_pose=call, **kw))
    assert torch.equal(torch.cat([o for _, _, o in got]), want) and not torch.equal(want, plain)
    assert w._bank_streams.pose_anchor_has.tolist() == [1, 1]
