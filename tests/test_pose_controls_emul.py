"""The pose controls of the batched entry points without a GPU: emo_mixing_theta_f32 and emo_theta_ema_scan_f32 (csrc/smallops.hip),
compiled for the host from the product's own sources (tests/emul/emulibs.stream), against the host code they restate
(hostglue.mixing_theta, hostglue.ema_scan); and InferenceWrapper.animate(mix=, smooth_pose=, target_theta=, identities=) on those
emulated kernels, with the driver pass replaced by a recorder of the thetas it is handed.
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
from bare_wrapper import bare_wrapper  # noqa: E402
from counting_lib import CountingLib as _Lib  # noqa: E402


@pytest.fixture(scope="module", params=[False, True], ids=["loop", "threads"])
def stream(request):
    import emulibs
    return emulibs.stream(request.param)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def mix(lib, target, source, index, mix_old):
    """the kernel on host buffers -> out [B,4,4] (NaN-filled before the call)"""
    target, source = _f32(target), _f32(source)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    out = np.full((target.shape[0], 4, 4), np.nan, np.float32)
    assert lib.emo_mixing_theta_f32(_p(target), _p(source), _p(idx), target.shape[0], source.shape[0], int(mix_old), _p(out),
                                    None) == 0
    return out


def scan(lib, values, stream_of, state, has, momentum):
    values = _f32(values).reshape(-1, 16)
    so = None if stream_of is None else np.ascontiguousarray(stream_of, dtype=np.int32)
    out = np.full_like(values, np.nan)
    assert lib.emo_theta_ema_scan_f32(_p(values), _p(so), _p(state), _p(has), values.shape[0], state.shape[0],
                                      ctypes.c_float(np.float32(momentum)), ctypes.c_float(np.float32(1 - momentum)), _p(out),
                                      None) == 0
    return out


def _homogeneous(lin, t):
    m = np.zeros((4, 4))
    m[:3, :3], m[:3, 3], m[3, 3] = lin, t, 1.0
    return m


def _rotation(rng, det=1.0):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) * det < 0:
        q[:, 0] = -q[:, 0]
    return q


def corpus(lib):
    """[M,4,4] fp32 thetas: seeded pose_theta outputs (the product's own kernel), shears, det < 0, conditioning 1 .. 1e4"""
    rng = np.random.default_rng(5)
    M = 24
    scale = _f32(1 + 0.1 * rng.standard_normal((M, 3)))
    rot, trans = _f32(0.5 * rng.standard_normal((M, 3))), _f32(0.1 * rng.standard_normal((M, 3)))
    pose = np.full((M, 4, 4), np.nan, np.float32)
    assert lib.emo_pose_theta_f32(_p(scale), 3, _p(rot), _p(trans), _p(pose), M, None) == 0
    out = list(pose)
    for k in range(12):                                                   # shears
        sh = np.eye(3)
        sh[rng.integers(3), rng.integers(3)] += rng.uniform(-0.8, 0.8)
        sh[0, 2] += rng.uniform(-0.5, 0.5)
        out.append(_homogeneous(_rotation(rng) @ sh * rng.uniform(0.7, 1.4), 0.1 * rng.standard_normal(3)))
    for k in range(12):                                                   # reflections
        out.append(_homogeneous(_rotation(rng, -1) @ np.diag(rng.uniform(0.5, 2, 3)) @ _rotation(rng),
                                0.1 * rng.standard_normal(3)))
    for cond in (10.0, 1e2, 1e3, 3e3, 1e4):                               # ill-conditioned, both signs of det
        for det in (1.0, -1.0):
            s = np.array([1.0, cond ** 0.5, cond]) / cond ** 0.5
            out.append(_homogeneous(_rotation(rng, det) @ np.diag(s) @ _rotation(rng), 0.1 * rng.standard_normal(3)))
    return _f32(np.stack(out))


def _ulps(a, b):
    a, b = _f32(a).view(np.int32).astype(np.int64), _f32(b).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def _want(source, target, mix_old):
    """hostglue.mixing_theta of one source and one target, as the kernel writes it: rows 0..2 rounded to fp32, row 3 (0,0,0,1)"""
    from emoportraits_amd import hostglue
    w = np.zeros((4, 4), np.float32)
    w[:3] = hostglue.mixing_theta(source[None], target[None], mix_old)[0]
    w[3, 3] = 1
    return w


@pytest.mark.parametrize("mix_old", [True, False])
def test_mixing_kernel_matches_hostglue_within_one_ulp(stream, mix_old):
    """every (source, target) pair drawn from the corpus: each element within 1 fp32 ulp of hostglue's fp64 result rounded"""
    th = corpus(stream)
    rng = np.random.default_rng(1 + int(mix_old))
    src_i = np.arange(th.shape[0])
    tgt_i = rng.permutation(th.shape[0])
    src_i, tgt_i = np.concatenate([src_i, tgt_i]), np.concatenate([tgt_i, src_i])
    got = mix(stream, th[tgt_i], th, src_i, mix_old)                      # the corpus as the bank
    worst = 0
    for n in range(len(src_i)):
        want = _want(th[src_i[n]], th[tgt_i[n]], mix_old)
        u = _ulps(got[n], want).max()
        worst = max(worst, u)
        assert u <= 1, (n, got[n], want)
    print(f"mix_old={mix_old}: {len(src_i)} pairs, worst {worst} ulp")


def test_mixing_kernel_on_the_reference_cases(stream, golden_dir):
    """tests/golden/hostglue.pt: the reference's own get_mixing_theta outputs (as test_host_logic.py holds the host code); with
    B sources the reference rolls the driver poses by one along the source axis -- frame b*T+t pairs source b with target
    ((b-1) mod B)*T+t, i.e. an index and a permuted target here"""
    glue = torch.load(os.path.join(golden_dir, "hostglue.pt"), weights_only=False)
    assert len(glue["mixing"]) == 6
    for m in glue["mixing"]:
        src, tgt = m["source"].numpy(), m["target"].numpy()
        B = src.shape[0]
        T = tgt.shape[0] // B
        order = [((b - 1) % B) * T + t for b in range(B) for t in range(T)]
        index = [b for b in range(B) for t in range(T)]
        got = mix(stream, tgt[order], src, index, m["mix_old"])
        assert np.abs(got[:, :3] - m["out"].numpy()).max() <= 1e-6
        assert np.array_equal(got[:, 3], np.tile(np.float32([0, 0, 0, 1]), (len(order), 1)))


def test_mixing_kernel_fallbacks_and_index_semantics(stream):
    th = corpus(stream)
    good_s, good_t = th[3], th[30]
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        b = good_s.copy()
        b[1, 2] = v
        bad.append(b)
    homog = lambda m: np.concatenate([m[:3], np.float32([[0, 0, 0, 1]])])
    for mix_old in (True, False):
        # non-finite source linear part: the target unchanged, exactly as hostglue (scipy's polar raises, :718-719)
        for b in bad:
            got = mix(stream, good_t[None], b[None], None, mix_old)
            assert np.array_equal(got[0], homog(good_t))
            assert np.array_equal(got[0], _want(b, good_t, mix_old))
        # non-finite target linear part: [P_s | 0] (:724-725) -- the zero translation and row 3 exactly, P_s (a decomposition)
        # within 1 ulp as above
        for b in bad:
            tb = good_t.copy()
            tb[:3, :3] = b[:3, :3]
            got = mix(stream, tb[None], good_s[None], None, mix_old)
            want = _want(good_s, tb, mix_old)
            assert _ulps(got[0], want).max() <= 1
            assert np.array_equal(got[0][:, 3], want[:, 3]) and np.array_equal(got[0][3], want[3])
            assert np.array_equal(got[0][:3, 3], np.zeros(3, np.float32))
        # a non-finite translation of the source does not matter (only the linear parts are decomposed)
        s_t = good_s.copy()
        s_t[0, 3] = np.nan
        assert np.array_equal(mix(stream, good_t[None], s_t[None], None, mix_old), mix(stream, good_t[None], good_s[None], None,
                                                                                   mix_old))
    # NULL index: every frame mixes with source 0; K > 1 with shuffled indices equals the per-frame single-source call
    K, B = 5, 13
    bank, tg = th[:K], th[K:K + B]
    rng = np.random.default_rng(9)
    idx = rng.integers(0, K, B)
    for mix_old in (True, False):
        null = mix(stream, tg, bank, None, mix_old)
        zero = mix(stream, tg, bank[:1], None, mix_old)
        assert np.array_equal(null, zero)
        got = mix(stream, tg, bank, idx, mix_old)
        for n in range(B):
            assert np.array_equal(got[n], mix(stream, tg[n:n + 1], bank[idx[n]:idx[n] + 1], None, mix_old)[0]), n
    # an index outside [0, K): the target passed through, and the source memory around the bank is not read -- the bank sits
    # between FINITE guard thetas (a stray read would mix with one of them and change the output)
    guard = np.tile(th[40], (4, 1, 1))
    whole = _f32(np.concatenate([guard, bank, guard]))
    view = whole[4:4 + K]
    assert view.ctypes.data == whole.ctypes.data + 4 * 64
    idx = np.int32([-1, 2, K, K + 3, -4, 0])
    tg6 = tg[:6]
    out = np.full((6, 4, 4), np.nan, np.float32)
    assert stream.emo_mixing_theta_f32(_p(tg6), ctypes.c_void_p(view.ctypes.data), _p(idx), 6, K, 1, _p(out), None) == 0
    for n in range(6):
        if 0 <= idx[n] < K:
            assert np.array_equal(out[n], mix(stream, tg6[n:n + 1], bank[idx[n]:idx[n] + 1], None, True)[0])
        else:
            assert np.array_equal(out[n], homog(tg6[n])), n
    # refusals
    assert stream.emo_mixing_theta_f32(None, _p(bank), None, 1, K, 1, _p(out), None) == -1
    assert stream.emo_mixing_theta_f32(_p(tg6), _p(bank), None, 1, 0, 1, _p(out), None) == -1
    assert stream.emo_mixing_theta_f32(_p(tg6), _p(bank), None, 0, K, 1, _p(out), None) == -1


@pytest.mark.parametrize("momentum", [0.5, 0.3, 0.01])
def test_ema_scan_is_hostglue_per_stream_bit_for_bit(stream, momentum):
    """interleaved streams, a stream that starts mid-chunk, one that never appears, state carried across two calls: every
    stream's frames are hostglue.ema_scan over that stream's own subsequence"""
    from emoportraits_amd import hostglue
    rng = np.random.default_rng(int(momentum * 100))
    K, n = 4, 29
    vals = _f32(rng.standard_normal((2 * n, 4, 4)))
    so = np.int32([(i * 7 + i // 3) % 2 for i in range(n)] + [(i % 3) for i in range(n)])   # stream 2 starts in the 2nd call
    so[n // 2] = 2                                                                          # ... and once mid-chunk in the 1st
    state = np.full((K, 16), np.nan, np.float32)
    has = np.zeros(K, np.int32)
    out = np.concatenate([scan(stream, vals[:n], so[:n], state, has, momentum),
                          scan(stream, vals[n:], so[n:], state, has, momentum)])
    for k in range(K):
        sel = np.nonzero(so == k)[0]
        if len(sel) == 0:                                                  # stream 3: untouched
            assert has[k] == 0 and np.isnan(state[k]).all()
            continue
        want, st = hostglue.ema_scan(vals[sel].reshape(-1, 16), None, momentum)
        assert np.array_equal(out[sel].view(np.uint32), want.view(np.uint32)), k
        assert has[k] == 1 and np.array_equal(state[k].view(np.uint32), st.view(np.uint32))
    # a given starting state; NULL stream_of = one stream, 0
    st0 = _f32(rng.standard_normal(16))
    state = np.tile(st0, (2, 1))
    has = np.int32([1, 0])
    got = scan(stream, vals[:n], None, state, has, momentum)
    want, st = hostglue.ema_scan(vals[:n].reshape(-1, 16), st0, momentum)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(state[0], st)
    assert np.array_equal(state[1], st0) and list(has) == [1, 0]


def test_ema_scan_refusals(stream):
    v = np.zeros((2, 16), np.float32)
    st = np.zeros((1, 16), np.float32)
    has = np.zeros(1, np.int32)
    out = np.zeros_like(v)
    call = lambda vals, state, flags, n, K: stream.emo_theta_ema_scan_f32(_p(vals), None, _p(state), _p(flags), n, K,
                                                                          ctypes.c_float(0.5), ctypes.c_float(0.5), _p(out), None)
    assert call(v, st, has, 2, 1) == 0
    assert call(None, st, has, 2, 1) == -1
    assert call(v, st, None, 2, 1) == -1
    assert call(v, st, has, 0, 1) == -1
    assert call(v, st, has, 2, 0) == -1


# ---- the wrapper on the emulated kernels ----------------------------------------------------------------------------------
@pytest.fixture()
def wrapper(monkeypatch):
    """an InferenceWrapper with a 3-slot bank and everything but the driver pass: that records (pose, theta, identity)"""
    import emulibs
    lib = _Lib(emulibs.stream(True))
    w = bare_wrapper(monkeypatch, lib, 3)
    th = corpus(lib)
    w.src_thetas = [torch.from_numpy(th[k]) for k in (2, 41, 47)]          # a pose_theta, a reflection, an ill-conditioned one
    for k in range(3):
        w._bank_write(k, torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), w.src_thetas[k])
    return w


def _drivers(N, seed):
    g = torch.Generator().manual_seed(seed)
    pose = torch.randn(N, 5, generator=g)
    srt = (1 + 0.05 * torch.randn(N, 3, generator=g), 0.3 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g))
    return pose, srt


def _run(w, pose, srt, **kw):
    w.recorded.clear()
    for _ in w.animate(pose, srt, batch_size=4, as_uint8=False, **kw):
        pass
    return torch.cat([r[1] for r in w.recorded]).numpy(), [r[2] for r in w.recorded]


def _predicted_mix(w, srt, ids, mix_old):
    from emoportraits_amd import ops
    th = ops.pose_theta(*[t.contiguous() for t in srt]).numpy()
    out = np.stack([mix(w.lib._lib, th[i:i + 1], w.src_thetas[ids[i]].numpy()[None], None, mix_old)[0] for i in range(len(ids))])
    for i in range(len(ids)):                                     # (and each within 1 ulp of the host restatement)
        assert _ulps(out[i], _want(w.src_thetas[ids[i]].numpy(), th[i], mix_old)).max() <= 1
    return out


def _predicted_smooth(values, ids, states, momentum):
    """hostglue.ema_scan over each identity's subsequence, starting from states[k] (None: a fresh stream); updates states"""
    from emoportraits_amd import hostglue
    out = np.empty_like(values)
    for k in sorted(set(ids)):
        sel = [i for i, s in enumerate(ids) if s == k]
        sm, states[k] = hostglue.ema_scan(values[sel].reshape(-1, 16), states.get(k), momentum)
        out[sel] = sm.reshape(-1, 4, 4)
    return out


@pytest.mark.parametrize("mix_old", [True, False])
def test_animate_bank_mix_and_smooth_feed_the_predicted_thetas(wrapper, mix_old):
    """animate(identities=..., mix=True, smooth_pose=True): the driver pass receives, bit for bit, the mixing kernel's theta
    of each frame against its own slot's source theta, smoothed within that slot's own frame sequence -- state carried from
    call to call per slot, reset by store_identity / drop_identity / reset_pose_state"""
    w = wrapper
    N = 11
    pose, srt = _drivers(N, 3)
    ids = [0, 2, 2, 0, 1, 0, 2, 0, 0, 2, 1]
    ids2 = [1, 1, 0, 2, 0, 2, 2, 1, 0, 0, 0]
    states = {}
    want = _predicted_smooth(_predicted_mix(w, srt, ids, mix_old), ids, states, 0.3)
    got, idents = _run(w, pose, srt, identities=ids, mix=True, mix_old=mix_old, smooth_pose=True,
                    smooth_per_identity=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert torch.cat(idents).tolist() == ids
    # the second call continues each slot's stream
    pose2, srt2 = _drivers(N, 4)
    want = _predicted_smooth(_predicted_mix(w, srt2, ids2, mix_old), ids2, states, 0.3)
    got, _ = _run(w, pose2, srt2, identities=ids2, mix=True, mix_old=mix_old, smooth_pose=True,
                    smooth_per_identity=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # storing into slot 1 and dropping + re-storing slot 2 restart those streams; slot 0 carries on
    w._canonical_cl, w.idt_embed, w.pred_source_theta = torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1), w.src_thetas[1]
    w.drop_identity(1)
    assert w.store_identity(1) == 1
    w.drop_identity(2)
    w.pred_source_theta = w.src_thetas[2]
    assert w.store_identity(2) == 2
    states.pop(1), states.pop(2)
    want = _predicted_smooth(_predicted_mix(w, srt, ids, mix_old), ids, states, 0.3)
    got, _ = _run(w, pose, srt, identities=ids, mix=True, mix_old=mix_old, smooth_pose=True,
                    smooth_per_identity=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # reset_pose_state(slots) restarts only those; forward(reset_tracking=True) all of them
    w.reset_pose_state([0])
    states.pop(0)
    want = _predicted_smooth(_predicted_mix(w, srt2, ids2, mix_old), ids2, states, 0.3)
    got, _ = _run(w, pose2, srt2, identities=ids2, mix=True, mix_old=mix_old, smooth_pose=True,
                    smooth_per_identity=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert w.forward(reset_tracking=True) is None
    assert w._bank_streams.theta_has.tolist() == [0, 0, 0]


def test_animate_single_identity_controls(wrapper):
    """no bank: mix against pred_source_theta; smooth_pose is one stream carried in self.theta (the device scan over the whole
    stream, = hostglue.ema_scan); target_theta=False renders every frame with the source theta; without smooth_pose and mix the
    thetas are pose_theta's exactly as before"""
    from emoportraits_amd import hostglue, ops
    w = wrapper
    w._canonical_cl, w.pred_source_theta = torch.zeros(1, 2, 2, 2, 4), w.src_thetas[1][None]
    N = 9
    pose, srt = _drivers(N, 5)
    plain = ops.pose_theta(*[t.contiguous() for t in srt]).numpy()
    got, idents = _run(w, pose, srt)
    assert np.array_equal(got, plain) and idents == [None] * 3
    mixed = _predicted_mix(w, srt, [1] * N, True)
    got, _ = _run(w, pose, srt, mix=True)
    assert np.array_equal(got, mixed)
    sm, st = hostglue.ema_scan(mixed.reshape(N, 16), None, 0.3)
    got, _ = _run(w, pose, srt, mix=True, smooth_pose=True)
    assert np.array_equal(got.reshape(N, 16), sm) and np.array_equal(w.theta.reshape(16).numpy(), st)
    sm2, st2 = hostglue.ema_scan(plain.reshape(N, 16), st, 0.3)
    got, _ = _run(w, pose, srt, smooth_pose=True, target_theta=False)
    assert np.array_equal(got, np.tile(w.src_thetas[1].numpy(), (N, 1, 1)))
    assert np.array_equal(w.theta.reshape(16).numpy(), st2)
    w.reset_pose_state()
    assert w.theta is None


def test_argument_checks_come_before_any_launch(wrapper):
    w = wrapper
    pose, srt = _drivers(4, 6)
    w.lib.calls.clear()
    w._canonical_cl = torch.zeros(1, 2, 2, 2, 4)
    w.pred_source_theta = None
    with pytest.raises(RuntimeError, match="source theta"):
        next(w.animate(pose, srt, mix=True))
    with pytest.raises(RuntimeError, match="source theta"):
        next(w.animate(pose, srt, target_theta=False))
    w.drop_identity(1)
    for bad in ([0, 1, 0, 0], [0, 3, 0, 0], [0, -1, 2, 2]):
        with pytest.raises(ValueError):
            next(w.animate(pose, srt, identities=bad, mix=True, smooth_pose=True))
    with pytest.raises(ValueError, match="smooth_per_identity"):       # per-slot streams are asked for explicitly
        next(w.animate(pose, srt, identities=[0, 0, 2, 2], smooth_pose=True))
    with pytest.raises(ValueError):
        w.reset_pose_state([3])
    assert w.lib.calls == {} and w.recorded == []
    w.reset_pose_state([1])                                      # (a free slot may be reset)
