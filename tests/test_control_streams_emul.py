"""Which event restarts which control stream, through the public API alone, without a GPU: a 3-slot wrapper on the host-compiled
control kernels (the recorder rig of tests/test_head_pose_controls_emul.py) runs
    animate(smooth_pose=True, smooth_per_identity=True, expression=dict(relative=True, smooth=True), head_pose=dict(relative=True))
over the bank and over the current identity, then one event happens, then the same two calls run again: the thetas and expressions
handed to the driver pass are the hostglue restatements whose states were restarted for exactly the streams the table below names
and carried on for every other one.  The streams: the smooth_pose EMA ("ema"), the relative-pose anchor ("anchor") and the
expression anchor and EMA, which always restart together ("expr"); of bank slots, or of the single stream of the current identity.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_head_pose_controls_emul import E5, _Lib, _bare_wrapper, _drivers, _f32, _same, _sources, pose_theta  # noqa: E402

N, K = 6, 3
IDS = [0, 2, 1, 0, 2, 1]
ALL = ("ema", "anchor", "expr")


class Streams:
    """the states of K streams for the restatements, carried from call to call as the wrapper's are"""

    def __init__(self, K, lib):
        self.K, self.lib = K, lib
        self.ema = {}
        self.anchor = (np.zeros((K, 9), np.float32), np.zeros(K, np.int32))
        self.expr = (np.zeros((K, E5), np.float32), np.zeros(K, np.int32), np.zeros((K, E5), np.float32), np.zeros(K, np.int32))

    def restart(self, rows, which):
        for k in range(self.K) if rows is None else rows:
            if "ema" in which:
                self.ema.pop(k, None)
            if "anchor" in which:
                self.anchor[1][k] = 0
            if "expr" in which:
                self.expr[1][k] = self.expr[3][k] = 0

    def __call__(self, pose, srt, ids, sources, neutrals, momentum):
        """-> (thetas [n,16], expressions [n,E]) of one call: relative head pose, smooth_pose on its thetas; relative + smooth"""
        from emoportraits_amd import hostglue
        rows, _ = hostglue.head_pose_controls(*[_f32(t) for t in srt], ids, _f32(sources), None, None, None, None, *self.anchor, True, False)
        theta = pose_theta(self.lib._lib, rows)
        streams = [0] * len(theta) if ids is None else ids
        for k in sorted(set(streams)):
            sel = [i for i, s in enumerate(streams) if s == k]
            theta[sel], self.ema[k] = hostglue.ema_scan(theta[sel], self.ema.get(k), momentum)
        return theta, hostglue.expression_controls(_f32(pose), ids, _f32(neutrals), None, None, *self.expr, True, 0.5)


class _HotPath:
    """what a source call, share_source and enrolment ask of the hot path, as zeros of the right shapes"""
    pad = "zeros"

    def __init__(self, cfg):
        self.vol = (cfg["latent_volume_channels"], cfg["latent_volume_depth"], cfg["latent_volume_size"], cfg["latent_volume_size"])

    def local_encoder(self, img):
        return torch.zeros(img.shape[0], self.vol[0] * self.vol[1], *self.vol[2:])

    def embed(self, pose, idt):
        return torch.zeros(1, 1)

    def xy_generator(self, emb):
        return torch.zeros(1, 3, *self.vol[1:])

    def volume_process(self, vol):
        return vol

    def prepare_canonical(self, vol):
        return vol.permute(0, 2, 3, 4, 1).contiguous()

    def source_pass(self, masked, idt, pose, theta):
        return torch.zeros(masked.shape[0], *self.vol)


class Rig:
    """the wrapper, its two sets of host streams, and the source rows both work about"""

    def __init__(self, monkeypatch):
        import emulibs
        from emoportraits_amd import ops
        w = self.w = _bare_wrapper(monkeypatch, _Lib(emulibs.stream(True)), K)
        w.cfg["source_volume_num_blocks"] = 0
        w.hot_path = _HotPath(w.cfg)
        vol = torch.zeros(1, *w.hot_path.vol)
        for name, fn in (("volume_to_channels_first", lambda cl: cl.permute(0, 4, 1, 2, 3).contiguous()),
                         ("volume_to_channels_last", lambda v: v), ("mat4_inverse", lambda t: t), ("affine_grid3d", lambda t, size: None),
                         ("grid_sample3d", lambda v, **kw: vol.clone()), ("mul_mask", lambda a, b: a * b),
                         ("volume_to_channels_last_indexed", lambda v, bank, rows: None)):
            monkeypatch.setattr(ops, name, fn)
        self.monkeypatch = monkeypatch
        self.sources, self.neutrals = _sources(K), torch.randn(K, E5, generator=torch.Generator().manual_seed(71))
        for k in range(K):
            w._bank_write(k, *self.blank(), torch.eye(4), self.neutrals[k], self.sources[k])
        self.fresh = _sources(K, 72) + 0.05, torch.randn(K, E5, generator=torch.Generator().manual_seed(73))   # rows of new identities
        # the current identity: what forward(source_image=) leaves behind
        w._canonical_cl, w.idt_embed = self.blank()
        w.target_latent_volume = vol
        w.pred_source_theta, w.pred_source_srt, w.pred_source_pose_embed = torch.eye(4)[None], self.fresh[0][2:3].clone(), self.fresh[1][2:3].clone()
        self.current = self.fresh[0][2:3].clone(), self.fresh[1][2:3].clone()
        self.bank, self.single = Streams(K, w.lib), Streams(1, w.lib)
        self.drivers = [_drivers(N, 3), _drivers(N, 4)]

    @staticmethod
    def blank():
        return torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 4, 1, 1)

    def run(self, ids, seed):
        pose, srt = self.drivers[seed]
        w = self.w
        w.recorded.clear()
        for _ in w.animate(pose, srt, batch_size=4, as_uint8=False, identities=ids, smooth_pose=True, smooth_per_identity=True,
                           expression=dict(relative=True, smooth=True), head_pose=dict(relative=True)):
            pass
        got = torch.cat([r[1] for r in w.recorded]).numpy().reshape(-1, 16), torch.cat([r[0] for r in w.recorded]).numpy()
        host = self.single if ids is None else self.bank
        want = host(pose, srt, ids, *(self.current if ids is None else (self.sources, self.neutrals)), 0.3)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), ("single" if ids is None else "bank", seed)

    def both(self, seed):
        self.run(IDS, seed)
        self.run(None, seed)


# ---- the events: each triggers itself on the wrapper and restarts, on the host, the streams the table gives it ------------------
def new_source(r):
    s, e = r.fresh[0][0:1], r.fresh[1][0:1]
    assert r.w.forward(source_image=torch.rand(1, 3, 8, 8), source_mask=torch.ones(1, 1, 8, 8), crop=False, custome_idt_embed=r.blank()[1],
                       custome_source_theta_embed=(s[:, 0:3], s[:, 3:6], s[:, 6:9]), custome_source_pose_embed=e) is None
    r.current = s, e
    r.single.restart(None, ("anchor",))                     # (the single stream's expression and smooth_pose streams run on)


def load_identity(r):
    r.w.load_identity(1)
    r.current = r.sources[1:2], r.neutrals[1:2]
    r.single.restart(None, ("anchor",))


def share_source(r):
    r.w.share_source()
    r.single.restart(None, ("anchor",))


def store_identity(r):
    assert r.w.store_identity(1) == 1
    r.sources[1], r.neutrals[1] = r.current[0][0], r.current[1][0]
    r.bank.restart([1], ALL)


def bank_write(r):
    r.sources[2], r.neutrals[2] = r.fresh[0][1], r.fresh[1][1]
    r.w._bank_write(2, *r.blank(), torch.eye(4), r.neutrals[2], r.sources[2])
    r.bank.restart([2], ALL)


def drop_identity(r):
    """(a dropped slot renders nothing until it is stored again, which restarts it as well: the pair is what can be observed)"""
    r.w.drop_identity(0)
    assert r.w.identities() == [1, 2]
    store_identity_into(r, 0)


def store_identity_into(r, k):
    assert r.w.store_identity(k) == k
    r.sources[k], r.neutrals[k] = r.current[0][0], r.current[1][0]
    r.bank.restart([k], ALL)


def enrol_identities(r):
    s, e = r.fresh
    slots = r.w.enrol_identities(torch.rand(2, 3, 8, 8), source_masks=torch.ones(2, 1, 8, 8), slots=[2, 0], custome_idt_embed=torch.zeros(2, 4, 1, 1),
                                 custome_source_pose_embed=e[:2], custome_source_theta_embed=(s[:2, 0:3], s[:2, 3:6], s[:2, 6:9]))
    assert slots == [2, 0]
    r.sources[[2, 0]], r.neutrals[[2, 0]] = s[:2], e[:2]
    r.bank.restart([2, 0], ALL)


def share_identity_received(r):
    from emoportraits_amd import parallel
    s, e = r.fresh[0][1:2], r.fresh[1][1:2]
    sent = dict(canonical_cl=r.blank()[0], idt_embed=r.blank()[1], theta_src=torch.eye(4)[None], expr_src=e, srt_src=s)
    r.monkeypatch.setattr(parallel, "broadcast_source_cache", lambda rows, **kw: sent)
    r.w.rank = 1                                             # (rank 0 sends: this wrapper receives)
    r.w.share_identity(1, src_rank=0)
    r.w.rank = 0
    r.sources[1], r.neutrals[1] = s[0], e[0]
    r.bank.restart([1], ALL)


def reset_pose_state(r):
    r.w.reset_pose_state()
    r.bank.restart(None, ("ema", "anchor")), r.single.restart(None, ("ema", "anchor"))


def reset_pose_state_of_slots(r):
    r.w.reset_pose_state([0, 2])
    r.bank.restart([0, 2], ("ema", "anchor"))


def reset_expression_state(r):
    r.w.reset_expression_state()
    r.bank.restart(None, ("expr",)), r.single.restart(None, ("expr",))


def reset_expression_state_of_slots(r):
    r.w.reset_expression_state([1])
    r.bank.restart([1], ("expr",))


def reset_tracking(r):
    assert r.w.forward(reset_tracking=True) is None
    r.bank.restart(None, ALL), r.single.restart(None, ALL)


def nothing(r):
    """(the control: every stream of both sets carries on)"""


EVENTS = [nothing, new_source, load_identity, share_source, store_identity, bank_write, drop_identity, enrol_identities,
          share_identity_received, reset_pose_state, reset_pose_state_of_slots, reset_expression_state, reset_expression_state_of_slots,
          reset_tracking]


@pytest.mark.parametrize("event", EVENTS, ids=[e.__name__ for e in EVENTS])
def test_an_event_restarts_the_streams_the_table_names_and_no_other(monkeypatch, event):
    r = Rig(monkeypatch)
    r.both(0)
    event(r)
    r.both(1)
    r.both(0)                                                # (and every stream, restarted or not, carries on from there)
