"""Every conv launch the product makes, against fp64, on every frame.

ops.conv_igemm and ops.conv_head are wrapped (the networks call them as ops.<name>), and the passes run eagerly at their real
shapes, batch, launch plan and activations: the R512 driver pass at B = 16 (what bench.py times) in every precision mode and
at B = 1 (K splits), the R512 source pass, and stage 2 at 512^2.  Each launch runs on the caller's own tensors (a clone would
change the 16-byte alignment the planner reads); its inputs are copied first, and its output is compared at once, sample by
sample, with the fp64 reference of tests/conv_reference.py under the bounds of its plan's arithmetic.  Split launches
(bf16x3 / f16x2) are held to the exact-fp32 MFMA kernel's error on the same inputs; launches that return tile statistics are
held to a direct reduction of their output.  Only a summary row per launch is kept.

One PARITY line per pass: worst per-frame relative max and worst mean-error ratio to the fp32 kernel (with layer and frame),
and the inventory (plan precision, block config, K split, form) -> launches.
"""
import inspect
from collections import Counter

import pytest
import torch

import conv_reference as R
from conv_plans import executed
from emoportraits_amd import config, nets, ops, pack, random_init, stage2
from test_nets_gpu import _full_size

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"

_REAL_IGEMM, _REAL_HEAD = ops.conv_igemm, ops.conv_head
_IGEMM_SIG = inspect.signature(_REAL_IGEMM)
_HEAD_SIG = inspect.signature(_REAL_HEAD)


def packed_convs(*roots):
    """every pack.PackedConv reachable from the given network objects (attributes, lists, tuples, dicts)"""
    seen, found = set(), {}

    def walk(o):
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, pack.PackedConv):
            found[id(o)] = o
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif type(o).__module__.startswith("emoportraits_amd") and hasattr(o, "__dict__"):
            for v in vars(o).values():
                walk(v)

    for r in roots:
        walk(r)
    return list(found.values())


def _clone(t):
    return None if t is None else t.clone()


class LaunchChecker:
    """stands in for ops.conv_igemm / ops.conv_head while a pass runs: real launch, fp64 check, one summary row"""

    def __init__(self, tag):
        self.tag = tag
        self.rows = []
        self.intercepted = 0
        self._in_head = False
        self._f32_layers = {}     # id(layer) -> (layer, fp32 MFMA twin): the yardstick of the split kernels, built once per layer

    def install(self, mp):
        mp.setattr(ops, "conv_igemm", self.conv_igemm)
        mp.setattr(ops, "conv_head", self.conv_head)

    def _f32_twin(self, layer):
        hit = self._f32_layers.get(id(layer))
        if hit is None or hit[0] is not layer:
            hit = (layer, pack.PackedConv(layer.name + "[f32]", layer._weight, layer.bias, DEV, precision="f32"))
            self._f32_layers[id(layer)] = hit
        return hit[1]

    def conv_igemm(self, *args, **kwargs):
        if self._in_head:                    # (conv_head's fallback onto the GEMM kernel: checked as the head's launch)
            return _REAL_IGEMM(*args, **kwargs)
        a = _IGEMM_SIG.bind(*args, **kwargs)
        a.apply_defaults()
        a = a.arguments
        return self._launch(_REAL_IGEMM, args, kwargs, a)

    def conv_head(self, *args, **kwargs):
        a = _HEAD_SIG.bind(*args, **kwargs)
        a.apply_defaults()
        a = dict(a.arguments, ups=False, res=None, res_ups=False, want_stats=False)
        self._in_head = True
        try:
            return self._launch(_REAL_HEAD, args, kwargs, a)
        finally:
            self._in_head = False

    def _launch(self, real, args, kwargs, a):
        self.intercepted += 1
        layer, x = a["layer"], a["x"]
        xc, sc, sh, rc = _clone(x), _clone(a["scale"]), _clone(a["shift"]), _clone(a["res"])
        result = real(*args, **kwargs)
        out, st = result if a["want_stats"] else (result, None)
        prec, cfg, ks, form = executed(layer, out)
        flags = dict(relu_in=a["relu_in"], ups=a["ups"], res_ups=a["res_ups"], act=a["act"])
        yard = None
        if prec in R.SPLIT_MEAN:
            yard = _REAL_IGEMM(xc, self._f32_twin(layer), sc, sh, res=rc, **flags)
        groups = 32 if layer.cout % 32 == 0 else None
        fig = R.check_launch(out, xc, layer._weight, layer.bias, sc, sh, res=rc, precision=prec, yardstick=yard,
                             stats=st, groups=groups, **flags)
        if st is not None and groups is None:
            fig["failures"].append("tile statistics without a GroupNorm to check them against")
        del xc, sc, sh, rc, yard
        n_worst = max(range(len(fig["frames"])), key=lambda i: fig["frame_rel_max"][i])
        self.rows.append(dict(
            layer=layer, name=layer.name, shape=(tuple(x.shape), tuple(out.shape)), plan=(prec, cfg, ks, form),
            flags=dict(flags, affine=a["scale"] is not None, res=a["res"] is not None, stats=st is not None),
            frames=len(fig["frames"]), frame_rel=fig["frame_rel_max"][n_worst], frame=fig["frames"][n_worst],
            mean_rel=fig["mean_err"] / max(fig["scale"], 1e-300), max_rel=fig["max_err"] / max(fig["scale"], 1e-300),
            mean_of_max=fig["mean_err"] / max(fig["ref_max"], 1e-300),
            ratio=fig["mean_err"] / fig["f32_mean_err"] if fig.get("f32_mean_err") else None,
            max_ratio=fig["max_err"] / fig["f32_max_err"] if fig.get("f32_max_err") else None,
            stats=(fig.get("stats_scale_rel"), fig.get("stats_shift_abs")), failures=fig["failures"],
            in_w=x.shape[-1]))
        return result

    # ---- after the pass ------------------------------------------------------------------------------------------------
    def report(self, batch):
        rows = self.rows
        assert rows, f"{self.tag}: no conv launch was intercepted"
        inv = Counter(r["plan"] for r in rows)
        wf = max(rows, key=lambda r: r["frame_rel"])
        split = [r for r in rows if r["ratio"] is not None]
        f16 = [r for r in rows if r["plan"][0] in R.F16_PLANS]
        st = [r["stats"] for r in rows if r["stats"][0] is not None]
        line = (f"PARITY conv launches vs fp64 [{self.tag}]: {len(rows)} launches x {batch} frames; worst per-frame max "
                f"{wf['frame_rel']:.2e} of max|ref| ({wf['name']} {wf['plan']}, frame {wf['frame']})")
        if split:
            wr = max(split, key=lambda r: r["ratio"])
            wm = max(split, key=lambda r: r["max_ratio"])
            line += (f"; worst mean-error ratio to the fp32 MFMA kernel {wr['ratio']:.3f} ({wr['name']} {wr['plan']}, "
                     f"rel mean {wr['mean_rel']:.2e}), worst max-error ratio {wm['max_ratio']:.3f} ({wm['name']})")
        if f16:
            w16 = max(f16, key=lambda r: r["mean_of_max"])
            line += f"; fp16 operands: worst launch mean {w16['mean_of_max']:.2e} of max|ref| ({w16['name']} {w16['plan']})"
        if st:
            line += (f"; tile statistics of {len(st)} launches: scale {max(s[0] for s in st):.1e} rel, "
                     f"shift {max(s[1] for s in st):.1e} abs")
        line += "; inventory (precision, cfg, ksplit, form) -> launches: " + str(dict(sorted(inv.items(), key=str)))
        print(line)
        return inv

    def assert_clean(self, batch, networks):
        bad = [f"{r['name']} {r['shape']} {r['plan']} {r['flags']}: {f}" for r in self.rows for f in r["failures"]]
        assert not bad, f"{self.tag}: {len(bad)} violations:\n" + "\n".join(bad[:40])
        assert len(self.rows) == self.intercepted
        assert all(r["frames"] == r["shape"][1][0] == batch for r in self.rows), "a launch was not checked on every frame"
        launched = {id(r["layer"]) for r in self.rows}
        missed = [c.name for c in packed_convs(*networks) if id(c) not in launched]
        assert not missed, f"{self.tag}: layers never launched: {missed}"


def _run(monkeypatch, tag, batch, networks, fn, guard):
    chk = LaunchChecker(tag)
    with monkeypatch.context() as mp:
        chk.install(mp)
        fn()
    torch.cuda.synchronize()
    inv = chk.report(batch)
    assert guard() == {}, f"{tag}: a split launch was replaced by its guarded recomputation: {guard()}"
    chk.assert_clean(batch, networks)
    return chk, inv


@pytest.fixture(scope="module")
def driver_setup():
    cfg = config.hot_path_config(overrides={"image_size": 512})
    sd = random_init.trained_like_state_dict(cfg, seed=0, with_source=False)
    _, _, x = _full_size(512, 16, seed=512)
    return cfg, sd, x


def _driver(hp, x, frames):
    d = lambda t: t.to(DEV)
    ccl = hp.prepare_canonical(d(x["canonical"]))
    return lambda: hp.driver_pass(ccl, d(x["idt"]), d(x["pose_t"][frames]), d(x["th_t"][frames]))


@pytest.mark.parametrize("mode", [nets.DEFAULT_PRECISION, "bf16x3", "f32", "f16"])
def test_driver_pass_B16_every_launch_vs_fp64(mode, driver_setup, monkeypatch):
    """the bench step: R512 driver pass, 16 frames, trained-like checkpoint"""
    cfg, sd, x = driver_setup
    hp = nets.HotPath(sd, cfg, DEV, with_source=False, precision=mode)
    chk, inv = _run(monkeypatch, f"driver R512 B=16 {mode}", 16, (hp.uv_generator, hp.decoder), _driver(hp, x, slice(0, 16)),
                    hp.overflow_events)
    rows = chk.rows
    if mode == "f16x2":
        up_conv1 = {id(blk.conv1) for blk, ups in hp.decoder.up if ups}
        seen = {(id(r["layer"]), r["in_w"]) for r in rows if r["plan"][3] == "up2"}
        assert {w for lid, w in seen if lid in up_conv1} == {64, 128, 256} and {lid for lid, _ in seen} == up_conv1, seen
        assert any(r["plan"][3] == "pointwise" for r in rows), inv
        assert any(r["plan"][0] == "f16x2" and r["plan"][1] == pack.CFG_F for r in rows), inv
    if mode == "f16":
        assert any(r["plan"][:1] == ("f16w8",) and r["plan"][3] == "direct" for r in rows), inv
        assert any(r["plan"][3] == "f16w8_rest" and r["layer"].cout == 320 for r in rows), inv


@pytest.mark.parametrize("mode", [nets.DEFAULT_PRECISION, "f32"])
def test_driver_pass_B1_every_launch_vs_fp64(mode, driver_setup, monkeypatch):
    """one frame per call: the planner splits the K loop of the small launches"""
    cfg, sd, x = driver_setup
    hp = nets.HotPath(sd, cfg, DEV, with_source=False, precision=mode)
    chk, inv = _run(monkeypatch, f"driver R512 B=1 {mode}", 1, (hp.uv_generator, hp.decoder), _driver(hp, x, slice(0, 1)),
                    hp.overflow_events)
    assert any(r["plan"][2] > 1 for r in chk.rows), inv


@pytest.mark.parametrize("mode", [nets.DEFAULT_PRECISION, "f32"])
def test_source_pass_R512_every_launch_vs_fp64(mode, monkeypatch):
    cfg, sd, x = _full_size(512, 1, seed=21)
    hp = nets.HotPath(sd, cfg, DEV, precision=mode)
    d = lambda t: t.to(DEV)
    nets_used = (hp.local_encoder, hp.xy_generator, hp.volume_source, hp.volume_process)
    _run(monkeypatch, f"source R512 {mode}", 1, nets_used,
         lambda: hp.source_pass(d(x["img"]), d(x["idt"]), d(x["pose_s"]), d(x["th_s"])), hp.overflow_events)


@pytest.mark.parametrize("variant", ["bn", "gn_ws"])
def test_stage2_R512_every_launch_vs_fp64(variant, monkeypatch):
    over = dict(output_size_s2=512)
    if variant == "gn_ws":
        over.update(norm_layer_type="gn", use_ws=True)
    cfg = stage2.stage2_config(overrides=over)
    sd = stage2.random_state_dict(cfg, seed=5)
    B = 4
    g = torch.Generator().manual_seed(6)
    img = torch.rand(B, 3, 512, 512, generator=g).to(DEV)
    mask = (torch.rand(B, 1, 512, 512, generator=g) > 0.1).float().to(DEV)
    face = (torch.rand(B, 1, 512, 512, generator=g) > 0.3).float().to(DEV)
    s2 = stage2.Stage2(sd, cfg, DEV, precision=nets.DEFAULT_PRECISION)
    _run(monkeypatch, f"stage2 R512 {variant} B={B}", B, (s2,), lambda: s2.refine(img, mask, face),
         lambda: ops.overflow_events(s2.device))
