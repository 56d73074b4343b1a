"""Every C-ABI call the convolution ops make, as a record that can be held against another commit's.

ops.conv_igemm / ops.conv_head / ops.stage2_head run as they are -- planner, packing, allocation, launch arguments -- on CPU
tensors against the stub library of tools/host_overhead.py (every kernel entry point returns EMO_OK, the pack-info queries go to
the real library).  Each call of an emo_conv_igemm*, emo_conv_head_f32 or emo_stage2_head_f32 entry is written down: integers and
floats by value, pointers as tokens that do not depend on the addresses of a run --
  null                      a null pointer
  <role>+<bytes>            a known tensor of the op call and the byte offset into it: x, scale, shift, res, bias, out (the caller's
                            out=), flags (the overflow-flag pool), img, mask, face_mask; two roles that share memory are joined
                            with '|' (out= aliasing res)
  weight:<key>              the address of layer._packed[key]
  new#i%r                   a buffer the op allocated, numbered by first appearance within the op call; r = its address % 16
-- and, after the op returns, layer.last_plan / layer.last_form, whether the result is the caller's out, and the shape and cnt of
the returned TileStats.  A case is a list of such op records; the fixture tests/golden/conv_launch_trace.json holds the first 16
hex digits of the sha256 of every case's canonical JSON, and tests/test_conv_launch_trace.py regenerates and compares them.

    python tools/conv_launch_trace.py                  the fixture, to stdout
    python tools/conv_launch_trace.py --write PATH     the fixture, to a file
    python tools/conv_launch_trace.py --list           the case keys
    python tools/conv_launch_trace.py --dump KEY       the full record of one case (diff it against another checkout's)

The cases (CASES below): the plan lattice of tests/test_conv_plan_lattice_gpu.py in its four modes and its EXTRA entries, under the
product's fill thresholds and under the lowered ones; the fp16-split lattice with the guard off; explicit ksplit= and pinned block
configs; out= aliasing res; HotPath.driver_pass and the stage-2 passes in the four conv modes.  pack.cu_count is pinned to 256
(the planner's questions to the library carry it) and every case starts with an empty overflow-flag pool, so a record depends neither
on the machine nor on the cases that ran before it.
"""
import contextlib
import ctypes
import functools
import hashlib
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import host_overhead  # noqa: E402
import test_conv_plan_lattice_gpu as L  # noqa: E402
from emoportraits_amd import config, hip, nets, ops, pack, random_init, stage2  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_launch_trace.json")
OPS = ("conv_igemm", "conv_head", "stage2_head")
ROLES = ("x", "scale", "shift", "res", "bias", "out", "flags", "img", "mask", "face_mask")


def _traced_entry(name):
    return (name.startswith("emo_conv_igemm") and name != "emo_conv_igemm_ksplit") or name in ("emo_conv_head_f32", "emo_stage2_head_f32")


class Tracer:
    """the library the ops see (traced entries are written down, everything else goes to the stub) and the wrappers of the ops"""

    def __init__(self, stub):
        self.stub, self.records, self.stack = stub, [], []

    def __getattr__(self, name):
        if _traced_entry(name):
            return functools.partial(self._launch, name)
        return getattr(self.stub, name)

    def _token(self, ctx, addr):
        for key, t in ctx["layer"]._packed.items():
            if t.data_ptr() == addr:
                return f"weight:{key}"
        hits = [f"{role}+{addr - t.data_ptr()}" for role, t in ctx["roles"]
                if t.data_ptr() <= addr < t.data_ptr() + max(1, t.numel() * t.element_size())]
        if hits:
            return "|".join(hits)
        i = ctx["new"].setdefault(addr, len(ctx["new"]))
        return f"new#{i}%{addr % 16}"

    def _launch(self, name, *args):
        ctx = self.stack[-1]
        types = hip.SIGNATURES[name]
        assert len(types) == len(args), (name, len(types), len(args))
        out = []
        for a, ty in zip(args, types):
            if ty is ctypes.c_void_p:
                addr = a.value if isinstance(a, ctypes.c_void_p) else a
                out.append("null" if not addr else self._token(ctx, int(addr)))
            else:
                out.append(float(a) if ty is ctypes.c_float else int(a))
        ctx["record"]["launches"].append({"entry": name, "args": out})
        return 0

    def wrap(self, name, real):
        sig = inspect.signature(real)

        @functools.wraps(real)
        def op(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            layer, caller_out = a["layer"], a.get("out") if isinstance(a.get("out"), torch.Tensor) else None
            known = dict(x=a["x"], scale=a.get("scale"), shift=a.get("shift"), res=a.get("res"), bias=layer.bias, out=caller_out,
                         flags=pack._flag_pool(a["x"].device)[0], img=a.get("img"), mask=a.get("mask"), face_mask=a.get("face_mask"))
            record = {"op": name, "layer": layer.name, "launches": []}
            self.records.append(record)
            self.stack.append({"layer": layer, "roles": [(r, known[r]) for r in ROLES if known[r] is not None], "new": {}, "record": record})
            try:
                ret = real(*args, **kwargs)
            except Exception as e:
                record["error"] = [type(e).__name__, str(e)]
                raise
            finally:
                self.stack.pop()
            first = ret[0] if isinstance(ret, tuple) else ret
            stats = ret[1] if name == "conv_igemm" and a["want_stats"] else None
            plan = getattr(layer, "last_plan", None)
            record["after"] = {"last_plan": None if plan is None else list(plan), "last_form": getattr(layer, "last_form", None),
                               "returns_out": caller_out is not None and first is caller_out,
                               "stats": None if stats is None else [list(stats.stats.shape), stats.cnt]}
            return ret
        return op


@contextlib.contextmanager
def tracing(low_fill=False, guard=True):
    """the ops of emoportraits_amd against a Tracer; everything is put back on exit -> the Tracer"""
    mp = pytest.MonkeyPatch()
    try:
        tracer = Tracer(host_overhead.install_stub(mp.setattr))
        mp.setattr(hip, "load", lambda: tracer)
        pack.cu_count.cache_clear()
        mp.setattr(pack, "cu_count", lambda: 256)
        mp.setattr(pack, "_flag_pools", {})
        mp.delenv("EMO_CONV_CT2_MIN_ITEMS", raising=False)
        mp.delenv("EMO_F16X2_P1_MIN_ITEMS", raising=False)
        if low_fill:
            L.low_fill_thresholds(mp)
        mp.setattr(ops, "F16X2_GUARD", guard)         # (a module attribute, as bench.py sets it)
        for name in OPS:
            mp.setattr(ops, name, tracer.wrap(name, getattr(ops, name)))
        yield tracer
    finally:
        mp.undo()
        pack.cu_count.cache_clear()


# ---- one launch of a lattice geometry ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4096)
def _operands(g):
    return L._operands(g, 0, "cpu")


def geometry_case(g, low_fill=False, guard=True, cfg=None, alias_res=False, **kwargs):
    """one op call of geometry g, set up as _planned of tests/test_conv_plan_lattice_emul.py sets it up -> the case's records"""
    x, w, b, sc, sh, res, oshape = _operands(g)
    kd = w.shape[2] if w.dim() == 5 else 1
    with tracing(low_fill, guard) as tr:
        try:
            layer = pack.PackedConv("plan", w, b, "cpu", cfg=cfg, precision=L.layer_precision(g.mode, g.cout, g.cin, kd, w.shape[-2], w.shape[-1]))
            if g.entry == "head":
                ops.conv_head(x, layer, sc, sh, relu_in=g.relu_in)
            else:
                out = res if alias_res else torch.empty(oshape, dtype=torch.float32)
                if g.offset == "out" and not alias_res:
                    out = L._offset4(out)
                ops.conv_igemm(x, layer, sc, sh, relu_in=g.relu_in, ups=g.ups, res=res, res_ups=g.res == "up2", out=out, want_stats=g.stats,
                               **kwargs)
        except Exception as e:
            if not tr.records or "error" not in tr.records[-1]:          # (refused before the op: the layer's constructor)
                tr.records.append({"op": "PackedConv", "error": [type(e).__name__, str(e)]})
        return tr.records


def _pinned_geometries():
    """six accepted geometries of the lattice and of EXTRA (64 wide at least, so that the split and fp16 kernels take them): 1x1 (a
    pointwise-split layer in the f16x2 mode), 3x3, 3x3x3, a fused upsample, tile statistics, a residual; and 'up2', the fused
    upsample with whole 64-channel tiles, which the phase form of the fp16 split takes"""
    wanted = (("1x1", lambda g: g.taps == "1x1" and pack.supports_f16x2_pointwise(g.cout, g.cin, 1, 1, 1)),
              ("3x3", lambda g: g.taps == "3x3" and not g.ups and g.res == "none" and not g.stats and g.offset == "none"),
              ("3x3x3", lambda g: g.taps == "3x3x3"),
              ("ups", lambda g: g.taps == "3x3" and g.ups and g.W >= 128 and g.res == "none" and g.offset == "none"),
              ("stats", lambda g: g.taps == "3x3" and g.stats and not g.ups and g.offset == "none"),
              ("res", lambda g: g.taps == "3x3" and g.res == "plain" and not g.ups))
    geoms = [g for g in L.lattice("f32") + list(L.EXTRA) if L.refusing_rule(g) is None and g.W >= 64 and g.Hl >= 4]
    picked = [(name, next(g for g in geoms if pred(g))) for name, pred in wanted]
    return picked + [("up2", dict(picked)["ups"]._replace(cout=192))]


# ---- whole passes ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hot_path_checkpoint(S):
    cfg = config.hot_path_config(overrides={"image_size": S})
    return cfg, random_init.trained_like_state_dict(cfg, seed=0, with_source=False)


def driver_case(S, B, mode):
    """HotPath.driver_pass as test_driver_pass_host_side_against_a_stub_library of tests/test_host_logic.py runs it"""
    cfg, sd = _hot_path_checkpoint(S)
    with tracing() as tr:
        hp = nets.HotPath(sd, cfg, "cpu", with_source=False, precision=mode)
        c, d, s = cfg["latent_volume_channels"], cfg["latent_volume_depth"], cfg["latent_volume_size"]
        ccl = hp.prepare_canonical(torch.empty(1, c, d, s, s))
        g = torch.Generator().manual_seed(0)
        hp.driver_pass(ccl, torch.randn(1, cfg["gen_max_channels"], 4, 4, generator=g),
                       torch.randn(B, cfg["lpe_output_channels_expression"], generator=g), torch.eye(4)[None].repeat(B, 1, 1).contiguous())
        return tr.records


@functools.lru_cache(maxsize=None)
def _stage2_checkpoint():
    cfg = stage2.stage2_config(overrides=dict(output_size_s2=512))
    return cfg, stage2.random_state_dict(cfg, seed=0)


def stage2_case(prec, call):
    """Stage2 at 512 x 512, 8 frames: 'refine'; 'frames' (refine_frames: the stream tail, ops.stage2_head); 'frames_unaligned' (an
    image 4 bytes off a 16-byte boundary: the tail's fallback onto conv_igemm)"""
    cfg, sd = _stage2_checkpoint()
    with tracing() as tr:
        s2 = stage2.Stage2(sd, cfg, "cpu", precision=prec)
        img, m, f = torch.empty(8, 3, 512, 512), torch.empty(8, 1, 512, 512), torch.empty(8, 1, 512, 512)
        if call == "refine":
            s2.refine(img, m, f)
        else:
            s2.refine_frames(L._offset4(img) if call == "frames_unaligned" else img, m, f)
        return tr.records


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _cases():
    """{key: function that makes the case's records}, in a fixed order"""
    cases = {}
    for fill in ("product", "low"):
        for mode in L.MODES:
            for i, g in enumerate(L.lattice(mode)):
                cases[f"a/{fill}/{mode}/{i:03d}"] = functools.partial(geometry_case, g, fill == "low")
        for i, g in enumerate(L.EXTRA):
            cases[f"a/{fill}/extra/{i:02d}"] = functools.partial(geometry_case, g, fill == "low")
    for i, g in enumerate(L.lattice("f16x2")):
        cases[f"b/unguarded/{i:03d}"] = functools.partial(geometry_case, g, True, False)
    for name, g32 in _pinned_geometries():
        for mode in L.MODES:
            g = g32._replace(mode=mode)
            for ks in (1, 2, 4):
                cases[f"c/{name}/{mode}/ksplit{ks}"] = functools.partial(geometry_case, g, True, ksplit=ks)
            for letter in "ABCDEFG":
                cases[f"c/{name}/{mode}/cfg{letter}"] = functools.partial(geometry_case, g, True, cfg=getattr(pack, "CFG_" + letter))
    alias = {"3x3": L.Geometry("f16x2", "3x3", 128, 4, False, 96, 8, 1, True, True, "plain", True, "none"),
             "pointwise": L.Geometry("f16x2", "1x1", 64, 4, False, 128, 64, 1, False, False, "plain", True, "none")}
    for name, g in alias.items():
        for guard in (True, False):
            for stats in (True, False):
                cases[f"d/{name}/{'guarded' if guard else 'unguarded'}/{'stats' if stats else 'plain'}"] = \
                    functools.partial(geometry_case, g._replace(stats=stats), True, guard, alias_res=True)
    for S, B in ((512, 16), (512, 1), (256, 32)):
        for mode in L.MODES:
            cases[f"e/R{S}/B{B}/{mode}"] = functools.partial(driver_case, S, B, mode)
    for prec in ("f32", "bf16x3", "f16x2", "f16"):
        for call in ("refine", "frames", "frames_unaligned"):
            cases[f"f/{prec}/{call}"] = functools.partial(stage2_case, prec, call)
    return cases


CASES = _cases()


def canonical(records):
    return json.dumps(records, sort_keys=True, separators=(",", ":"))


def digest(key):
    return hashlib.sha256(canonical(CASES[key]()).encode()).hexdigest()[:16]


def digests():
    try:
        return {key: digest(key) for key in CASES}
    finally:
        for cache in (_operands, _hot_path_checkpoint, _stage2_checkpoint):
            cache.cache_clear()


def fixture_text(d):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in d.items()) + "\n}\n"


def main(argv):
    if argv[:1] == ["--list"]:
        print("\n".join(CASES))
    elif argv[:1] == ["--dump"]:
        print(json.dumps(CASES[argv[1]](), sort_keys=True, indent=1))
    elif argv[:1] == ["--write"]:
        with open(argv[1], "w") as f:
            f.write(fixture_text(digests()))
    else:
        sys.stdout.write(fixture_text(digests()))


if __name__ == "__main__":
    main(sys.argv[1:])
