"""The plan lattice of tests/test_conv_plan_lattice_gpu.py on the host, before it touches a GPU.

The lattice probes the edges of the planner and of the C launchers; here an out-of-range access is a host crash, not a GPU fault.
ops.conv_igemm runs as it is -- planner, packing, launch arguments -- with the host-compiled copy of the conv library
(tests/emul/convlib.py) in place of the product library and CPU tensors in place of device tensors.  Per precision mode:
  * EVERY geometry that REFUSED describes (a refused launch costs nothing): properties 2 - 4, the list against the C code itself;
  * of the accepted geometries of the product, the smallest one of every distinct (executed plan, taps, fused upsample, width
    class), and every geometry of EXTRA: properties 1, 3, 5 and 6 with the same checker and bounds (tile statistics through
    conv_reference.groupnorm_affine_fp64).

What the host does not run, and why.  A block of the emulation is 256 OS threads, about a second per 10 M multiply-adds, so a
geometry of more than HOST_MACS is not run here.  For a group of the product whose smallest geometry is larger, the same
code-selecting axes are tried with smaller drawn ones (channel counts, N = 1) and taken where the executed plan stays the same.
What is still too large -- plans the planner makes only for launches that fill the chip, the Cin = 1032 case, the N = 32 and
256- / 512-channel entries of EXTRA -- is left to the GPU run and counted in the PARITY line.  In the modes other than f32, a
geometry whose launch the planner puts on the fp32 kernel is the launch the f32 mode makes of the same geometry (the same TABLE
row, the same fp32 weights and plan): it runs once, in the f32 mode, and the other modes only hold its key to the f32 mode's.

The plan of a geometry is read from a planning-only call (a library stand-in that refuses every launch) with the geometry's own
N and its tensors at their offsets, so the selection runs no kernel and groups by the plan that will execute.  The drawn table is
held to its generator here as well.

Every C call of a refused or a run geometry also goes, with the same arguments, to emo_conv_accepts (_Asked): the question the
planner plans by returns the code the entry returns."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import convlib  # noqa: E402
import conv_reference as R  # noqa: E402
import test_conv_plan_lattice_gpu as L  # noqa: E402
from conv_plans import executed  # noqa: E402
from emoportraits_amd import hip, ops, pack  # noqa: E402

needs_lib = pytest.mark.skipif(not convlib.available(), reason="needs ROCm clang++ and the built product library")


class _Refuser:
    """a conv library that refuses every launch: ops.conv_igemm plans, packs, and raises"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.startswith("emo_conv_igemm") and name != "emo_conv_igemm_ksplit":
            return lambda *a: -2
        return getattr(self._real, name)


@pytest.fixture(scope="module")
def host():
    """ops.conv_igemm on CPU tensors through the host-compiled conv library -> the library"""
    lib = convlib.build()
    for name, argtypes in hip.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
            getattr(lib, name).restype = ctypes.c_int
    mp = pytest.MonkeyPatch()
    mp.setattr(hip, "load", lambda: lib)
    mp.setattr(hip, "require_cuda_f32", lambda *t: None)
    mp.setattr(hip, "current_stream", lambda: None)
    L.low_fill_thresholds(mp)
    _PLANS.clear()
    yield lib
    mp.undo()


_ENTRY_OF = {"emo_conv_igemm_f32": "f32", "emo_conv_igemm_f32_guarded": "f32_guarded", "emo_conv_igemm_bf16x3": "bf16x3",
             "emo_conv_igemm_f16x2": "f16x2", "emo_conv_igemm_f16acc32": "f16", "emo_conv_igemm_f16w8": "f16w8",
             "emo_conv_igemm_f16w8_rest": "f16w8_rest"}


class _Asked:
    """the host library, whose convolution entries first put their own arguments to emo_conv_accepts (tensors as null or not and
    their address modulo 16, the library's CU count): the question's code must be the code the entry then returns"""

    def __init__(self, lib):
        self._lib, self.asked, self.bad = lib, 0, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _ENTRY_OF:
            return fn

        def entry(*args):
            k = 3 if name.endswith("_rest") else 2          # x, the weights, then what all entries share: bias .. stream
            x, w, w16 = args[0], args[1], args[2] if k == 3 else None
            ints, (ws, gn, _), extra = args[k + 5:k + 20], args[k + 20:k + 23], args[k + 23:]
            in_scale, w_scale, flag, run_if = 1.0, 1.0, None, None
            if name == "emo_conv_igemm_f16x2":
                in_scale, w_scale, flag = extra
            elif name in ("emo_conv_igemm_bf16x3", "emo_conv_igemm_f32_guarded"):
                run_if, = extra
            elif extra:
                w_scale, = extra
            addr = [p.value if isinstance(p, ctypes.c_void_p) else p for p in (x, w, w16, *args[k:k + 5], ws, gn, flag, run_if)]
            tensors = (ctypes.c_int * 12)(*(-1 if not a else a % 16 for a in addr))
            code = self._lib.emo_conv_accepts(pack._ENTRIES[_ENTRY_OF[name]], tensors, *ints, in_scale, w_scale, 0)
            rc = fn(*args)
            self.asked += 1
            if rc != code:
                self.bad.append(f"{name}{tuple(ints)}: the entry returned {rc}, emo_conv_accepts {code}")
            return rc
        return entry


_PLANS = {}     # geometry -> its planned launch (one planning call per geometry and session)


def _planned(g, lib, mp):
    """executed() of the launch run_geometry will make for g -- its N, its input and output at their offsets -- without running a
    kernel -> (precision, cfg, K split > 1, form)"""
    if g in _PLANS:
        return _PLANS[g]
    x, w, b, sc, sh, res, oshape = L._operands(g, 0, "cpu")
    kd = w.shape[2] if w.dim() == 5 else 1
    layer = pack.PackedConv("plan", w, b, "cpu", precision=L.layer_precision(g.mode, g.cout, g.cin, kd, w.shape[-2], w.shape[-1]))
    out = torch.empty(oshape, dtype=torch.float32)
    if g.offset == "out":
        out = L._offset4(out)
    mp.setattr(hip, "load", lambda: _Refuser(lib))
    try:
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            ops.conv_igemm(x, layer, sc, sh, relu_in=g.relu_in, ups=g.ups, res=res, res_ups=g.res == "up2", out=out, want_stats=g.stats)
    finally:
        mp.setattr(hip, "load", lambda: lib)
    prec, cfg, ks, form = executed(layer, out)
    _PLANS[g] = (prec, cfg, ks > 1, form)
    return _PLANS[g]


def _work(g):
    return g.N * g.cout * g.cin * g.Hl * g.W * {"1x1": 1, "3x3": 9, "3x3x3": 81, "stem": 49}[g.taps]


HOST_MACS = 20e6


def _groups(mode, lib, mp):
    """-> (every geometry of the product REFUSED describes, {(planned launch, taps, upsample, width class): smallest geometry})"""
    refused, groups = [], {}
    for g in L.lattice(mode):
        if L.refusing_rule(g) is not None:
            refused.append(g)
            continue
        key = (_planned(g, lib, mp), g.taps, g.ups, pack.width_class(g.W))
        if key not in groups or _work(g) < _work(groups[key]):
            groups[key] = g
    return refused, groups


def subset(mode, lib, mp):
    """-> (refused geometries, accepted geometries to run, groups and extras left to the GPU run)"""
    refused, groups = _groups(mode, lib, mp)
    if mode != "f32":
        # a launch on the fp32 kernel is the f32 mode's launch of the same geometry: run there, held to its key here
        f32_keys = set(_groups("f32", lib, mp)[1])
        on_f32 = {k for k in groups if k[0][0] == "f32"}
        assert on_f32 <= f32_keys, sorted(on_f32 - f32_keys, key=str)
        groups = {k: g for k, g in groups.items() if k not in on_f32}
    small, left = [], []
    for key, g in groups.items():
        if _work(g) > HOST_MACS:
            # the same code-selecting axes with smaller drawn ones (channel counts, N), where the launch stays the same plan
            shrunk = sorted((g._replace(N=1, cout=co, cin=ci) for co in L.COUTS for ci in L.CINS if g.cin <= 40), key=_work)
            g = next((c for c in shrunk if _work(c) <= HOST_MACS and _planned(c, lib, mp) == key[0]), None)
        if g is None:
            left.append(key)
        else:
            small.append(g)
    for g in L.EXTRA:
        if g.mode == mode:
            # (ops.conv_head's kernel is not part of the host-compiled conv library)
            (small if g.entry == "igemm" and _work(g) <= HOST_MACS else left).append(g)
    return refused, small, left


@needs_lib
@pytest.mark.parametrize("mode", L.MODES)
def test_lattice_subset_on_the_host(mode, host, monkeypatch):
    refused, accepted, left = subset(mode, host, monkeypatch)
    asked = _Asked(host)
    monkeypatch.setattr(hip, "load", lambda: asked)
    rows, bad = L.run_slice(refused + accepted, dev="cpu", affine=R.groupnorm_affine_fp64, seed0=1000 * L.MODES.index(mode))
    named = sorted(f"EXTRA {g.taps} {g.cout}<-{g.cin} {g.Hl}x{g.W} N={g.N}" if isinstance(g, L.Geometry) else str(g) for g in left)
    print(L.summary(f"host emulation, {mode}", rows) + f"; {len(left)} groups (plan, taps, upsample, width class) / entries of EXTRA "
          f"left to the GPU run: {named}")
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(bad[:40])
    ran = {r["plan"][2] for _, r in rows if r["status"] == "ran"}
    assert ran, "no accepted launch ran on the host"
    if mode != "f32":
        assert ran - {"f32"}, f"no launch of the {mode} mode ran one of its own kernels on the host: {ran}"
    assert pack.overflow_events("cpu") == {}
    assert asked.asked >= len(accepted) and not asked.bad, f"{len(asked.bad)} of {asked.asked} questions:\n" + "\n".join(asked.bad[:40])


def test_the_table_is_the_drawn_one():
    assert L.TABLE == L.draw_table(L.TABLE_SEED, L.TABLE_ROWS)


def test_every_refusal_rule_describes_some_geometry_and_the_table_covers_its_axes():
    geoms = L.lattice("f32")
    for quote, pred in L.REFUSED:
        assert any(pred(g) for g in geoms), quote
    for mode in L.MODES:
        geoms = L.lattice(mode)
        for field, values in (("cout", L.COUTS), ("cin", L.CINS + (1032,)), ("N", (1, 2)), ("affine", (False, True)), ("relu_in", (False, True)),
                              ("res", L.RES), ("stats", (False, True)), ("offset", L.OFFSETS)):
            assert {getattr(g, field) for g in geoms if g.taps != "stem" or field != "cin"} >= set(values), (mode, field)
