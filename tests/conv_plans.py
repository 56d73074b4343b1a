"""Which convolution kernel a launch ran (a helper module, not a test file).

executed() reads what ops.conv_igemm / ops.conv_head left on the layer and names the launch form; Expect is what a test case
declares about its launch, and check() holds a launch to it.  One copy: the parity tests (run_conv of tests/test_kernels_gpu.py),
the launch checker of tests/test_conv_launches_fp64_gpu.py and the plan lattice all derive "what ran" here.
"""
from collections import namedtuple

from emoportraits_amd import pack

FORMS = ("direct", "up2", "pointwise", "f16w8_rest", "stream")


def executed(layer, out):
    """(precision, block config, K split, form) of the last launch of `layer`, which wrote `out`.
    precision: 'f32' | 'bf16x3' | 'f16x2' | 'f16' | 'f16w8' | 'stream' (PackedConv.last_plan); form: 'stream' (ops.conv_head's
    kernel), 'pointwise' (the fp16 split's 1x1 kernel), 'f16w8_rest' (an odd channel-tile count: pairs on the eight-wave kernel, the
    last tile on the older fp16-operand kernel), 'up2' (the phase form of a fused-upsample 3x3) or 'direct'"""
    cfg, ks, prec = layer.last_plan
    if prec == "stream":
        form = "stream"
    elif prec == "f16x2" and layer.pointwise_split:
        form = "pointwise"
    elif prec == "f16w8" and pack.f16w8_rest_fits(layer.cout, out.shape[-2], out.shape[-1]):
        form = "f16w8_rest"
    else:
        form = getattr(layer, "last_form", None) or "direct"
    return prec, cfg, ks, form


class Expect(namedtuple("Expect", "prec cfg form split")):
    """what a conv case declares about its launch: plan precision, block config (None: the planner's choice), form (FORMS), and
    whether the K loop is split over the grid"""
    __slots__ = ()

    def __new__(cls, prec, cfg, form="direct", split=False):
        assert form in FORMS, form
        return super().__new__(cls, prec, cfg, form, bool(split))


# what an entry of a case table may declare about its launches next to run_conv's own arguments -- split: the K loop of the case's
# launch is split; f32_split: that of its fp32 twin is; odd_tiles: an odd channel-tile count >= 3 (the 'f16w8_rest' form)
DECLARATIONS = ("split", "f32_split", "odd_tiles")


def split_case(case):
    """a table entry -> (run_conv's arguments, its declarations: every key of DECLARATIONS, False where the entry has none)"""
    kw = {k: v for k, v in case.items() if k not in DECLARATIONS}
    return kw, {k: bool(case.get(k, False)) for k in DECLARATIONS}


def mismatch(expect, ran):
    """None when the launch `ran` (executed()'s tuple) is the one `expect` declares, else a message that names the plan that ran"""
    prec, cfg, ks, form = ran
    ok = prec == expect.prec and (expect.cfg is None or cfg == expect.cfg) and form == expect.form and (ks > 1) == expect.split
    if ok:
        return None
    return (f"the case declares {tuple(expect)} (precision, cfg, form, K split > 1); "
            f"the launch ran (precision, cfg, ksplit, form) = {(prec, cfg, ks, form)}")


def check(expect, layer, out):
    """assert that the last launch of `layer` is the declared one -> executed()'s tuple"""
    if not isinstance(expect, Expect):
        raise TypeError("expect must be a conv_plans.Expect")
    ran = executed(layer, out)
    bad = mismatch(expect, ran)
    assert bad is None, f"{layer.name}: {bad}"
    return ran
