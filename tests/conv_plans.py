"""Which convolution kernel a launch ran (a helper module, not a test file).

executed() reads the plan ops.conv_igemm / ops.conv_head left on the layer (last_launch: what the product ran); Expect is what a
test case declares about its launch, and check() holds a launch to it.  One copy: the parity tests (run_conv of
tests/test_kernels_gpu.py), the launch checker of tests/test_conv_launches_fp64_gpu.py and the plan lattice all read "what ran" here.
"""
from collections import namedtuple

FORMS = ("direct", "up2", "pointwise", "f16w8_rest", "stream")


def executed(layer, out):
    """(precision, block config, K split, form) of the last launch of `layer`, which wrote `out`: the product's own record of it
    (layer.last_launch, the pack.ConvPlan that ops.conv_igemm / conv_head / stage2_head executed), nothing derived here.
    precision: 'f32' | 'bf16x3' | 'f16x2' | 'f16' | 'f16w8' | 'stream'; form: 'stream' (ops.conv_head's kernel), 'pointwise' (the
    fp16 split's 1x1 kernel), 'f16w8_rest' (an odd channel-tile count: pairs on the eight-wave kernel, the last tile on the older
    fp16-operand kernel), 'up2' (the phase form of a fused-upsample 3x3) or 'direct'"""
    plan = layer.last_launch
    assert plan.form in FORMS and tuple(plan[:3]) == tuple(layer.last_plan), (plan, layer.last_plan)
    return plan.prec, plan.cfg, plan.ksplit, plan.form


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
