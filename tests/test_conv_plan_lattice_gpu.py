"""The planner against the C launcher on a lattice of small geometries, every accepted launch against fp64.

tests/test_kernels_gpu.py and its companions pick their geometries by hand; the edges of pack.PackedConv.plan_for -- height
residues, width classes, the fused upsample on narrow maps, Cin % 8, Cin > 1024 with an affine, 4-byte-aligned tensors -- are
swept here.  A geometry is ONE launch through ops.conv_igemm of a layer built for a precision mode the way the networks build
theirs (the mode where the layer's kernel exists, fp32 elsewhere), N <= 2, Cin <= 40: milliseconds.

The axes that select code are a full product (LATTICE): output width x output height x fused upsample x taps x precision mode.
The other axes (channel counts, input affine / ReLU, residual form, tile statistics, a tensor 4 bytes off a 16-byte boundary, N)
come from TABLE, drawn once from a seeded generator (draw_table) and written out below; geometry i of a mode takes row
i % len(TABLE), so every row -- every value of every axis -- occurs in every mode.  One geometry per mode carries Cin = 1032 with
an affine (the scale / shift table of the fp16 and split kernels holds 1024 channels).  EXTRA holds the geometries added for
launch forms of the R256 driver pass (the pass bench.py times as r256_fps) that the product does not produce -- among them the only
accepted 8-wide maps: that width class tiles the depth in pairs, and the product's depths are 1 and 3.

Per geometry, none skipped:
  1. the plan the planner chose is accepted by the C entry point, or
  2. the fp32 plan of the same geometry is refused as well, with EMO_ERR_UNSUPPORTED;
  3. (a split or fp16 plan that C refuses while the fp32 plan runs is a failure;)
  4. the geometries refused both ways are exactly those REFUSED describes, each rule quoting the C condition that refuses;
  5. an accepted launch meets the fp64 bounds of its plan's arithmetic (conv_reference.check_launch: FP32_FRAME, SPLIT_MEAN /
     SPLIT_MAX against the fp32 twin, F16_FRAME / F16_MEAN, STATS_TOL -- no tolerance of this file's own);
  6. a second launch on the same inputs is bit-identical, output and tile statistics.

The fill thresholds of the pair kernels (EMO_CONV_CT2_MIN_ITEMS, EMO_F16X2_P1_MIN_ITEMS: two items per CU by default) are set to
1, as the kernel tests do, so that launches this small reach the kernels the full-size passes run.

run_geometry / run_slice take the device and the statistics affine as arguments: tests/test_conv_plan_lattice_emul.py runs a
subset of the same geometries through the host-compiled conv library before this file goes to a GPU.
"""
import functools
import inspect
import itertools
import math
import random
from collections import namedtuple

import pytest
import torch

import conv_reference as R
from conv_plans import executed
from emoportraits_amd import config, nets, ops, pack, random_init

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"

MODES = ("f32", "f16", "bf16x3", "f16x2")
WIDTHS = (8, 16, 32, 64, 128, 192, 256)
HEIGHTS = (2, 4, 6, 8, 16)
TAPS = ("1x1", "3x3", "3x3x3", "stem")     # 3x3x3: D = 3; stem: the encoder's 7x7 on its [N, 3, H, 1, W] view (KD = 7 over rows, 1x7 taps)
UPS = (False, True)

COUTS = (32, 64, 96, 160, 192, 320)
CINS = (8, 12, 40)
RES = ("none", "plain", "up2")
OFFSETS = ("none", "in", "out")
TABLE_SEED, TABLE_ROWS = 20261, 23          # (a prime row count: no axis of the product walks the table in step)

Row = namedtuple("Row", "cout cin N affine relu_in res stats offset")
# entry: 'igemm' (ops.conv_igemm) | 'head' (ops.conv_head); D: depth of a 5-D input (None: 3 for 3x3x3 taps, a 4-D input for 1x1 / 3x3)
Geometry = namedtuple("Geometry", "mode taps W Hl ups cout cin N affine relu_in res stats offset entry D", defaults=("igemm", None))


def draw_table(seed=TABLE_SEED, rows=TABLE_ROWS):
    """every axis as a shuffled repetition of its values: each value occurs in at least rows // len(values) rows"""
    rng = random.Random(seed)

    def column(values):
        col = (list(values) * (-(-rows // len(values))))[:rows]
        rng.shuffle(col)
        return col

    cols = [column(COUTS), column(CINS), column((1, 2)), column((False, True)), column((False, True)), column(RES),
            column((False, True)), column(OFFSETS)]
    return tuple(Row(*r) for r in zip(*cols))


# draw_table() as drawn (tests/test_conv_plan_lattice_emul.py holds the two equal)
TABLE = (
    Row(cout=192, cin=8, N=2, affine=True, relu_in=True, res="up2", stats=False, offset="out"),
    Row(cout=160, cin=40, N=1, affine=True, relu_in=False, res="up2", stats=False, offset="in"),
    Row(cout=160, cin=8, N=2, affine=False, relu_in=True, res="none", stats=True, offset="none"),
    Row(cout=32, cin=40, N=2, affine=False, relu_in=False, res="up2", stats=True, offset="out"),
    Row(cout=320, cin=12, N=1, affine=False, relu_in=True, res="plain", stats=True, offset="none"),
    Row(cout=320, cin=12, N=1, affine=True, relu_in=True, res="none", stats=False, offset="in"),
    Row(cout=32, cin=8, N=1, affine=False, relu_in=True, res="up2", stats=False, offset="in"),
    Row(cout=32, cin=40, N=1, affine=False, relu_in=True, res="up2", stats=False, offset="none"),
    Row(cout=192, cin=40, N=2, affine=True, relu_in=True, res="plain", stats=True, offset="out"),
    Row(cout=32, cin=12, N=1, affine=True, relu_in=False, res="plain", stats=True, offset="out"),
    Row(cout=192, cin=12, N=1, affine=False, relu_in=False, res="up2", stats=True, offset="in"),
    Row(cout=64, cin=12, N=1, affine=True, relu_in=False, res="plain", stats=True, offset="in"),
    Row(cout=192, cin=8, N=2, affine=False, relu_in=True, res="plain", stats=True, offset="in"),
    Row(cout=64, cin=12, N=2, affine=False, relu_in=False, res="none", stats=True, offset="none"),
    Row(cout=320, cin=8, N=2, affine=True, relu_in=True, res="none", stats=False, offset="out"),
    Row(cout=160, cin=8, N=2, affine=False, relu_in=False, res="up2", stats=False, offset="out"),
    Row(cout=96, cin=12, N=2, affine=False, relu_in=False, res="none", stats=False, offset="out"),
    Row(cout=160, cin=12, N=2, affine=False, relu_in=False, res="plain", stats=True, offset="none"),
    Row(cout=64, cin=8, N=1, affine=True, relu_in=False, res="plain", stats=False, offset="none"),
    Row(cout=96, cin=8, N=1, affine=False, relu_in=False, res="none", stats=False, offset="in"),
    Row(cout=64, cin=40, N=2, affine=True, relu_in=True, res="none", stats=False, offset="none"),
    Row(cout=96, cin=40, N=1, affine=True, relu_in=True, res="none", stats=False, offset="in"),
    Row(cout=96, cin=40, N=1, affine=True, relu_in=False, res="plain", stats=True, offset="none"),
)


def lattice(mode):
    """the geometries of a precision mode: the full product of the code-selecting axes, each with its TABLE row"""
    out = []
    for i, (taps, W, Hl, ups) in enumerate(itertools.product(TAPS, WIDTHS, HEIGHTS, UPS)):
        r = TABLE[i % len(TABLE)]
        res = "plain" if (taps == "stem" and r.res == "up2") else r.res      # (the stem's plane is one row high: no x2 residual)
        out.append(Geometry(mode, taps, W, Hl, ups, r.cout, 3 if taps == "stem" else r.cin, r.N, r.affine, r.relu_in, res,
                            r.stats, r.offset))
    # Cin = 1032 with an affine: beyond the 1024-entry scale / shift tables of the fp16 and split kernels
    out.append(Geometry(mode, "3x3", 64, 8, False, 64, 1032, 1, True, True, "none", False, "none"))
    return out


# Launch forms of the R256 driver pass (B = 32 and B = 1, default mode and f32) that no geometry of the product has: the launches
# that fill the chip (the 256-position fp32 tiles, K splits at B = 1) need N = 32 or 256 / 512 channels, the 8-wide maps of the warp
# generator an even depth (D), which the product (D = 1 or 3) never has -- beyond the N <= 2, Cin <= 40 of the product, and still
# milliseconds each.  test_driver_pass_R256_launch_forms_are_in_the_lattice names a form that is missing here;
# test_every_extra_geometry_runs_a_form_of_its_own fails an entry that is not needed (any longer): one whose form the product or
# an earlier entry runs.  The 3x3 / 3x3x3 ones carry the input affine + ReLU of the norm in front of every such layer of the
# networks (the split kernels' bounds against the fp32 kernel are stated for such activations: conv_reference.SPLIT_MEAN)
EXTRA = (
    Geometry("f16x2", "3x3", 128, 4, False, 96, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, False, 96, 8, 1, True, True, "plain", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, False, 96, 8, 1, True, True, "up2", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, False, 160, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, False, 160, 8, 1, True, True, "plain", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, False, 160, 8, 1, True, True, "up2", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 64, 4, False, 128, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 64, 4, False, 128, 8, 1, True, True, "plain", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, True, 96, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 16, False, 128, 8, 1, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 16, False, 128, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 32, 8, False, 64, 8, 1, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 32, 8, False, 64, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "1x1", 64, 4, False, 128, 64, 1, False, False, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3", 64, 4, False, 128, 256, 1, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3", 64, 4, False, 128, 256, 1, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3", 128, 4, True, 3, 256, 1, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 16, False, 128, 96, 1, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 16, False, 128, 96, 1, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 32, 8, False, 64, 96, 1, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 64, 4, False, 32, 8, 1, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 64, 4, False, 32, 8, 1, True, True, "none", True, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 64, 4, False, 3, 8, 1, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "1x1", 16, 16, False, 512, 8, 32, False, False, "none", False, "none", "igemm", None),
    Geometry("f16x2", "1x1", 32, 64, False, 64, 8, 32, False, False, "none", False, "none", "igemm", None),
    Geometry("f16x2", "1x1", 64, 4, False, 512, 8, 32, False, False, "none", True, "none", "igemm", None),
    Geometry("f32", "1x1", 8, 8, False, 512, 8, 32, False, False, "none", False, "none", "igemm", 4),
    Geometry("f16x2", "3x3x3", 16, 8, False, 512, 8, 32, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 8, False, 512, 8, 32, True, True, "none", True, "none", "igemm", None),
    Geometry("f32", "3x3x3", 8, 8, False, 512, 8, 32, True, True, "plain", False, "none", "igemm", 4),
    Geometry("f32", "3x3x3", 8, 8, False, 512, 8, 32, True, True, "none", True, "none", "igemm", 4),
    Geometry("f16x2", "1x1", 64, 2, False, 256, 512, 32, False, False, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3", 256, 2, False, 160, 64, 32, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3", 256, 2, False, 160, 64, 32, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "3x3", 256, 2, False, 160, 64, 32, True, True, "up2", False, "none", "igemm", None),
    Geometry("f16x2", "3x3", 256, 2, True, 160, 64, 32, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 8, False, 128, 32, 8, True, True, "none", False, "none", "igemm", None),
    Geometry("f16x2", "3x3x3", 16, 8, False, 128, 32, 8, True, True, "plain", False, "none", "igemm", None),
    Geometry("f16x2", "1x1", 64, 2, False, 32, 8, 1, False, False, "none", False, "none", "igemm", None),
    Geometry("f16x2", "1x1", 16, 8, False, 64, 256, 1, False, False, "none", False, "none", "igemm", None),
    Geometry("f16x2", "1x1", 64, 2, False, 32, 256, 1, False, False, "none", False, "none", "igemm", None),
    Geometry("f32", "1x1", 8, 8, False, 64, 256, 1, False, False, "none", False, "none", "igemm", 2),
    Geometry("f32", "3x3x3", 8, 8, False, 64, 32, 1, True, True, "none", False, "none", "igemm", 2),
    Geometry("f32", "3x3x3", 8, 8, False, 64, 32, 1, True, True, "plain", False, "none", "igemm", 2),
    Geometry("f32", "3x3", 64, 8, False, 512, 8, 32, True, True, "none", True, "none", "igemm", None),
    Geometry("f32", "3x3", 64, 8, False, 512, 8, 32, True, True, "plain", True, "none", "igemm", None),
    Geometry("f32", "3x3x3", 32, 64, False, 64, 8, 32, True, True, "plain", False, "none", "igemm", None),
    Geometry("f32", "3x3x3", 32, 64, False, 64, 8, 32, True, True, "none", True, "none", "igemm", None),
    Geometry("f32", "3x3", 64, 4, False, 128, 256, 32, True, True, "none", False, "none", "igemm", None),
    Geometry("f32", "3x3", 64, 4, False, 128, 256, 32, True, True, "plain", False, "none", "igemm", None),
    Geometry("f32", "3x3x3", 32, 8, False, 192, 96, 8, True, True, "none", False, "none", "igemm", None),
    Geometry("f32", "3x3x3", 32, 8, False, 192, 96, 8, True, True, "plain", False, "none", "igemm", None),
    Geometry("f32", "3x3", 128, 32, False, 32, 8, 32, True, True, "none", True, "none", "igemm", None),
    Geometry("f32", "3x3", 128, 32, False, 32, 8, 32, True, True, "plain", True, "none", "igemm", None),
    Geometry("f32", "3x3", 128, 32, False, 32, 8, 32, True, True, "up2", True, "none", "igemm", None),
    Geometry("f32", "3x3", 128, 32, True, 32, 8, 32, True, True, "none", True, "none", "igemm", None),
    Geometry("f32", "3x3x3", 64, 32, False, 32, 8, 32, True, True, "plain", False, "none", "igemm", None),
    Geometry("f32", "3x3x3", 64, 32, False, 32, 8, 32, True, True, "none", True, "none", "igemm", None),
    Geometry("f32", "3x3x3", 64, 32, False, 3, 8, 32, True, True, "none", False, "none", "igemm", None),
    Geometry("f32", "3x3x3", 64, 4, False, 3, 64, 32, True, True, "none", False, "none", "igemm", None),
    Geometry("f32", "1x1", 128, 2, False, 3, 8, 1, False, False, "none", False, "none", "head", None),
)


# ---- the geometries the C entry point refuses whatever the plan (property 4) ----------------------------------------------------
# (Wl, Hl, Dl: the logical output; a 2-D layer has Dl = 1; the stem runs as D = image rows, H = 1)
def _out_dims(g):
    """(Dl, Hl, Wl, D of the input) as conv_igemm_dispatch sees them"""
    if g.taps == "stem":
        rows = g.Hl // 2 if g.ups else g.Hl
        return rows, (2 if g.ups else 1), g.W, rows
    d = g.D or (3 if g.taps == "3x3x3" else 1)
    return d, g.Hl, g.W, d


def _tile_rows(W):
    return {128: 1, 64: 2, 32: 4, 16: 8, 8: 8}[pack.width_class(W)]


REFUSED = (
    ("conv_api.hip, conv_igemm_dispatch: `const int shape = shape_of_width(a.Wl); if (shape < 0) return EMO_ERR_UNSUPPORTED;` "
     "(widths that are multiples of 128, or 64 / 32 / 16 / 8)",
     lambda g: pack.width_class(g.W) is None),
    ("conv_api.hip, conv_igemm_dispatch: `if (ups && D != 1) return EMO_ERR_UNSUPPORTED;`",
     lambda g: g.ups and _out_dims(g)[3] != 1),
    ("conv_inst_1x7_A.hip / conv_inst_1x7_B.hip, conv_lookup_1x7_*: `if (ups) return nullptr;`, then conv_api.hip "
     "`if (!fn) return EMO_ERR_UNSUPPORTED;`",
     lambda g: g.taps == "stem" and g.ups),
    ("conv_inst_1x7_A.hip / conv_inst_1x7_B.hip, conv_lookup_1x7_*: SHAPE_W128 and SHAPE_W64 only, `return nullptr;` for the rest, "
     "then conv_api.hip `if (!fn) return EMO_ERR_UNSUPPORTED;`",
     lambda g: g.taps == "stem" and g.W in (32, 16, 8)),
    ("conv_dispatch.h, CONV_FOR_SHAPE: `: (ups) ? (conv_launch_fn) nullptr` in front of SHAPE_W16 / SHAPE_W8, then conv_api.hip "
     "`if (!fn) return EMO_ERR_UNSUPPORTED;` (no fused upsample onto 16- / 8-wide maps)",
     lambda g: g.taps != "stem" and g.ups and g.W in (16, 8)),
    ("conv_dispatch.h, CONV_FOR_SHAPE: SHAPE_W8 is `conv_igemm_launch<KH, KW, KC, 2, 8, 8, ...>` (TZ = 2), and conv_igemm.h, "
     "conv_igemm_launch: `if (a.Wl % TW || a.Hl % TR || a.Dl % TZ) return EMO_ERR_UNSUPPORTED;` (an odd depth: 1 or 3)",
     lambda g: g.taps != "stem" and g.W == 8 and (_out_dims(g)[0] % 2 != 0 or g.Hl % 8 != 0)),
    ("conv_igemm.h, conv_igemm_launch: `if (a.Wl % TW || a.Hl % TR || a.Dl % TZ) return EMO_ERR_UNSUPPORTED;` with the 1 x 128 / "
     "2 x 64 / 4 x 32 / 8 x 16 position tiles of CONV_FOR_SHAPE (a height that is no multiple of the tile's rows)",
     lambda g: g.taps != "stem" and pack.width_class(g.W) is not None and g.Hl % _tile_rows(g.W) != 0),
)


def refusing_rule(g):
    """the first rule of REFUSED that describes g, or None"""
    for quote, pred in REFUSED:
        if pred(g):
            return quote
    return None


# ---- one geometry ------------------------------------------------------------------------------------------------------------
def layer_precision(mode, cout, cin, kd, kh, kw):
    """the precision PackedConv.from_state_dict gives a layer of a model built in `mode`"""
    if mode in ("bf16x3", "f16x2"):
        ok = pack.supports_bf16x3(cout, cin, kd, kh, kw, mode)
        if mode == "f16x2" and pack.F16X2_POINTWISE and pack.supports_f16x2_pointwise(cout, cin, kd, kh, kw):
            ok = True
    elif mode == "f16":
        ok = pack.supports_f16(cout, cin, kd, kh, kw)
    else:
        ok = True
    return mode if ok else "f32"


def taps_of(layer):
    if (layer.kh, layer.kw) == (1, 7):
        return "stem"
    if layer.kh == 1:
        return "1x1"
    return "3x3x3" if layer.kd == 3 else "3x3"


def form_key(layer, out, ups, res_kind, stats):
    """what a launch was, as far as it selects code: executed() with the K split as split / not split, then taps, fused upsample,
    width class of the output, parity of the channel-tile count, ragged last channel tile, tile statistics, residual kind.  The
    lattice and the R256 inventory compute it here, from the launch that ran."""
    prec, cfg, ks, form = executed(layer, out)
    bm = pack._BM.get(cfg)
    tiles = (None, None) if bm is None else ((-(-layer.cout // bm)) % 2, layer.cout % bm != 0)
    return (prec, cfg, ks > 1, form, taps_of(layer), bool(ups), pack.width_class(out.shape[-1])) + tiles + (bool(stats), res_kind)


def _offset4(t):
    """the same values in a tensor 4 bytes off a 16-byte boundary"""
    buf = ops.torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)    # (ops.torch: the guarded allocator where a test has it)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _operands(g, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    H, W = (g.Hl // 2, g.W // 2) if g.ups else (g.Hl, g.W)
    if g.taps == "stem":
        xs, ws, fan = (g.N, g.cin, H, 1, W), (g.cout, g.cin, 7, 1, 7), g.cin * 49
    elif g.taps == "3x3x3":
        xs, ws, fan = (g.N, g.cin, g.D or 3, H, W), (g.cout, g.cin, 3, 3, 3), g.cin * 27
    elif g.D is not None:                       # (a pointwise layer on a 5-D tensor)
        xs, ws, fan = (g.N, g.cin, g.D, H, W), (g.cout, g.cin, 1, 1, 1), g.cin
    else:
        k = 1 if g.taps == "1x1" else 3
        xs, ws, fan = (g.N, g.cin, H, W), (g.cout, g.cin, k, k), g.cin * k * k
    x = torch.randn(*xs, generator=gen)
    w = torch.randn(*ws, generator=gen) / math.sqrt(fan)
    b = torch.randn(g.cout, generator=gen)
    sc = sh = None
    if g.affine:
        sc, sh = (torch.rand(g.N, g.cin, generator=gen) + 0.5).to(dev), (torch.randn(g.N, g.cin, generator=gen) * 0.3).to(dev)
    oshape = list(xs)
    oshape[1] = g.cout
    if g.ups:
        oshape[-2], oshape[-1] = 2 * oshape[-2], 2 * oshape[-1]
    res = None
    if g.res != "none":
        rs = list(oshape)
        if g.res == "up2":
            rs[-2], rs[-1] = rs[-2] // 2, rs[-1] // 2
        res = torch.randn(*rs, generator=gen).to(dev)
    x = x.to(dev)
    if g.offset == "in":
        x = _offset4(x)
    return x, w, b, sc, sh, res, tuple(oshape)


def _unsupported(err):
    if "EMO_ERR_UNSUPPORTED" not in str(err):
        raise err
    return True


def run_geometry(g, seed, dev=DEV, affine=None):
    """-> dict(status: 'ran' | 'refused', plan, key, failures: list, figures).  Properties 1-3, 5 and 6 of the module docstring;
    `affine`: the GroupNorm affine the tile statistics are checked through (conv_reference.check_tile_stats; default
    ops.groupnorm_affine)"""
    x, w, b, sc, sh, res, oshape = _operands(g, seed, dev)
    kd = w.shape[2] if w.dim() == 5 else 1
    layer = pack.PackedConv(f"{g.mode}/{g.taps}", w, b, dev, precision=layer_precision(g.mode, g.cout, g.cin, kd, w.shape[-2], w.shape[-1]))
    flags = dict(relu_in=g.relu_in, ups=g.ups, res_ups=g.res == "up2", act="none")

    def out_buffer():
        o = ops.torch.empty(oshape, device=dev, dtype=torch.float32)
        return _offset4(o) if g.offset == "out" else o

    def launch(lay, want_stats):
        if g.entry == "head":
            return ops.conv_head(x, lay, sc, sh, relu_in=g.relu_in), None
        r = ops.conv_igemm(x, lay, sc, sh, res=res, out=out_buffer(), want_stats=want_stats, **flags)
        return r if want_stats else (r, None)

    failures = []
    refused = False
    try:
        out, st = launch(layer, g.stats)
    except RuntimeError as e:
        refused = _unsupported(e)
    plan = tuple(layer.last_plan)
    if refused:
        if plan[2] == "f32" and layer.precision == "f32":
            return dict(status="refused", plan=plan, key=None, failures=failures, figures=None)
        twin = pack.PackedConv("twin", w, b, dev, precision="f32")
        try:
            launch(twin, False)
        except RuntimeError as e:
            _unsupported(e)
            return dict(status="refused", plan=plan, key=None, failures=failures, figures=None)
        failures.append(f"plan {plan} is refused by the C entry point while the fp32 plan {tuple(twin.last_plan)} runs")
        return dict(status="mismatch", plan=plan, key=None, failures=failures, figures=None)
    key = form_key(layer, out, g.ups, g.res, st is not None)
    prec = plan[2]
    yard = None
    if prec in R.SPLIT_MEAN:
        yard = ops.conv_igemm(x, pack.PackedConv("twin", w, b, dev, precision="f32"), sc, sh, res=res, **flags)
    fig = R.check_launch(out, x, w, b, sc, sh, res=res, precision=prec, yardstick=yard, stats=st, groups=32 if st is not None else None,
                         affine=affine, **flags)
    failures += fig["failures"]
    out2, st2 = launch(layer, g.stats)
    if tuple(layer.last_plan) != plan:
        failures.append(f"second launch planned {tuple(layer.last_plan)}, first {plan}")
    if not torch.equal(out, out2):
        failures.append("two launches on the same inputs differ")
    if st is not None and not torch.equal(st.stats, st2.stats):
        failures.append("the tile statistics of two launches on the same inputs differ")
    return dict(status="ran", plan=plan, key=key, failures=failures, figures=fig)


def run_slice(geometries, dev=DEV, affine=None, seed0=0):
    """every geometry of the list -> (rows [(geometry, result)], violations [str]); property 4 on the list"""
    rows, bad = [], []
    for i, g in enumerate(geometries):
        r = run_geometry(g, seed0 + i, dev, affine)
        rows.append((g, r))
        bad += [f"{g}: {f}" for f in r["failures"]]
        rule = refusing_rule(g)
        if r["status"] == "refused" and rule is None:
            bad.append(f"{g}: refused with plan {r['plan']}, and no entry of REFUSED describes it")
        if r["status"] == "ran" and rule is not None:
            bad.append(f"{g}: ran with plan {r['plan']}, but REFUSED lists it: {rule}")
    return rows, bad


def summary(tag, rows):
    ran = [r for _, r in rows if r["status"] == "ran"]
    line = f"PARITY conv plan lattice [{tag}]: {len(rows)} geometries, {len(ran)} accepted, {len(rows) - len(ran)} refused by every plan"
    if ran:
        worst = max(ran, key=lambda r: max(r["figures"]["frame_rel_max"]))
        line += f"; worst per-frame max {max(worst['figures']['frame_rel_max']):.2e} of max|ref| (plan {worst['plan']})"
        ratios = [(r["figures"]["mean_err"] / r["figures"]["f32_mean_err"], r["plan"]) for r in ran if r["figures"].get("f32_mean_err")]
        if ratios:
            line += f"; worst mean-error ratio to the fp32 kernel {max(ratios)[0]:.3f} (plan {max(ratios)[1]})"
        st = [r["figures"]["stats_scale_rel"] for r in ran if "stats_scale_rel" in r["figures"]]
        if st:
            line += f"; tile statistics of {len(st)} launches: scale {max(st):.1e} rel"
        line += f"; distinct plans {sorted({r['plan'] for r in ran}, key=str)}"
    return line


def low_fill_thresholds(mp):
    mp.setenv("EMO_CONV_CT2_MIN_ITEMS", "1")
    mp.setenv("EMO_F16X2_P1_MIN_ITEMS", "1")


_SLICES_RUN = set()         # the (mode, taps) slices that have run: a later test reads the cached rows and launches nothing


@functools.lru_cache(maxsize=None)
def _gpu_slice(mode, taps):
    _SLICES_RUN.add((mode, taps))
    mp = pytest.MonkeyPatch()
    try:
        low_fill_thresholds(mp)
        ops.clear_overflow_flags(DEV)
        geoms = [g for g in lattice(mode) if g.taps == taps] if taps != "extra" else [g for g in EXTRA if g.mode == mode]
        rows, bad = run_slice(geoms, seed0=1000 * MODES.index(mode) + 100 * (TAPS + ("extra",)).index(taps))
        torch.cuda.synchronize()
        if ops.overflow_events(DEV):
            bad.append(f"a split launch was replaced by its guarded recomputation: {ops.overflow_events(DEV)}")
    finally:
        mp.undo()
    return rows, bad


@pytest.mark.parametrize("taps", TAPS + ("extra",))
@pytest.mark.parametrize("mode", MODES)
def test_planner_and_launcher_agree_and_launches_meet_fp64(mode, taps, guarded_outputs):
    """properties 1 - 6 of the module docstring on one (mode, taps) slice of the product, or on the mode's entries of EXTRA"""
    cached = (mode, taps) in _SLICES_RUN
    rows, bad = _gpu_slice(mode, taps)
    if cached or not rows:
        guarded_outputs.may_serve_nothing("the slice ran in an earlier test of the session (its rows are cached), or EXTRA has no entry for the mode")
    print(summary(f"{mode} {taps}", rows))
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(bad[:40])
    assert all(r["status"] in ("ran", "refused") for _, r in rows)
    if taps != "extra":
        assert len(rows) == len(WIDTHS) * len(HEIGHTS) * len(UPS) + (taps == "3x3")


def test_every_extra_geometry_runs_a_form_of_its_own(guarded_outputs):
    """EXTRA is there for launch forms the product does not run: an entry whose form the product runs, or an earlier entry, is not
    needed and goes"""
    if all((mode, taps) in _SLICES_RUN for mode in MODES for taps in TAPS + ("extra",)):
        guarded_outputs.may_serve_nothing("every slice ran in an earlier test of the session: only their cached rows are read")
    product = {r["key"] for mode in MODES for taps in TAPS for _, r in _gpu_slice(mode, taps)[0] if r["status"] == "ran"}
    seen, spare = set(), []
    for mode in MODES:
        for g, r in _gpu_slice(mode, "extra")[0]:
            assert r["status"] == "ran", (g, r["status"])
            if r["key"] in product or r["key"] in seen:
                spare.append((g, r["key"]))
            seen.add(r["key"])
    assert not spare, f"{len(spare)} entries of EXTRA run a form that the product or an earlier entry runs:\n" + "\n".join(map(str, spare))


# ---- the launch plan bench.py times at R256 -----------------------------------------------------------------------------------
_REAL_IGEMM, _REAL_HEAD = ops.conv_igemm, ops.conv_head
_IGEMM_SIG, _HEAD_SIG = inspect.signature(_REAL_IGEMM), inspect.signature(_REAL_HEAD)


class FormRecorder:
    """stands in for ops.conv_igemm / ops.conv_head while a pass runs: the real launch, then its form_key.  Records only."""

    def __init__(self):
        self.keys = {}          # key -> [launches, name of the first layer]
        self._in_head = False

    def install(self, mp):
        mp.setattr(ops, "conv_igemm", self.conv_igemm)
        mp.setattr(ops, "conv_head", self.conv_head)

    def _note(self, layer, out, ups, res, res_ups, st):
        key = form_key(layer, out, ups, "none" if res is None else ("up2" if res_ups else "plain"), st is not None)
        self.keys.setdefault(key, [0, layer.name])[0] += 1

    def conv_igemm(self, *args, **kwargs):
        result = _REAL_IGEMM(*args, **kwargs)
        if not self._in_head:                 # (conv_head's fallback onto the GEMM kernel is recorded as the head's launch)
            a = _IGEMM_SIG.bind(*args, **kwargs)
            a.apply_defaults()
            a = a.arguments
            out, st = result if a["want_stats"] else (result, None)
            self._note(a["layer"], out, a["ups"], a["res"], a["res_ups"], st)
        return result

    def conv_head(self, *args, **kwargs):
        self._in_head = True
        try:
            out = _REAL_HEAD(*args, **kwargs)
        finally:
            self._in_head = False
        self._note(_HEAD_SIG.bind(*args, **kwargs).arguments["layer"], out, False, None, False, None)
        return out


def lattice_keys():
    """form_key of every accepted launch of the lattice and of EXTRA, as executed (the slices run once per session)"""
    return {r["key"] for mode in MODES for taps in TAPS + ("extra",) for _, r in _gpu_slice(mode, taps)[0] if r["status"] == "ran"}


@pytest.fixture(scope="module")
def r256_setup():
    """the R256 driver pass as bench.py builds it for r256_fps: trained-like checkpoint, 32 frames of seeded poses; the canonical
    volume and the identity embedding (bench.py: the R512 source pass's) are a smooth random volume and a random embedding"""
    from test_nets_gpu import _full_size
    cfg = config.hot_path_config(overrides={"image_size": 256})
    sd = random_init.trained_like_state_dict(cfg, seed=0, with_source=False)
    _, _, x = _full_size(256, 1, seed=256)
    g = torch.Generator().manual_seed(12)
    B = 32
    pose = torch.randn(B, cfg["lpe_output_channels_expression"], generator=g).to(DEV)
    theta = ops.pose_theta(*[t.to(DEV) for t in (1 + 0.05 * torch.randn(B, 3, generator=g), 0.3 * torch.randn(B, 3, generator=g),
                                                 0.05 * torch.randn(B, 3, generator=g))])
    return cfg, sd, x["canonical"].to(DEV), x["idt"].to(DEV), pose, theta


@pytest.mark.parametrize("B", [32, 1])
@pytest.mark.parametrize("mode", [nets.DEFAULT_PRECISION, "f32"])
def test_driver_pass_R256_launch_forms_are_in_the_lattice(mode, B, r256_setup, monkeypatch):
    """bench.py times the R256 driver pass at 32 frames per call; its decoder widths (256 / 160 / 96 channels) put ragged and odd
    channel-tile counts on the pair kernels.  Every launch form of that pass -- and of the one-frame call, whose plan splits K --
    must be a form some geometry of the lattice ran (and so checked against fp64): compared on the EXECUTED keys of both"""
    cfg, sd, canonical, idt, pose, theta = r256_setup
    hp = nets.HotPath(sd, cfg, DEV, with_source=False, precision=mode)
    ccl = hp.prepare_canonical(canonical)
    rec = FormRecorder()
    with monkeypatch.context() as mp:
        rec.install(mp)
        hp.driver_pass(ccl, idt, pose[:B], theta[:B])
    torch.cuda.synchronize()
    print(f"PARITY conv launch forms [driver R256 B={B} {mode}]: {sum(v[0] for v in rec.keys.values())} launches, {len(rec.keys)} forms "
          "(precision, cfg, K split, form, taps, upsample, width class, channel-tile parity, ragged tile, statistics, residual) -> "
          "launches: " + str({k: v[0] for k, v in sorted(rec.keys.items(), key=str)}))
    assert rec.keys, "no conv launch was recorded"
    ran = lattice_keys()
    missing = {k: v for k, v in rec.keys.items() if k not in ran}
    assert not missing, (f"{len(missing)} launch forms of the R256 pass that no geometry of the lattice ran (add the smallest geometry "
                         f"with each to EXTRA): " + str({k: v[1] for k, v in sorted(missing.items(), key=str)}))
