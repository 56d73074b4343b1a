"""The launch forms of the non-convolution ops (csrc/resample.hip, groupnorm.hip, smallops.hip, embed_ops.hip): the cases only, one
list per op (a helper module, not a test file).  tests/test_op_launch_forms_gpu.py runs every case on the device,
tests/test_op_launch_forms_emul.py the same cases through the host-compiled stream libraries (without the ones marked `wrap`).

A case is a dict: 'id', 'form' (what it is there for -- for upsample_trilinear, avgpool and groupnorm_affine the form name that
emo_op_launch_form must report for its arguments), 'plan' (the plan integers that entry point must report), 'wrap' (the launch has
more work items than the capped grid has threads: 8192 blocks of 256, so the kernel's grid-stride step is taken), and the
shapes.  The shapes are the smallest that reach the form, read from the launchers; where a shape is not the obvious one the
reason stands next to it.  x of upsample_trilinear / avgpool: (NC; D, H, W).
"""
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
GRID_CAP = 8192 * 256               # work items of one trip of a capped grid-stride launch (grid_for in resample.hip, smallops.hip)


def case(id, form=None, plan=None, wrap=False, **kw):
    return dict(id=id, form=form, plan=plan or {}, wrap=wrap, **kw)


def ids(cases):
    return [c["id"].replace(" ", "_") for c in cases]


# ---- upsample_trilinear --------------------------------------------------------------------------------------------------
# Block kernel: fw = 2, W even, out 16-byte aligned.  (An even W is all the float4 store needs: an output row is 2 W floats, a
# multiple of 4, and a quad starts at 4 xq; the listed widths 6, 34, 128 and 2 are no special choice.)  Blocks of outputs per
# volume qvol = (D + 1 | D)(H + 1 | H) W / 2; volumes are grouped into runs of cr (doubling while qvol cr < 2048 and NC % 2 cr
# == 0); split = min(ceil(qrun / 2048), 64) slices of per = ceil(qrun / split).
UPSAMPLE = [
    case("generic odd W", "generic", nc=3, dims=(2, 4, 7), factors=(2, 2, 2)),
    case("generic fw 1", "generic", nc=2, dims=(2, 4, 6), factors=(2, 2, 1)),
    case("generic out 4 bytes off", "generic", nc=3, dims=(2, 4, 6), factors=(2, 2, 2), out_offset=1),
    case("block cr 1 split 1", "block", dict(cr=1, runs=3, split=1, per=45, run_items=45), nc=3, dims=(2, 4, 6), factors=(2, 2, 2)),
    case("block cr 8 one run", "block", dict(cr=8, runs=1, split=1, per=360, run_items=360), nc=8, dims=(2, 4, 6), factors=(2, 2, 2)),
    case("block split 2 ragged", "block", dict(cr=1, runs=1, split=2, per=1301, run_items=2601), nc=1, dims=(8, 16, 34), factors=(2, 2, 2)),
    case("block split capped at 64", "block", dict(cr=1, runs=1, split=64, per=4160, run_items=266240), nc=1, dims=(64, 64, 128),
         factors=(1, 2, 2)),
    case("block single rows 222", "block", dict(cr=2, runs=1, split=1, per=8, run_items=8), nc=2, dims=(1, 1, 2), factors=(2, 2, 2)),
    case("block single rows 112", "block", dict(cr=2, runs=1, split=1, per=2, run_items=2), nc=2, dims=(1, 1, 2), factors=(1, 1, 2)),
    case("generic wrap", "generic", dict(grid=8192, items=2129920), wrap=True, nc=8, dims=(8, 64, 65), factors=(2, 2, 2)),
]

# upsample_trilinear(gn_groups=): a run is a GroupNorm group of C / G = 2 channels here, so a run is twice a volume.
#   ragged: (7, 16, 34) x (2, 2, 2) has qrun = 2 * 8 * 17 * 17 = 4624 = 3 slices of 1542, 1542 and 1540.  ((8, 16, 34), the plain
#           call's ragged shape, gives 5202 = 3 * 1734 here: three equal slices)
#   capped: (32, 64, 64) x (1, 2, 2) has qrun = 2 * 32 * 65 * 32 = 133120 > 64 * 2048: 64 slices of 2080
UPSAMPLE_GN = [
    case(f"{name} N{N} C{C} G{G}", "block", dict(cr=2, runs=N * G, **plan), N=N, C=C, G=G, dims=dims, factors=factors)
    for name, dims, factors, plan in (("ragged", (7, 16, 34), (2, 2, 2), dict(split=3, per=1542, run_items=4624)),
                                      ("capped", (32, 64, 64), (1, 2, 2), dict(split=64, per=2080, run_items=133120)))
    for N, C, G in ((1, 2, 1), (2, 4, 2))
]

# ---- avgpool -------------------------------------------------------------------------------------------------------------
# x4 kernels: kw in {1, 2}, W % (4 kw) == 0, x and out 16-byte aligned; Wq = W / (4 kw) quads per output row
AVGPOOL = [
    case("x4_w1 depth", "x4_w1", nc=6, dims=(4, 6, 8), kernel=(2, 1, 1)),                      # Wq = 2
    case("x4_w1 window 16 16 1", "x4_w1", nc=1, dims=(16, 16, 8), kernel=(16, 16, 1)),
    case("x4_w2 Wq 3 222", "x4_w2", nc=6, dims=(4, 6, 24), kernel=(2, 2, 2)),
    case("x4_w2 Wq 3 122", "x4_w2", nc=6, dims=(4, 6, 24), kernel=(1, 2, 2)),
    case("generic W 12", "generic", nc=6, dims=(4, 6, 12), kernel=(2, 2, 2)),                  # 12 % 8 != 0
    case("generic kw 4", "generic", nc=2, dims=(4, 8, 16), kernel=(1, 4, 4)),
    case("generic window 16 16 16", "generic", nc=1, dims=(16, 16, 32), kernel=(16, 16, 16)),
    case("generic window 3 1 3", "generic", nc=2, dims=(3, 6, 9), kernel=(3, 1, 3)),
    case("generic x 4 bytes off", "generic", nc=6, dims=(4, 6, 24), kernel=(2, 2, 2), x_offset=1),   # an x4_w2 shape: same bits
    case("4-D", "x4_w2", shape4=(2, 3, 6, 8), kernel=(2, 2)),
    case("x4_w1 wrap", "x4_w1", dict(grid=8192, items=2105344), wrap=True, nc=8, dims=(2, 1024, 1028), kernel=(2, 1, 1)),
    case("generic wrap", "generic", dict(grid=8192, items=2101248), wrap=True, nc=8, dims=(1, 512, 1539), kernel=(1, 1, 3)),
]
AVGPOOL_REFUSED = [
    case("window 17", nc=1, dims=(17, 4, 8), kernel=(17, 1, 1)),
    case("D % kd", nc=1, dims=(5, 4, 8), kernel=(2, 1, 1)),
    case("W % kw", nc=1, dims=(4, 4, 9), kernel=(1, 1, 2)),
]

# ---- add -----------------------------------------------------------------------------------------------------------------
# a [rows, ...] (the checker's frames are the rows), b tiles the flattened a: period = b.numel()
ADD = [case(f"n {n} period n alpha {alpha:g}", "period n", a=(1, n), b=(n,), alpha=alpha) for n, alpha in ((255, 1.0), (256, 0.5), (257, -3.0))]
ADD += [case(f"n {n} period 1 alpha {alpha:g}", "period 1", a=(1, n), b=(1,), alpha=alpha) for n, alpha in ((255, -3.0), (256, 1.0), (257, 0.5))]
ADD += [case(f"period n / N alpha {alpha:g}", "period n / N", a=(2, 3, 6, 7), b=(3, 6, 7), alpha=alpha) for alpha in (1.0, 0.5, -3.0)]
# wrap: 2100 x 1000 elements as three rows; the period 1000 divides neither 256 nor the grid's stride 8192 * 256
ADD += [case("wrap period 1000", "period n / N", wrap=True, a=(3, 700000), b=(1000,), alpha=0.5)]

# ---- add_rows_indexed ----------------------------------------------------------------------------------------------------
# grid (x, B): x = ceil(row / 256) blocks below row = 16384, else 64 blocks that stride over the row
ADD_ROWS = [
    case("row 300", "blocks", row=300, K=3, index=[2, 2, 0, -1, 3], alpha=0.5),                 # two blocks, the second partial
    case("row 20000", "strided", row=20000, K=3, index=[2, 2, 0, -1, 3], alpha=-3.0),
    case("row 300 B 1", "blocks", row=300, K=3, index=[1], alpha=1.0),
    case("row 20000 extreme indices", "strided", row=20000, K=2, index=[INT32_MIN, 1, INT32_MAX], alpha=1.0),
    case("row 300 extreme indices", "blocks", row=300, K=2, index=[INT32_MAX, 0, INT32_MIN], alpha=0.5),
]
ADD_ROWS_STRIDED_FROM = 256 * 64

# ---- groupnorm_affine, own pass ------------------------------------------------------------------------------------------
# L = (C / G) S elements per (sample, group); split = min(ceil(L / 16384), 64); the float4 path needs L % 4 == 0 and a 16-byte base
GROUPNORM = [
    case("split 1", "pass", dict(split=1, run_items=70), shape=(2, 8, 5, 7), groups=4),
    case("vector split 2", "pass", dict(split=2, run_items=16400), shape=(2, 4, 8200), groups=2),        # 16388 is no multiple of 4
    case("scalar split 2", "pass", dict(split=2, run_items=16387), shape=(2, 1, 16387), groups=1),
    case("beyond the cap", "pass", dict(split=64, run_items=2200000), shape=(1, 2, 1100, 1000), groups=1),   # slices of 34376
]
GROUPNORM_CAP_FROM = 64 * 16384      # L above this: the 64 slices are longer than 16384 elements

# ---- small_gemm ----------------------------------------------------------------------------------------------------------
_NN, _K, _M, _BATCH = (1, 2, 4, 16), (5, 64, 65, 300), (1, 5, 70), (1, 3)
SMALL_GEMM = [case(f"NN {NN} K {K} M {_M[(i + j) % 3]} batch {_BATCH[(i + j) % 2]}", f"NN {NN}", NN=NN, K=K, M=_M[(i + j) % 3],
                   batch=_BATCH[(i + j) % 2]) for i, NN in enumerate(_NN) for j, K in enumerate(_K)]
SMALL_GEMM_AXES = dict(NN=_NN, K=_K, M=_M, batch=_BATCH)

# ---- projector_finalize --------------------------------------------------------------------------------------------------
# one thread per (b, r); V holds 3 norms; norm_of_row[0] = norm_of_row[-1] = `edge`, the rows between drawn at random
PROJECTOR = [case(f"B {B} R {R} E {E} edge norm {v}", "rows", B=B, R=R, E=E, edge=v)
             for (B, R, E), v in zip(((1, 256, 16), (1, 257, 16), (257, 1, 1), (2, 128, 1), (3, 50, 16), (256, 1, 16)), (0, 1, 2, 2, 1, 0))]

# ---- mul_mask / stage2_compose -------------------------------------------------------------------------------------------
COMPOSE = [
    case("2 3 5 7", "items", shape=(2, 3, 5, 7), face="random"),
    case("1 1 1 1", "items", shape=(1, 1, 1, 1), face="ones"),
    case("2 3 16 16 face zeros", "items", shape=(2, 3, 16, 16), face="zeros"),
    case("2 3 16 16 face ones", "items", shape=(2, 3, 16, 16), face="ones"),
    case("wrap", "items", wrap=True, shape=(3, 3, 512, 512), face="random"),                    # 2 359 296 elements
]

# ---- pack_rgb8 / unpack_rgb8 ---------------------------------------------------------------------------------------------
RGB8 = [
    case("edge values", "items", image="edges"),                                                # 4 x 193 pixels: no multiple of 256
    case("random 2 3 16 24", "items", image=(2, 3, 16, 24)),
    case("wrap", "items", wrap=True, image=(9, 3, 512, 512)),                                   # 2 359 296 pixels
]

# ---- resize2d ------------------------------------------------------------------------------------------------------------
RESIZE_FRAME = (96, 128)             # H x W of the frame the windows lie in
# Planes: 2 x 3, but 64 x 3 where the source or the output plane is ONE pixel.  The checker holds the launch's largest error to
# twice the largest error of ATen's fp32 kernel: a comparison of two maxima, which says something once both have been sampled.
# On a 1 x 1 source every tap is the pixel p, an output is p (sum wx)(sum wy), and what varies over a plane is one of 15 pairs of
# weight sums; how the last products and sums round depends on p alone.  Six planes are six values of p -- either maximum is
# then whatever those six happen to hit (0.5 ulp of p is 3e-08 ... 6e-08, a tenth of the errors compared).  192 values of p
# bring both maxima within about 1 / 192 of what uniformly spread roundings can reach.  The same holds for a 1 x 1 output: one
# output per plane.
RESIZE_ONE_PIXEL_PLANES = (64, 3)
RESIZE = [case(f"{mode} {src} to {dst}", mode, mode=mode, src=src, dst=dst,
               **(dict(batch=RESIZE_ONE_PIXEL_PLANES) if (1, 1) in (src, dst) else {}))
          for mode in ("bilinear", "bicubic")
          for src, dst in (((37, 53), (64, 64)), ((64, 64), (64, 64)), ((1, 1), (5, 3)), ((8, 8), (1, 1)), ((128, 96), (32, 24)),
                           ((16, 16), (128, 128)))]
RESIZE += [case(f"{mode} window {name}", mode, mode=mode, window=w, dst=(64, 64))
           for mode in ("bilinear", "bicubic")
           for name, w in (("first corner", (0, 0, 40, 30)), ("last corner", (128 - 40, 96 - 30, 40, 30)), ("interior", (33, 21, 40, 30)))]
RESIZE += [case(f"{mode} clamp01", mode, mode=mode, window=(33, 21, 40, 30), dst=(64, 64), clamp01=True) for mode in ("bilinear", "bicubic")]
RESIZE += [case(f"{mode} clamp01 equal size", mode, mode=mode, window=(33, 21, 40, 30), dst=(30, 40), clamp01=True) for mode in ("bilinear", "bicubic")]
RESIZE += [case(f"{mode} wrap", mode, wrap=True, mode=mode, src=(128, 128), dst=(512, 512), batch=(3, 3)) for mode in ("bilinear", "bicubic")]

# ---- maxpool2d / affine_add_relu / grid_sample2d -------------------------------------------------------------------------
MAXPOOL = [case(f"{k} {s} {p} {'affine ' if affine else ''}{'relu ' if relu else ''}{shape[2]}x{shape[3]}", "items", k=k, stride=s, pad=p,
                affine=affine, relu=relu, shape=shape)
           for k, s, p in ((3, 2, 1), (2, 2, 0), (3, 1, 1)) for affine in (False, True) for relu in (False, True)
           for shape in ((2, 5, 33, 21), (2, 5, 1, 21))
           if not (shape[2] == 1 and (k, s, p) == (2, 2, 0))]                                  # (a 2-row window has no output on H = 1)
AFFINE_ADD = [case(f"sa {int(sa)} b {int(b)} sb {int(sb)} relu {int(relu)} S {S}", "items", sa=sa, b=b, sb=sb, relu=relu, S=S)
              for sa in (False, True) for b, sb in ((False, False), (True, False), (True, True)) for relu in (False, True)
              for S in (1, 63, 256)]
GRID_SAMPLE2D = [
    case("grid C 1", "grid", C=1, N=2, src=(9, 12), out=(7, 11)),
    case("grid Ho != Wo", "grid", C=3, N=2, src=(16, 10), out=(5, 13)),
    case("theta", "theta", C=3, N=2, src=(12, 12), out=(8, 8)),
]

BY_OP = dict(upsample_trilinear=UPSAMPLE, upsample_trilinear_gn_sums=UPSAMPLE_GN, avgpool=AVGPOOL, add=ADD, add_rows_indexed=ADD_ROWS,
             groupnorm_affine=GROUPNORM, small_gemm=SMALL_GEMM, projector_finalize=PROJECTOR, mul_mask=COMPOSE, stage2_compose=COMPOSE,
             pack_rgb8=RGB8, unpack_rgb8=RGB8, resize2d=RESIZE, maxpool2d=MAXPOOL, affine_add_relu=AFFINE_ADD, grid_sample2d=GRID_SAMPLE2D)


# ---- what the cases must cover -------------------------------------------------------------------------------------------
def plan_edges(op, plan):
    """the plan edges a reported plan (hip.op_launch_form) lies on"""
    e = {"form " + plan["form"]}
    if op in ("upsample_trilinear", "upsample_trilinear_gn_sums") and plan["form"] == "block":
        e.add("cr 1" if plan["cr"] == 1 else "cr > 1")
        e.add({1: "split 1", 2: "split 2", 64: "split 64"}.get(plan["split"], "split other"))
        if plan["run_items"] != plan["split"] * plan["per"]:
            assert 0 < plan["run_items"] - (plan["split"] - 1) * plan["per"] < plan["per"], plan
            e.add("ragged slice")
    if op == "groupnorm_affine":
        e.add("split 64 capped" if plan["run_items"] > GROUPNORM_CAP_FROM else
              {1: "split 1", 2: "split 2"}.get(plan["split"], "split other"))
    if plan["items"] > 256 * plan["grid"] and op != "groupnorm_affine" and plan["form"] != "block":
        e.add("wrap")
    return e


REQUIRED_EDGES = {
    "upsample_trilinear": {"cr 1", "cr > 1", "split 1", "split 2", "split 64", "ragged slice", "wrap"},
    "upsample_trilinear_gn_sums": {"split 64", "ragged slice"},
    "avgpool": {"wrap"},
    "groupnorm_affine": {"split 1", "split 2", "split 64 capped"},
}


def form_dims(op, c):
    """the integer shape arguments of the launcher, as emo_op_launch_form takes them"""
    if op == "upsample_trilinear":
        return (c["nc"],) + tuple(c["dims"]) + tuple(c["factors"])
    if op == "upsample_trilinear_gn_sums":
        return (c["N"], c["C"], c["G"]) + tuple(c["dims"]) + tuple(c["factors"])
    if op == "avgpool":
        if "shape4" in c:
            N, C, H, W = c["shape4"]
            return (N * C, 1, H, W, 1) + tuple(c["kernel"])
        return (c["nc"],) + tuple(c["dims"]) + tuple(c["kernel"])
    if op == "groupnorm_affine":
        N, C = c["shape"][:2]
        S = 1
        for s in c["shape"][2:]:
            S *= s
        return (N, C, S, c["groups"])
    raise KeyError(op)
