"""The launch forms of the 3-D sampler (csrc/grid_sample3d.hip, gs3d_tile_launch.h) and of the repack kernels: the cases only, one
list per family (a helper module, not a test file).  tests/test_sampler_launch_forms_gpu.py runs every case on the device,
tests/test_sampler_launch_forms_emul.py the direct-form cases through the host-compiled sampler library.

A case is a dict: 'id', 'form' and 'plan' (the form name and the plan integers emo_grid_sample3d_launch_form must report: ABI 29,
hip.sampler_launch_form), the layouts, 'variant', N, C, 'out' = the output lattice (Do, Ho, Wo) and 'vol' = the volume's (D, H, W)
in `grid` and `delta` mode -- different from the lattice, so that a D / Do mix-up shows; in `theta` mode ops fixes the output to
the volume's size and the volume takes the lattice's extents.  No plan integer depends on the volume's extents.  'shared': one
volume for the N samples; 'index' + 'K': the indexed entry over a bank of K volumes; 'slow': too many blocks for the OS-thread
emulation (a block is 256 threads there).  The shapes are the smallest that reach the form, read from direct_form and tile_form;
where a shape is not the obvious one the reason stands next to it.
"""
from emoportraits_amd.ops import tile_variant

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
TILE = 1 << 30
VOL = (3, 5, 7)                     # default volume of grid / delta mode: no extent equals an extent of any case's lattice
BANK_INDEX = [2, 0, 2, 1, 0]        # K = 3: unordered, repeated
BAD_ARG, UNSUPPORTED = -1, -2


def case(id, form, plan=None, *, N=2, C=4, out, vol=VOL, in_layout="ncdhw", out_layout="ncdhw", variant=0, shared=False, index=None,
         K=0, slow=False):
    if index is not None:
        N, K = len(index), K or 3
    return dict(id=id, form=form, plan=plan or {}, N=N, C=C, out=tuple(out), vol=tuple(vol), in_layout=in_layout, out_layout=out_layout,
                variant=variant, shared=shared, index=index, K=K, slow=slow)


def ids(cases):
    return [c["id"].replace(" ", "_") for c in cases]


def vol_dims(c, mode):
    return c["out"] if mode == "theta" else c["vol"]


# ---- planar direct gather: NCDHW -> NCDHW -----------------------------------------------------------------------------------
# grid (ceil(nvox / 256), ceil(C / cpb), N); cpb = variant > 0 ? variant : 8, clipped to C; a chunk runs in quads + a scalar tail
PLANAR = [
    case("cpb default 8 C 9", "planar", dict(cpb=8, grid_x=1, grid_y=2, grid_z=2, last_vox=70), C=9, out=(2, 5, 7)),   # chunks 8 + 1
    case("cpb clipped to C 3", "planar", dict(cpb=3, grid_y=1, last_vox=70), C=3, out=(2, 5, 7)),
    case("cpb asked 96 clipped to C 5", "planar", dict(cpb=5, grid_y=1), C=5, variant=96, out=(2, 5, 7)),
    case("cpb 1", "planar", dict(cpb=1, grid_y=3), C=3, variant=1, out=(2, 5, 7)),
    case("cpb 6 scalar tail", "planar", dict(cpb=6, grid_y=2), C=12, variant=6, out=(2, 5, 7)),                  # a chunk: 4 + 2
    case("C 7 cpb 4 ragged chunk", "planar", dict(cpb=4, grid_y=2), C=7, variant=4, out=(2, 5, 7)),              # chunks 4 + 3
    case("two blocks ragged", "planar", dict(cpb=8, grid_x=2, bps=2, last_vox=74), C=8, out=(3, 10, 11)),         # 330 voxels
    case("one full block", "planar", dict(grid_x=1, last_vox=256), C=4, out=(4, 8, 8)),
    case("one voxel", "planar", dict(grid_x=1, last_vox=1, cpb=2), C=2, out=(1, 1, 1)),
    case("shared volume N 3", "planar", dict(grid_z=3, bank=0), N=3, C=7, variant=4, shared=True, out=(2, 5, 7)),
    case("banked", "planar", dict(bank=1, cpb=4, grid_y=2, grid_z=5, grid_x=2, last_vox=74), C=7, variant=4, index=BANK_INDEX,
         out=(3, 10, 11)),
]


# ---- channels-last rows, both outputs ---------------------------------------------------------------------------------------
# 64 consecutive output voxels per block, bps = ceil(nvox / 64), grid bps N.  An NCDHW output transposes through
# 64 * 80 + C * 65 * 4 = 5120 + 260 C bytes of dynamic LDS: C = 232 is the last that fits 64 KiB (65 440).
def rows(id, plan, *, outs=("ndhwc", "ncdhw"), **kw):
    cs = []
    for ol in outs:
        p = dict(plan, fma=int(bool(kw.get("variant", 0) & 4)), bank=int(kw.get("index") is not None))
        p["nt"] = int(bool(kw.get("variant", 0) & 2) and ol == "ncdhw")
        p["lds"] = 5120 + 260 * kw.get("C", 4) if ol == "ncdhw" else 0
        p["cpb"] = kw.get("C", 4)
        cs.append(case(f"{id} to {ol}", "rows" if ol == "ndhwc" else "rows_ncdhw", p, in_layout="ndhwc", out_layout=ol, **kw))
    return cs


# ORDER 3 (row-group-major over an XCD's samples): a shared volume, no bank, N % 8 == 0, nvox % 64 == 0, bps % Do == 0,
# (bps / Do) % 8 == 0.  N = 8 is one sample per XCD -- no interleave to get wrong; N = 16 on (2, 16, 32): two samples per XCD,
# bps = 16 = two slices of one row group of 8.  Each fall-back below breaks ONE of the conditions and keeps the rest.
O3 = dict(N=16, C=4, shared=True, slow=True)
ROWS = (
    rows("order 1 LPV 3", dict(order=1, bps=2, grid_x=4, last_vox=64), C=12, out=(2, 8, 8))
    + rows("order 3 taken", dict(order=3, bps=16, grid_x=256, last_vox=64), out=(2, 16, 32), **O3)
    + rows("order 3 taken two row groups a slice", dict(order=3, bps=16, grid_x=256), out=(1, 32, 32), **O3)   # bps / Do = 16
    + rows("order 3 fma", dict(order=3, bps=16, grid_x=256), out=(2, 16, 32), variant=4, **O3)
    + rows("order 3 fma nt", dict(order=3, bps=16, grid_x=256), out=(2, 16, 32), variant=6, **O3)
    + rows("order 3 back N 12", dict(order=1, bps=16, grid_x=192), out=(2, 16, 32), **dict(O3, N=12))
    + rows("order 3 back nvox % 64", dict(order=1, bps=8, grid_x=128, last_vox=32), out=(1, 15, 32), **O3)   # 480 voxels: bps 8, Do 1
    # bps % Do alone: bps = 17 over Do = 2, and 17 / 2 = 8 in integers keeps the row-group condition.  ((2, 8, 12), bps = 3, also
    # breaks that one -- 3 / 2 = 1 -- and would hide a dropped `bps % Do`)
    + rows("order 3 back bps % Do", dict(order=1, bps=17, grid_x=272, last_vox=64), out=(2, 16, 34), **O3)
    + rows("order 3 back bps % Do and row groups", dict(order=1, bps=3, grid_x=48, last_vox=64), out=(2, 8, 12), **dict(O3, slow=False))
    + rows("order 3 back row groups", dict(order=1, bps=8, grid_x=128, last_vox=64), out=(2, 16, 16), **O3)  # bps / Do = 4
    + rows("order 3 back own volumes", dict(order=1, bps=16, grid_x=256), out=(2, 16, 32), **dict(O3, shared=False))
    + rows("shared N 3", dict(order=1, bps=2, grid_x=6), N=3, C=8, shared=True, out=(2, 8, 8))
    + rows("ragged last block", dict(order=1, bps=2, grid_x=4, last_vox=41), C=8, out=(3, 5, 7))             # 105 voxels
    + rows("nvox 15", dict(order=1, bps=1, grid_x=2, last_vox=15), C=4, out=(1, 3, 5))
    + rows("LPV 24", dict(order=1, bps=2, last_vox=41), C=96, out=(3, 5, 7))
    # LPV = 257 > 256 threads: ItemWalk's dv = 0 walk; 6 voxels x 257 quads = 7 trips of the block.  NDHWC output only (LDS)
    + rows("LPV 257", dict(order=1, bps=1, last_vox=6), outs=("ndhwc",), C=1028, vol=(2, 2, 2), out=(1, 2, 3))
    + rows("C 232 last that fits the LDS", dict(order=1, bps=1, last_vox=15), C=232, out=(1, 3, 5))
    + rows("fma", dict(order=1, bps=2, last_vox=41), C=12, variant=4, out=(3, 5, 7))
    + rows("nt", dict(order=1, bps=2, last_vox=41), C=12, variant=2, out=(3, 5, 7))
    + rows("fma nt", dict(order=1, bps=2, last_vox=41), C=12, variant=6, out=(3, 5, 7))
    + rows("banked", dict(order=1, bps=2, grid_x=10, last_vox=41), C=8, index=BANK_INDEX, out=(3, 5, 7))
    + rows("banked fma nt", dict(order=1, bps=2, grid_x=10, last_vox=41), C=8, variant=6, index=BANK_INDEX, out=(3, 5, 7))
)
ROWS_REFUSED = [
    (case("C 236 to ncdhw", None, C=236, in_layout="ndhwc", out_layout="ncdhw", out=(1, 3, 5)), UNSUPPORTED),   # 66 480 bytes
    (case("C 6", None, C=6, in_layout="ndhwc", out_layout="ndhwc", out=(1, 3, 5)), UNSUPPORTED),
    (case("variant 8", None, C=4, variant=8, in_layout="ndhwc", out_layout="ndhwc", out=(1, 3, 5)), BAD_ARG),
]

# ---- channels-last bricks: NDHWC -> NDHWC, variant bit 1, Do / Ho / Wo multiples of 4 ----------------------------------------
_CL = dict(in_layout="ndhwc", out_layout="ndhwc")
_B = dict(form="brick", order=1, fma=0, nt=0, last_vox=64)
BRICK = [
    case("taken", "brick", dict(_B, bps=2, grid_x=4, cpb=12), C=12, variant=1, out=(4, 4, 8), **_CL),
    case("taken LPV 24 two by two bricks", "brick", dict(_B, bps=4, grid_x=8), C=96, variant=1, out=(4, 8, 8), **_CL),
    case("variant 5 takes the brick kernel", "brick", dict(_B, bps=2), C=12, variant=5, out=(4, 4, 8), **_CL),
    case("variant 3", "brick", dict(_B, bps=2), C=12, variant=3, out=(4, 4, 8), **_CL),
    case("shared N 16 stays order 1", "brick", dict(_B, bps=16, grid_x=256), N=16, C=4, variant=1, shared=True, slow=True,
         out=(4, 16, 16), **_CL),
    case("banked", "brick", dict(_B, bank=1, bps=2, grid_x=10), C=8, variant=1, index=BANK_INDEX, out=(4, 4, 8), **_CL),
    case("back Do % 4", "rows", dict(order=1, fma=0, bps=1), C=12, variant=1, out=(2, 4, 8), **_CL),
    case("back Ho % 4", "rows", dict(order=1, fma=0, bps=3), C=12, variant=1, out=(4, 6, 8), **_CL),
    case("back Wo % 4", "rows", dict(order=1, fma=0, bps=2, last_vox=32), C=12, variant=1, out=(4, 4, 6), **_CL),
    case("back NCDHW output", "rows_ncdhw", dict(order=1, fma=0, nt=0, bps=2), C=12, variant=1, in_layout="ndhwc", out=(4, 4, 8)),
    case("variant 5 back Wo % 4 keeps fma", "rows", dict(order=1, fma=1, bps=2), C=12, variant=5, out=(4, 4, 6), **_CL),
]

# ---- LDS-staged tile kernels ----------------------------------------------------------------------------------------------
# (tag, tuning word) of the LDS-staged kernels: default; one voxel per thread; two bricks per thread; 512-thread blocks;
# a 2 KiB stage (union box never fits: brick-by-brick and direct passes); 1 channel unit per block
TILE_TUNINGS = [("", 0), ("_8x8x4", tile_variant((8, 8, 4))), ("_16x8x4", tile_variant((16, 8, 4), units_per_block=5)),
                ("_8x8x16_512", tile_variant((8, 8, 16), threads=512)),
                ("_tiny_stage", tile_variant((8, 8, 8), lds_kib=2)), ("_upb1", tile_variant((4, 8, 8), units_per_block=1, lds_kib=16))]
# P4 -> NCDHW keeps 16 bytes per thread of transposition scratch next to the stage: the 2 KiB tuning is rejected there (BAD_ARG), its
# tiny stage is 6 KiB
TILE_TINY_P4_NCDHW = tile_variant((8, 8, 8), lds_kib=6)
# what each word asks for: threads, voxels per thread, log2 tile (x, y, z), units per block asked (0: all, at most 31), LDS KiB
_TUNED = {"": (256, 1, (3, 3, 2), 0, 40), "_8x8x4": (256, 1, (3, 3, 2), 0, 40), "_16x8x4": (256, 2, (4, 3, 2), 5, 40),
          "_8x8x16_512": (512, 2, (3, 3, 4), 0, 80), "_tiny_stage": (256, 2, (3, 3, 3), 0, 2), "_upb1": (256, 1, (2, 3, 3), 1, 16)}
TILE_OUT, TILE_VOL, TILE_C = (5, 9, 20), (3, 6, 8), 24     # ragged tiles in z, y and x; W, Wo % 4 == 0 (planar); 6 / 24 units


def _tile_cases():
    cs = []
    for il, ol, form in (("p4", "p4", "tile_p4"), ("p4", "ncdhw", "tile_p4_ncdhw"), ("ncdhw", "ncdhw", "tile_planar")):
        for tag, var in TILE_TUNINGS:
            threads, vpt, (tx, ty, tz), upb, kib = _TUNED[tag]
            if tag == "_tiny_stage" and form == "tile_p4_ncdhw":
                var, kib = TILE_TINY_P4_NCDHW, 6
            units = TILE_C // 4 if il == "p4" else TILE_C
            upb = min(upb or 31, units)
            scratch = 16 * threads if form == "tile_p4_ncdhw" else 0
            tiles = [-(-n // (1 << s)) for n, s in zip(TILE_OUT, (tz, ty, tx))]
            bps = -(-units // upb) * tiles[0] * tiles[1] * tiles[2]
            plan = dict(threads=threads, vpt=vpt, txs=tx, tys=ty, tzs=tz, upb=upb, lds=kib * 1024, bps=bps, grid_x=2 * bps, order=0,
                        stage_slots=min((kib * 1024 - 128 - scratch) // 16, 10 * threads))     # header 128 bytes; 10 slots a thread
            cs.append(case(f"{form}{tag or '_default'}", form, plan, C=TILE_C, vol=TILE_VOL, out=TILE_OUT, in_layout=il, out_layout=ol,
                           variant=var | (TILE if il == "ncdhw" else 0)))
    # default tile 8 x 8 x 4 on a flat lattice: z, then y, halve into x while the tile is at least twice the lattice's extent:
    # (1, 2, 64) -> 128 x 2 x 1
    cs.append(case("tile_p4 default tile on a flat lattice", "tile_p4", dict(txs=7, tys=1, tzs=0, threads=256, vpt=1), C=8, vol=TILE_VOL,
                   out=(1, 2, 64), in_layout="p4", out_layout="p4"))
    # a planar volume whose rows are no multiple of 16 bytes falls through to the direct gather with variant 0
    cs.append(case("tile_planar W % 4 falls through to planar", "planar", dict(cpb=8, threads=0), C=9, vol=(3, 5, 7), out=(2, 5, 7),
                   variant=TILE | tile_variant((8, 8, 4))))
    return cs


TILE_CASES = _tile_cases()
TILE_REFUSED = [
    (case("p4 to ncdhw 2 KiB", None, C=8, vol=TILE_VOL, out=(4, 8, 8), in_layout="p4", out_layout="ncdhw", variant=tile_variant((8, 8, 4), lds_kib=2)),
     BAD_ARG),
    (case("tile of 128 voxels", None, C=8, vol=TILE_VOL, out=(4, 8, 8), in_layout="p4", out_layout="p4", variant=tile_variant((4, 4, 8))), BAD_ARG),
    (case("p4 to ndhwc", None, C=8, vol=TILE_VOL, out=(4, 8, 8), in_layout="p4", out_layout="ndhwc"), UNSUPPORTED),
    (case("banked p4", None, C=8, vol=TILE_VOL, out=(4, 8, 8), in_layout="p4", out_layout="p4", index=BANK_INDEX), UNSUPPORTED),
]

FAMILIES = dict(planar=PLANAR, rows=ROWS, brick=BRICK, tile=TILE_CASES)
REFUSED = ROWS_REFUSED + TILE_REFUSED

# ---- repack ------------------------------------------------------------------------------------------------------------------
# [N][R][cols] -> [N][cols][R] through 64 x 64 tiles, grid (ceil(cols / 64), ceil(R / 64), N); to channels-last R = C, cols = DHW.
# R and columns from {5, 63, 64, 65, 130}: below, one short of, exactly, one past a tile, and two tiles + 2 -- in both dimensions
_RC = ((5, 130), (63, 65), (64, 64), (65, 63), (130, 5), (65, 130))
REPACK = [dict(id=f"{d} C {C} DHW {S}", direction=d, N=3, C=C, DHW=S, to_channels_last=t, indexed=d.endswith("indexed"),
               plan=dict(grid_x=-(-(S if t else C) // 64), grid_y=-(-(C if t else S) // 64), grid_z=3))
          for d, t in (("to_channels_last", 1), ("from_channels_last", 0), ("to_channels_last_indexed", 1)) for C, S in _RC]
# packed-4: one thread per (quad, position), grid (ceil(C / 4 * DHW / 256), N)
REPACK += [dict(id=f"{d} C {C} DHW {S}", direction=d, N=3, C=C, DHW=S, to_channels_last=t, indexed=False,
                plan=dict(grid_x=-(-(C // 4 * S) // 256), grid_y=3, grid_z=1))
           for d, t in (("to_p4", 4), ("from_p4", 5)) for C, S in ((4, 5), (4, 63), (64, 64), (8, 65), (64, 130), (132, 5))]
# the transpose grid's y is rows / 64: more than 65535 tiles of rows are refused before any launch
REPACK_REFUSED = [
    (dict(id="from channels-last DHW 65536 * 64", N=1, C=1, DHW=65536 * 64, to_channels_last=0, indexed=False), UNSUPPORTED),
    (dict(id="to channels-last C 65536 * 64", N=1, C=65536 * 64, DHW=1, to_channels_last=1, indexed=False), UNSUPPORTED),
    (dict(id="indexed C 65536 * 64", N=1, C=65536 * 64, DHW=1, to_channels_last=1, indexed=True), UNSUPPORTED),
    (dict(id="to p4 C 6", N=1, C=6, DHW=8, to_channels_last=4, indexed=False), UNSUPPORTED),
    (dict(id="direction 2", N=1, C=4, DHW=8, to_channels_last=2, indexed=False), BAD_ARG),
]
REPACK_LAST_ROW_TILE = dict(id="DHW 65535 * 64 is the last that runs", N=1, C=1, DHW=65535 * 64, to_channels_last=0, indexed=False)


# ---- what the cases must cover -----------------------------------------------------------------------------------------------
def plan_edges(plan, c):
    """the edges a reported plan (hip.sampler_launch_form) lies on, for the case's shape"""
    f, C, var = plan["form"], c["C"], c["variant"]
    nvox = c["out"][0] * c["out"][1] * c["out"][2]
    e = {"form " + f}
    if plan["bank"]:
        e.add(f + " banked")
    if f == "planar":
        assert plan["grid_y"] == -(-C // plan["cpb"]) and plan["grid_x"] == plan["bps"] == -(-nvox // 256), plan
        assert plan["last_vox"] == nvox - 256 * (plan["bps"] - 1), plan
        if var & TILE:
            e.add("tile flag falls through to planar")
        elif plan["cpb"] == 8 and var == 0:
            e.add("cpb default 8")
        elif plan["cpb"] == C and (var == 0 or var > C):
            e.add("cpb clipped to C")
        if plan["cpb"] == 1:
            e.add("cpb 1")
        if plan["cpb"] % 4 and plan["cpb"] > 4:
            e.add("chunk with a scalar tail")
        if C % plan["cpb"]:
            e.add("ragged last channel chunk")
        e.add("nvox 1" if nvox == 1 else "nvox < 256" if nvox < 256 else "nvox % 256" if nvox % 256 else "nvox full blocks")
    elif f in ("rows", "rows_ncdhw"):
        assert plan["bps"] == -(-nvox // 64) and plan["grid_x"] == plan["bps"] * c["N"] and plan["last_vox"] == nvox - 64 * (plan["bps"] - 1), plan
        e.add(f"{f} order {plan['order']}")
        wants3 = c["shared"] and c["index"] is None and c["N"] >= 8
        if plan["order"] == 3:
            assert wants3, plan
            e.add(f"{f} order 3 fma {plan['fma']}")
        elif wants3 and not var & 1:
            Do, bps = c["out"][0], plan["bps"]
            broken = [n for n, b in (("N % 8", c["N"] % 8), ("nvox % 64", nvox % 64), ("bps % Do", bps % Do),
                                     ("(bps / Do) % 8", (bps // Do) % 8)) if b]      # (as direct_form computes them)
            assert broken, plan
            if len(broken) == 1:
                e.add(f"{f} order 3 back {broken[0]}")
        if c["shared"] and c["N"] < 8:
            e.add(f"{f} shared N < 8")
        e.add(f"{f} fma {plan['fma']}")
        if f == "rows_ncdhw":
            e.add(f"nt {plan['nt']}")
            if plan["lds"] > 65536 - 4 * 260:
                e.add("rows_ncdhw last C that fits the LDS")
        elif var & 2:
            e.add("nt ignored for an NDHWC output")
        if plan["last_vox"] < 64:
            e.add(f"{f} nvox < 64" if nvox < 64 else f"{f} ragged last block")
        lpv = C // 4
        e.add(f"{f} LPV {lpv}" if lpv in (1, 3, 24, 257) else f"{f} LPV other")
        if var & 1:
            e.add("brick back " + ("NCDHW output" if f == "rows_ncdhw" else "Do % 4" if c["out"][0] % 4 else "Ho % 4" if c["out"][1] % 4
                                   else "Wo % 4"))
    elif f == "brick":
        assert plan["order"] == 1 and plan["fma"] == 0 and plan["bps"] * 64 == nvox, plan
        if var & 4:
            e.add("variant 5 takes the brick kernel")
    else:
        e.add(f"{f} threads {plan['threads']} vpt {plan['vpt']}")
        if plan["upb"] < (C // 4 if f != "tile_planar" else C):
            e.add(f"{f} channel groups")
        if plan["lds"] < 8 * 1024:
            e.add(f"{f} tiny stage")
    return e


_ROWS_EDGES = ["order 1", "order 3", "order 3 fma 0", "order 3 fma 1", "order 3 back N % 8", "order 3 back nvox % 64", "order 3 back bps % Do",
               "order 3 back (bps / Do) % 8", "shared N < 8", "ragged last block", "nvox < 64", "LPV 1", "LPV 3", "LPV 24", "fma 0", "fma 1",
               "banked"]
REQUIRED_EDGES = (
    {"cpb default 8", "cpb clipped to C", "cpb 1", "chunk with a scalar tail", "ragged last channel chunk", "nvox % 256", "nvox < 256", "nvox 1",
     "planar banked", "tile flag falls through to planar"}
    | {f"{f} {e}" for f in ("rows", "rows_ncdhw") for e in _ROWS_EDGES}
    | {"rows LPV 257", "nt 0", "nt 1", "nt ignored for an NDHWC output", "rows_ncdhw last C that fits the LDS"}
    | {"brick banked", "variant 5 takes the brick kernel", "brick back Do % 4", "brick back Ho % 4", "brick back Wo % 4", "brick back NCDHW output"}
    | {f"{f} threads {t} vpt {v}" for f in ("tile_p4", "tile_p4_ncdhw", "tile_planar") for t, v in ((256, 1), (256, 2), (512, 2))}
    | {f"{f} {e}" for f in ("tile_p4", "tile_p4_ncdhw", "tile_planar") for e in ("channel groups", "tiny stage")}
)
REQUIRED_REFUSALS = {"C 236 to ncdhw"}
REPACK_REQUIRED_SIZES = {5, 63, 64, 65, 130}
