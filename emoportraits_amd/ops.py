"""Host-side wrappers of the HIP kernels: torch tensors in, torch tensors out, raw pointers underneath.

Names and argument meaning follow the torch ops the reference calls on the hot path, so that
the parity tests read like `ours(x) == torch_cpu(x)`.
"""
import ctypes
import functools
import os

import torch

from . import hip
from . import pack as pack_mod


@functools.lru_cache(maxsize=None)
def _lattice(n, device_index):
    """torch.linspace(-1, 1, n): the identity lattice of models/stage_1/volumetric_avatar/va.py:101-105.
    Computed by torch on the CPU so that the values are the reference's, then kept resident on the device."""
    return torch.linspace(-1, 1, n).to(torch.device("cuda", device_index))


def grid_sample3d(vol, grid=None, theta=None, padding_mode="zeros", in_layout="ncdhw", out_layout="ncdhw",
                  variant=0, out=None, delta=None, vol_index=None):
    """5-D trilinear grid_sample, align_corners=False  (== F.grid_sample(vol, grid, padding_mode=...)).

    vol    [Nv,C,D,H,W] ('ncdhw'), [Nv,C/4,D,H,W,4] ('p4': packed channel quads, the layout of the LDS-staged tile kernels,
           out_layout 'p4' or 'ncdhw') or [Nv,D,H,W,C] ('ndhwc': channels-last, the driver pass's layout; out_layout 'ndhwc'
           or 'ncdhw'); Nv == N or 1 (volume shared by all N samples).
    variant  'p4' input (always the LDS-staged tile kernels): tile_variant(...) tuning word, 0 = defaults;
             'ncdhw' -> 'ncdhw': TILE | tile_variant(...) selects the LDS-staged planar kernel instead of the direct gather.
    grid   [N,Do,Ho,Wo,3]; or None with theta [N,3,4] / [N,4,4]: the sampling grid is then the head-pose affine of
           the identity lattice (notebooks/infer.py:583-588), generated inside the kernel, output size = D,H,W.
    delta  [N,3,Do,Ho,Wo] planar deltas: grid = identity lattice + delta (WarpGenerator output,
           warp_generator_resnet.py:178) without materialising the grid.
    vol_index  int32 [N] on the volume's device: sample n reads volume vol_index[n] of the bank `vol` (any Nv >= 1; layouts
           'ndhwc' -> 'ndhwc' / 'ncdhw' and 'ncdhw' -> 'ncdhw' with the direct gather).  An index outside [0, Nv) gives a zero
           sample: the device reads the index, so the host cannot check it at launch.
    """
    lib = hip.load()
    hip.require_cuda_f32(vol, grid, delta)
    if theta is not None:
        theta = theta.float().contiguous()      # e.g. torch.linalg.inv returns a column-major result
        hip.require_cuda_f32(theta)
    layouts = {"ncdhw": hip.LAYOUT_NCDHW, "ndhwc": hip.LAYOUT_NDHWC, "p4": hip.LAYOUT_P4}
    if in_layout not in layouts or out_layout not in layouts:
        raise ValueError("layouts are 'ncdhw', 'ndhwc' or 'p4'")
    if in_layout == "p4":
        Nv, Q4, D, H, W, four = vol.shape
        if four != 4:
            raise ValueError("a 'p4' volume is [N, C/4, D, H, W, 4]")
        C = 4 * Q4
    elif in_layout == "ndhwc":
        Nv, D, H, W, C = vol.shape
    else:
        Nv, C, D, H, W = vol.shape
    lx = ly = lz = None
    grid_kind = 0
    idx = vol.device.index if vol.device.index is not None else torch.cuda.current_device()
    if delta is not None:
        if grid is not None or theta is not None:
            raise ValueError("pass exactly one of grid / theta / delta")
        if delta.dim() != 5 or delta.shape[1] != 3:
            raise ValueError("delta must be [N,3,Do,Ho,Wo]")
        N, _, Do, Ho, Wo = delta.shape
        lx, ly, lz = _lattice(Wo, idx), _lattice(Ho, idx), _lattice(Do, idx)
        grid, grid_kind = delta, 1
    elif theta is not None:
        if grid is not None:
            raise ValueError("pass exactly one of grid / theta / delta")
        if theta.dim() != 3 or theta.shape[1] not in (3, 4) or theta.shape[2] != 4:
            raise ValueError("theta must be [N,3,4] or [N,4,4]")
        theta = theta[:, :3].contiguous()
        N = theta.shape[0]
        Do, Ho, Wo = D, H, W
        lx, ly, lz = _lattice(Wo, idx), _lattice(Ho, idx), _lattice(Do, idx)
    else:
        if grid is None or grid.dim() != 5 or grid.shape[-1] != 3:
            raise ValueError("grid must be [N,Do,Ho,Wo,3]")
        N, Do, Ho, Wo, _ = grid.shape
    if vol_index is not None:
        return _grid_sample3d_indexed(lib, vol, vol_index, grid, theta, lx, ly, lz, N, C, D, H, W, Do, Ho, Wo, padding_mode,
                                      in_layout, out_layout, variant, grid_kind, out, layouts)
    if Nv not in (1, N):
        raise ValueError(f"volume batch {Nv} does not match grid batch {N}")
    stride = 0 if (Nv == 1 and N > 1) else C * D * H * W
    if (in_layout == "ncdhw" and out_layout == "ncdhw" and variant == 0 and C % 4 == 0 and C >= 16
            and Nv * C * D * H * W >= (1 << 20)
            # limits of the channels-last kernels the redirect lands on (csrc/grid_sample3d.hip): 64 tap records + C rows of 65
            # floats in <= 64 KiB of LDS, 32-bit byte offsets inside one volume.  Beyond them the direct NCDHW gather runs
            and C * 260 + 5120 <= 65536 and C * D * H * W * 4 < 2 ** 32):
        # the reference's call shape (model.grid_sample(NCDHW, grid) -> NCDHW, va.py:264-265) on a large volume: one repack
        # to channels-last + the channels-last gather (NCDHW out) moves 51 MB in 23 us, the NCDHW gather needs 35 us
        # (its 4-byte corner loads are bound by the vector-memory instruction rate; archive/profiles/r3_sampler_seam.jsonl)
        return grid_sample3d(volume_to_channels_last(vol), grid if delta is None else None, theta, padding_mode, "ndhwc",
                             "ncdhw", 0, out, delta)
    shape = {"ndhwc": (N, Do, Ho, Wo, C), "ncdhw": (N, C, Do, Ho, Wo), "p4": (N, C // 4, Do, Ho, Wo, 4)}[out_layout]
    if out is None:
        out = torch.empty(shape, device=vol.device, dtype=torch.float32)
    else:
        hip.require_cuda_f32(out)
        if tuple(out.shape) != shape:
            raise ValueError("bad out shape")
    rc = lib.emo_grid_sample3d_f32(hip.ptr(vol), hip.ptr(grid), hip.ptr(theta), hip.ptr(lx), hip.ptr(ly), hip.ptr(lz),
                                   hip.ptr(out), N, C, D, H, W, Do, Ho, Wo, stride, hip.PAD_MODES[padding_mode],
                                   layouts[in_layout], layouts[out_layout], int(variant), grid_kind, hip.current_stream())
    hip.check(rc, "emo_grid_sample3d_f32")
    return out


def _check_index(index, n, device, what):
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32:
        raise ValueError(f"{what} must be an int32 tensor")
    if index.device != device:
        raise ValueError(f"{what} is on {index.device}, the data on {device}")
    if index.dim() != 1 or index.shape[0] != n or not index.is_contiguous():
        raise ValueError(f"{what} must be a contiguous [{n}] tensor, got {tuple(index.shape)}")


def _grid_sample3d_indexed(lib, vol, vol_index, grid, theta, lx, ly, lz, N, C, D, H, W, Do, Ho, Wo, padding_mode, in_layout,
                           out_layout, variant, grid_kind, out, layouts):
    """grid_sample3d(vol_index=...): emo_grid_sample3d_indexed_f32 over the bank `vol` [K, ...]"""
    _check_index(vol_index, N, vol.device, "vol_index")
    if in_layout == "p4" or (in_layout == "ncdhw" and out_layout != "ncdhw") or (in_layout == "ndhwc" and out_layout == "p4"):
        raise ValueError("vol_index: the layouts are 'ndhwc' -> 'ndhwc' / 'ncdhw' and 'ncdhw' -> 'ncdhw'")
    if in_layout == "ncdhw" and int(variant) & TILE:
        raise ValueError("vol_index: the LDS-staged planar kernel (TILE) takes no bank")
    shape = {"ndhwc": (N, Do, Ho, Wo, C), "ncdhw": (N, C, Do, Ho, Wo)}[out_layout]
    if out is None:
        out = torch.empty(shape, device=vol.device, dtype=torch.float32)
    else:
        hip.require_cuda_f32(out)
        if tuple(out.shape) != shape:
            raise ValueError("bad out shape")
    rc = lib.emo_grid_sample3d_indexed_f32(hip.ptr(vol), hip.ptr(vol_index), vol.shape[0], hip.ptr(grid), hip.ptr(theta),
                                           hip.ptr(lx), hip.ptr(ly), hip.ptr(lz), hip.ptr(out), N, C, D, H, W, Do, Ho, Wo,
                                           hip.PAD_MODES[padding_mode], layouts[in_layout], layouts[out_layout], int(variant),
                                           grid_kind, hip.current_stream())
    hip.check(rc, "emo_grid_sample3d_indexed_f32")
    return out


def affine_grid3d(theta, size):
    """identity_grid_3d.bmm(theta[:, :3].transpose(1, 2)).view(N, d, s, s, 3) (notebooks/infer.py:441-444, :583-588): the
    rotation warp the theta variant of grid_sample3d generates in-kernel, as a tensor.  size = (d, h, w)."""
    lib = hip.load()
    theta = theta.float()[:, :3].contiguous()
    hip.require_cuda_f32(theta)
    if theta.dim() != 3 or theta.shape[1:] != (3, 4):
        raise ValueError("theta must be [N,3,4] or [N,4,4]")
    N = theta.shape[0]
    D, H, W = size
    idx = theta.device.index if theta.device.index is not None else torch.cuda.current_device()
    grid = torch.empty((N, D, H, W, 3), device=theta.device, dtype=torch.float32)
    hip.check(lib.emo_affine_grid3d_f32(hip.ptr(theta), hip.ptr(_lattice(W, idx)), hip.ptr(_lattice(H, idx)),
                                        hip.ptr(_lattice(D, idx)), hip.ptr(grid), N, D, H, W, hip.current_stream()),
              "emo_affine_grid3d_f32")
    return grid


def volume_to_channels_last(vol):
    """[N,C,D,H,W] -> [N,D,H,W,C] (one pass through a 64x64 LDS tile)."""
    lib = hip.load()
    hip.require_cuda_f32(vol)
    N, C, D, H, W = vol.shape
    out = torch.empty((N, D, H, W, C), device=vol.device, dtype=torch.float32)
    hip.check(lib.emo_volume_repack_f32(hip.ptr(vol), hip.ptr(out), N, C, D * H * W, 1, hip.current_stream()),
              "emo_volume_repack_f32")
    return out


def volume_to_channels_last_indexed(vol, bank, row):
    """bank[row[n]] = volume_to_channels_last(vol[n:n+1]) bit for bit, in one launch: vol [N,C,D,H,W], bank [K,D,H,W,C] (written
    in place), row int32 [N] on the same device.  A row outside [0, K) writes nothing: the device reads the rows, so the host
    cannot check them at launch.  Returns bank."""
    lib = hip.load()
    hip.require_cuda_f32(vol, bank)
    if vol.dim() != 5 or bank.dim() != 5:
        raise ValueError(f"vol {tuple(vol.shape)} and bank {tuple(bank.shape)} must be 5-D")
    N, C, D, H, W = vol.shape
    if tuple(bank.shape[1:]) != (D, H, W, C):
        raise ValueError(f"a row of bank {tuple(bank.shape)} does not hold the channels-last volume {(D, H, W, C)}")
    _check_index(row, N, vol.device, "row")
    hip.check(lib.emo_volume_repack_indexed_f32(hip.ptr(vol), hip.ptr(bank), hip.ptr(row), N, C, D * H * W, bank.shape[0],
                                                hip.current_stream()), "emo_volume_repack_indexed_f32")
    return bank


TILE = 1 << 30      # grid_sample3d(variant=TILE | tuning): NCDHW -> NCDHW through the LDS-staged planar kernel


def tile_variant(tile=None, units_per_block=0, lds_kib=0, threads=256):
    """tuning word of the LDS-staged sampler (include/emo_hip.h): tile = (tx, ty, tz) output voxels per block, powers of two
    with tx * ty * tz in {threads, 2 * threads}; 0 / None = the kernel's default"""
    v = 0
    if tile is not None:
        tx, ty, tz = (int(t).bit_length() - 1 for t in tile)
        v |= tx | (ty << 4) | (tz << 8)
    v |= (int(units_per_block) & 31) << 12
    v |= (int(lds_kib) & 255) << 17
    if threads == 512:
        v |= 1 << 25
    return v


def volume_to_p4(vol):
    """[N,C,D,H,W] -> [N,C/4,D,H,W,4] (EMO_LAYOUT_P4: a voxel's channel quad is one 16-byte slot)"""
    lib = hip.load()
    hip.require_cuda_f32(vol)
    N, C, D, H, W = vol.shape
    out = torch.empty((N, C // 4, D, H, W, 4), device=vol.device, dtype=torch.float32)
    hip.check(lib.emo_volume_repack_f32(hip.ptr(vol), hip.ptr(out), N, C, D * H * W, 4, hip.current_stream()),
              "emo_volume_repack_f32")
    return out


def volume_from_p4(vol):
    """[N,C/4,D,H,W,4] -> [N,C,D,H,W]"""
    lib = hip.load()
    hip.require_cuda_f32(vol)
    N, Q, D, H, W, _ = vol.shape
    out = torch.empty((N, 4 * Q, D, H, W), device=vol.device, dtype=torch.float32)
    hip.check(lib.emo_volume_repack_f32(hip.ptr(vol), hip.ptr(out), N, 4 * Q, D * H * W, 5, hip.current_stream()),
              "emo_volume_repack_f32")
    return out


def volume_to_channels_first(vol):
    """[N,D,H,W,C] -> [N,C,D,H,W]"""
    lib = hip.load()
    hip.require_cuda_f32(vol)
    N, D, H, W, C = vol.shape
    out = torch.empty((N, C, D, H, W), device=vol.device, dtype=torch.float32)
    hip.check(lib.emo_volume_repack_f32(hip.ptr(vol), hip.ptr(out), N, C, D * H * W, 0, hip.current_stream()),
              "emo_volume_repack_f32")
    return out


# ----------------------------------------------------------------------------------------------------------------
# GroupNorm -> per-(sample, channel) affine
# ----------------------------------------------------------------------------------------------------------------
def _gn_workspace(N, G, device):
    """per-call scratch for the split partial sums (stream-ordered through torch's caching allocator, so concurrent
    streams never share it)"""
    lib = hip.load()
    need = lib.emo_groupnorm_workspace_bytes(N, G)
    return torch.empty(need, dtype=torch.uint8, device=device), need


def _ada_views(ada_gamma, ada_beta, N, C):
    ada_stride = 0
    if ada_gamma is not None:
        for t in (ada_gamma, ada_beta):
            if not t.is_cuda or t.dtype != torch.float32 or t.stride(-1) != 1 or t.shape != (N, C):
                raise RuntimeError("ada_gamma/ada_beta must be float32 cuda [N,C] with unit inner stride")
        if ada_gamma.stride(0) != ada_beta.stride(0):
            raise RuntimeError("ada_gamma/ada_beta must share the row stride")
        ada_stride = ada_gamma.stride(0)
    return ada_stride


def groupnorm_affine(x, gamma=None, beta=None, ada_gamma=None, ada_beta=None, groups=32, eps=1e-5, want_stats=False,
                     stats=None):
    """scale, shift [N,C] such that GroupNorm(x) == x*scale + shift (per sample and channel).
    ada_gamma / ada_beta: [N, C] views (row stride arbitrary, unit column stride) of the adaptive weights.
    stats: the TileStats the producing conv_igemm(..., want_stats=True) returned for x -- the statistics are then
    combined from the tiles and x itself is not read; or the RunSums of upsample_trilinear(..., gn_groups=)."""
    lib = hip.load()
    hip.require_cuda_f32(x, gamma, beta)
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    ada_stride = _ada_views(ada_gamma, ada_beta, N, C)
    scale = torch.empty((N, C), device=x.device, dtype=torch.float32)
    shift = torch.empty((N, C), device=x.device, dtype=torch.float32)
    mean = rstd = None
    if want_stats:
        mean = torch.empty((N, groups), device=x.device, dtype=torch.float32)
        rstd = torch.empty((N, groups), device=x.device, dtype=torch.float32)
    if isinstance(stats, RunSums):
        if stats.shape != tuple(x.shape) or stats.groups != groups:
            raise ValueError("run sums do not belong to this tensor")
        rc = lib.emo_groupnorm_affine_from_sums_f32(hip.ptr(stats.partial), stats.split, N, C, S, groups, eps, hip.ptr(gamma),
                                                    hip.ptr(beta), hip.ptr(ada_gamma), hip.ptr(ada_beta), ada_stride,
                                                    hip.ptr(scale), hip.ptr(shift), hip.ptr(mean), hip.ptr(rstd),
                                                    hip.current_stream())
        hip.check(rc, "emo_groupnorm_affine_from_sums_f32")
    elif stats is not None:
        T = stats.stats.shape[1]
        if tuple(stats.stats.shape) != (N, T, C, 2) or T * stats.cnt != S:
            raise ValueError("tile statistics do not belong to this tensor")
        rc = lib.emo_groupnorm_affine_from_tiles_f32(hip.ptr(stats.stats), N, C, T, stats.cnt, groups, eps, hip.ptr(gamma),
                                                     hip.ptr(beta), hip.ptr(ada_gamma), hip.ptr(ada_beta), ada_stride,
                                                     hip.ptr(scale), hip.ptr(shift), hip.ptr(mean), hip.ptr(rstd),
                                                     hip.current_stream())
        hip.check(rc, "emo_groupnorm_affine_from_tiles_f32")
    else:
        ws, need = _gn_workspace(N, groups, x.device)
        rc = lib.emo_groupnorm_affine_f32(hip.ptr(x), N, C, S, groups, eps, hip.ptr(gamma), hip.ptr(beta),
                                          hip.ptr(ada_gamma), hip.ptr(ada_beta), ada_stride, hip.ptr(scale),
                                          hip.ptr(shift), hip.ptr(mean), hip.ptr(rstd), hip.ptr(ws), ws.numel(),
                                          hip.current_stream())
        hip.check(rc, "emo_groupnorm_affine_f32")
    if want_stats:
        return scale, shift, mean, rstd
    return scale, shift


# ----------------------------------------------------------------------------------------------------------------
# implicit-GEMM convolution
# ----------------------------------------------------------------------------------------------------------------
class RunSums:
    """fp64 (sum, sum of squares) slices per (sample, group) of a tensor, in the GroupNorm workspace layout
    ([N * G][64][2] doubles), written by the kernel that produced the tensor (upsample_trilinear(..., gn_groups=))."""
    __slots__ = ("partial", "split", "shape", "groups")

    def __init__(self, partial, split, shape, groups):
        self.partial, self.split, self.shape, self.groups = partial, split, tuple(shape), groups


class TileStats:
    """Per-tile GroupNorm statistics written by the conv epilogue: stats [N, T, C, 2] = (mean, centred sum of squares)
    of `cnt` output values per (sample, tile, channel).  Handed to groupnorm_affine(..., stats=) instead of the tensor."""
    __slots__ = ("stats", "cnt")

    def __init__(self, stats, cnt):
        self.stats, self.cnt = stats, cnt


def _shares_storage(a, b):
    """True when the two tensors overlap in memory (same allocation and intersecting byte ranges)"""
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def conv_igemm(x, layer, scale=None, shift=None, relu_in=False, ups=False, res=None, res_ups=False, act="none",
               out=None, ksplit=None, want_stats=False):
    """layer: emoportraits_amd.pack.PackedConv.  x [N,Cin,H,W] or [N,Cin,D,H,W].
    ksplit: K-loop split of the launch (None: the planner decides it together with the block config).
    want_stats: also return the TileStats of the output (None when this launch cannot produce them: K-split launches)
    -> (out, stats).  Execution only: checks the shapes, asks layer.launch_plan for the launch (pack.ConvPlan), allocates what the
    plan names and makes its one or two C calls; the layer keeps the plan as last_launch (last_plan, last_form: parts of it)."""
    lib = hip.load()
    hip.require_cuda_f32(x, scale, shift, res)
    three_d = x.dim() == 5
    N, Cin, D, H, W = x.shape if three_d else (*x.shape[:2], 1, *x.shape[2:])
    if Cin != layer.cin:
        raise ValueError(f"conv expects {layer.cin} input channels, got {Cin}")
    if (layer.kd == 3) != three_d and layer.kd == 3:
        raise ValueError("3x3x3 conv needs a 5-D input")
    Hl, Wl = (2 * H, 2 * W) if ups else (H, W)
    shape = (N, layer.cout, D, Hl, Wl) if three_d else (N, layer.cout, Hl, Wl)
    new = functools.partial(torch.empty, device=x.device, dtype=torch.float32)
    if out is None:
        out = new(shape)
    elif tuple(out.shape) != shape:
        raise ValueError("bad out shape")
    elif _shares_storage(out, x):
        raise ValueError("out overlaps x: tiles read their neighbours' input halo while others write")
    if res is not None and res.numel() != N * layer.cout * D * ((Hl // 2) * (Wl // 2) if res_ups else Hl * Wl):
        raise ValueError("bad residual shape")
    plan = layer.launch_plan(N, D, H, W, ups, affine=scale is not None, res=res is not None, act=act, x16=x.data_ptr() % 16 == 0,
                             out16=out.data_ptr() % 16 == 0, res16=res is None or res.data_ptr() % 16 == 0,
                             in_elems_per_sample=x.numel() // max(1, N), ksplit=ksplit, want_stats=want_stats, guard=F16X2_GUARD)
    cfg, ks, prec = layer.last_plan = plan[:3]       # which kernel ran (bench.py meters the kernels separately)
    layer.last_launch, layer.last_form = plan, "up2" if plan.form == "up2" else None
    ws = new((ks, out.numel())) if ks > 1 else None
    stats = TileStats(new((N, D * Hl * Wl // plan.stats_bp, layer.cout, 2)), plan.stats_bp) if plan.stats_bp else None
    caller_out = None
    if plan.guard and res is not None and _shares_storage(out, res):
        # the guarded launch re-reads res AFTER the first launch has written out: an output that aliases it (a residual updated in
        # place) would feed the first launch's result into the recomputation -- conv + clipped conv + res.  Both launches write a
        # private buffer; the caller's `out` receives the result behind them: `out=` means the same in every mode and guard state
        caller_out, out = out, new(shape)

    tensors, stream = tuple(map(hip.ptr, (layer.bias, scale, shift, res, out))), hip.current_stream()

    def args(*weights, cfg=cfg, ksplit=ks, workspace=ws, stats=stats):      # what all conv entries share, from x to the stream
        return (hip.ptr(x), *map(hip.ptr, weights), *tensors, N, Cin, layer.cout, D, H, W, layer.kd, layer.kh, layer.kw, int(ups),
                int(relu_in), hip.ACT[act], int(res_ups), cfg, ksplit, hip.ptr(workspace),
                None if stats is None else hip.ptr(stats.stats), stream)

    wpk = layer.packed(cfg, prec)
    if prec == "f16x2":
        # the fp16 split checks its operand range on the device (overflow word of the layer); the guarded launch behind it
        # recomputes the layer with exact operands when the word is raised -- no host synchronisation, graph-capturable
        flag = None
        if plan.guard:      # (its weights are packed BEFORE the fp16-split launch is enqueued)
            gprec, gcfg, gks = plan.guard
            gw, flag = layer.packed(gcfg, gprec), pack_mod.overflow_flag_ptr(x.device, layer.flag_slot)
        up2 = plan.form == "up2"        # (the phase form: the same entry with the phase weights and their layout's cfg word)
        w1, cfg1 = (layer.packed(cfg, "f16x2_up2"), pack_mod.CFG_F16X2_UP2) if up2 else (wpk, cfg)
        rc = lib.emo_conv_igemm_f16x2(*args(w1, cfg=cfg1), pack_mod.F16X2_IN_SCALE, layer.w_scale_up2 if up2 else layer.w_scale, flag)
        hip.check(rc, f"emo_conv_igemm_f16x2[{layer.name}{', phase form' if up2 else ''}]")
        if plan.guard:
            # (the bf16 split runs on the first launch's K split and workspace; the fp32 MFMA kernel has a plan of its own)
            gws = ws if gprec == "bf16x3" else new((gks, out.numel())) if gks > 1 else None
            gname = "emo_conv_igemm_bf16x3" if gprec == "bf16x3" else "emo_conv_igemm_f32_guarded"
            hip.check(getattr(lib, gname)(*args(gw, cfg=gcfg, ksplit=gks, workspace=gws, stats=stats if gks == 1 else None), flag),
                      f"{gname}[{layer.name}, guarded]")
        if caller_out is not None:
            out = caller_out.copy_(out)
    elif plan.form == "f16w8_rest":
        # the channel-tile pairs on the eight-wave two-tile kernel, the odd last tile on the older fp16-operand kernel (ABI 10)
        rc = lib.emo_conv_igemm_f16w8_rest(*args(wpk, layer.packed(pack_mod.CFG_D, "f16")), layer.w_scale16)
        hip.check(rc, f"emo_conv_igemm_f16w8_rest[{layer.name}]")
    else:
        # (f16w8: plain fp16 operands on the eight-wave two-tile kernel, csrc/conv_igemm_f16x2_w8.h NPROD = 1; bf16x3: no flag)
        entry = getattr(lib, "emo_conv_igemm_f16acc32" if prec == "f16" else "emo_conv_igemm_" + prec)
        extra = (layer.w_scale16,) if prec == "f16w8" else (None,) if prec == "bf16x3" else ()
        hip.check(entry(*args(wpk), *extra), f"emo_conv_igemm_{prec}[{layer.name}]")
    return (out, stats) if want_stats else out


def _stream_head_takes(layer, N, S, *views):
    """the stream kernel (csrc/conv_head.hip) takes this launch: a 1x1(x1) layer with at most 4 output channels, S positions per
    channel a multiple of 4, contiguous 16-byte aligned views, EMO_CONV_HEAD not 0"""
    return (CONV_HEAD_STREAM and (layer.kd, layer.kh, layer.kw) == (1, 1, 1) and layer.cout <= 4 and S % 4 == 0 and N <= 65535
            and all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in views))


def conv_head(x, layer, scale=None, shift=None, relu_in=False, act="none"):
    """A 1x1(x1) convolution with at most 4 output channels as a stream (csrc/conv_head.hip; the decoder's image head):
    same arguments and result as conv_igemm(x, layer, scale, shift, relu_in=, act=).  Launch forms the stream kernel does not
    take (positions per channel not a multiple of 4, unaligned views, EMO_CONV_HEAD=0) run conv_igemm."""
    lib = hip.load()
    hip.require_cuda_f32(x, scale, shift)
    N, Cin = x.shape[0], x.shape[1]
    S = x.numel() // max(1, N * Cin)
    if not _stream_head_takes(layer, N, S, x):
        return conv_igemm(x, layer, scale, shift, relu_in=relu_in, act=act)
    if Cin != layer.cin:
        raise ValueError(f"conv expects {layer.cin} input channels, got {Cin}")
    out = torch.empty((N, layer.cout) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    layer.last_launch, layer.last_plan = pack_mod.STREAM_PLAN, ("head", 1, "stream")
    hip.check(lib.emo_conv_head_f32(hip.ptr(x), hip.ptr(layer.plain_weight()), hip.ptr(layer.bias), hip.ptr(scale), hip.ptr(shift),
                                    hip.ptr(out), N, Cin, layer.cout, S, int(relu_in), hip.ACT[act], hip.current_stream()),
              f"emo_conv_head_f32[{layer.name}]")
    return out


# A/B switch (measurements only): 0 runs the image head on the fp32 MFMA implicit-GEMM kernel, as round 4 did
CONV_HEAD_STREAM = os.environ.get("EMO_CONV_HEAD", "1") != "0"


# A/B switch (measurements only): 0 launches the fp16 split without its device-side range check and guarded recomputation
F16X2_GUARD = pack_mod.F16X2_GUARD_DEFAULT
clear_overflow_flags = pack_mod.clear_overflow_flags
overflow_events = pack_mod.overflow_events


# ----------------------------------------------------------------------------------------------------------------
# resampling / pointwise
# ----------------------------------------------------------------------------------------------------------------
def upsample_trilinear(x, factors, gn_groups=None):
    """F.interpolate(x, scale_factor=factors, mode='trilinear') for 5-D x, factors in {1,2}^3.
    gn_groups: also return the RunSums of the OUTPUT for a GroupNorm of that many groups (reduced by the upsampling kernel
    from the values it writes) -> (out, sums); sums is None where the fused kernel does not apply (width factor 1, odd width)."""
    lib = hip.load()
    hip.require_cuda_f32(x)
    N, C, D, H, W = x.shape
    fd, fh, fw = factors
    out = torch.empty((N, C, D * fd, H * fh, W * fw), device=x.device, dtype=torch.float32)
    if gn_groups is not None and FUSE_UPSAMPLE_STATS and fw == 2 and W % 2 == 0 and C % gn_groups == 0:
        ws, need = _gn_workspace(N, gn_groups, x.device)
        split = ctypes.c_int(0)
        hip.check(lib.emo_upsample_trilinear_gn_sums_f32(hip.ptr(x), hip.ptr(out), N, C, gn_groups, D, H, W, fd, fh, fw,
                                                         hip.ptr(ws), need, ctypes.byref(split), hip.current_stream()),
                  "emo_upsample_trilinear_gn_sums_f32")
        return out, RunSums(ws, split.value, out.shape, gn_groups)
    hip.check(lib.emo_upsample_trilinear_f32(hip.ptr(x), hip.ptr(out), N * C, D, H, W, fd, fh, fw, hip.current_stream()),
              "emo_upsample_trilinear_f32")
    return (out, None) if gn_groups is not None else out


# A/B switch (measurements only): 0 reduces the statistics of an upsampled tensor with a pass of its own, as round 4 did
FUSE_UPSAMPLE_STATS = os.environ.get("EMO_FUSE_UPSAMPLE_STATS", "1") != "0"


def avgpool(x, kernel):
    """nn.AvgPool3d(kernel, stride=kernel) (5-D, kernel=(kd,kh,kw)) or nn.AvgPool2d (4-D, kernel=(kh,kw))"""
    lib = hip.load()
    hip.require_cuda_f32(x)
    if x.dim() == 5:
        N, C, D, H, W = x.shape
        kd, kh, kw = kernel
        oshape = (N, C, D // kd, H // kh, W // kw)
    else:
        N, C, H, W = x.shape
        D, kd = 1, 1
        kh, kw = kernel
        oshape = (N, C, H // kh, W // kw)
    out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    hip.check(lib.emo_avgpool_f32(hip.ptr(x), hip.ptr(out), N * C, D, H, W, kd, kh, kw, hip.current_stream()),
              "emo_avgpool_f32")
    return out


def add(a, b, alpha=1.0, out=None):
    """(a + b) * alpha; b is broadcast over the leading dimension when it is smaller (period = b.numel())"""
    lib = hip.load()
    hip.require_cuda_f32(a, b)
    if a.numel() % b.numel():
        raise ValueError("b does not tile a")
    if out is None:
        out = torch.empty_like(a)
    hip.check(lib.emo_add_f32(hip.ptr(a), hip.ptr(b), hip.ptr(out), a.numel(), b.numel(), float(alpha), hip.current_stream()),
              "emo_add_f32")
    return out


def add_rows_indexed(a, table, index, alpha=1.0, out=None):
    """(a[b] + table[index[b]]) * alpha per row b: a [B, ...], table [K, ...] with the same row shape, index int32 [B] on the
    same device.  An index outside [0, K) gives a zero row.  Equal indices give bit for bit add(a, table[k], alpha)."""
    lib = hip.load()
    hip.require_cuda_f32(a, table)
    B, K = a.shape[0], table.shape[0]
    if a.dim() < 1 or table.dim() < 1 or a[0].numel() != table[0].numel() or a.numel() == 0 or K == 0:
        raise ValueError(f"rows of a {tuple(a.shape)} and table {tuple(table.shape)} differ")
    _check_index(index, B, a.device, "index")
    if out is None:
        out = torch.empty_like(a)
    hip.check(lib.emo_add_rows_indexed_f32(hip.ptr(a), hip.ptr(table), hip.ptr(index), hip.ptr(out), B, K, a[0].numel(),
                                           float(alpha), hip.current_stream()), "emo_add_rows_indexed_f32")
    return out


def small_gemm(A, B, NN):
    """C[b][m][:NN] = sum_k A[m][k] * B[b][k][:NN];  A [M,K], B [batch,K,NN] -> [batch,M,NN]"""
    lib = hip.load()
    hip.require_cuda_f32(A, B)
    M, K = A.shape
    batch = B.shape[0]
    if B.numel() != batch * K * NN:
        raise ValueError("bad B shape")
    C = torch.empty((batch, M, NN), device=A.device, dtype=torch.float32)
    hip.check(lib.emo_small_gemm_f32(hip.ptr(A), hip.ptr(B), hip.ptr(C), M, K, NN, batch, K * NN, M * NN, hip.current_stream()),
              "emo_small_gemm_f32")
    return C


def projector_finalize(T, V, norm_of_row, gamma, beta):
    """T [B,R,E], V [n,E,2], norm_of_row [R] int32, gamma/beta [R] -> ada_gamma, ada_beta [B,R]"""
    lib = hip.load()
    hip.require_cuda_f32(T, V, gamma, beta)
    B, R, E = T.shape
    ag = torch.empty((B, R), device=T.device, dtype=torch.float32)
    ab = torch.empty((B, R), device=T.device, dtype=torch.float32)
    hip.check(lib.emo_projector_finalize_f32(hip.ptr(T), hip.ptr(V), hip.ptr(norm_of_row), hip.ptr(gamma), hip.ptr(beta),
                                             hip.ptr(ag), hip.ptr(ab), B, R, E, hip.current_stream()),
              "emo_projector_finalize_f32")
    return ag, ab


def pose_theta(scale, rotation, translation):
    """utils/point_transforms.py:188-242 get_transform_matrix on the device -> [B,4,4]"""
    lib = hip.load()
    hip.require_cuda_f32(scale, rotation, translation)
    B = scale.shape[0]
    theta = torch.empty((B, 4, 4), device=scale.device, dtype=torch.float32)
    hip.check(lib.emo_pose_theta_f32(hip.ptr(scale), scale.shape[1], hip.ptr(rotation), hip.ptr(translation),
                                     hip.ptr(theta), B, hip.current_stream()), "emo_pose_theta_f32")
    return theta


def pack_rgb8(img):
    """[N,3,H,W] fp32 -> [N,H,W,3] uint8 = clamp(0,1)*255 truncated (notebooks/infer.py:641-644 + ToPILImage)"""
    lib = hip.load()
    hip.require_cuda_f32(img)
    N, C, H, W = img.shape
    if C != 3:
        raise ValueError("expected 3 channels")
    out = torch.empty((N, H, W, 3), device=img.device, dtype=torch.uint8)
    hip.check(lib.emo_pack_rgb8(hip.ptr(img), hip.ptr(out), N, H, W, hip.current_stream()), "emo_pack_rgb8")
    return out


def unpack_rgb8(frames_u8):
    """[N,H,W,3] uint8 (decoded video frames) -> [N,3,H,W] fp32 in [0,1] = byte / 255 (notebooks/infer.py:211-223)"""
    lib = hip.load()
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous():
        raise RuntimeError("unpack_rgb8 expects a contiguous uint8 cuda tensor [N,H,W,3]")
    N, H, W, C = frames_u8.shape
    if C != 3:
        raise ValueError("expected 3 channels")
    out = torch.empty((N, 3, H, W), device=frames_u8.device, dtype=torch.float32)
    hip.check(lib.emo_unpack_rgb8(hip.ptr(frames_u8), hip.ptr(out), N, H, W, hip.current_stream()), "emo_unpack_rgb8")
    return out


def mul_mask(img, mask):
    """img [N,C,H,W] * mask [N,1,H,W]  (notebooks/infer_s2.py:370)"""
    lib = hip.load()
    hip.require_cuda_f32(img, mask)
    N, C, H, W = img.shape
    if mask.numel() != N * H * W:
        raise ValueError("mask must be [N,1,H,W]")
    out = torch.empty_like(img)
    hip.check(lib.emo_mul_mask_f32(hip.ptr(img), hip.ptr(mask), hip.ptr(out), N, C, H * W, hip.current_stream()),
              "emo_mul_mask_f32")
    return out


def stage2_compose(img, add_img, mask, face_mask):
    """clamp(img + add * (mask * face_mask), 0, 1)  (notebooks/infer_s2.py:365,373-375)"""
    lib = hip.load()
    hip.require_cuda_f32(img, add_img, mask, face_mask)
    N, C, H, W = img.shape
    if mask.numel() != N * H * W or face_mask.numel() != N * H * W or add_img.shape != img.shape:
        raise ValueError("bad shapes")
    out = torch.empty_like(img)
    hip.check(lib.emo_stage2_compose_f32(hip.ptr(img), hip.ptr(add_img), hip.ptr(mask), hip.ptr(face_mask), hip.ptr(out),
                                         N, C, H * W, hip.current_stream()), "emo_stage2_compose_f32")
    return out


def stage2_head(x, layer, scale, shift, img, mask, face_mask=None, out="u8", relu_in=True):
    """The tail of stage 2 in one launch (csrc/conv_head.hip, emo_stage2_head_f32): clamp(img + tanh(conv1x1(in(x))) *
    (mask * face_mask), 0, 1) with in() the folded norm + ReLU of conv_head; x [N,Cin,H,W], layer a 1x1 conv to 3 channels, img
    [N,3,H,W], mask / face_mask [N,1,H,W] (face_mask None = ones).  out 'u8': uint8 [N,H,W,3] as pack_rgb8 writes it; 'f32': the
    fp32 [N,3,H,W] image; 'both': (f32, u8).  Bit-identical to conv_head(act='tanh') -> stage2_compose -> pack_rgb8, which is
    what launch forms the stream kernel does not take run (positions not a multiple of 4, unaligned views, EMO_CONV_HEAD=0),
    with the head on conv_igemm as Stage2.refine has it."""
    lib = hip.load()
    hip.require_cuda_f32(x, scale, shift, img, mask, face_mask)
    if out not in ("u8", "f32", "both"):
        raise ValueError(f"out={out!r}: 'u8', 'f32' or 'both'")
    N, Cin, H, W = x.shape
    S = H * W
    if tuple(img.shape) != (N, 3, H, W) or mask.numel() != N * S or (face_mask is not None and face_mask.numel() != N * S):
        raise ValueError(f"stage-2 tail: image {tuple(img.shape)} / masks do not match the activation {tuple(x.shape)}")
    if (layer.kd, layer.kh, layer.kw) != (1, 1, 1) or layer.cout != 3:
        raise ValueError("stage-2 tail: the head is a 1x1 convolution to 3 channels")
    if Cin != layer.cin:
        raise ValueError(f"conv expects {layer.cin} input channels, got {Cin}")
    if not _stream_head_takes(layer, N, S, x, img, mask, *(() if face_mask is None else (face_mask,))):
        add = conv_igemm(x, layer, scale, shift, relu_in=relu_in, act="tanh")
        f32 = stage2_compose(img, add, mask, torch.ones_like(mask) if face_mask is None else face_mask)
        return f32 if out == "f32" else pack_rgb8(f32) if out == "u8" else (f32, pack_rgb8(f32))
    f32 = torch.empty_like(img) if out != "u8" else None
    u8 = torch.empty((N, H, W, 3), device=img.device, dtype=torch.uint8) if out != "f32" else None
    layer.last_launch, layer.last_plan = pack_mod.STREAM_PLAN, ("head", 1, "stream")
    hip.check(lib.emo_stage2_head_f32(hip.ptr(x), hip.ptr(layer.plain_weight()), hip.ptr(layer.bias), hip.ptr(scale), hip.ptr(shift),
                                      hip.ptr(img), hip.ptr(mask), hip.ptr(face_mask), hip.ptr(f32), hip.ptr(u8), N, Cin, S,
                                      int(relu_in), hip.current_stream()), f"emo_stage2_head_f32[{layer.name}]")
    return f32 if out == "f32" else u8 if out == "u8" else (f32, u8)


def resize2d(x, size, mode="bilinear", window=None, clamp01=False):
    """F.interpolate(x[..., y0:y0+h, x0:x0+w], size=size, mode=mode, align_corners=False) for 4-D x; mode 'bilinear' or
    'bicubic'; window = (x0, y0, w, h) reads a crop of the frame in place (default: the whole frame)"""
    lib = hip.load()
    hip.require_cuda_f32(x)
    N, C, H, W = x.shape
    x0, y0, w, h = window if window is not None else (0, 0, W, H)
    if not (0 <= x0 and 0 <= y0 and w > 0 and h > 0 and x0 + w <= W and y0 + h <= H):
        raise ValueError(f"resize window {(x0, y0, w, h)} is not inside the {W}x{H} frame")
    Ho, Wo = size
    out = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
    first = ctypes.c_void_p(x.data_ptr() + 4 * (y0 * W + x0))
    hip.check(lib.emo_resize2d_f32(first, H * W, W, hip.ptr(out), N * C, h, w, Ho, Wo,
                                   {"bilinear": 0, "bicubic": 1}[mode], int(clamp01), hip.current_stream()),
              "emo_resize2d_f32")
    return out


def _frame_of_arg(frame_of, F, device):
    """frame_of, the frame of each of M faces as a host sequence -> (int32 [M] device tensor, the host tensor), checked here:
    non-decreasing (the faces of a frame are consecutive, in paste order) and inside [0, F)"""
    host = torch.tensor([int(v) for v in frame_of], dtype=torch.int32).reshape(-1)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= F):
        raise ValueError(f"frame_of names a frame outside the {F} given")
    if bool((host[1:] < host[:-1]).any()):
        raise ValueError("frame_of must be non-decreasing: the faces of a frame are consecutive")
    return host.to(device, non_blocking=True), host


def windows_host(windows, M, size, what, rows="frames", paste_S=None):
    """The host check of a window list, written once: a host sequence of M windows (x0, y0, w, h) -> int32 [M,4] host tensor, every
    window inside its frame -- size = the (W, H) of all frames, or an [M,2] tensor, the (W, H) of each face's OWN frame -- and,
    for a paste into an S x S image (paste_S = S), square with a side of at least S / 4.  ValueError; no device, no upload."""
    host = torch.tensor([[int(v) for v in w] for w in windows], dtype=torch.int32).reshape(-1, 4)
    if host.shape[0] != M:
        raise ValueError(f"{host.shape[0]} windows for {M} {rows}")
    lo, hi = host[:, :2], host[:, :2] + host[:, 2:]
    if not (bool((lo >= 0).all()) and bool((host[:, 2:] > 0).all()) and bool((hi <= torch.as_tensor(size)).all())):
        where = "its own frame" if isinstance(size, torch.Tensor) else f"the {size[0]}x{size[1]} frame"
        raise ValueError(f"a {what} window is not inside {where}")
    if paste_S is not None:
        if not bool((host[:, 2] == host[:, 3]).all()):
            raise ValueError("paste windows must be square")
        if not bool((4 * host[:, 2] >= paste_S).all()):
            raise ValueError(f"a paste window is smaller than a quarter of the {paste_S}x{paste_S} image: downscaling stops at S / 4")
    return host


class DeviceWindows:
    """int32 [M,4] windows that lie in the frames' memory already and were formed there -- crop_track's outputs -- as the `windows`
    of the crop and paste ops: taken like a cuda tensor (no host copy, so no host check: crop_track has made the test against each
    row's frame, and the paste kernels repeat it) wherever the frames are.  Slicing gives the windows of those rows."""

    def __init__(self, tensor):
        self.tensor = tensor

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, rows):
        return DeviceWindows(self.tensor[rows])


def _windows_arg(windows, M, size, device, what, rows="frames", paste_S=None):
    """windows -> (int32 [M,4] device tensor, host tensor or None): a host sequence goes through windows_host and is uploaded
    (16 bytes per window); a ready device tensor (or DeviceWindows) is checked for device, dtype and shape (RuntimeError) and
    trusted otherwise"""
    formed = isinstance(windows, DeviceWindows)
    if formed:
        windows = windows.tensor
    if formed or isinstance(windows, torch.Tensor) and windows.is_cuda:
        if windows.device != device or windows.dtype != torch.int32 or tuple(windows.shape) != (M, 4) or not windows.is_contiguous():
            raise RuntimeError("windows must be a contiguous int32 tensor [M,4] on the frames' device" if isinstance(size, torch.Tensor)
                               else "windows must be a contiguous int32 cuda tensor [N,4]")
        return windows, None
    host = windows_host(windows, M, size, what, rows, paste_S)
    return host.to(device, non_blocking=True), host


def resize2d_windows(x, size, windows, mode="bicubic", clamp01=False, frame_of=None):
    """torch.cat([F.interpolate(x[i:i+1, :, y0:y0+h, x0:x0+w], size=size, mode=mode, align_corners=False) for i ...]) in ONE
    launch (notebooks/infer.py:301-352 crops every frame around its own face box): windows = one (x0, y0, w, h) per frame --
    a host sequence (uploaded here: 16 bytes per frame) or an int32 [N,4] device tensor.  Bit-identical to resize2d per frame.
    frame_of (a host sequence of M ints, non-decreasing, inside [0, N)): several faces per frame -- windows has M rows, row m is
    cut out of frame frame_of[m], and the result has M rows (emo_resize2d_faces_f32: the same bits as this op on x[frame_of])."""
    lib = hip.load()
    hip.require_cuda_f32(x)
    N, C, H, W = x.shape
    M = N if frame_of is None else len(frame_of)
    win, _ = _windows_arg(windows, M, (W, H), x.device, "resize", "frames" if frame_of is None else "faces")
    Ho, Wo = size
    out = torch.empty((M, C, Ho, Wo), device=x.device, dtype=torch.float32)
    bicubic = {"bilinear": 0, "bicubic": 1}[mode]
    if frame_of is not None:
        fof, _ = _frame_of_arg(frame_of, N, x.device)
        if M == 0:
            return out
        hip.check(lib.emo_resize2d_faces_f32(hip.ptr(x), H * W, W, hip.ptr(win), hip.ptr(fof), hip.ptr(out), M, N, C, Ho, Wo, bicubic,
                                             int(clamp01), hip.current_stream()), "emo_resize2d_faces_f32")
        return out
    hip.check(lib.emo_resize2d_windows_f32(hip.ptr(x), H * W, W, hip.ptr(win), hip.ptr(out), N, C, Ho, Wo,
                                           bicubic, int(clamp01), hip.current_stream()),
              "emo_resize2d_windows_f32")
    return out


def _paste_args(img, matte, feather, rows, bad_img):
    """what the paste ops check on img [rows,3,S,S] (rows None: never right; bad_img: the message), matte and feather -> S"""
    if rows is None or img.dim() != 4 or img.shape[0] != rows or img.shape[1] != 3 or img.shape[2] != img.shape[3]:
        raise ValueError(bad_img)
    S = img.shape[2]
    if matte is not None and tuple(matte.shape) != (rows, 1, S, S):
        raise ValueError(f"matte {tuple(matte.shape)}: expected {(rows, 1, S, S)}")
    if not 0.0 <= float(feather) <= 0.5:
        raise ValueError(f"feather {feather} is a fraction of the window side: 0 ... 0.5")
    return S


def paste_windows(frames_u8, img, windows, feather=0.0, matte=None, frame_of=None):
    """The inverse of resize2d_windows' crop, in ONE launch and IN PLACE: img [N,3,S,S] fp32 (the renderer's output) goes back
    into frames_u8 [N,Hf,Wf,3] uint8 where each frame's SQUARE window (x0, y0, s, s) was -- bicubic resize to (s, s)
    (antialiased where s < S), clamp(0,1) * 255, blended as (1 - a) * frame + a * image and truncated like pack_rgb8, with a =
    the feather ramp of width feather * s from the window's edge (1 where feather == 0) times `matte` [N,1,S,S] in [0,1]
    resized bilinearly (include/emo_hip.h has the definition).  windows = one (x0, y0, w, h) per frame: a host sequence
    (checked and uploaded here: inside the frame, square, s >= S / 4) or an int32 [N,4] device tensor (trusted: the kernel
    leaves the frame of a window that fails those checks untouched).  Bytes outside the windows are neither read nor written.
    Returns frames_u8.
    frame_of (a host sequence of M ints, non-decreasing, inside [0, N)): several faces per frame -- img, matte and windows have M
    rows, face m goes into frame frame_of[m], and the faces of a frame are pasted in list order, the later one on top, still in
    one launch (emo_paste_faces_rgb8: the bytes of pasting them one after another with this op)."""
    lib = hip.load()
    hip.require_cuda_f32(img, matte)
    if frames_u8.device != img.device or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous() or frames_u8.dim() != 4:
        raise RuntimeError("paste_windows expects a contiguous uint8 tensor [N,H,W,3] on the images' device")
    N, Hf, Wf, C = frames_u8.shape
    F, N = N, (N if frame_of is None else len(frame_of))                     # F frames, N rows of img / matte / windows
    S = _paste_args(img, matte, feather, N if C == 3 else None,
                    f"frames {tuple(frames_u8.shape)} and images {tuple(img.shape)}: expected [N,Hf,Wf,3] and [N,3,S,S]")
    win, host = _windows_arg(windows, N, (Wf, Hf), frames_u8.device, "paste", "frames" if frame_of is None else "faces", S)
    if frame_of is not None:
        fof, fof_host = _frame_of_arg(frame_of, F, frames_u8.device)
        if N == 0:
            return frames_u8
        hip.check(lib.emo_paste_faces_rgb8(hip.ptr(img), hip.ptr(matte), hip.ptr(win), hip.ptr(host), hip.ptr(fof), hip.ptr(fof_host),
                                           hip.ptr(frames_u8), N, F, S, Hf, Wf, float(feather), hip.current_stream()),
                  "emo_paste_faces_rgb8")
        return frames_u8
    if N == 0:
        return frames_u8
    hip.check(lib.emo_paste_windows_rgb8(hip.ptr(img), hip.ptr(matte), hip.ptr(win), hip.ptr(host), hip.ptr(frames_u8), N, S, Hf, Wf,
                                         float(feather), hip.current_stream()), "emo_paste_windows_rgb8")
    return frames_u8


NV12_MATRICES = {"bt709": 0, "bt601": 1}


def _nv12_matrix(colorspace):
    if colorspace not in NV12_MATRICES:
        raise ValueError(f"colorspace {colorspace!r}: 'bt709' or 'bt601'")
    return NV12_MATRICES[colorspace]


def nv12_windows(nv12, size=None, windows=None, colorspace="bt709", full_range=False, frame_of=None):
    """NV12 frames uint8 [N, 3H/2, W] on the device -> fp32 [N,3,Ho,Wo] in [0,1], ONE launch (yuv420_windows, layout 0): each frame's
    window (x0, y0, w, h) of the converted frame, resized bicubically to size = (Ho, Wo) and clamped -- bit for bit
    resize2d_windows(..., 'bicubic', clamp01=True) of the whole-frame conversion, which is never written.  windows: a host
    sequence (checked, uploaded), an int32 [N,4] device tensor (a window that leaves the frame gives zeros), or None = the whole
    frame; size None = (H, W), with windows None the plain conversion.  include/emo_hip.h has the definition.
    frame_of (a host sequence of M ints, non-decreasing, inside [0, N)): several faces per frame -- windows has M rows, row m is
    cut out of frame frame_of[m], and the result has M rows (the same bits as this op on nv12[frame_of])."""
    return yuv420_windows(nv12, "nv12", size, windows, colorspace, full_range, frame_of)


def pack_nv12(img, colorspace="bt709", full_range=False, out=None):
    """[N,3,H,W] fp32 -> NV12 uint8 [N, 3H/2, W] (pack_yuv420, layout 0: clamp(0,1), the matrix, luma rounded per pixel, chroma the
    rounded mean of each 2x2 block); H and W even.  out: NV12 frames to write into (a strided view is fine)."""
    return pack_yuv420(img, "nv12", colorspace, full_range, out)


def paste_windows_nv12(nv12, img, windows, feather=0.0, matte=None, colorspace="bt709", full_range=False, frame_of=None):
    """paste_windows on NV12 frames uint8 [N, 3Hf/2, Wf], IN PLACE and in one launch (paste_windows_yuv420, layout 0): the resized,
    clamped image and the blend weight a of paste_windows; luma blended per pixel, each chroma sample under the window with the
    mean of its (up to four) window pixels' weights and weighted chroma (include/emo_hip.h has the definition).  windows as in
    paste_windows.  Bytes outside a window's luma rectangle and its covering chroma rectangle are neither read nor written.
    Returns nv12.
    frame_of: several faces per frame as in paste_windows -- img, matte and windows have M rows, face m goes into frame
    frame_of[m], the faces of a frame in list order, one launch."""
    return paste_windows_yuv420(nv12, "nv12", img, windows, feather, matte, colorspace, full_range, frame_of)


# ---- YUV 4:2:0 frames in the four sample layouts, all through the ABI 22 entry points (NV12 is layout 0; the NV12 entry points
# of ABI 17 - 19 are the same kernels for C callers) ----------------------------------------------------------------------------
YUV420_LAYOUTS = {"nv12": 0, "yuv420p": 1, "p010": 2, "yuv420p10": 3}           # frame_format -> the C ABI's layout id


def yuv420_name(frame_format):
    """the format as the messages call it"""
    return {"nv12": "NV12"}.get(frame_format, frame_format)


def yuv420_dtype(frame_format):
    """the dtype of a frame tensor [N, 3H/2, W] of the format: bytes, or 16-bit little-endian words for the 10-bit formats"""
    return torch.uint16 if frame_format in ("p010", "yuv420p10") else torch.uint8


def yuv420_planar(frame_format):
    return frame_format in ("yuv420p", "yuv420p10")


def yuv420_geometry(t, frame_format, what):
    """One frame's [3H/2, W] rows of a YUV 4:2:0 tensor (its last two dimensions), checked (ValueError) -> (H, W, pitch in
    bytes): the format's dtype, H and W even, stride 1 along a row; interleaved chroma (nv12, p010): a row pitch >= W samples (a
    [..., :W] view of a padded surface is taken as it is); planar chroma (yuv420p, yuv420p10): dense rows, the U and V planes of
    H/2 x W/2 samples each straight after Y -- ffmpeg's rawvideo layout; with H/2 odd the V plane begins mid-row of the tensor"""
    if frame_format not in YUV420_LAYOUTS:
        raise ValueError(f"frame_format={frame_format!r}: one of {', '.join(YUV420_LAYOUTS)}")
    dt, fmt = yuv420_dtype(frame_format), yuv420_name(frame_format)
    name = str(dt).replace("torch.", "")
    if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() < 2:
        raise ValueError(f"{what}: {fmt} frames are {name} [N, 3H/2, W]")
    rows, W = t.shape[-2:]
    if rows % 3 or W % 2 or rows == 0 or W == 0:
        raise ValueError(f"{what}: {fmt} frames {tuple(t.shape)}: expected {name} [N, 3H/2, W] with H and W even")
    pitch = t.stride(-2)
    if yuv420_planar(frame_format):
        if t.stride(-1) != 1 or pitch != W:
            raise ValueError(f"{what}: {fmt} frames need dense rows (stride 1 along a row, a row stride of W): "
                             f"the chroma planes lie straight after Y")
    elif t.stride(-1) != 1 or pitch < W:
        raise ValueError(f"{what}: {fmt} frames need stride 1 along a row and a row pitch >= W")
    return rows // 3 * 2, W, pitch * t.element_size()


def _yuv420_planes(t, frame_format, what):
    """[N, 3H/2, W] frames of the format -> (layout id, Y, U, V pointers, luma pitch, chroma pitch, frame stride -- in bytes --
    N, H, W), as the ABI 22 entry points take them"""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"{what}: {yuv420_name(frame_format)} frames are [N, 3H/2, W]")
    H, W, pitch = yuv420_geometry(t, frame_format, what)
    N, B = t.shape[0], t.element_size()
    fstride = t.stride(0) * B if N > 0 else 3 * H // 2 * pitch
    if N > 1 and fstride < 3 * H // 2 * pitch:
        raise ValueError(f"{what}: {yuv420_name(frame_format)} frames must not overlap")
    base = t.data_ptr()
    u = base + H * pitch
    if yuv420_planar(frame_format):
        pitch_c, v = pitch // 2, u + (H // 2) * (pitch // 2)
    else:
        pitch_c, v = pitch, None
    return (YUV420_LAYOUTS[frame_format], ctypes.c_void_p(base), ctypes.c_void_p(u), None if v is None else ctypes.c_void_p(v), pitch,
            pitch_c, fstride, N, H, W)


def yuv420_windows(frames, frame_format, size=None, windows=None, colorspace="bt709", full_range=False, frame_of=None):
    """The crop nv12_windows describes, on any of the four YUV 4:2:0 layouts (emo_yuv420_crop_f32, ONE launch, windows and faces
    form alike): frames [N, 3H/2, W] of the format's dtype on the device (yuv420_geometry has the forms) -> fp32 [N,3,Ho,Wo] in
    [0,1]; size, windows, colorspace, full_range and frame_of as there.  10-bit codes: 'p010' the high ten bits of a word,
    'yuv420p10' the low ten; the other six bits are ignored.  include/emo_hip.h (ABI 22) has the definition."""
    lib = hip.load()
    layout, y, u, v, pitch_y, pitch_c, fstride, N, H, W = _yuv420_planes(frames, frame_format, "yuv420_windows")
    matrix = _nv12_matrix(colorspace)
    Ho, Wo = (H, W) if size is None else size
    if frame_of is not None and windows is None:
        raise ValueError("frame_of= needs windows=: one per face")
    M = N if frame_of is None else len(frame_of)
    out = torch.empty((M, 3, Ho, Wo), device=frames.device, dtype=torch.float32)
    hip.require_cuda_f32(out)                                    # (the frames' device: GPU only, like every op)
    win, host = (None, None) if windows is None else _windows_arg(windows, M, (W, H), frames.device, "crop")
    fof, fof_host = (None, None) if frame_of is None else _frame_of_arg(frame_of, N, frames.device)
    if M == 0:
        return out
    hip.check(lib.emo_yuv420_crop_f32(layout, y, u, v, pitch_y, pitch_c, fstride, H, W, hip.ptr(win), hip.ptr(host), hip.ptr(fof),
                                      hip.ptr(fof_host), hip.ptr(out), M, N, Ho, Wo, matrix, int(bool(full_range)), hip.current_stream()),
              "emo_yuv420_crop_f32")
    return out


def pack_yuv420(img, frame_format, colorspace="bt709", full_range=False, out=None):
    """The packing pack_nv12 describes, into any of the four YUV 4:2:0 layouts (emo_pack_yuv420): [N,3,H,W] fp32 -> frames
    [N, 3H/2, W] of the format's dtype, H and W even; a written sample holds its code and zeros in the format's unused bits.
    out: frames to write into."""
    lib = hip.load()
    hip.require_cuda_f32(img)
    N, C, H, W = img.shape
    if C != 3:
        raise ValueError("expected 3 channels")
    if H % 2 or W % 2:
        raise ValueError(f"{yuv420_name(frame_format)} needs an even height and width, got {H}x{W}")
    if frame_format not in YUV420_LAYOUTS:
        raise ValueError(f"frame_format={frame_format!r}: one of {', '.join(YUV420_LAYOUTS)}")
    matrix = _nv12_matrix(colorspace)
    if out is None:
        out = torch.empty((N, 3 * H // 2, W), device=img.device, dtype=yuv420_dtype(frame_format))
    layout, y, u, v, pitch_y, pitch_c, fstride, n, h, w = _yuv420_planes(out, frame_format, "pack_yuv420")
    if (n, h, w) != (N, H, W) or out.device != img.device:
        raise ValueError(f"out {tuple(out.shape)} does not hold {N} {yuv420_name(frame_format)} frames of {W}x{H} on the image's device")
    if N == 0:
        return out
    hip.check(lib.emo_pack_yuv420(layout, hip.ptr(img), y, u, v, pitch_y, pitch_c, fstride, N, H, W, matrix, int(bool(full_range)),
                                  hip.current_stream()), "emo_pack_yuv420")
    return out


def paste_windows_yuv420(frames, frame_format, img, windows, feather=0.0, matte=None, colorspace="bt709", full_range=False,
                         frame_of=None):
    """The paste paste_windows_nv12 describes, on any of the four YUV 4:2:0 layouts, IN PLACE and in one launch (emo_paste_yuv420,
    windows and faces form alike); every argument as there.  A sample outside the windows' luma rectangles and their covering chroma rectangles keeps all its bits; a sample
    inside comes out as its code with zeros in the format's unused bits.  Returns frames."""
    lib = hip.load()
    hip.require_cuda_f32(img, matte)
    if isinstance(frames, torch.Tensor) and frames.device != img.device:
        raise RuntimeError("paste_windows_yuv420 expects the frames on the images' device")
    layout, y, u, v, pitch_y, pitch_c, fstride, N, Hf, Wf = _yuv420_planes(frames, frame_format, "paste_windows_yuv420")
    matrix = _nv12_matrix(colorspace)
    F, N = N, (N if frame_of is None else len(frame_of))                     # F frames, N rows of img / matte / windows
    S = _paste_args(img, matte, feather, N, f"frames {tuple(frames.shape)} and images {tuple(img.shape)}: expected [N,3Hf/2,Wf] and [N,3,S,S]")
    win, host = _windows_arg(windows, N, (Wf, Hf), img.device, "paste", paste_S=S)
    fof, fof_host = (None, None) if frame_of is None else _frame_of_arg(frame_of, F, img.device)
    if N == 0:
        return frames
    hip.check(lib.emo_paste_yuv420(layout, hip.ptr(img), hip.ptr(matte), hip.ptr(win), hip.ptr(host), hip.ptr(fof), hip.ptr(fof_host),
                                   y, u, v, pitch_y, pitch_c, fstride, N, F, S, Hf, Wf, float(feather), matrix, int(bool(full_range)),
                                   hip.current_stream()), "emo_paste_yuv420")
    return frames


def _mixed_rows(frames, frame_format, what):
    """frames: a list of tensors, one per frame, uint8 [H,W,3] (rgb8) or [3H/2,W] of a YUV 4:2:0 layout (yuv420_geometry has the
    forms), all on one device, stride 1 along a row (a row-pitch view is taken as it is where the layout allows one) ->
    [(address, pitch in bytes, H, W)] of the CHECKED tensors"""
    rgb = frame_format == "rgb8"
    if not rgb and frame_format not in YUV420_LAYOUTS:
        raise ValueError(f"frame_format={frame_format!r}: 'rgb8', {', '.join(repr(f) for f in YUV420_LAYOUTS)}")
    if not isinstance(frames, (list, tuple)) or not frames:
        raise ValueError(f"{what} takes a non-empty list of frame tensors, one per frame")
    rows = []
    for i, t in enumerate(frames):
        if not isinstance(t, torch.Tensor) or t.device != frames[0].device or (rgb and t.dtype != torch.uint8):
            raise RuntimeError(f"{what}: frame {i} must be a {'uint8 ' if rgb else ''}tensor on the device of frame 0")
        if rgb:
            if t.dim() != 3 or t.shape[2] != 3 or 0 in t.shape:
                raise ValueError(f"{what}: frame {i} is {tuple(t.shape)}, expected uint8 [H,W,3]")
            H, W, pitch = t.shape[0], t.shape[1], t.stride(0)
            if t.stride(2) != 1 or t.stride(1) != 3 or pitch < 3 * W:
                raise RuntimeError(f"{what}: frame {i} needs stride 1 along a row and a row pitch of at least the row's {3 * W} bytes")
        else:
            if t.dim() != 2:
                raise ValueError(f"{what}: frame {i} is {tuple(t.shape)}, expected {yuv420_name(frame_format)} [3H/2, W] with H and W even")
            H, W, pitch = yuv420_geometry(t, frame_format, f"{what}: frame {i}")
        rows.append((t.data_ptr(), pitch, H, W))
    return rows


def frame_table(frames, frame_format="rgb8"):
    """The frame table of the mixed-size entry points (ABI 19) for a list of frame tensors, one per frame, each uint8 [H_i,W_i,3]
    or [3H_i/2,W_i] of a YUV 4:2:0 layout on the device: int64 [F,4] rows (byte address of the first row, row pitch in bytes, H, W) ->
    (device tensor, host tensor).  The rows are raw device addresses, so they are only ever formed here, from tensors whose
    device, dtype, dimensions, row stride and pitch have been checked; the caller keeps the tensors alive while the table is
    in use.  crop_faces_mixed / paste_faces_mixed build their own: no op takes a ready-made table."""
    host = torch.tensor(_mixed_rows(frames, frame_format, "frame_table"), dtype=torch.int64).reshape(-1, 4)
    return host.to(frames[0].device, non_blocking=True), host


def _mixed_windows(windows, frame_of, table_host, device, S, what):
    """the windows of M faces and their frames -> (windows device, windows host or None, frame_of device, frame_of host).  A host
    sequence of windows is checked against each face's OWN frame (ValueError): inside it and, for a paste into an S x S image
    (S not None), square with a side of at least S / 4 -- the checks of paste_windows"""
    F = table_host.shape[0]
    fof, fof_host = _frame_of_arg(frame_of, F, device)
    M = fof_host.numel()
    own = table_host[fof_host.long()][:, [3, 2]]                                 # (W, H) of each face's own frame
    return _windows_arg(windows, M, own, device, what, "faces", S) + (fof, fof_host)


def crop_faces_mixed(frames, size, windows, frame_of, frame_format="rgb8", colorspace="bt709", full_range=False):
    """The crops of M faces out of frames of DIFFERENT sizes in ONE launch (emo_rgb8_faces_ragged_f32 /
    emo_yuv420_crop_ragged_f32): frames a list of device tensors, one per frame, uint8 [H_i,W_i,3] or [3H_i/2,W_i] of a YUV 4:2:0
    layout (row-pitch views are taken as they are where the layout allows them); windows[m] = (x0, y0, w, h) is cut out of frames[frame_of[m]] (frame_of a host sequence,
    non-decreasing), resized bicubically to size (an int or (Ho, Wo)) and clamped -> fp32 [M,3,Ho,Wo].  rgb8: bit for bit
    unpack_rgb8 + resize2d_windows(..., 'bicubic', clamp01=True, frame_of=) of each frame, but only the bytes under the windows
    are read: no full-frame fp32 picture.  YUV 4:2:0: yuv420_windows(frame_of=)'s arithmetic.  windows: a host sequence (checked
    against each face's own frame, ValueError) or an int32 [M,4] device tensor (a window that leaves its frame gives zeros).
    The frame table is built here from the checked tensors (frame_table)."""
    lib = hip.load()
    rows = _mixed_rows(frames, frame_format, "crop_faces_mixed")
    matrix = _nv12_matrix(colorspace)
    device = frames[0].device
    table_host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    win, host, fof, fof_host = _mixed_windows(windows, frame_of, table_host, device, None, "crop")
    Ho, Wo = (size, size) if isinstance(size, int) else size
    M, F = fof_host.numel(), len(rows)
    out = torch.empty((M, 3, Ho, Wo), device=device, dtype=torch.float32)
    hip.require_cuda_f32(out)                                    # (the frames' device: GPU only, like every op)
    if M == 0:
        return out
    table = table_host.to(device, non_blocking=True)
    if frame_format != "rgb8":
        hip.check(lib.emo_yuv420_crop_ragged_f32(YUV420_LAYOUTS[frame_format], hip.ptr(table), hip.ptr(table_host), hip.ptr(win),
                                                 hip.ptr(host), hip.ptr(fof), hip.ptr(fof_host), hip.ptr(out), M, F, Ho, Wo, matrix,
                                                 int(bool(full_range)), hip.current_stream()), "emo_yuv420_crop_ragged_f32")
    else:
        hip.check(lib.emo_rgb8_faces_ragged_f32(hip.ptr(table), hip.ptr(table_host), hip.ptr(win), hip.ptr(host), hip.ptr(fof),
                                                hip.ptr(fof_host), hip.ptr(out), M, F, Ho, Wo, hip.current_stream()),
                  "emo_rgb8_faces_ragged_f32")
    return out


def paste_faces_mixed(frames, img, windows, frame_of, feather=0.0, matte=None, frame_format="rgb8", colorspace="bt709",
                      full_range=False):
    """paste_windows(frame_of=) / paste_windows_yuv420(frame_of=) into frames of DIFFERENT sizes, IN PLACE and in ONE launch
    (emo_paste_faces_ragged_rgb8 / emo_paste_ragged_yuv420): frames as in crop_faces_mixed, img [M,3,S,S] fp32, matte
    [M,1,S,S] or None; face m goes into frames[frame_of[m]] where its square window is, the faces of a frame in list order, the
    later one on top.  windows: a host sequence, checked against each face's OWN frame before anything is launched (inside it,
    square, side >= S / 4: ValueError), or an int32 [M,4] device tensor (a window that fails those checks against its frame is
    left out by the kernel).  Bytes outside the windows are neither read nor written.  Returns frames."""
    lib = hip.load()
    hip.require_cuda_f32(img, matte)
    rows = _mixed_rows(frames, frame_format, "paste_faces_mixed")
    matrix = _nv12_matrix(colorspace)
    device = frames[0].device
    if device != img.device:
        raise RuntimeError("paste_faces_mixed expects the frames on the images' device")
    S = _paste_args(img, matte, feather, img.shape[0] if img.dim() else None, f"images {tuple(img.shape)}: expected [M,3,S,S]")
    M, F = img.shape[0], len(rows)
    table_host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    win, host, fof, fof_host = _mixed_windows(windows, frame_of, table_host, device, S, "paste")
    if fof_host.numel() != M:
        raise ValueError(f"{fof_host.numel()} entries of frame_of for {M} images")
    if M == 0:
        return frames
    table = table_host.to(device, non_blocking=True)
    if frame_format != "rgb8":
        hip.check(lib.emo_paste_ragged_yuv420(YUV420_LAYOUTS[frame_format], hip.ptr(img), hip.ptr(matte), hip.ptr(table),
                                              hip.ptr(table_host), hip.ptr(win), hip.ptr(host), hip.ptr(fof), hip.ptr(fof_host), M, F,
                                              S, float(feather), matrix, int(bool(full_range)), hip.current_stream()),
                  "emo_paste_ragged_yuv420")
    else:
        hip.check(lib.emo_paste_faces_ragged_rgb8(hip.ptr(img), hip.ptr(matte), hip.ptr(table), hip.ptr(table_host), hip.ptr(win),
                                                  hip.ptr(host), hip.ptr(fof), hip.ptr(fof_host), M, F, S, float(feather),
                                                  hip.current_stream()), "emo_paste_faces_ragged_rgb8")
    return frames


def device_cu_count():
    """compute units of the current device as the C launchers count them (include/emo_hip.h, ABI 9)"""
    return hip.load().emo_device_cu_count()


def mfma_stream(iters=2000, lds_reads=False, sink=None):
    """one launch of the bare fp16 MFMA stream (diagnostic: bench.py `roofline.sustained_peak`) -> MFMA instructions issued"""
    lib = hip.load()
    if sink is None:
        sink = torch.empty(256 * device_cu_count(), device="cuda", dtype=torch.float32)
    n = ctypes.c_int64(0)
    hip.check(lib.emo_mfma_stream_f16(hip.ptr(sink), int(iters), int(bool(lds_reads)), ctypes.byref(n), hip.current_stream()),
              "emo_mfma_stream_f16")
    return n.value


# ---- embedder ResNets -----------------------------------------------------------------------
def conv2d_generic(x, wt, cout, kh, kw, stride, pad, bias=None, scale=None, shift=None, relu_in=False, splits=None):
    """F.conv2d(relu?(x*scale+shift), w, bias, stride, pad); wt = pack.pack_generic(w) [Cin*kh*kw, CoutP].
    relu_in belongs to the affine: without scale / shift the input is read as it is (include/emo_hip.h).
    splits: K split count (None = the library's launch heuristic)"""
    lib = hip.load()
    hip.require_cuda_f32(x)
    N, Cin, H, W = x.shape
    if wt.shape[0] != Cin * kh * kw:
        raise ValueError(f"packed weight has K={wt.shape[0]}, input needs {Cin * kh * kw}")
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    out = torch.empty((N, cout, Ho, Wo), device=x.device, dtype=torch.float32)
    if splits is None:
        splits = lib.emo_conv2d_generic_splits(N, Cin, H, W, cout, kh, kw, stride, pad)
        if splits < 1:
            hip.check(splits, "emo_conv2d_generic_splits")
    ws = torch.empty((splits, out.numel()), device=x.device, dtype=torch.float32) if splits > 1 else None
    hip.check(lib.emo_conv2d_generic_f32(hip.ptr(x), hip.ptr(wt), hip.ptr(bias), hip.ptr(scale), hip.ptr(shift),
                                         hip.ptr(out), N, Cin, H, W, cout, kh, kw, stride, pad, int(relu_in), splits,
                                         hip.ptr(ws), hip.current_stream()), "emo_conv2d_generic_f32")
    return out


def maxpool2d(x, k, stride, pad, scale=None, shift=None, relu=False):
    lib = hip.load()
    hip.require_cuda_f32(x)
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
    hip.check(lib.emo_maxpool2d_f32(hip.ptr(x), hip.ptr(scale), hip.ptr(shift), hip.ptr(out), N * C, H, W, k, stride,
                                    pad, int(relu), hip.current_stream()), "emo_maxpool2d_f32")
    return out


def affine_add_relu(a, sa=None, ta=None, b=None, sb=None, tb=None, relu=True):
    """relu?((a*sa+ta) + (b*sb+tb)) with per-(n,c) affines"""
    lib = hip.load()
    hip.require_cuda_f32(a)
    N, C = a.shape[:2]
    S = a.numel() // (N * C)
    if b is not None and b.shape != a.shape:
        raise ValueError("affine_add_relu: shape mismatch")
    out = torch.empty_like(a)
    hip.check(lib.emo_affine_add_relu_f32(hip.ptr(a), hip.ptr(sa), hip.ptr(ta), hip.ptr(b), hip.ptr(sb), hip.ptr(tb),
                                          hip.ptr(out), N * C, S, int(relu), hip.current_stream()),
              "emo_affine_add_relu_f32")
    return out


def grid_sample2d(img, grid=None, theta=None, size=None, want_grid=False):
    """F.grid_sample(img, grid) (bilinear, zeros, align_corners=False); or theta [N,2,3] on the square
    linspace(-1,1,size) lattice of ExpressionEmbed"""
    lib = hip.load()
    hip.require_cuda_f32(img)
    N, C, H, W = img.shape
    lin = None
    if grid is not None:
        Ho, Wo = grid.shape[1:3]
    else:
        Ho = Wo = int(size)
        lin = _lattice(Ho, img.device.index)
        theta = theta.float().contiguous()
    out = torch.empty((N, C, Ho, Wo), device=img.device, dtype=torch.float32)
    gout = torch.empty((N, Ho, Wo, 2), device=img.device, dtype=torch.float32) if want_grid else None
    hip.check(lib.emo_grid_sample2d_f32(hip.ptr(img), hip.ptr(grid), hip.ptr(theta), hip.ptr(lin), hip.ptr(out),
                                        hip.ptr(gout), N, C, H, W, Ho, Wo, hip.current_stream()), "emo_grid_sample2d_f32")
    return (out, gout) if want_grid else out


def mat4_inverse(m):
    """[B,4,4] -> inverse, on the device (no host LAPACK round trip)"""
    lib = hip.load()
    hip.require_cuda_f32(m)
    if m.shape[1:] != (4, 4):
        raise ValueError("mat4_inverse expects [B,4,4]")
    out = torch.empty_like(m)
    hip.check(lib.emo_mat4_inverse_f32(hip.ptr(m), hip.ptr(out), m.shape[0], hip.current_stream()), "emo_mat4_inverse_f32")
    return out


def mixing_theta(target, source_bank, index=None, mix_old=True):
    """notebooks/infer.py:686-736 get_mixing_theta on the device, per frame: the stretch of its source theta
    source_bank[index[n]] with the rotation and translation of target[n].  target [B,4,4], source_bank [K,4,4], index int32 [B]
    on the same device or None (every frame: source 0) -> [B,4,4] (row 3 = (0,0,0,1)).  An index outside [0, K) passes the
    target through.  fp64 inside, as hostglue.mixing_theta; no host synchronisation."""
    lib = hip.load()
    hip.require_cuda_f32(target, source_bank)
    if target.dim() != 3 or target.shape[1:] != (4, 4) or source_bank.dim() != 3 or source_bank.shape[1:] != (4, 4):
        raise ValueError(f"mixing_theta expects [B,4,4] and [K,4,4], got {tuple(target.shape)} and {tuple(source_bank.shape)}")
    B, K = target.shape[0], source_bank.shape[0]
    if B == 0 or K == 0:
        raise ValueError("mixing_theta: empty target or source bank")
    if index is not None:
        _check_index(index, B, target.device, "index")
    out = torch.empty_like(target)
    hip.check(lib.emo_mixing_theta_f32(hip.ptr(target), hip.ptr(source_bank), hip.ptr(index), B, K, int(bool(mix_old)),
                                       hip.ptr(out), hip.current_stream()), "emo_mixing_theta_f32")
    return out


def _row_masks(restart, present, n, device):
    """the row masks of the control streams (restart, present: int32 [n] on the rows' device, or None), checked like stream_of
    -> their pointers, or None where neither is given: the entry point without masks is then the one to call"""
    if restart is None and present is None:
        return None
    if restart is not None:
        _check_index(restart, n, device, "restart")
    if present is not None:
        _check_index(present, n, device, "present")
    return hip.ptr(restart), hip.ptr(present)


def theta_ema_scan(values, stream_of, state, has_state, momentum, restart=None, present=None):
    """notebooks/infer.py:571-581 smooth_pose over a batch IN FRAME ORDER with one EMA stream per identity, on the device:
    values [n,4,4], stream_of int32 [n] (or None: one stream, 0), state [K,4,4] and has_state int32 [K] updated in place.
    Per stream bit for bit hostglue.ema_scan (1 - momentum rounded to fp32 once, as there) -> smoothed [n,4,4].
    restart, present: int32 [n] on the values' device or None -- the streams follow face tracks (emo_theta_ema_scan_tracks_f32; bit
    for bit hostglue.ema_scan_tracks): a row with restart != 0 first drops its stream's state, a row with present == 0 is
    smoothed from a copy of the state and leaves the stream as it was."""
    import numpy as np
    lib = hip.load()
    hip.require_cuda_f32(values, state)
    if values.dim() != 3 or values.shape[1:] != (4, 4) or state.dim() != 3 or state.shape[1:] != (4, 4):
        raise ValueError(f"theta_ema_scan expects [n,4,4] values and [K,4,4] state, got {tuple(values.shape)}, {tuple(state.shape)}")
    n, K = values.shape[0], state.shape[0]
    if n == 0 or K == 0:
        raise ValueError("theta_ema_scan: no frames or no streams")
    _check_index(has_state, K, state.device, "has_state")
    if stream_of is not None:
        _check_index(stream_of, n, values.device, "stream_of")
    masks = _row_masks(restart, present, n, values.device)
    out = torch.empty_like(values)
    m, om = float(np.float32(momentum)), float(np.float32(1 - momentum))
    args = (hip.ptr(values), hip.ptr(stream_of), hip.ptr(state), hip.ptr(has_state), n, K, m, om)
    if masks is None:
        hip.check(lib.emo_theta_ema_scan_f32(*args, hip.ptr(out), hip.current_stream()), "emo_theta_ema_scan_f32")
    else:
        hip.check(lib.emo_theta_ema_scan_tracks_f32(*args, *masks, hip.ptr(out), hip.current_stream()), "emo_theta_ema_scan_tracks_f32")
    return out


def expression_controls(values, stream_of=None, neutral=None, gain=None, offset=None, anchor=None, has_anchor=None, ema=None,
                        has_ema=None, relative=False, momentum=None, out=None, restart=None, present=None):
    """The expression controls of the batched entry points on the device (emo_expr_controls_f32; bit for bit
    hostglue.expression_controls, which states the arithmetic): values [n,E] IN FRAME ORDER, stream_of int32 [n] (or None: one
    stream, 0), neutral [K,E] or None, gain a float or [n] or None, offset [E] or [n,E] or None -- a scalar gain and an [E]
    offset are broadcast to the rows here; anchor, ema [K,E] and has_anchor, has_ema int32 [K] are the streams' states, updated
    in place; momentum None = no smoothing (else 1 - momentum is rounded to fp32 once, as in theta_ema_scan).  -> [n,E]
    (`out`, which may be `values`, or a new tensor).  One launch, no host synchronisation.
    restart, present: int32 [n] on the values' device or None -- the streams follow face tracks (emo_expr_controls_tracks_f32; bit
    for bit hostglue.expression_controls(restart=, present=)): a row with restart != 0 first drops its stream's anchor and EMA, a
    row with present == 0 is computed from a copy of the stream's state and leaves the stream as it was."""
    import numpy as np
    lib = hip.load()
    hip.require_cuda_f32(values, neutral, offset, anchor, ema, out)
    if values.dim() != 2 or values.shape[0] == 0 or values.shape[1] == 0:
        raise ValueError(f"expression_controls expects [n,E] values, got {tuple(values.shape)}")
    n, E = values.shape
    dev = values.device
    smooth = momentum is not None
    if (relative or gain is not None) and neutral is None:
        raise ValueError("expression_controls: relative transfer and gain need neutral")
    if relative and (anchor is None or has_anchor is None):
        raise ValueError("expression_controls: relative transfer needs anchor and has_anchor")
    if smooth and (ema is None or has_ema is None):
        raise ValueError("expression_controls: smoothing needs ema and has_ema")
    if smooth and not 0.0 < float(momentum) <= 1.0:
        raise ValueError(f"expression_controls: momentum {momentum} is not in (0, 1]")
    banks = [t for t in (neutral, anchor if relative else None, ema if smooth else None) if t is not None]
    K = banks[0].shape[0] if banks else 1
    for t in banks:
        if t.dim() != 2 or tuple(t.shape) != (K, E) or K == 0:
            raise ValueError(f"expression_controls: neutral, anchor and ema must be [K,{E}], got {tuple(t.shape)}")
    if relative:
        _check_index(has_anchor, K, dev, "has_anchor")
    if smooth:
        _check_index(has_ema, K, dev, "has_ema")
    if stream_of is not None:
        _check_index(stream_of, n, dev, "stream_of")
    if gain is not None:
        if isinstance(gain, torch.Tensor) and gain.dim() == 1:
            hip.require_cuda_f32(gain)
            if gain.shape[0] != n:
                raise ValueError(f"expression_controls: gain has {gain.shape[0]} entries for {n} rows")
        else:
            gain = torch.full((n,), float(gain), dtype=torch.float32, device=dev)
    if offset is not None:
        if offset.dim() == 1 and offset.shape[0] == E:
            offset = offset.expand(n, E).contiguous()
        elif tuple(offset.shape) != (n, E):
            raise ValueError(f"expression_controls: offset must be [{E}] or [{n},{E}], got {tuple(offset.shape)}")
    masks = _row_masks(restart, present, n, dev)
    if out is None:
        out = torch.empty_like(values)
    elif tuple(out.shape) != (n, E):
        raise ValueError(f"expression_controls: out must be [{n},{E}], got {tuple(out.shape)}")
    m, om = (float(np.float32(momentum)), float(np.float32(1 - momentum))) if smooth else (0.0, 0.0)
    args = (hip.ptr(values), hip.ptr(stream_of), hip.ptr(neutral), hip.ptr(gain), hip.ptr(offset),
            hip.ptr(anchor if relative else None), hip.ptr(has_anchor if relative else None), hip.ptr(ema if smooth else None),
            hip.ptr(has_ema if smooth else None), n, K, E, int(bool(relative)), int(smooth), m, om)
    if masks is None:
        hip.check(lib.emo_expr_controls_f32(*args, hip.ptr(out), hip.current_stream()), "emo_expr_controls_f32")
    else:
        hip.check(lib.emo_expr_controls_tracks_f32(*args, *masks, hip.ptr(out), hip.current_stream()), "emo_expr_controls_tracks_f32")
    return out


def head_pose_controls(scale, rotation, translation, stream_of=None, source=None, gain=None, rotation_offset=None,
                       translation_offset=None, zoom=None, anchor=None, has_anchor=None, relative=False, frontal=False, restart=None,
                       present=None):
    """The head-pose controls of the batched entry points on the device (emo_head_pose_controls_f32; bit for bit
    hostglue.head_pose_controls, which states the arithmetic): scale [n,1] or [n,3], rotation and translation [n,3] IN FRAME
    ORDER, stream_of int32 [n] (or None: one stream, 0), source [K,9] or None (needed by relative and gain), gain and zoom a
    float or [n] or None, rotation_offset and translation_offset [3] or [n,3] or None -- a scalar gain / zoom and a [3] offset
    are broadcast to the rows here; anchor [K,9] and has_anchor int32 [K] are the streams' state for `relative`, updated in
    place.  -> (srt [n,9] = the edited rows, theta [n,4,4] = ops.pose_theta of them), both new tensors: the kernel's outputs
    alias none of its inputs.  One launch, no host synchronisation.
    restart, present: int32 [n] on the rows' device or None -- the streams follow face tracks (emo_head_pose_controls_tracks_f32;
    bit for bit hostglue.head_pose_controls(restart=, present=)): under `relative` a row with restart != 0 first drops its
    stream's anchor, and a row with present == 0 never becomes one (it is its own reference where the stream has none)."""
    lib = hip.load()
    hip.require_cuda_f32(scale, rotation, translation, source, anchor)
    if scale.dim() != 2 or scale.shape[0] == 0 or scale.shape[1] not in (1, 3):
        raise ValueError(f"head_pose_controls expects a [n,1] or [n,3] scale, got {tuple(scale.shape)}")
    n, dev = scale.shape[0], scale.device
    for t, what in ((rotation, "rotation"), (translation, "translation")):
        if tuple(t.shape) != (n, 3):
            raise ValueError(f"head_pose_controls: {what} must be [{n},3], got {tuple(t.shape)}")
    if relative and frontal:
        raise ValueError("head_pose_controls: frontal zeroes what relative transfers")
    if (relative or gain is not None) and source is None:
        raise ValueError("head_pose_controls: relative transfer and gain need source")
    if relative and (anchor is None or has_anchor is None):
        raise ValueError("head_pose_controls: relative transfer needs anchor and has_anchor")
    banks = [t for t in (source, anchor if relative else None) if t is not None]
    K = banks[0].shape[0] if banks else 1
    for t in banks:
        if t.dim() != 2 or tuple(t.shape) != (K, 9) or K == 0:
            raise ValueError(f"head_pose_controls: source and anchor must be [K,9], got {tuple(t.shape)}")
    if relative:
        _check_index(has_anchor, K, dev, "has_anchor")
    if stream_of is not None:
        _check_index(stream_of, n, dev, "stream_of")
    masks = _row_masks(restart, present, n, dev)

    def per_row(v, what):
        if v is None:
            return None
        if isinstance(v, torch.Tensor) and v.dim() == 1:
            hip.require_cuda_f32(v)
            if v.shape[0] != n:
                raise ValueError(f"head_pose_controls: {what} has {v.shape[0]} entries for {n} rows")
            return v
        return torch.full((n,), float(v), dtype=torch.float32, device=dev)

    def rows3(v, what):
        if v is None:
            return None
        hip.require_cuda_f32(v)
        if tuple(v.shape) == (3,):
            return v.expand(n, 3).contiguous()
        if tuple(v.shape) != (n, 3):
            raise ValueError(f"head_pose_controls: {what} must be [3] or [{n},3], got {tuple(v.shape)}")
        return v
    gain, zoom = per_row(gain, "gain"), per_row(zoom, "zoom")
    rotation_offset, translation_offset = rows3(rotation_offset, "rotation_offset"), rows3(translation_offset, "translation_offset")
    srt = torch.empty((n, 9), device=dev, dtype=torch.float32)
    theta = torch.empty((n, 4, 4), device=dev, dtype=torch.float32)
    args = (hip.ptr(scale), scale.shape[1], hip.ptr(rotation), hip.ptr(translation), hip.ptr(stream_of), hip.ptr(source), hip.ptr(gain),
            hip.ptr(rotation_offset), hip.ptr(translation_offset), hip.ptr(zoom), hip.ptr(anchor if relative else None),
            hip.ptr(has_anchor if relative else None), n, K, int(bool(relative)), int(bool(frontal)))
    out = (hip.ptr(srt), hip.ptr(theta), hip.current_stream())
    if masks is None:
        hip.check(lib.emo_head_pose_controls_f32(*args, *out), "emo_head_pose_controls_f32")
    else:
        hip.check(lib.emo_head_pose_controls_tracks_f32(*args, *masks, *out), "emo_head_pose_controls_tracks_f32")
    return srt, theta


def crop_track(boxes, stream_of=None, size=None, state=None, has_state=None, last=None, momentum=0.01, smooth=False, fixed=False,
               scale=1.0, box_format="xyxy", missing="skip", min_side=2, K=None, restart=None):
    """Face boxes -> crop and paste windows on the device, the crop tracker's state carried along the row order
    (emo_crop_track_f64; bit for bit hostglue.crop_track, which states the arithmetic: crop_image's, notebooks/infer.py:301-352).
    boxes [M,4] float32 or float64 on the device (widened exactly to float64), IN FRAME ORDER; stream_of int32 [M] (or None: one
    stream, 0); size = (W, H) of every row's frame, or one (W, H) per row as a host sequence (checked and uploaded here) or an
    int32 [M,2] device tensor; state [K,3] float64, has_state [K] int32 and last [K,4] int32 are the streams' state, updated in
    place (state and has_state are needed by `smooth`, last by missing='hold'; K says the number of streams where none is given).
    -> (crop int32 [M,4], paste int32 [M,4], face_scale float64 [M]): every crop window can be read from its row's frame, a paste
    window of side 0 says that the row has no face.  One launch, no host synchronisation.
    restart: int32 [M] on the boxes' device or None (track_assign's, flattened to the rows): a row with restart != 0 first clears
    its stream's EMA flag and last window (emo_crop_track_restarts_f64; hostglue.crop_track(restart=))."""
    from . import hostglue
    lib = hip.load()
    if not isinstance(boxes, torch.Tensor) or boxes.dtype not in (torch.float32, torch.float64):
        raise ValueError("crop_track: boxes must be a float32 or float64 tensor")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] == 0:
        raise ValueError(f"crop_track expects [M,4] boxes, got {tuple(boxes.shape)}")
    hip.require_cuda_f32(torch.empty(0, device=boxes.device))                # (GPU only, like every op)
    M, dev = boxes.shape[0], boxes.device
    boxes = boxes.double().contiguous()
    if box_format not in hostglue.CROP_BOX_FORMATS:
        raise ValueError(f"crop_track: box_format {box_format!r}: 'xyxy' or 'relative'")
    if missing not in hostglue.CROP_MISSING:
        raise ValueError(f"crop_track: missing {missing!r}: 'skip' or 'hold'")
    m = float(momentum)
    if not 0.0 < m <= 1.0:
        raise ValueError(f"crop_track: momentum {momentum} is not in (0, 1]")
    scale = float(scale)
    if scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError(f"crop_track: scale {scale} is not finite")
    if int(min_side) < 1:
        raise ValueError(f"crop_track: min_side {min_side} is below 1")
    hold = missing == "hold"
    if smooth and (state is None or has_state is None):
        raise ValueError("crop_track: smoothing needs state and has_state")
    if hold and last is None:
        raise ValueError("crop_track: missing='hold' needs last")
    given = [t.shape[0] for t in (state, has_state, last) if t is not None]
    K = given[0] if given else (1 if K is None else int(K))
    if K < 1:
        raise ValueError("crop_track: no streams")
    if state is not None and (state.dtype != torch.float64 or state.device != dev or tuple(state.shape) != (K, 3) or not state.is_contiguous()):
        raise ValueError(f"crop_track: state must be a contiguous float64 [{K},3] tensor on the boxes' device")
    if has_state is not None:
        _check_index(has_state, K, dev, "has_state")
    if last is not None and (last.dtype != torch.int32 or last.device != dev or tuple(last.shape) != (K, 4) or not last.is_contiguous()):
        raise ValueError(f"crop_track: last must be a contiguous int32 [{K},4] tensor on the boxes' device")
    if stream_of is not None:
        _check_index(stream_of, M, dev, "stream_of")
    if restart is not None:
        _check_index(restart, M, dev, "restart")
    sizes, Wf, Hf = None, 0, 0
    if isinstance(size, torch.Tensor) and size.device == dev and size.dtype == torch.int32 and size.dim() == 2:
        if tuple(size.shape) != (M, 2) or not size.is_contiguous():
            raise ValueError(f"crop_track: per-row sizes must be a contiguous int32 [{M},2] tensor, got {tuple(size.shape)}")
        sizes = size
    else:
        host = torch.as_tensor(size, dtype=torch.int64)
        if tuple(host.shape) not in ((2,), (M, 2)) or bool((host < 1).any()) or bool((host >= 1 << 30).any()):
            raise ValueError(f"crop_track: size is the (W, H) of every frame or one per row, positive: got {size!r}")
        if host.dim() == 1:
            Wf, Hf = int(host[0]), int(host[1])
        else:
            sizes = host.to(torch.int32).to(dev, non_blocking=True)
    crop = torch.empty((M, 4), device=dev, dtype=torch.int32)
    paste = torch.empty((M, 4), device=dev, dtype=torch.int32)
    face_scale = torch.empty((M,), device=dev, dtype=torch.float64)
    args = (hip.ptr(boxes), hip.ptr(stream_of), hip.ptr(sizes), Wf, Hf, hip.ptr(state if smooth else None),
            hip.ptr(has_state if smooth else None), hip.ptr(last), M, K, m, 1.0 - m, int(bool(smooth)), int(bool(fixed)), scale,
            hostglue.CROP_BOX_FORMATS[box_format], int(hold), int(min_side))
    out = (hip.ptr(crop), hip.ptr(paste), hip.ptr(face_scale), hip.current_stream())
    if restart is None:
        hip.check(lib.emo_crop_track_f64(*args, *out), "emo_crop_track_f64")
    else:
        hip.check(lib.emo_crop_track_restarts_f64(*args, hip.ptr(restart), *out), "emo_crop_track_restarts_f64")
    return crop, paste, face_scale


def track_assign(dets, stream_of=None, ref=None, age=None, min_iou=0.3, max_missed=15, box_format="xyxy"):
    """Unordered face detections -> ordered track rows on the device, the tracks' state carried along the frame order
    (emo_track_assign_f64; bit for bit hostglue.track_assign, which states the association: greedy, by IoU, per video stream).
    dets [F,D,4] float32 or float64 on the device (widened exactly to float64), IN FRAME ORDER, D <= 32, NaN rows = padding;
    stream_of int32 [F] (or None: one stream, 0); ref [K,P,4] float64 and age [K,P] int32 (-1 = free) are the streams' tracks,
    updated in place, P <= 16; min_iou in (0, 1]; max_missed >= 0; box_format 'xyxy' | 'relative'.
    -> (boxes float64 [F,P,4]: the detection of track p in frame f as it came, NaN where it has none; restart int32 [F,P]: 1
    where the track was born or died in that frame; track_of int32 [F,D]: the track of each detection or -1).  One launch, one
    wave per stream, no host synchronisation."""
    from . import hostglue
    lib = hip.load()
    if not isinstance(dets, torch.Tensor) or dets.dtype not in (torch.float32, torch.float64):
        raise ValueError("track_assign: dets must be a float32 or float64 tensor")
    if dets.dim() != 3 or dets.shape[2] != 4 or dets.shape[0] == 0 or dets.shape[1] == 0:
        raise ValueError(f"track_assign expects [F,D,4] detections, got {tuple(dets.shape)}")
    F, D, dev = dets.shape[0], dets.shape[1], dets.device
    if D > hostglue.TRACK_MAX_DETECTIONS:
        raise ValueError(f"track_assign: {D} detections per frame, at most {hostglue.TRACK_MAX_DETECTIONS} are served")
    hip.require_cuda_f32(torch.empty(0, device=dev))                         # (GPU only, like every op)
    if box_format not in hostglue.CROP_BOX_FORMATS:
        raise ValueError(f"track_assign: box_format {box_format!r}: 'xyxy' or 'relative'")
    min_iou = float(min_iou)
    if not 0.0 < min_iou <= 1.0:
        raise ValueError(f"track_assign: min_iou {min_iou} is not in (0, 1]")
    if isinstance(max_missed, bool) or not isinstance(max_missed, int) or max_missed < 0:
        raise ValueError(f"track_assign: max_missed {max_missed!r} is not an integer >= 0")
    if not isinstance(ref, torch.Tensor) or not isinstance(age, torch.Tensor) or ref.dim() != 3 or age.dim() != 2:
        raise ValueError("track_assign: the tracks' state is missing: ref float64 [K,P,4] and age int32 [K,P]")
    K, P = age.shape
    if K < 1 or not 1 <= P <= hostglue.TRACK_MAX_TRACKS:
        raise ValueError(f"track_assign: age is {tuple(age.shape)}: [K,P] with K >= 1 and 1 <= P <= {hostglue.TRACK_MAX_TRACKS}")
    if ref.dtype != torch.float64 or ref.device != dev or tuple(ref.shape) != (K, P, 4) or not ref.is_contiguous():
        raise ValueError(f"track_assign: ref must be a contiguous float64 [{K},{P},4] tensor on the detections' device")
    if age.dtype != torch.int32 or age.device != dev or not age.is_contiguous():
        raise ValueError(f"track_assign: age must be a contiguous int32 [{K},{P}] tensor on the detections' device")
    if stream_of is not None:
        _check_index(stream_of, F, dev, "stream_of")
    dets = dets.double().contiguous()
    boxes = torch.empty((F, P, 4), device=dev, dtype=torch.float64)
    restart = torch.empty((F, P), device=dev, dtype=torch.int32)
    track_of = torch.empty((F, D), device=dev, dtype=torch.int32)
    hip.check(lib.emo_track_assign_f64(hip.ptr(dets), hip.ptr(stream_of), F, D, P, K, hip.ptr(ref), hip.ptr(age), min_iou, max_missed,
                                       hostglue.CROP_BOX_FORMATS[box_format], hip.ptr(boxes), hip.ptr(restart), hip.ptr(track_of),
                                       hip.current_stream()), "emo_track_assign_f64")
    return boxes, restart, track_of


def present_rows(crop, paste, F, P):
    """The present rows of the tracker's windows, first and in order, on the device (emo_present_rows_i32; bit for bit
    hostglue.present_rows, which states the contract): a stable compaction of the M = F * P frame-major rows of crop_track's
    crop and paste [M,4] int32 (contiguous, on one device); row i is present iff paste[i][2] > 0.
    -> (count int32 [F]: the present rows of every frame; first int32 [F + 1]: those in front of every frame, first[F] = T their
    total; row_of int32 [M]: the index of the j-th present row, -1 from T on; crop_out, paste_out int32 [M,4]: their windows,
    zeros from T on).  One launch of one block, no host synchronisation."""
    from . import hostglue
    lib = hip.load()
    F, P = int(F), int(P)
    if F <= 0 or not 1 <= P <= hostglue.TRACK_MAX_TRACKS or F * P > hostglue.PRESENT_MAX_ROWS:
        raise ValueError(f"present_rows: F = {F} frames of P = {P} rows: F >= 1, 1 <= P <= {hostglue.TRACK_MAX_TRACKS}, F * P <= 2^24")
    M = F * P
    for t, name in ((crop, "crop"), (paste, "paste")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (M, 4) or not t.is_contiguous():
            raise ValueError(f"present_rows: {name} must be a contiguous int32 [{M},4] tensor, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    dev = crop.device
    if paste.device != dev:
        raise ValueError("present_rows: crop and paste are on different devices")
    hip.require_cuda_f32(torch.empty(0, device=dev))                         # (GPU only, like every op)
    count = torch.empty((F,), device=dev, dtype=torch.int32)
    first = torch.empty((F + 1,), device=dev, dtype=torch.int32)
    row_of = torch.empty((M,), device=dev, dtype=torch.int32)
    crop_out = torch.empty((M, 4), device=dev, dtype=torch.int32)
    paste_out = torch.empty((M, 4), device=dev, dtype=torch.int32)
    hip.check(lib.emo_present_rows_i32(hip.ptr(crop), hip.ptr(paste), F, P, hip.ptr(count), hip.ptr(first), hip.ptr(row_of),
                                       hip.ptr(crop_out), hip.ptr(paste_out), hip.current_stream()), "emo_present_rows_i32")
    return count, first, row_of, crop_out, paste_out
