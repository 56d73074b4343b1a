"""fp64 references and error checkers for single launches of the non-convolution ops the passes make (a helper module, not a
test file; the sibling of conv_reference.py): volume_to_channels_last, add, add_rows_indexed, avgpool, upsample_trilinear,
groupnorm_affine (own pass / TileStats / RunSums), small_gemm, projector_finalize, mat4_inverse and grid_sample3d (delta= /
theta=, with and without vol_index); for the launches of the embedders (emoportraits_amd/embedders.py): conv2d_generic,
maxpool2d, affine_add_relu, grid_sample2d (grid= / theta= with its warp), resize2d (both modes, window=, clamp01=) and
pose_theta; and for the stage-2 and frame glue: mul_mask, stage2_compose, pack_rgb8 and unpack_rgb8.

Every reference is plain torch in fp64, computed one sample at a time on whatever device the inputs live on; none calls a
kernel of the project.  Every checker compares a launch's output with that reference sample by sample and returns a dict of
figures: 'frames' (the samples checked), 'frame_fig' (the worst figure of each, in 'unit'), 'worst', 'worst_frame' and
'failures' (the violations; empty when the launch passes) -- one host synchronisation per launch.

The bounds are the operation's own arithmetic (u = 2^-24, the unit roundoff of fp32) or constants the suite already states
(conv_reference.FP32_FRAME, STATS_TOL, SPLIT_MAX and the fp16 split's mean margin); each checker's docstring derives its own.
"""
import os
import sys

import torch
import torch.nn.functional as F

from conv_reference import FP32_FRAME, SPLIT_MAX, SPLIT_MEAN, STATS_TOL

U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -149                  # the smallest fp32 subnormal: what a rounding can cost where the result underflows
# the sampler against ATen's fp32 CPU kernel on the same inputs: the margins the conv checker grants a split kernel over the
# fp32 kernel (a different, equally valid order of fp32 operations), each plus SAMPLER_FLOOR x mean |ref|
SAMPLER_MAX, SAMPLER_MEAN, SAMPLER_FLOOR = SPLIT_MAX, SPLIT_MEAN["f16x2"], 1e-7


def _f64(t):
    return t.to(torch.float64)


def _bounded_row(got, ref, bound):
    """-> [worst |err| / bound, outputs outside the bound (NaN included), max |err|, max |ref|] as one fp64 tensor"""
    assert ref.dtype == torch.float64 and bound.dtype == torch.float64, (ref.dtype, bound.dtype)
    if got.shape != ref.shape:
        raise ValueError(f"output {tuple(got.shape)} vs reference {tuple(ref.shape)}")
    e = (_f64(got) - ref).abs()
    bad = ~(e <= bound)
    ratio = torch.where(e == 0, torch.zeros_like(e), torch.nan_to_num(e / bound.clamp_min(1e-300), nan=float("inf")))
    return torch.stack([ratio.max(), _f64(bad.sum()), torch.nan_to_num(e, nan=float("inf")).max(), ref.abs().max()])


def _bounded_fig(rows, frames, what):
    """figures of a launch held to a per-output bound: rows = _bounded_row per frame"""
    t = torch.stack(rows).cpu()                       # one host synchronisation per launch
    frame_fig = t[:, 0].tolist()
    w = max(range(len(frames)), key=lambda i: frame_fig[i])
    bad = [f"{what}: frame {n}: {int(t[i, 1])} outputs outside the bound, worst {t[i, 0]:.3g} x bound (max err {t[i, 2]:.3e}, "
           f"max|ref| {t[i, 3]:.3e})" for i, n in enumerate(frames) if t[i, 1] != 0]
    return dict(frames=list(frames), frame_fig=frame_fig, unit="x bound", worst=frame_fig[w], worst_frame=frames[w],
                max_err=float(t[:, 2].max()), ref_max=float(t[:, 3].max()), failures=bad)


def _frames(n, frames):
    return list(range(n)) if frames is None else list(frames)


# ---- volume_to_channels_last ---------------------------------------------------------------------------------------------
def channels_last_fp64(vol):
    """[N,C,D,H,W] -> [N,D,H,W,C] in fp64 (a permutation: no arithmetic)"""
    return _f64(vol).permute(0, 2, 3, 4, 1).contiguous()


def check_channels_last(out, vol, frames=None):
    """bit equality with the permutation, sample by sample; the figure is the count of differing elements"""
    fr = _frames(vol.shape[0], frames)
    if tuple(out.shape) != (vol.shape[0],) + tuple(vol.shape[2:]) + (vol.shape[1],):
        raise ValueError(f"output {tuple(out.shape)} is not the channels-last form of {tuple(vol.shape)}")
    rows = [(out[n].view(torch.int32) != vol[n].permute(1, 2, 3, 0).contiguous().view(torch.int32)).sum() for n in fr]
    t = torch.stack(rows).cpu().tolist()
    w = max(range(len(fr)), key=lambda i: t[i])
    bad = [f"volume_to_channels_last: frame {n}: {t[i]} elements differ from the permutation" for i, n in enumerate(fr) if t[i]]
    return dict(frames=fr, frame_fig=[float(v) for v in t], unit="differing elements", worst=float(t[w]), worst_frame=fr[w],
                failures=bad)


# ---- add / add_rows_indexed ----------------------------------------------------------------------------------------------
def _alpha32(alpha):
    return float(torch.tensor(float(alpha), dtype=torch.float32))      # the kernel takes alpha as an fp32 argument


def add_fp64(a, b, alpha=1.0):
    """(a + b[i % period]) * alpha in fp64 from the fp32 operands; period = b.numel() (b tiles the flattened a)"""
    if a.numel() % b.numel():
        raise ValueError("b does not tile a")
    out = (_f64(a).reshape(-1, b.numel()) + _f64(b).reshape(1, -1)) * _alpha32(alpha)
    return out.reshape(a.shape)


def add_rows_indexed_fp64(a, table, index, alpha=1.0):
    """(a[b] + table[index[b]]) * alpha in fp64; an index outside [0, K) gives a zero row"""
    K = table.shape[0]
    idx = index.to(torch.int64)
    ok = (idx >= 0) & (idx < K)
    rows = _f64(table).reshape(K, -1)[idx.clamp(0, K - 1)]
    out = (_f64(a).reshape(a.shape[0], -1) + rows) * _alpha32(alpha)
    out = torch.where(ok[:, None], out, torch.zeros_like(out))
    return out.reshape(a.shape)


def _check_add(out, ref, frames, what):
    """The kernel rounds twice: s = fl(a + b) = (a + b)(1 + d1), out = fl(s alpha) = (a + b) alpha (1 + d1)(1 + d2), |d| <= u.
    Per element |out - ref| <= (2u + u^2) |ref| <= 2u (1 + u) |ref|, plus TINY where the product underflows (the fp64 reference
    itself is exact to 2^-52 |ref|, inside the u^2 term's slack)."""
    fr = _frames(out.shape[0], frames)
    rows = []
    for n in fr:
        r = ref[n]
        rows.append(_bounded_row(out[n], r, 2.0 * U * (1.0 + U) * r.abs() + TINY))
    return _bounded_fig(rows, fr, what)


def check_add(out, a, b, alpha=1.0, frames=None):
    """ops.add against add_fp64 under the per-element bound of _check_add; frames = rows of the leading dimension"""
    return _check_add(out, add_fp64(a, b, alpha), frames, "add")


def check_add_rows_indexed(out, a, table, index, alpha=1.0, frames=None):
    """ops.add_rows_indexed against add_rows_indexed_fp64 under the same per-element bound (a zero row must be exactly zero)"""
    return _check_add(out, add_rows_indexed_fp64(a, table, index, alpha), frames, "add_rows_indexed")


# ---- avgpool -------------------------------------------------------------------------------------------------------------
def _pool_windows(v, kernel):
    """v [C, (D,) H, W] -> [C, Do, kd, Ho, kh, Wo, kw]"""
    if v.dim() == 3:
        v = v.unsqueeze(1)
        kernel = (1,) + tuple(kernel)
    kd, kh, kw = kernel
    C, D, H, W = v.shape
    if D % kd or H % kh or W % kw:
        raise ValueError(f"window {kernel} does not tile {(D, H, W)}")
    return v.reshape(C, D // kd, kd, H // kh, kh, W // kw, kw)


def avgpool_frames(x, kernel, frames=None):
    """yields (n, fp64 mean of every window [C, (Do,) Ho, Wo], fp64 max |x| of every window) per sample: AvgPool with
    stride == kernel, 5-D x with (kd, kh, kw) or 4-D x with (kh, kw)"""
    for n in _frames(x.shape[0], frames):
        w = _pool_windows(_f64(x[n]), kernel)
        mean, amax = w.mean(dim=(2, 4, 6)), w.abs().amax(dim=(2, 4, 6))
        if x.dim() == 4:
            mean, amax = mean[:, 0], amax[:, 0]
        yield n, mean, amax


def avgpool_fp64(x, kernel):
    return torch.stack([m for _, m, _ in avgpool_frames(x, kernel)])


def check_avgpool(out, x, kernel, frames=None):
    """The kernel adds the n = kd kh kw values of a window one after the other in fp32 and multiplies by fl(1 / n): n - 1
    rounded additions (the first lands on 0), the rounding of the reciprocal and of the product, n + 1 roundings.  With M the
    largest |value| of the window every partial sum is at most k M, so the additions cost at most u M (n (n + 1) / 2 - 1) / n
    on the mean and the last two u M each: (n + 1) / 2 + 2 - 1 / n <= n + 1 for n >= 2 (n = 1: two roundings).  Per output
    |out - ref| <= (n + 1) u M (1 + u) with M of its OWN window (an fp64 max-pool of |x|), plus TINY."""
    n_win = 1
    for k in kernel:
        n_win *= int(k)
    fr = _frames(x.shape[0], frames)
    rows = [_bounded_row(out[n], mean, (n_win + 1) * U * (1.0 + U) * amax + TINY) for n, mean, amax in avgpool_frames(x, kernel, fr)]
    return _bounded_fig(rows, fr, f"avgpool {tuple(kernel)}")


# ---- upsample_trilinear --------------------------------------------------------------------------------------------------
def _lin_taps(out_size, in_size, factor, device):
    """ATen's area_pixel_compute_source_index for align_corners=False and scale 1 / factor: src = 0.5 (o + 0.5) - 0.5 clamped at
    0 -> (i0, i1, l0, l1); all exact in binary for factor 2"""
    o = torch.arange(out_size, dtype=torch.float64, device=device)
    if factor == 1:
        i = o.to(torch.int64)
        return i, i, torch.ones_like(o), torch.zeros_like(o)
    if factor != 2:
        raise ValueError("factors are 1 or 2")
    src = (0.5 * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().to(torch.int64)
    i1 = i0 + (i0 < in_size - 1).to(torch.int64)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def upsample_trilinear_frames(x, factors, frames=None):
    """yields (n, fp64 F.interpolate(x[n], scale_factor=factors, mode='trilinear') [C, Do, Ho, Wo], fp64 largest |tap| that
    carries weight in each output) per sample of the 5-D x"""
    D, H, W = x.shape[2:]
    taps = [_lin_taps(s * f, s, f, x.device) for s, f in zip((D, H, W), factors)]
    for n in _frames(x.shape[0], frames):
        v = _f64(x[n])
        a = v.abs()
        for axis in (3, 2, 1):
            i0, i1, l0, l1 = taps[axis - 1]
            shape = [1, 1, 1, 1]
            shape[axis] = -1
            v = l0.view(shape) * v.index_select(axis, i0) + l1.view(shape) * v.index_select(axis, i1)
            a1 = torch.where((l1 > 0).view(shape), a.index_select(axis, i1), torch.zeros((), dtype=torch.float64, device=x.device))
            a = torch.maximum(a.index_select(axis, i0), a1)
        yield n, v, a


def upsample_trilinear_fp64(x, factors):
    return torch.stack([v for _, v, _ in upsample_trilinear_frames(x, factors)])


UPSAMPLE_ROUNDINGS = 7


def check_upsample_trilinear(out, x, factors, frames=None):
    """The kernel evaluates ATen's nested form t0 (h0 (w0 a + w1 b) + h1 (...)) + t1 (...): every intermediate is a convex
    combination of the taps, at most M = the largest |tap| of the output in magnitude, and the longest chain from a tap to the
    output passes UPSAMPLE_ROUNDINGS = 7 rounded operations (product and sum per axis, and the last sum): per output
    |out - ref| <= 7 u M (1 + u) with M of its OWN taps, plus TINY."""
    fr = _frames(x.shape[0], frames)
    rows = [_bounded_row(out[n], ref, UPSAMPLE_ROUNDINGS * U * (1.0 + U) * amax + TINY)
            for n, ref, amax in upsample_trilinear_frames(x, factors, fr)]
    return _bounded_fig(rows, fr, f"upsample_trilinear {tuple(factors)}")


# ---- groupnorm_affine ----------------------------------------------------------------------------------------------------
def groupnorm_affine_frames(x, gamma=None, beta=None, ada_gamma=None, ada_beta=None, groups=32, eps=1e-5, frames=None):
    """yields (n, scale [C], shift [C]) in fp64 such that GroupNorm(groups)(x)[n, c] == x[n, c] * scale[c] + shift[c], from a
    direct fp64 reduction of x[n].  gamma / beta: the static affine; ada_gamma / ada_beta [N, C] (any row stride): the adaptive
    form WITH the reference's quirk (csrc/groupnorm.hip: AdaptiveGroupNorm applies its static affine first): sc ag, sh ag + ab"""
    C = x.shape[1]
    cg = C // groups
    if C % groups:
        raise ValueError(f"{C} channels in {groups} groups")
    for n in _frames(x.shape[0], frames):
        v = _f64(x[n]).reshape(groups, -1)
        mean = v.mean(-1)
        var = ((v - mean[:, None]) ** 2).mean(-1)
        rstd = (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).repeat_interleave(cg)
        mean = mean.repeat_interleave(cg)
        sc = rstd * _f64(gamma) if gamma is not None else rstd
        sh = -mean * sc
        if beta is not None:
            sh = sh + _f64(beta)
        if ada_gamma is not None:
            ag, ab = _f64(ada_gamma[n]), _f64(ada_beta[n])
            sc, sh = sc * ag, sh * ag + ab
        yield n, sc, sh


def groupnorm_affine_fp64(x, gamma=None, beta=None, ada_gamma=None, ada_beta=None, groups=32, eps=1e-5):
    rows = list(groupnorm_affine_frames(x, gamma, beta, ada_gamma, ada_beta, groups, eps))
    return torch.stack([s for _, s, _ in rows]), torch.stack([h for _, _, h in rows])


def check_groupnorm_affine(scale, shift, x, gamma=None, beta=None, ada_gamma=None, ada_beta=None, groups=32, eps=1e-5, frames=None):
    """(scale, shift) of any of the three forms (own pass, TileStats, RunSums) against the fp64 statistics of x itself, under
    the suite's STATS_TOL as test_conv_epilogue_groupnorm_statistics applies it: |scale - ref| <= STATS_TOL max |ref scale| of
    the launch, |shift - ref| <= STATS_TOL max(1, max |ref shift| of the launch).  The figure is the larger of the two ratios."""
    fr = _frames(x.shape[0], frames)
    rows = []
    for n, sc, sh in groupnorm_affine_frames(x, gamma, beta, ada_gamma, ada_beta, groups, eps, fr):
        ds, dh = (_f64(scale[n]) - sc).abs(), (_f64(shift[n]) - sh).abs()
        rows.append(torch.stack([torch.nan_to_num(ds, nan=float("inf")).max(), sc.abs().max(),
                                 torch.nan_to_num(dh, nan=float("inf")).max(), sh.abs().max()]))
    t = torch.stack(rows).cpu()
    s_ref, h_ref = float(t[:, 1].max()), max(1.0, float(t[:, 3].max()))
    s_rel, h_rel = (t[:, 0] / max(s_ref, 1e-300)).tolist(), (t[:, 2] / h_ref).tolist()
    frame_fig = [max(a, b) / STATS_TOL for a, b in zip(s_rel, h_rel)]
    w = max(range(len(fr)), key=lambda i: frame_fig[i])
    bad = []
    for i, n in enumerate(fr):
        if not s_rel[i] <= STATS_TOL:
            bad.append(f"groupnorm_affine: frame {n}: scale differs by {s_rel[i]:.3e} of max|scale| > {STATS_TOL:g}")
        if not h_rel[i] <= STATS_TOL:
            bad.append(f"groupnorm_affine: frame {n}: shift differs by {h_rel[i]:.3e} of max(1, max|shift|) > {STATS_TOL:g}")
    return dict(frames=fr, frame_fig=frame_fig, unit="x STATS_TOL", worst=frame_fig[w], worst_frame=fr[w],
                scale_rel=max(s_rel), shift_rel=max(h_rel), failures=bad)


# ---- small_gemm / projector_finalize -------------------------------------------------------------------------------------
def small_gemm_fp64(A, B, NN):
    """C[b][m][:NN] = sum_k A[m][k] B[b][k][:NN] in fp64: A [M, K], B [batch, K * NN] in any shape -> [batch, M, NN]"""
    M, K = A.shape
    return torch.einsum("mk,bkn->bmn", _f64(A), _f64(B).reshape(B.shape[0], K, NN))


def _check_rows(pairs, frames, what):
    """every (out, ref) pair, each batch row against FP32_FRAME x max |ref of that row| (the suite's bound of an fp32 dot
    product, conv_reference.FP32_FRAME)"""
    rows = []
    for n in frames:
        worst = []
        for out, ref in pairs:
            assert ref.dtype == torch.float64
            if tuple(out.shape) != tuple(ref.shape):
                raise ValueError(f"output {tuple(out.shape)} vs reference {tuple(ref.shape)}")
            e = torch.nan_to_num((_f64(out[n]) - ref[n]).abs(), nan=float("inf")).max()
            worst.append(e / ref[n].abs().max().clamp_min(1e-300))
        rows.append(torch.stack(worst).max())
    t = torch.stack(rows).cpu().tolist()
    w = max(range(len(frames)), key=lambda i: t[i])
    bad = [f"{what}: frame {n}: max err {t[i]:.3e} of max|ref| > {FP32_FRAME:g}" for i, n in enumerate(frames) if not t[i] <= FP32_FRAME]
    return dict(frames=list(frames), frame_fig=t, unit="of max|ref|", worst=t[w], worst_frame=frames[w], failures=bad)


def check_small_gemm(out, A, B, NN, frames=None):
    return _check_rows([(out, small_gemm_fp64(A, B, NN))], _frames(B.shape[0], frames), f"small_gemm NN={NN}")


def projector_finalize_fp64(T, V, norm_of_row, gamma, beta):
    """T [B, R, E], V [n, E, 2], norm_of_row [R], gamma / beta [R] -> (ada_gamma, ada_beta) [B, R] in fp64:
    gamma[r] + sum_e T[b, r, e] V[norm_of_row[r], e, 0] and beta[r] + sum_e T[b, r, e] V[norm_of_row[r], e, 1]"""
    Vr = _f64(V)[norm_of_row.to(torch.int64)]                            # [R, E, 2]
    d = torch.einsum("bre,rej->brj", _f64(T), Vr)
    return _f64(gamma)[None] + d[..., 0], _f64(beta)[None] + d[..., 1]


def check_projector_finalize(ag, ab, T, V, norm_of_row, gamma, beta, frames=None):
    rg, rb = projector_finalize_fp64(T, V, norm_of_row, gamma, beta)
    return _check_rows([(ag, rg), (ab, rb)], _frames(T.shape[0], frames), "projector_finalize")


# ---- mat4_inverse --------------------------------------------------------------------------------------------------------
def mat4_inverse_fp64(m):
    """torch.linalg.inv of the fp32 matrices in fp64 (on the CPU: 4 x 4 matrices, no device solver involved)"""
    return torch.linalg.inv(_f64(m).cpu())


def check_mat4_inverse(out, m, frames=None):
    """The kernel eliminates in double (error ~ cond 2^-53, nothing at fp32 scale for a head-pose affine) and rounds each
    entry once: per matrix |out - ref| <= 2^-23 max |inverse| (the rounding of the largest entry is at most 2^-24 of it; the
    other half is room for the elimination's own error, which a value check cannot tell from the rounding)."""
    fr = _frames(m.shape[0], frames)
    ref = mat4_inverse_fp64(m)
    e = torch.nan_to_num((_f64(out).cpu() - ref).abs(), nan=float("inf")).reshape(m.shape[0], -1).amax(1)
    lim = 2.0 ** -23 * ref.abs().reshape(m.shape[0], -1).amax(1)
    fig = [float(e[n] / lim[n].clamp_min(1e-300)) for n in fr]
    w = max(range(len(fr)), key=lambda i: fig[i])
    bad = [f"mat4_inverse: matrix {n}: max err {float(e[n]):.3e} > 2^-23 x max|inverse| = {float(lim[n]):.3e}"
           for n in fr if not bool(e[n] <= lim[n])]
    return dict(frames=fr, frame_fig=fig, unit="x 2^-23 max|inverse|", worst=fig[w], worst_frame=fr[w], failures=bad)


# ---- launches held to a yardstick ------------------------------------------------------------------------------------------
def _yardstick_row(got, ref, yard, n):
    """frame n -> [max |err|, sum |err|, the yardstick's max |err|, its sum |err|, sum |ref|, elements] of one frame as one fp64 tensor"""
    assert ref.dtype == torch.float64 and yard.dtype == torch.float32, (ref.dtype, yard.dtype)
    if got.shape != ref.shape:
        raise ValueError(f"frame {n}: output {tuple(got.shape)} vs reference {tuple(ref.shape)}")
    e = torch.nan_to_num((_f64(got) - ref).abs(), nan=float("inf"))
    ey = (_f64(yard.to(ref.device)) - ref).abs()
    return torch.stack([e.max(), e.sum(), ey.max(), ey.sum(), ref.abs().sum(),
                        torch.tensor(float(ref.numel()), dtype=torch.float64, device=ref.device)])


def _yardstick_fig(rows, fr, what, yardstick="ATen fp32"):
    """figures of a launch held to a yardstick's error against the same fp64 reference (rows = _yardstick_row per frame): over
    the launch, max |err| <= SAMPLER_MAX x the yardstick's and mean |err| <= SAMPLER_MEAN x the yardstick's, each plus
    SAMPLER_FLOOR x mean |ref|; 'yardstick' names what the ratios are taken to"""
    t = torch.stack(rows).cpu()                       # one host synchronisation per launch
    count = float(t[:, 5].sum())
    max_err, mean_err = float(t[:, 0].max()), float(t[:, 1].sum()) / count
    y_max, y_mean = float(t[:, 2].max()), float(t[:, 3].sum()) / count
    scale = float(t[:, 4].sum()) / count
    allow_max, allow_mean = SAMPLER_MAX * y_max + SAMPLER_FLOOR * scale, SAMPLER_MEAN * y_mean + SAMPLER_FLOOR * scale
    frame_fig = (t[:, 0] / max(allow_max, 1e-300)).tolist()
    w = max(range(len(fr)), key=lambda i: frame_fig[i])
    bad = []
    if not max_err <= allow_max:
        bad.append(f"{what}: max err {max_err:.3e} (frame {fr[w]}) > {SAMPLER_MAX} x {yardstick}'s {y_max:.3e} + "
                   f"{SAMPLER_FLOOR:g} x {scale:.3e}")
    if not mean_err <= allow_mean:
        bad.append(f"{what}: mean err {mean_err:.3e} > {SAMPLER_MEAN} x {yardstick}'s {y_mean:.3e} + {SAMPLER_FLOOR:g} x {scale:.3e}")
    return dict(frames=fr, frame_fig=frame_fig, unit="x allowed max err", worst=frame_fig[w], worst_frame=fr[w], yardstick=yardstick,
                max_err=max_err, mean_err=mean_err, yard_max_err=y_max, yard_mean_err=y_mean, scale=scale,
                max_ratio=max_err / y_max if y_max > 0 else (0.0 if max_err == 0 else float("inf")),
                mean_ratio=mean_err / y_mean if y_mean > 0 else (0.0 if mean_err == 0 else float("inf")), failures=bad)


# ---- grid_sample3d -------------------------------------------------------------------------------------------------------
def lattice(n, device):
    """torch.linspace(-1, 1, n) in fp32, computed on the CPU (the reference's identity lattice), on `device`"""
    return torch.linspace(-1, 1, n).to(device)


def _ncdhw(v, layout):
    """one volume in `layout` -> its [C, D, H, W] view"""
    if layout == "ndhwc":
        return v.permute(3, 0, 1, 2)
    if layout == "ncdhw":
        return v
    raise ValueError(f"layout {layout!r}: 'ncdhw' or 'ndhwc'")


def delta_grid_f32(delta_n):
    """delta [3, Do, Ho, Wo] of one sample -> grid [Do, Ho, Wo, 3] = identity lattice + delta, ONE fp32 addition per coordinate
    (the contract of ops.grid_sample3d(delta=))"""
    _, Do, Ho, Wo = delta_n.shape
    dev = delta_n.device
    d = delta_n.float()
    return torch.stack([lattice(Wo, dev).view(1, 1, Wo) + d[0], lattice(Ho, dev).view(1, Ho, 1) + d[1],
                        lattice(Do, dev).view(Do, 1, 1) + d[2]], dim=-1)


def _lattice_points(size, device, dtype):
    """[Do, Ho, Wo, 4]: (x, y, z, 1) of the identity lattice, x fastest"""
    Do, Ho, Wo = size
    z, y, x = torch.meshgrid(lattice(Do, device).to(dtype), lattice(Ho, device).to(dtype), lattice(Wo, device).to(dtype),
                             indexing="ij")
    return torch.stack([x, y, z, torch.ones_like(x)], dim=-1)


def theta_grid_fp64(theta_n, size):
    """theta [3 or 4, 4] of one sample -> grid [Do, Ho, Wo, 3] fp64 = fp64 product of the fp32 lattice and the fp32 theta"""
    return _lattice_points(size, theta_n.device, torch.float64) @ _f64(theta_n[:3]).t()


def theta_grid_f32(theta_n, size):
    """the same as the reference code builds it: identity_grid.bmm(theta[:, :3].transpose(1, 2)) in fp32"""
    p = _lattice_points(size, theta_n.device, torch.float32)
    return p.reshape(1, -1, 4).bmm(theta_n[:3].float().t().unsqueeze(0)).reshape(tuple(size) + (3,))


def grid_sample3d_frames(vol, delta=None, theta=None, padding_mode="zeros", in_layout="ncdhw", vol_index=None, frames=None,
                         yardstick=True):
    """yields (n, fp64 reference [C, Do, Ho, Wo], yardstick or None) per sample of ops.grid_sample3d(vol, delta= / theta=,
    padding_mode=, in_layout=, vol_index=): F.grid_sample in fp64 (align_corners=False) on the NCDHW view of the sample's volume
    -- vol[vol_index[n]] (an index outside the bank: zeros), vol[n], or the one shared volume -- and ATen's fp32 CPU
    F.grid_sample on the same inputs (delta: the same fp32 grid; theta: the fp32 bmm grid) as the yardstick."""
    if (delta is None) == (theta is None):
        raise ValueError("exactly one of delta / theta")
    N = delta.shape[0] if delta is not None else theta.shape[0]
    Nv = vol.shape[0]
    index = None if vol_index is None else vol_index.cpu().tolist()       # (with the launch's one synchronisation in mind: [N] ints)
    if index is None and Nv not in (1, N):
        raise ValueError(f"volume batch {Nv} does not match grid batch {N}")
    cpu_vol = {}
    for n in _frames(N, frames):
        k = index[n] if index is not None else (n if Nv > 1 else 0)
        v = _ncdhw(vol[min(max(k, 0), Nv - 1)], in_layout)
        C, D, H, W = v.shape
        if delta is not None:
            g32 = delta_grid_f32(delta[n])
            g64 = _f64(g32)
        else:
            g64 = theta_grid_fp64(theta[n], (D, H, W))
        if not 0 <= k < Nv:
            yield n, torch.zeros((C,) + tuple(g64.shape[:3]), dtype=torch.float64, device=vol.device), \
                (torch.zeros((C,) + tuple(g64.shape[:3])) if yardstick else None)
            continue
        ref = F.grid_sample(_f64(v)[None], g64[None], mode="bilinear", padding_mode=padding_mode, align_corners=False)[0]
        assert ref.dtype == torch.float64
        yard = None
        if yardstick:
            if k not in cpu_vol:
                cpu_vol.clear()                                            # (one volume resident at a time)
                cpu_vol[k] = v.float().cpu().contiguous()
            g = g32.cpu() if delta is not None else theta_grid_f32(theta[n].cpu(), (D, H, W))
            yard = F.grid_sample(cpu_vol[k][None], g[None], mode="bilinear", padding_mode=padding_mode, align_corners=False)[0]
            assert yard.dtype == torch.float32 and yard.device.type == "cpu"
        yield n, ref, yard


def grid_sample3d_fp64(vol, delta=None, theta=None, padding_mode="zeros", in_layout="ncdhw", vol_index=None):
    return torch.stack([r for _, r, _ in grid_sample3d_frames(vol, delta, theta, padding_mode, in_layout, vol_index, yardstick=False)])


def check_grid_sample3d(out, vol, delta=None, theta=None, padding_mode="zeros", in_layout="ncdhw", out_layout="ncdhw",
                        vol_index=None, frames=None):
    """The sampler's error is conditioned by the volume's gradient (a coordinate off by one ulp moves the result by ulp x
    gradient), so it is held to ATen's fp32 CPU F.grid_sample on the same inputs, measured against the same fp64 reference:
    over the launch, max |err| <= SAMPLER_MAX (2) x the yardstick's and mean |err| <= SAMPLER_MEAN (1.25) x the yardstick's,
    each plus SAMPLER_FLOOR (1e-7) x mean |ref|.  Figures: 'max_ratio' / 'mean_ratio' to the yardstick; 'frame_fig' is each
    frame's max |err| over the launch's allowance."""
    N = delta.shape[0] if delta is not None else theta.shape[0]
    fr = _frames(N, frames)
    rows = []
    for n, ref, yard in grid_sample3d_frames(vol, delta, theta, padding_mode, in_layout, vol_index, fr):
        rows.append(_yardstick_row(_ncdhw(out[n], out_layout), ref, yard, n))
        del ref, yard
    return _yardstick_fig(rows, fr, "grid_sample3d")


# ---- conv2d_generic ------------------------------------------------------------------------------------------------------
GENERIC_KC = 32                     # the K chunk of conv2d_generic_kernel (csrc/conv_generic.hip, GKC)


def unpack_generic(wt, cout, cin, kh, kw):
    """the weight [Cout, Cin, kh, kw] back from the packed wt [K][CoutP] of pack.pack_generic: a transpose and a slice"""
    if wt.dim() != 2 or wt.shape[0] != cin * kh * kw or wt.shape[1] < cout:
        raise ValueError(f"packed weight {tuple(wt.shape)} does not hold a [{cout}, {cin}, {kh}, {kw}] weight")
    return wt[:, :cout].t().reshape(cout, cin, kh, kw)


def generic_splits_run(K, splits):
    """the K split count emo_conv2d_generic_f32 really runs for a request: clamped to the chunk count, then without the empty
    splits that rounding the chunks per split up leaves behind (144 chunks, 32 asked: 5 per split, 29 splits)"""
    chunks = -(-int(K) // GENERIC_KC)
    per = -(-chunks // min(max(int(splits), 1), chunks))
    return -(-chunks // per)


def conv2d_generic_frames(x, wt, cout, kh, kw, stride, pad, bias=None, scale=None, shift=None, relu_in=False, frames=None):
    """yields (n, ref [Cout, Ho, Wo], A [Cout, Ho, Wo]) in fp64 per sample of ops.conv2d_generic: x' = relu?(x scale + shift)
    (the ReLU belongs to the affine: include/emo_hip.h applies it 'when scale/shift are given'), F.unfold of x' with the stride
    and the zero padding, a matmul with the unpacked weight, the bias; A = sum |w| |x'| + |bias| from the same unfold of |x'|"""
    N, Cin, H, W = x.shape
    w = _f64(unpack_generic(wt, cout, Cin, kh, kw)).reshape(cout, -1)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    b = None if bias is None else _f64(bias).reshape(cout, 1)
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift come together")
    for n in _frames(N, frames):
        v = _f64(x[n])
        if scale is not None:
            v = v * _f64(scale.reshape(N, Cin)[n]).view(Cin, 1, 1) + _f64(shift.reshape(N, Cin)[n]).view(Cin, 1, 1)
            if relu_in:
                v = v.clamp_min(0.0)
        cols = F.unfold(v[None], (kh, kw), padding=pad, stride=stride)[0]             # [K, Ho Wo]
        assert cols.dtype == torch.float64
        ref, mag = w @ cols, w.abs() @ cols.abs()
        if b is not None:
            ref, mag = ref + b, mag + b.abs()
        yield n, ref.reshape(cout, Ho, Wo), mag.reshape(cout, Ho, Wo)


def conv2d_generic_fp64(x, wt, cout, kh, kw, stride, pad, bias=None, scale=None, shift=None, relu_in=False):
    return torch.stack([r for _, r, _ in conv2d_generic_frames(x, wt, cout, kh, kw, stride, pad, bias, scale, shift, relu_in)])


def check_conv2d_generic(out, x, wt, cout, kh, kw, stride, pad, bias=None, scale=None, shift=None, relu_in=False, splits=1,
                         frames=None):
    """Every output of the kernel is a sum of K = Cin kh kw products and a bias that passes n = K + splits + 2 roundings at
    most: one for the folded affine (x' = fl(fma(x, scale, shift)) = x'(1 + d); ReLU and the zero padding are exact), the K-term
    fp32 accumulation of the MFMA pipe in whatever order it takes the terms (at most one rounding per term on any path from a
    product to the sum), splits - 1 additions of the fixed-order reduction, and the bias (two are room).  With
    A = sum |w| |x'| + |bias| of the output's OWN terms, the classical bound of a rounded sum gives, per output,
        |out - ref| <= gamma_n A + TINY,      gamma_n = n u / (1 - n u).
    `splits` is the count asked of the launcher; the count that enters n is the one the launcher really ran (generic_splits_run:
    the request clamped to the chunk count, empty splits dropped).  The floor stays TINY: by the MI355X programming guide the
    C / D operands of an MFMA never flush and its fp32 A / B operands follow the kernel's denormal mode, which hipcc's default
    keeps at 'preserve', so an underflowing result costs what one rounding to a subnormal costs.
    At K = 4608 gamma_n A is about one average term, so every frame is ALSO held to max |err| <= FP32_FRAME x max |ref of that
    frame| (conv_reference.FP32_FRAME, the suite's bound of an fp32-result convolution).
    Figures besides _bounded_fig's: 'frame_rel' (each frame's max |err| / max |ref|), 'rms_rel' (rms err / rms ref of the
    launch; reported, not asserted), 'splits_run'."""
    N, Cin = x.shape[:2]
    K = Cin * kh * kw
    run = generic_splits_run(K, splits)
    n_round = K + run + 2
    gamma = n_round * U / (1.0 - n_round * U)
    fr = _frames(N, frames)
    what = f"conv2d_generic {kh}x{kw}/{stride} K={K} splits={run}"
    if tuple(out.shape[:2]) != (N, cout):
        raise ValueError(f"output {tuple(out.shape)} of a launch with N = {N}, Cout = {cout}")
    rows = []
    for n, ref, mag in conv2d_generic_frames(x, wt, cout, kh, kw, stride, pad, bias, scale, shift, relu_in, fr):
        e = torch.nan_to_num(_f64(out[n]) - ref, nan=float("inf"))
        rows.append(torch.cat([_bounded_row(out[n], ref, gamma * mag + TINY), torch.stack([(e * e).sum(), (ref * ref).sum()])]))
        del ref, mag, e
    t = torch.stack(rows).cpu()                       # the launch's one host synchronisation
    fig = _bounded_fig(list(t[:, :4]), fr, what)
    frame_rel = (t[:, 2] / t[:, 3].clamp_min(1e-300)).tolist()
    fig["failures"] += [f"{what}: frame {n}: max err {frame_rel[i]:.3e} of max|ref| > {FP32_FRAME:g}"
                        for i, n in enumerate(fr) if not frame_rel[i] <= FP32_FRAME]
    fig.update(frame_rel=frame_rel, splits_run=run,
               rms_rel=float(torch.sqrt(t[:, 4].sum() / t[:, 5].sum().clamp_min(1e-300))))
    return fig


# ---- maxpool2d -----------------------------------------------------------------------------------------------------------
def _per_channel(v, scale_n, shift_n):
    """v [C, ...] * scale [C] + shift [C] in fp64"""
    b = (-1,) + (1,) * (v.dim() - 1)
    return v * _f64(scale_n).view(b) + _f64(shift_n).view(b)


def maxpool2d_frames(x, k, stride, pad, scale=None, shift=None, relu=False, frames=None):
    """yields (n, fp64 F.max_pool2d(relu?(x[n] scale[n] + shift[n]), k, stride, pad) [C, Ho, Wo]) (padding: -inf)"""
    N, C = x.shape[:2]
    for n in _frames(N, frames):
        v = _f64(x[n])
        if scale is not None:
            v = _per_channel(v, scale.reshape(N, C)[n], shift.reshape(N, C)[n])
        if relu:
            v = v.clamp_min(0.0)
        yield n, F.max_pool2d(v[None], k, stride, pad)[0]


def maxpool2d_fp64(x, k, stride, pad, scale=None, shift=None, relu=False):
    return torch.stack([r for _, r in maxpool2d_frames(x, k, stride, pad, scale, shift, relu)])


def check_maxpool2d(out, x, k, stride, pad, scale=None, shift=None, relu=False, frames=None):
    """The kernel rounds each value of the window once, v = fl(fma(x, scale, shift)), and takes maxima (ReLU is a maximum with
    0).  Rounding is monotone, so max_i fl(v_i) = fl(max_i v_i): the output IS the rounded reference, per output
    |out - ref| <= u |ref| + TINY.  Without a scale nothing is rounded: the output must be bit-equal (bound 0), the -inf
    padding of the border windows included."""
    fr = _frames(x.shape[0], frames)
    rows = []
    for n, ref in maxpool2d_frames(x, k, stride, pad, scale, shift, relu, fr):
        rows.append(_bounded_row(out[n], ref, U * ref.abs() + TINY if scale is not None else torch.zeros_like(ref)))
    return _bounded_fig(rows, fr, f"maxpool2d {k}/{stride}/{pad}")


# ---- affine_add_relu -----------------------------------------------------------------------------------------------------
def affine_add_relu_frames(a, sa=None, ta=None, b=None, sb=None, tb=None, relu=True, frames=None):
    """yields (n, ref, fp64 bound without TINY) per sample of relu?((a sa + ta) + (b sb + tb)); see check_affine_add_relu"""
    N, C = a.shape[:2]
    for n in _frames(N, frames):
        A = _f64(a[n])
        mag = torch.zeros_like(A)
        if sa is not None:
            A = _per_channel(A, sa.reshape(N, C)[n], ta.reshape(N, C)[n])
            mag = mag + A.abs()
        ref = A
        if b is not None:
            B = _f64(b[n])
            if sb is not None:
                B = _per_channel(B, sb.reshape(N, C)[n], tb.reshape(N, C)[n])
                mag = mag + B.abs()
            ref = A + B
            mag = mag + ref.abs()
        yield n, (ref.clamp_min(0.0) if relu else ref), U * (1.0 + U) * mag


def affine_add_relu_fp64(a, sa=None, ta=None, b=None, sb=None, tb=None, relu=True):
    return torch.stack([r for _, r, _ in affine_add_relu_frames(a, sa, ta, b, sb, tb, relu)])


def check_affine_add_relu(out, a, sa=None, ta=None, b=None, sb=None, tb=None, relu=True, frames=None):
    """With A = a sa + ta and B = b sb + tb in fp64 the kernel computes A^ = fl(fma(a, sa, ta)) = A (1 + d1),
    B^ = B (1 + d2) and fl(A^ + B^) = (A^ + B^)(1 + d3), |d| <= u: the error is at most u |A| + u |B| + u |A^ + B^| with
    |A^ + B^| <= |A + B| + u (|A| + |B|), so per output |out - ref| <= u (1 + u) (|A| + |B| + |A + B|) + TINY.  An operand
    without an affine is exact and drops its term (b as the block input: no |B|); without b there is no sum and no |A + B|.
    ReLU is 1-Lipschitz, so the bound carries through it."""
    fr = _frames(a.shape[0], frames)
    rows = [_bounded_row(out[n], ref, bound + TINY) for n, ref, bound in affine_add_relu_frames(a, sa, ta, b, sb, tb, relu, fr)]
    return _bounded_fig(rows, fr, "affine_add_relu" + (" +downsample affine" if sb is not None else ""))


# ---- grid_sample2d -------------------------------------------------------------------------------------------------------
def _lattice_points2d(size, device, dtype):
    """[S, S, 3]: (u, v, 1) of the square identity lattice of ExpressionEmbed, u fastest"""
    lin = lattice(size, device).to(dtype)
    v, u = torch.meshgrid(lin, lin, indexing="ij")
    return torch.stack([u, v, torch.ones_like(u)], dim=-1)


def theta_grid2d_fp64(theta_n, size):
    """theta [2, 3] of one sample -> grid [S, S, 2] fp64 = fp64 product of the fp32 lattice and the fp32 theta"""
    return _lattice_points2d(size, theta_n.device, torch.float64) @ _f64(theta_n).t()


def theta_grid2d_f32(theta_n, size):
    """the same as the reference code builds it: identity_grid.bmm(theta.transpose(1, 2)) in fp32"""
    p = _lattice_points2d(size, theta_n.device, torch.float32)
    return p.reshape(1, -1, 3).bmm(theta_n.float().t().unsqueeze(0)).reshape(size, size, 2)


def grid_sample2d_frames(img, grid=None, theta=None, size=None, frames=None, yardstick=True):
    """yields (n, fp64 reference [C, Ho, Wo], yardstick or None) per sample of ops.grid_sample2d(img, grid= / theta=, size=):
    F.grid_sample in fp64 (bilinear, zeros, align_corners=False), and ATen's fp32 CPU F.grid_sample on the same inputs (grid=:
    the same fp32 grid; theta=: the fp32 bmm grid) as the yardstick"""
    if (grid is None) == (theta is None):
        raise ValueError("exactly one of grid / theta")
    for n in _frames(img.shape[0], frames):
        g64 = _f64(grid[n]) if grid is not None else theta_grid2d_fp64(theta[n], int(size))
        ref = F.grid_sample(_f64(img[n])[None], g64[None], mode="bilinear", padding_mode="zeros", align_corners=False)[0]
        assert ref.dtype == torch.float64
        yard = None
        if yardstick:
            g = grid[n].float().cpu() if grid is not None else theta_grid2d_f32(theta[n].cpu(), int(size))
            yard = F.grid_sample(img[n].float().cpu()[None], g[None], mode="bilinear", padding_mode="zeros", align_corners=False)[0]
            assert yard.dtype == torch.float32 and yard.device.type == "cpu"
        yield n, ref, yard


def grid_sample2d_fp64(img, grid=None, theta=None, size=None):
    return torch.stack([r for _, r, _ in grid_sample2d_frames(img, grid, theta, size, yardstick=False)])


def warp2d_frames(theta, size, frames=None):
    """yields (n, fp64 warp [S, S, 2], fp64 bound without TINY) of the theta form's returned grid.  The kernel computes, per
    coordinate j, p^ = fl(u t[j][0]), q^ = fl(fma(v, t[j][1], p^)) and g^ = fl(fma(1, t[j][2], q^)): three roundings.  On the
    exact intermediates p = u t0, q = v t1 + p, g = t2 + q: |p^ - p| <= u |p|; |q^ - q| <= |p^ - p| + u (|q| + |p^ - p|);
    |g^ - g| <= |q^ - q| + u (|g| + |q^ - q|) <= u (1 + u)^2 (|p| + |q| + |g|)."""
    for n in _frames(theta.shape[0], frames):
        pts = _lattice_points2d(int(size), theta.device, torch.float64)
        t = _f64(theta[n])                                                           # [2, 3]
        p = pts[..., 0:1] * t[:, 0]
        q = pts[..., 1:2] * t[:, 1] + p
        g = t[:, 2] + q
        yield n, g, U * (1.0 + U) ** 2 * (p.abs() + q.abs() + g.abs())


def check_grid_sample2d(out, img, grid=None, theta=None, size=None, warp=None, frames=None):
    """The sampled image is held as check_grid_sample3d holds the 3-D sampler: to ATen's fp32 CPU F.grid_sample on the same
    inputs against the same fp64 reference, max |err| <= SAMPLER_MAX x and mean |err| <= SAMPLER_MEAN x the yardstick's, each
    plus SAMPLER_FLOOR x mean |ref|.  warp = the grid the launch returned (want_grid): with theta= every coordinate is held to
    the fp64 product under the bound of warp2d_frames (+ TINY); with grid= it must be the given grid bit for bit.  Figures
    besides the yardstick's: 'warp_worst' (x bound)."""
    fr = _frames(img.shape[0], frames)
    rows = [_yardstick_row(out[n], ref, yard, n) for n, ref, yard in grid_sample2d_frames(img, grid, theta, size, fr)]
    fig = _yardstick_fig(rows, fr, "grid_sample2d")
    if warp is not None:
        if theta is not None:
            wrows = [_bounded_row(warp[n], g, bound + TINY) for n, g, bound in warp2d_frames(theta, size, fr)]
        else:
            wrows = [_bounded_row(warp[n], _f64(grid[n]), torch.zeros_like(grid[n], dtype=torch.float64)) for n in fr]
        wfig = _bounded_fig(wrows, fr, "grid_sample2d warp")
        fig["failures"] += wfig["failures"]
        fig["warp_worst"] = wfig["worst"]
    return fig


# ---- resize2d ------------------------------------------------------------------------------------------------------------
def _window(v, window):
    """v [C, H, W] -> its window (x0, y0, w, h); None: the whole frame"""
    if window is None:
        return v
    x0, y0, w, h = (int(k) for k in window)
    H, W = v.shape[-2:]
    if not (0 <= x0 and 0 <= y0 and w > 0 and h > 0 and x0 + w <= W and y0 + h <= H):
        raise ValueError(f"window {tuple(window)} is not inside the {W}x{H} frame")
    return v[:, y0:y0 + h, x0:x0 + w]


def resize2d_frames(x, size, mode="bilinear", window=None, clamp01=False, frames=None, yardstick=True):
    """yields (n, fp64 F.interpolate(window of x[n], size, mode, align_corners=False) [C, Ho, Wo] -- clamped to [0, 1] with
    clamp01 --, ATen's fp32 CPU result of the same or None).  The window is a SLICE: what lies outside it does not exist for the
    interpolation, so a tap that leaves the window is clamped into the window, not into the frame"""
    if mode not in ("bilinear", "bicubic"):
        raise ValueError(f"mode {mode!r}: 'bilinear' or 'bicubic'")
    for n in _frames(x.shape[0], frames):
        v = _window(x[n], window)
        ref = F.interpolate(_f64(v)[None], size=tuple(size), mode=mode, align_corners=False)[0]
        assert ref.dtype == torch.float64
        yard = F.interpolate(v.float().cpu().contiguous()[None], size=tuple(size), mode=mode, align_corners=False)[0] if yardstick else None
        if clamp01:
            ref, yard = ref.clamp(0.0, 1.0), (None if yard is None else yard.clamp(0.0, 1.0))
        yield n, ref, yard


def resize2d_fp64(x, size, mode="bilinear", window=None, clamp01=False):
    return torch.stack([r for _, r, _ in resize2d_frames(x, size, mode, window, clamp01, yardstick=False)])


def check_resize2d(out, x, size, mode="bilinear", window=None, clamp01=False, frames=None):
    """ops.resize2d(x, size, mode, window=, clamp01=) against the fp64 interpolation of the window's slice, held to ATen's fp32 CPU
    kernel on the same slice with the sampler's margins (the same construction as check_grid_sample2d: another valid order of
    the same fp32 operations).  Two things hold exactly, whatever the margins would allow:
      * a window as large as the output is the input itself, bit for bit, in both modes: every source index is an integer, the
        bilinear weights are (1, 0) and the bicubic ones at t = 0 are (0, 1, 0, 0) in fp32 (cubic2(1) = A - 5A + 8A - 4A = 0,
        cubic1(0) = 1, cubic1(1) = (A + 2) - (A + 3) + 1 = 0, cubic2(2) = 0 for A = -0.75, every step exact), so each output is
        one tap times 1 plus zeros (clamp01: that value clamped);
      * with clamp01 no output lies outside [0, 1]: the bicubic overshoot is clipped to exactly 0 or 1.
    Figures besides the yardstick's: 'exact_bad' (outputs that miss one of the two)."""
    fr = _frames(x.shape[0], frames)
    size = tuple(int(s) for s in size)
    what = f"resize2d {mode} -> {size}" + (f" window {tuple(window)}" if window is not None else "") + (" clamp01" if clamp01 else "")
    rows, exact = [], []
    for n, ref, yard in resize2d_frames(x, size, mode, window, clamp01, fr):
        rows.append(_yardstick_row(out[n], ref, yard, n))
        bad = torch.zeros((), dtype=torch.int64, device=out.device)
        if clamp01:
            bad = bad + (~((out[n] >= 0.0) & (out[n] <= 1.0))).sum()
        v = _window(x[n], window)
        if tuple(v.shape[-2:]) == size:
            same = v.float().clamp(0.0, 1.0) if clamp01 else v.float()
            bad = bad + (out[n].contiguous().view(torch.int32) != same.contiguous().view(torch.int32)).sum()
        exact.append(bad)
    fig = _yardstick_fig(rows, fr, what)
    e = torch.stack(exact).cpu().tolist()
    fig["exact_bad"] = int(sum(e))
    fig["failures"] += [f"{what}: frame {n}: {e[i]} outputs outside [0, 1] under clamp01 or not the input's bits at equal size"
                        for i, n in enumerate(fr) if e[i]]
    return fig


# ---- mul_mask / stage2_compose -------------------------------------------------------------------------------------------
def _mask_of(mask, n, hw):
    """mask [N, 1, H, W] (or [N, H, W]) -> sample n as [1, H, W]"""
    return mask[n].reshape((1,) + tuple(hw))


def _bits_fig(rows, fr, what):
    """figures of a launch held to bit equality: rows = the count of differing elements per frame"""
    t = torch.stack(rows).cpu().tolist()
    w = max(range(len(fr)), key=lambda i: t[i])
    bad = [f"{what}: frame {n}: {t[i]} elements differ from the reference's bits" for i, n in enumerate(fr) if t[i]]
    return dict(frames=fr, frame_fig=[float(v) for v in t], unit="differing elements", worst=float(t[w]), worst_frame=fr[w], failures=bad)


def mul_mask_fp64(img, mask):
    """img [N, C, H, W] * mask [N, 1, H, W] in fp64: exact (two 24-bit significands)"""
    return torch.stack([_f64(img[n]) * _f64(_mask_of(mask, n, img.shape[2:])) for n in range(img.shape[0])])


def check_mul_mask(out, img, mask, frames=None):
    """The kernel rounds once: out = fl(img mask).  The fp64 product of two fp32 values is exact, so its rounding to fp32 IS the
    kernel's result: bit equality, sample by sample (signed zeros included); the figure is the count of differing elements."""
    fr = _frames(img.shape[0], frames)
    if tuple(out.shape) != tuple(img.shape):
        raise ValueError(f"output {tuple(out.shape)} of an image {tuple(img.shape)}")
    rows = []
    for n in fr:
        ref = (_f64(img[n]) * _f64(_mask_of(mask, n, img.shape[2:]))).float()
        rows.append((out[n].contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)).sum())
    return _bits_fig(rows, fr, "mul_mask")


def stage2_compose_frames(img, add, mask, face_mask, frames=None):
    """yields (n, r = img + add (mask face_mask) in fp64 BEFORE the clamp [C, H, W], fp64 bound without the floor, |add|) per
    sample; see check_stage2_compose"""
    hw = img.shape[2:]
    for n in _frames(img.shape[0], frames):
        M = _f64(_mask_of(mask, n, hw)) * _f64(_mask_of(face_mask, n, hw))          # exact
        P = _f64(add[n]) * M
        r = _f64(img[n]) + P
        yield n, r, U * (1.0 + U) ** 2 * (2.0 * P.abs() + r.abs()), _f64(add[n]).abs()


def stage2_compose_fp64(img, add, mask, face_mask):
    return torch.stack([r.clamp(0.0, 1.0) for _, r, _, _ in stage2_compose_frames(img, add, mask, face_mask)])


def check_stage2_compose(out, img, add, mask, face_mask, frames=None):
    """The kernel computes m^ = fl(mask face) = M (1 + d1), p^ = fl(add m^) = add M (1 + d1)(1 + d2), v = fl(img + p^) =
    (img + p^)(1 + d3), |d| <= u, then clamps.  With P = add M and r = img + P exact: |p^ - P| <= |P| (2u + u^2) and
    |v - r| <= |p^ - P| (1 + u) + u |r| <= u (1 + u)^2 (2 |P| + |r|).  A compiler that contracts the last two operations into one
    FMA drops d2: fewer roundings, the same bound.  Where m^ or p^ underflows a rounding costs TINY instead (m^'s times |add|):
    + TINY (2 + |add|).  The clamp is 1-Lipschitz, so the bound holds for the clamped values -- and where r lies outside [0, 1]
    by more than the bound the clamp decides the output alone: it must be exactly 0 or 1 (bound 0 there).  No output may lie
    outside [0, 1] at all."""
    fr = _frames(img.shape[0], frames)
    rows, outside = [], []
    for n, r, bound, amag in stage2_compose_frames(img, add, mask, face_mask, fr):
        bound = bound + TINY * (2.0 + amag)
        decided = (r < -bound) | (r > 1.0 + bound)
        rows.append(_bounded_row(out[n], r.clamp(0.0, 1.0), torch.where(decided, torch.zeros_like(bound), bound)))
        outside.append((~((out[n] >= 0.0) & (out[n] <= 1.0))).sum())
    fig = _bounded_fig(rows, fr, "stage2_compose")
    o = torch.stack(outside).cpu().tolist()
    fig["failures"] += [f"stage2_compose: frame {n}: {o[i]} outputs outside [0, 1]" for i, n in enumerate(fr) if o[i]]
    return fig


# ---- pack_rgb8 / unpack_rgb8 ---------------------------------------------------------------------------------------------
def rgb8_edge_image():
    """[1, 3, 4, 193] fp32 on the CPU, the pixels at which a packing can go wrong: k / 255 for every byte k and the fp32 values on
    either side of each; -0.0, -1e-3, 1 + 2^-23 and 1 - 2^-24.  Every channel holds all of them, in another order"""
    k = torch.arange(256, dtype=torch.float32) / 255
    v = torch.cat([k, torch.nextafter(k, torch.tensor(-9.0)), torch.nextafter(k, torch.tensor(9.0)),
                   torch.tensor([-0.0, -1e-3, 1 + 2.0 ** -23, 1 - 2.0 ** -24])])
    assert v.numel() == 4 * 193
    return torch.stack([v, v.flip(0), v.roll(97)]).reshape(1, 3, 4, 193)


def pack_rgb8_ref(img):
    """[N, 3, H, W] fp32 -> [N, H, W, 3] uint8: clamp(0, 1) * 255 in fp64 (exact: 24 + 8 bits), rounded to fp32 as the kernel's one
    product is, truncated -- torch's img.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1), the reference wrapper's ToPILImage.
    Finite inputs only (the byte of a NaN is undefined)"""
    return torch.stack([(_f64(img[n]).clamp(0.0, 1.0) * 255.0).float().to(torch.uint8).permute(1, 2, 0) for n in range(img.shape[0])])


def check_pack_rgb8(out, img, frames=None):
    """byte equality with pack_rgb8_ref, sample by sample: one rounded product and a truncation, nothing to bound"""
    fr = _frames(img.shape[0], frames)
    if tuple(out.shape) != (img.shape[0],) + tuple(img.shape[2:]) + (3,) or out.dtype != torch.uint8:
        raise ValueError(f"output {tuple(out.shape)} {out.dtype} is not the HWC byte form of {tuple(img.shape)}")
    rows = [(out[n] != pack_rgb8_ref(img[n:n + 1])[0]).sum() for n in fr]
    return _bits_fig(rows, fr, "pack_rgb8")


def unpack_rgb8_fp64(frames_u8):
    """[N, H, W, 3] uint8 -> [N, 3, H, W] fp64 = byte / 255"""
    return _f64(frames_u8).permute(0, 3, 1, 2) / 255.0


def check_unpack_rgb8(out, frames_u8, frames=None):
    """The kernel divides in fp32, correctly rounded: out = fl(byte / 255) -- torch's byte.float() / 255.  The fp64 quotient
    rounded to fp32 is the same number for each of the 256 bytes (no quotient lies close enough to the middle of two fp32
    values for the first rounding to move it across; tests/test_ops_reference.py compares all 256): bit equality."""
    fr = _frames(frames_u8.shape[0], frames)
    if tuple(out.shape) != (frames_u8.shape[0], 3) + tuple(frames_u8.shape[1:3]) or out.dtype != torch.float32:
        raise ValueError(f"output {tuple(out.shape)} {out.dtype} is not the CHW float form of {tuple(frames_u8.shape)}")
    rows = []
    for n in fr:
        ref = (_f64(frames_u8[n]).permute(2, 0, 1) / 255.0).float()
        rows.append((out[n].contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)).sum())
    return _bits_fig(rows, fr, "unpack_rgb8")


# ---- pose_theta ----------------------------------------------------------------------------------------------------------
def _restate():
    oracle = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    if oracle not in sys.path:
        sys.path.insert(0, oracle)
    import restate
    return restate


def pose_theta_fp64(scale, rotation, translation):
    """oracle/restate.get_transform_matrix (S @ R @ T of utils/point_transforms.py) in fp64 on the fp32 inputs, on the CPU"""
    return _restate().get_transform_matrix(_f64(scale).cpu(), _f64(rotation).cpu(), _f64(translation).cpu())


def check_pose_theta(out, scale, rotation, translation, frames=None):
    """ops.pose_theta against pose_theta_fp64, held to the same function in fp32 on the CPU (torch's sin / cos and two fp32
    matrix products) with the sampler's margins: the device sinf / cosf carry no stated accuracy to derive an ulp bound from,
    so the yardstick is another fp32 evaluation of the same formula.  One row of figures per matrix."""
    fr = _frames(scale.shape[0], frames)
    ref = pose_theta_fp64(scale, rotation, translation)
    yard = _restate().get_transform_matrix(scale.float().cpu(), rotation.float().cpu(), translation.float().cpu())
    assert ref.dtype == torch.float64 and yard.dtype == torch.float32
    got = out.cpu()
    return _yardstick_fig([_yardstick_row(got[n], ref[n], yard[n], n) for n in fr], fr, "pose_theta", yardstick="torch fp32")
