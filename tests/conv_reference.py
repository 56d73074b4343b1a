"""fp64 reference and error checker for single launches of ops.conv_igemm / ops.conv_head (a helper module, not a test file).

reference() computes in fp64 exactly what ops.conv_igemm computes -- input affine + ReLU prologue, nearest x2 upsample, conv
(padding k // 2 per dimension), residual (nearest-upsampled with res_ups), activation -- from plain tensors, on whatever
device the input lives on.  The convolution is a sum over kernel taps of fp64 matrix products ([Cout, Cin] x [Cin, positions])
per sample and per block of output rows: no im2col buffer, bounded memory, the same code on the CPU and on the GPU, and no
dependence on which backend torch picks for an fp64 F.conv2d / F.conv3d.

check_launch() compares a kernel's output with that reference frame by frame and applies the bounds the suite states for
each arithmetic (the constants below); check_tile_stats() holds the GroupNorm tile statistics a launch returned to the affine of a
direct reduction of the output.
"""
import itertools
import math

import torch
import torch.nn.functional as F

# window of one tap in fp64 elements (256 MB): output rows per block are chosen so that no copy exceeds it
CHUNK_ELEMS = 1 << 25

# every frame of every launch of an fp32-result arithmetic: max |err| <= FP32_FRAME * max |ref of that frame| (the bound of
# tests/test_kernels_gpu.py against an fp32 CPU convolution)
FP32_FRAME = 2e-5
FP32_PLANS = ("f32", "bf16x3", "f16x2", "stream")
# split kernels against the exact-fp32 MFMA kernel on the same inputs (test_conv_bf16x3_is_as_close_to_fp64_as_the_fp32_kernel):
# mean error <= k * fp32 kernel's + 1e-8 * mean |ref|, max error <= 2 * fp32 kernel's + 1e-7 * mean |ref|
SPLIT_MEAN = {"f16x2": 1.25, "bf16x3": 1.1}
SPLIT_MAX = 2.0
# fp16 operands, fp32 accumulation (test_conv_fp16_operands): every frame max <= 3e-3 * max |ref of that frame|, every launch
# mean <= 3e-4 * max |ref|
F16_PLANS = ("f16", "f16w8")
F16_FRAME = 3e-3
F16_MEAN = 3e-4
# tile statistics: affine from the tiles vs affine of a direct reduction (2e-6 relative on the scale, absolute on the shift)
STATS_TOL = 2e-6


def _act(v, act):
    if act == "none":
        return v
    return {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}[act](v)


def _up2(v):
    """nearest x2 on the last two dimensions (H, W; the depth of a 5-D tensor is not upsampled)"""
    return v.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def _conv_taps(xp, w):
    """xp [Cin, *padded spatial] fp64, w [Cout, Cin, *k] fp64 -> [Cout, *out spatial] (valid convolution)"""
    cout, cin = w.shape[:2]
    ks = tuple(w.shape[2:])
    osp = tuple(xp.shape[1 + i] - ks[i] + 1 for i in range(len(ks)))
    wt = w.permute(*range(2, w.dim()), 0, 1).contiguous()           # [*k, Cout, Cin]
    out = torch.empty((cout,) + osp, dtype=torch.float64, device=xp.device)
    inner = math.prod(osp[1:])
    rows = max(1, CHUNK_ELEMS // max(1, cin * inner))
    for r0 in range(0, osp[0], rows):
        r1 = min(osp[0], r0 + rows)
        acc = torch.zeros((cout, (r1 - r0) * inner), dtype=torch.float64, device=xp.device)
        for tap in itertools.product(*(range(k) for k in ks)):
            win = xp[(slice(None), slice(r0 + tap[0], r1 + tap[0]))
                     + tuple(slice(t, t + o) for t, o in zip(tap[1:], osp[1:]))]
            acc.addmm_(wt[tap], win.reshape(cin, -1))
        out[:, r0:r1] = acc.view((cout, r1 - r0) + osp[1:])
    return out


def _prepare(x, weight, bias, res, ups, res_ups):
    """-> (fp64 weight on x's device, fp64 bias or None, residual viewed [N, Cout, *spatial of res] or None)"""
    w = weight.to(device=x.device, dtype=torch.float64)
    if w.dim() == 4 and x.dim() == 5:
        w = w.unsqueeze(2)
    elif w.dim() == 5 and x.dim() == 4:
        if w.shape[2] != 1:
            raise ValueError("3-D kernel on a 4-D input")
        w = w[:, :, 0]
    if w.shape[1] != x.shape[1]:
        raise ValueError(f"weight has {w.shape[1]} input channels, x {x.shape[1]}")
    b = None if bias is None else bias.to(device=x.device, dtype=torch.float64)
    r = None
    if res is not None:
        sp = list(x.shape[2:])
        if ups:
            sp[-2:] = [2 * sp[-2], 2 * sp[-1]]
        if res_ups:
            sp[-2:] = [sp[-2] // 2, sp[-1] // 2]
        r = res.reshape([x.shape[0], w.shape[0]] + sp)
    return w, b, r


def reference_frames(x, weight, bias=None, scale=None, shift=None, relu_in=False, ups=False, res=None, res_ups=False, act="none",
                     frames=None):
    """yields (n, fp64 [Cout, *out spatial]) for every sample n of `frames` (default: all) -- the fp64 value of
    ops.conv_igemm(x, layer with `weight` / `bias`, scale, shift, relu_in=, ups=, res=, res_ups=, act=) for that sample.
    Computed on x's device, one sample at a time."""
    w, b, r = _prepare(x, weight, bias, res, ups, res_ups)
    nsp = x.dim() - 2
    pad = []
    for k in reversed(w.shape[2:]):
        pad += [k // 2, k // 2]
    bshape = (-1,) + (1,) * nsp
    for n in (range(x.shape[0]) if frames is None else frames):
        v = x[n].to(torch.float64)
        if scale is not None:
            v = v * scale[n].to(torch.float64).view(bshape)
        if shift is not None:
            v = v + shift[n].to(torch.float64).view(bshape)
        if relu_in:
            v = torch.relu(v)
        if ups:
            v = _up2(v)
        o = _conv_taps(F.pad(v, pad), w)
        del v
        if b is not None:
            o += b.view(bshape)
        if r is not None:
            rn = r[n].to(torch.float64)
            o += _up2(rn) if res_ups else rn
        o = _act(o, act)
        assert o.dtype == torch.float64, o.dtype          # no fp32 reference slips in
        yield n, o


def reference(x, weight, bias=None, scale=None, shift=None, relu_in=False, ups=False, res=None, res_ups=False, act="none"):
    """the whole fp64 output [N, Cout, *out spatial] (small shapes; the launch checker works frame by frame)"""
    out = torch.stack([o for _, o in reference_frames(x, weight, bias, scale, shift, relu_in, ups, res, res_ups, act)])
    assert out.dtype == torch.float64
    return out


def launch_errors(out, frames, yardstick=None):
    """out [N, Cout, ...] (the kernel's), frames: iterable of (n, fp64 reference of sample n); yardstick: the fp32 MFMA kernel's
    output on the same inputs, or None.  -> dict of per-frame and per-launch error figures (absolute; see verdict())."""
    rows = []
    idx = []
    for n, ref in frames:
        assert ref.dtype == torch.float64, ref.dtype
        got = out[n].to(torch.float64)
        if got.shape != ref.shape:
            raise ValueError(f"frame {n}: output {tuple(got.shape)} vs reference {tuple(ref.shape)}")
        e = (got - ref).abs()
        a = ref.abs()
        row = [e.max(), a.max(), e.sum(), a.sum(), torch.tensor(float(ref.numel()), dtype=torch.float64, device=ref.device)]
        if yardstick is not None:
            ey = (yardstick[n].to(torch.float64) - ref).abs()
            row += [ey.max(), ey.sum()]
            del ey
        rows.append(torch.stack(row))
        idx.append(n)
        del got, e, a, ref
    t = torch.stack(rows).cpu()                   # one host synchronisation per launch
    count = float(t[:, 4].sum())
    frame_rel = (t[:, 0] / t[:, 1].clamp_min(1e-300)).tolist()
    fig = dict(frames=idx, frame_rel_max=frame_rel, max_err=float(t[:, 0].max()), ref_max=float(t[:, 1].max()),
               mean_err=float(t[:, 2].sum()) / count, scale=float(t[:, 3].sum()) / count)
    if yardstick is not None:
        fig.update(f32_max_err=float(t[:, 5].max()), f32_mean_err=float(t[:, 6].sum()) / count)
    return fig


def verdict(fig, plan_precision):
    """the bounds of the launch's arithmetic (its plan precision: 'f32' | 'bf16x3' | 'f16x2' | 'stream' | 'f16' | 'f16w8')
    -> list of violations (empty: the launch passes)"""
    bad = []
    scale = max(fig["scale"], 1e-300)
    if plan_precision in FP32_PLANS or plan_precision in F16_PLANS:
        tol = FP32_FRAME if plan_precision in FP32_PLANS else F16_FRAME
        for n, r in zip(fig["frames"], fig["frame_rel_max"]):
            if not r <= tol:
                bad.append(f"frame {n}: max err {r:.3e} of max|ref| > {tol:g}")
    else:
        bad.append(f"no bound for plan precision {plan_precision!r}")
    if plan_precision in SPLIT_MEAN:
        if "f32_mean_err" not in fig:
            bad.append("split launch without the fp32 kernel's error as its yardstick")
        else:
            k = SPLIT_MEAN[plan_precision]
            if not fig["mean_err"] <= k * fig["f32_mean_err"] + 1e-8 * scale:
                bad.append(f"mean err {fig['mean_err']:.3e} > {k} x fp32 kernel's {fig['f32_mean_err']:.3e} + 1e-8 x {scale:.3e}")
            if not fig["max_err"] <= SPLIT_MAX * fig["f32_max_err"] + 1e-7 * scale:
                bad.append(f"max err {fig['max_err']:.3e} > {SPLIT_MAX} x fp32 kernel's {fig['f32_max_err']:.3e} + 1e-7 x {scale:.3e}")
    if plan_precision in F16_PLANS and not fig["mean_err"] <= F16_MEAN * fig["ref_max"]:
        bad.append(f"mean err {fig['mean_err']:.3e} > {F16_MEAN:g} x max|ref| {fig['ref_max']:.3e}")
    return bad


def groupnorm_affine_fp64(out, stats=None, groups=32, eps=1e-5):
    """(scale, shift) [N, C] of GroupNorm(groups) without affine parameters, in fp64 and plain torch: from a direct reduction of
    `out`, or, with `stats` (ops.TileStats: stats [N, T, C, 2] = (mean, centred sum of squares) of `cnt` values per tile and
    channel), combined from the tiles alone.  The CPU stand-in of ops.groupnorm_affine for the checker's own tests."""
    N, C = out.shape[:2]
    cg = C // groups
    if stats is None:
        v = out.to(torch.float64).reshape(N, groups, -1)
        mean, var = v.mean(-1), v.var(-1, unbiased=False)
    else:
        st = stats.stats.to(torch.float64)
        T = st.shape[1]
        st = st.view(N, T, groups, cg, 2)
        m, m2 = st[..., 0], st[..., 1]
        mean = m.mean(dim=(1, 3))
        var = (m2.sum(dim=(1, 3)) + stats.cnt * ((m - mean[:, None, :, None]) ** 2).sum(dim=(1, 3))) / (T * cg * stats.cnt)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = rstd.repeat_interleave(cg, dim=1)
    shift = (-mean * rstd).repeat_interleave(cg, dim=1)
    return scale, shift


def _ops_affine(out, stats, groups):
    from emoportraits_amd import ops
    return ops.groupnorm_affine(out, stats=stats, groups=groups)


def check_tile_stats(out, stats, groups, affine=None):
    """the tile statistics a launch returned against a direct reduction of its own output, through `affine(out, stats, groups)`
    (default ops.groupnorm_affine) -> (figures, violations)"""
    affine = affine or _ops_affine
    s1, h1 = affine(out, stats, groups)
    s0, h0 = affine(out, None, groups)
    ds = ((s1.double() - s0.double()).abs().max() / s0.double().abs().max().clamp_min(1e-300)).item()
    dh = (h1.double() - h0.double()).abs().max().item()
    fig = dict(stats_scale_rel=ds, stats_shift_abs=dh)
    bad = []
    if not ds <= STATS_TOL:
        bad.append(f"tile statistics: scale differs by {ds:.3e} of max > {STATS_TOL:g}")
    if not dh <= STATS_TOL:
        bad.append(f"tile statistics: shift differs by {dh:.3e} > {STATS_TOL:g}")
    return fig, bad


def check_launch(out, x, weight, bias=None, scale=None, shift=None, relu_in=False, ups=False, res=None, res_ups=False, act="none",
                 precision="f32", yardstick=None, stats=None, groups=None, affine=None):
    """one launch against the fp64 reference, every frame.  precision: the plan precision the launch ran (bounds: verdict());
    yardstick: the fp32 MFMA kernel's output on the same inputs (required for the split kernels); stats / groups: the
    TileStats the launch returned and the group count of the norm that consumes them.
    -> figures (dict; 'failures': list of violations, empty when the launch passes)"""
    fig = launch_errors(out, reference_frames(x, weight, bias, scale, shift, relu_in, ups, res, res_ups, act), yardstick)
    bad = verdict(fig, precision)
    if stats is not None:
        sfig, sbad = check_tile_stats(out, stats, groups, affine)
        fig.update(sfig)
        bad += sbad
    fig["failures"] = bad
    return fig
