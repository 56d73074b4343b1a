"""The fp64 references and launch checkers of tests/ops_reference.py, on the CPU: each reference equals the plain fp32 torch
composition of its operation (the embedders' references: torch's own fp64 evaluation, to fp64 rounding), each checker passes an output that carries only fp32 rounding noise, and each checker reports
the kernel faults it is there to catch (planted in that output)."""
import pytest
import torch
import torch.nn.functional as F

import ops_reference as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(ref64, f32, tol=2e-6):
    assert ref64.dtype == torch.float64 and f32.dtype == torch.float32
    assert tuple(ref64.shape) == tuple(f32.shape)
    return (ref64 - f32.double()).abs().max().item() <= tol * max(1.0, ref64.abs().max().item())


def _same64(ref64, own64, tol=1e-14):
    """a reference against torch's own fp64 evaluation of the operation: the same numbers up to fp64 rounding"""
    assert ref64.dtype == own64.dtype == torch.float64 and tuple(ref64.shape) == tuple(own64.shape)
    return (ref64 - own64).abs().max().item() <= tol * max(1.0, own64.abs().max().item())


def _clean(fig):
    assert fig["failures"] == [], fig["failures"]
    assert len(fig["frames"]) == len(fig["frame_fig"])
    return fig


def _caught(fig):
    assert fig["failures"], f"the planted fault went unreported: {fig}"
    return fig


# ---- volume_to_channels_last ---------------------------------------------------------------------------------------------
def test_channels_last():
    vol = torch.randn(2, 6, 3, 4, 5, generator=_g(0))
    out = vol.permute(0, 2, 3, 4, 1).contiguous()
    assert torch.equal(R.channels_last_fp64(vol), out.double()) and R.channels_last_fp64(vol).dtype == torch.float64
    assert _clean(R.check_channels_last(out, vol))["frames"] == [0, 1]
    bad = out.clone()
    bad[1, 2, 3, 4, 0] = torch.nextafter(bad[1, 2, 3, 4, 0], torch.tensor(9.0))          # one ulp in one element
    assert _caught(R.check_channels_last(bad, vol))["worst_frame"] == 1
    swapped = vol.permute(0, 2, 4, 3, 1).reshape(out.shape)                               # H and W exchanged
    _caught(R.check_channels_last(swapped, vol))


# ---- add / add_rows_indexed ----------------------------------------------------------------------------------------------
def test_add_reference_and_wrong_period():
    g = _g(1)
    a, b = torch.randn(3, 8, 5, generator=g), torch.randn(8, 5, generator=g)
    out = (a + b) * 0.5
    assert _close(R.add_fp64(a, b, 0.5), out, 1.2e-7)
    _clean(R.check_add(out, a, b, 0.5))
    full = torch.randn(3, 8, 5, generator=g)
    _clean(R.check_add((a + full) * 0.3, a, full, 0.3))                                   # period = the whole tensor
    # the wrong period: b restarted every 32 elements instead of every 40
    wrong = ((a.reshape(-1) + b.reshape(-1)[torch.arange(a.numel()) % 32]) * 0.5).reshape(a.shape)
    _caught(R.check_add(wrong, a, b, 0.5))
    # one rounding too many is outside the bound's reach only if it is large: a single-ulp error on one element passes,
    # a 4-ulp one does not
    off = out.clone()
    i = out.abs().reshape(-1).argmax()
    off.view(-1)[i] = out.view(-1)[i] * (1 + 4 * 2.0 ** -23)
    _caught(R.check_add(off, a, b, 0.5))


def test_add_rows_indexed_reference_and_row_of_index_0():
    g = _g(2)
    a, table = torch.randn(5, 37, 1, generator=g), torch.randn(3, 37, 1, generator=g)
    index = torch.tensor([2, 0, 7, 1, -1], dtype=torch.int32)                             # 7 and -1: outside the bank
    ok = torch.tensor([1, 1, 0, 1, 0.0]).view(5, 1, 1)
    out = (a + table[index.long().clamp(0, 2)]) * 0.5 * ok
    ref = R.add_rows_indexed_fp64(a, table, index, 0.5)
    assert _close(ref, out, 1.2e-7) and ref[2].abs().max() == 0 and ref[4].abs().max() == 0
    _clean(R.check_add_rows_indexed(out, a, table, index, 0.5))
    every_b_reads_index_0 = (a + table[2]) * 0.5 * ok
    fig = _caught(R.check_add_rows_indexed(every_b_reads_index_0, a, table, index, 0.5))
    assert fig["frame_fig"][0] <= 1 and fig["frame_fig"][1] > 1 and fig["frame_fig"][3] > 1
    not_zeroed = (a + table[index.long().clamp(0, 2)]) * 0.5
    _caught(R.check_add_rows_indexed(not_zeroed, a, table, index, 0.5))


# ---- avgpool -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [(2, 1, 1), (1, 2, 2), (2, 2, 2), (2, 2), (3, 2, 1)])
def test_avgpool_reference_equals_torch(kernel):
    g = _g(3)
    x = torch.randn(2, 5, 6, 8, 12, generator=g) if len(kernel) == 3 else torch.randn(2, 5, 8, 12, generator=g)
    out = (F.avg_pool3d if len(kernel) == 3 else F.avg_pool2d)(x, kernel)
    assert _close(R.avgpool_fp64(x, kernel), out, 2.4e-7)
    _clean(R.check_avgpool(out, x, kernel))


def test_avgpool_window_one_row_off_beyond_a_threshold():
    """the second trip of a grid-stride loop reading one row off: only outputs past an index threshold are wrong (the
    threshold stands in for the 8192 * 1024 outputs of the first trip), and only by the difference of two neighbouring rows"""
    g = _g(4)
    # a tensor whose magnitude varies over five decades between channels: the fault sits in the SMALL channels, where a bound
    # taken from the tensor's maximum would hide it
    x = torch.randn(2, 6, 4, 8, 8, generator=g) * torch.tensor([1e3, 1.0, 1e-2, 1e3, 1.0, 1e-2]).view(1, 6, 1, 1, 1)
    kernel = (2, 1, 1)
    out = F.avg_pool3d(x, kernel)
    shifted = F.avg_pool3d(torch.roll(x, -1, dims=3), kernel)                             # every window one row further down
    i = torch.arange(out.numel()).reshape(out.shape)
    threshold = out[0].numel() + 2 * out[0, 0].numel()                                    # sample 1 from its channel 2 (1e-2) on
    bad = torch.where((i >= threshold) & (i < threshold + out[0, 0].numel()), shifted, out)
    assert (bad - out).abs().max().item() < 1e-4 * out.abs().max().item()                 # under any whole-tensor bound
    fig = _caught(R.check_avgpool(bad, x, kernel))
    assert fig["frame_fig"][0] <= 1 < fig["frame_fig"][1]


# ---- upsample_trilinear --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factors", [(2, 2, 2), (1, 2, 2), (2, 1, 1), (1, 1, 2)])
def test_upsample_reference_equals_torch(factors):
    x = torch.randn(2, 3, 4, 5, 6, generator=_g(5))
    out = F.interpolate(x, scale_factor=tuple(float(f) for f in factors), mode="trilinear", align_corners=False)
    assert _close(R.upsample_trilinear_fp64(x, factors), out, 2.4e-7)
    assert _clean(R.check_upsample_trilinear(out, x, factors))["worst"] <= 1


def _upsample_case():
    g = _g(6)
    x = torch.randn(2, 4, 4, 6, 8, generator=g) * torch.tensor([1e2, 1.0, 1e-2, 1.0]).view(1, 4, 1, 1, 1)
    return x, F.interpolate(x, scale_factor=(2.0, 2.0, 2.0), mode="trilinear", align_corners=False)


def test_upsample_first_column_faults():
    """The first output column of a row has the source index clamped to 0: taps (0, 1) with weights (1, 0).  Taking taps (0, 0)
    with the same weights is the SAME value on finite data (1 * x[0] + 0 * x[0]), so it is no fault a value check can see;
    what a kernel that gets this column wrong produces is one of the two forms planted here."""
    x, out = _upsample_case()
    same = out.clone()
    same[..., 0] = F.interpolate(x[..., :1].expand(-1, -1, -1, -1, 2), scale_factor=(2.0, 2.0, 1.0), mode="trilinear")[..., 0]
    assert torch.equal(same, out)                                                         # taps (0, 0), weights (1, 0)
    col = lambda w0, w1: F.interpolate(w0 * x[..., 0:1] + w1 * x[..., 1:2], scale_factor=(2.0, 2.0, 1.0), mode="trilinear")[..., 0]
    interior = out.clone()
    interior[..., 0] = col(0.25, 0.75)              # taps (0, 1) with the weights an interior column 4m has
    _caught(R.check_upsample_trilinear(interior, x, (2, 2, 2)))
    unclamped = out.clone()
    unclamped[..., 0] = col(1.25, -0.25)            # the source index -0.25 not clamped at 0
    _caught(R.check_upsample_trilinear(unclamped, x, (2, 2, 2)))
    # in the small channel alone (1e-4 of the tensor's maximum): the bound is per output
    small = out.clone()
    small[:, 2, :, :, 0] = col(0.25, 0.75)[:, 2]
    assert (small - out).abs().max().item() < 1e-3 * out.abs().max().item()
    _caught(R.check_upsample_trilinear(small, x, (2, 2, 2)))


def test_upsample_last_depth_pair_duplicated():
    x, out = _upsample_case()
    bad = out.clone()
    bad[:, :, -1] = bad[:, :, -2]
    fig = _caught(R.check_upsample_trilinear(bad, x, (2, 2, 2)))
    assert all(f > 1 for f in fig["frame_fig"])


# ---- groupnorm_affine ----------------------------------------------------------------------------------------------------
def _gn_case(ada):
    g = _g(7)
    N, C, G = 3, 16, 4
    x = torch.randn(N, C, 4, 6, 8, generator=g) * 2 + 0.7
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    wide = torch.randn(N, 2, 3 * C, generator=g)                                         # column views with a row stride
    ag, ab = (wide[:, 0, C:2 * C], wide[:, 1, C:2 * C]) if ada else (None, None)
    return x, gamma, beta, ag, ab, G


@pytest.mark.parametrize("ada", [False, True])
def test_groupnorm_reference_equals_torch(ada):
    x, gamma, beta, ag, ab, G = _gn_case(ada)
    sc, sh = R.groupnorm_affine_fp64(x, gamma, beta, ag, ab, groups=G)
    assert sc.dtype == sh.dtype == torch.float64 and tuple(sc.shape) == (3, 16)
    y = F.group_norm(x, G, gamma, beta)
    b = (3, 16, 1, 1, 1)
    if ada:
        y = y * ag.reshape(b) + ab.reshape(b)                                             # the static affine first, then the adaptive
    got = x.double() * sc.view(b) + sh.view(b)
    assert (got - y.double()).abs().max().item() <= 2e-5 * y.abs().max().item()
    _clean(R.check_groupnorm_affine(sc.float(), sh.float(), x, gamma, beta, ag, ab, groups=G))
    sc0, sh0 = R.groupnorm_affine_fp64(x, groups=G)
    assert (x.double() * sc0.view(b) + sh0.view(b) - F.group_norm(x, G).double()).abs().max().item() <= 2e-5


def _affine_from_sums(x, gamma, beta, ag, ab, G, drop=None, ada_rows=None, quirk=True, slices=64):
    """what the kernels compute, from `slices` partial (sum, sum of squares) per (sample, group), with the faults to plant"""
    N, C = x.shape[:2]
    cg = C // G
    v = x.double().reshape(N, G, slices, -1)
    s, q = v.sum(-1), (v * v).sum(-1)
    if drop is not None:
        s[drop], q[drop] = 0.0, 0.0
    L = v.shape[2] * v.shape[3]
    mean = s.sum(-1) / L
    var = q.sum(-1) / L - mean * mean
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(1e-5)))
    sc = rstd.repeat_interleave(cg, 1) * gamma.double()
    mc = mean.repeat_interleave(cg, 1)
    if ag is None:
        return (sc, beta.double() - mc * sc)
    rows = list(range(N)) if ada_rows is None else ada_rows
    a, b = ag.double()[rows], ab.double()[rows]
    if quirk:
        return sc * a, (beta.double() - mc * sc) * a + b
    return sc * a, (-mc * sc) * a + b                                                     # beta once: only inside ab = beta + d_beta


def test_groupnorm_checker_reports_the_planted_faults():
    x, gamma, beta, ag, ab, G = _gn_case(True)
    x = x.reshape(3, 16, -1)[..., :192 // 64 * 64].reshape(3, 16, 4, 6, 8)
    f32 = lambda p: (p[0].float(), p[1].float())
    chk = lambda p, *ada: R.check_groupnorm_affine(*f32(p), x, gamma, beta, *ada, groups=G)
    _clean(chk(_affine_from_sums(x, gamma, beta, None, None, G)))
    _clean(chk(_affine_from_sums(x, gamma, beta, ag, ab, G), ag, ab))
    # one of the 64 slices of one group of one sample dropped from the sums
    fig = _caught(chk(_affine_from_sums(x, gamma, beta, None, None, G, drop=(1, 2, 63))))
    assert fig["frame_fig"][0] <= 1 and fig["frame_fig"][2] <= 1 < fig["frame_fig"][1]
    # the adaptive weights of the neighbouring sample's row
    _caught(chk(_affine_from_sums(x, gamma, beta, ag, ab, G, ada_rows=[1, 2, 0]), ag, ab))
    # beta applied once instead of through the quirk
    _caught(chk(_affine_from_sums(x, gamma, beta, ag, ab, G, quirk=False), ag, ab))


# ---- small_gemm / projector_finalize -------------------------------------------------------------------------------------
@pytest.mark.parametrize("NN", [1, 16])
def test_small_gemm_reference_and_dropped_tail(NN):
    g = _g(8)
    M, K, batch = 12, 300, 3
    A, B = torch.randn(M, K, generator=g), torch.randn(batch, K, NN, generator=g)
    out = torch.einsum("mk,bkn->bmn", A, B)
    ref = R.small_gemm_fp64(A, B.reshape(batch, -1, 1) if NN == 1 else B, NN)
    assert _close(ref, out, 2e-6)
    _clean(R.check_small_gemm(out, A, B, NN))
    k_kept = K - K % 256
    dropped = torch.einsum("mk,bkn->bmn", A[:, :k_kept], B[:, :k_kept])                  # the last K % 256 terms missing
    assert all(f > R.FP32_FRAME for f in _caught(R.check_small_gemm(dropped, A, B, NN))["frame_fig"])


def test_projector_finalize_reference_and_faults():
    g = _g(9)
    Bn, E, nn = 3, 20, 4
    rows = [0] * 5 + [1] * 7 + [2] * 3
    R_ = len(rows)
    T, V = torch.randn(Bn, R_, E, generator=g), torch.randn(3, E, 2, generator=g)
    nor = torch.tensor(rows, dtype=torch.int32)
    gamma, beta = torch.randn(R_, generator=g), torch.randn(R_, generator=g)
    Vr = V[nor.long()]
    ag = gamma[None] + torch.einsum("bre,re->br", T, Vr[..., 0])
    ab = beta[None] + torch.einsum("bre,re->br", T, Vr[..., 1])
    rg, rb = R.projector_finalize_fp64(T, V, nor, gamma, beta)
    assert _close(rg, ag, 2e-6) and _close(rb, ab, 2e-6)
    _clean(R.check_projector_finalize(ag, ab, T, V, nor, gamma, beta))
    _caught(R.check_projector_finalize(ab, ag, T, V, nor, gamma, beta))                   # the two columns of v exchanged
    first_v = gamma[None] + torch.einsum("bre,e->br", T, V[0, :, 0])                      # norm_of_row ignored
    _caught(R.check_projector_finalize(first_v, ab, T, V, nor, gamma, beta))


# ---- mat4_inverse --------------------------------------------------------------------------------------------------------
def _gauss_jordan(m, pivot):
    """the kernel's elimination in double, with or without the row exchange"""
    out = []
    for a in m.double():
        w = torch.cat([a, torch.eye(4, dtype=torch.float64)], dim=1)
        for c in range(4):
            if pivot:
                p = c + int(w[c:, c].abs().argmax())
                if p != c:
                    w[[c, p]] = w[[p, c]]
            w[c] = w[c] / w[c, c]
            for r in range(4):
                if r != c:
                    w[r] = w[r] - w[r, c] * w[c]
        out.append(w[:, 4:])
    return torch.stack(out).float()


def test_mat4_inverse_reference_and_missing_row_exchange():
    g = _g(10)
    m = torch.eye(4).repeat(5, 1, 1)
    m[:, :3, :3] += 0.3 * torch.randn(5, 3, 3, generator=g)
    m[:, :3, 3] = 0.1 * torch.randn(5, 3, generator=g)
    m[2, :3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) * 1.1    # a 90 degree rotation: m[0][0] = 0
    ref = R.mat4_inverse_fp64(m)
    assert ref.dtype == torch.float64 and _close(ref, torch.linalg.inv(m), 2e-6)
    _clean(R.check_mat4_inverse(_gauss_jordan(m, pivot=True), m))
    _clean(R.check_mat4_inverse(torch.linalg.inv(m.double()).float(), m))
    fig = _caught(R.check_mat4_inverse(_gauss_jordan(m, pivot=False), m))                 # 1 / 0: the matrix comes out non-finite
    assert [i for i, f in enumerate(fig["frame_fig"]) if f > 1] == [2]


# ---- grid_sample3d -------------------------------------------------------------------------------------------------------
def _sampler_case(K=1, N=2):
    g = _g(11)
    C, D, H, W = 8, 4, 6, 7
    smooth = F.interpolate(torch.randn(K, C, 2, 3, 3, generator=g), size=(D, H, W), mode="trilinear", align_corners=True)
    vol = (smooth + 0.05 * torch.randn(K, C, D, H, W, generator=g)).contiguous()
    delta = 0.3 * torch.randn(N, 3, D, H, W, generator=g)                                 # reaches past the border: the padding matters
    theta = torch.eye(4)[:3].repeat(N, 1, 1) + 0.2 * torch.randn(N, 3, 4, generator=g)
    return vol, delta, theta


@pytest.mark.parametrize("pad", ["zeros", "border", "reflection"])
@pytest.mark.parametrize("form", ["delta", "theta"])
def test_sampler_reference_equals_torch(pad, form):
    vol, delta, theta = _sampler_case(K=2)
    D, H, W = vol.shape[2:]
    if form == "delta":
        grid = torch.stack([R.delta_grid_f32(d) for d in delta])
        assert torch.equal(grid[..., 0], torch.linspace(-1, 1, W).view(1, 1, 1, W) + delta[:, 0])
        kw = dict(delta=delta)
    else:
        grid = torch.stack([R.theta_grid_f32(t, (D, H, W)) for t in theta])
        assert _close(torch.stack([R.theta_grid_fp64(t, (D, H, W)) for t in theta]), grid, 2.4e-7)
        assert _close(F.affine_grid(theta, (2, 1, D, H, W), align_corners=True).double(), grid, 2.4e-7)   # the same lattice
        kw = dict(theta=theta)
    out = F.grid_sample(vol, grid, padding_mode=pad, align_corners=False)
    ref = R.grid_sample3d_fp64(vol, padding_mode=pad, **kw)
    assert _close(ref, out, 2e-5)
    cl = vol.permute(0, 2, 3, 4, 1).contiguous()
    assert torch.equal(R.grid_sample3d_fp64(cl, padding_mode=pad, in_layout="ndhwc", **kw), ref)
    fig = _clean(R.check_grid_sample3d(out, vol, padding_mode=pad, **kw))
    assert fig["max_ratio"] == fig["mean_ratio"] == 1.0                                   # the yardstick itself
    fig = _clean(R.check_grid_sample3d(out.permute(0, 2, 3, 4, 1).contiguous(), cl, padding_mode=pad, in_layout="ndhwc",
                                       out_layout="ndhwc", **kw))
    assert fig["frames"] == [0, 1]
    shared = R.grid_sample3d_fp64(vol[:1], padding_mode=pad, **kw)                        # one volume for every sample
    assert torch.equal(shared[0], ref[0]) and not torch.equal(shared[1], ref[1])


def _trilinear_by_hand(vol_n, grid, pad, swap=False):
    """ATen's 3-D grid_sample (align_corners=False) spelled out for one [C, D, H, W] volume in fp32: `swap` exchanges the
    weights of the two corners (x0, y0, z0) and (x1, y0, z0)"""
    C, D, H, W = vol_n.shape
    out = torch.zeros((C,) + tuple(grid.shape[:3]))
    idx = []
    for c, size in zip(grid.unbind(-1), (W, H, D)):
        i = ((c + 1) * size - 1) / 2
        if pad == "border":
            i = i.clamp(0, size - 1)
        elif pad == "reflection":
            t = (i + 0.5).abs()
            extra, flips = torch.fmod(t, size), torch.floor(t / size)
            i = torch.where(flips % 2 == 0, extra - 0.5, size - extra - 0.5).clamp(0, size - 1)
        idx.append(i)
    ix, iy, iz = idx
    x0, y0, z0 = ix.floor(), iy.floor(), iz.floor()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ddx = 1 - dx if (swap and dy == 0 and dz == 0) else dx
                w = ((ix - x0) if ddx else (x0 + 1 - ix)) * ((iy - y0) if dy else (y0 + 1 - iy)) * ((iz - z0) if dz else (z0 + 1 - iz))
                xi, yi, zi = (x0 + dx).long(), (y0 + dy).long(), (z0 + dz).long()
                ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & (zi >= 0) & (zi < D)
                v = vol_n[:, zi.clamp(0, D - 1), yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
                out += v * (w * ok)[None]
    return out


def test_sampler_checker_reports_the_planted_faults():
    vol, delta, theta = _sampler_case(K=2)
    grid = torch.stack([R.delta_grid_f32(d) for d in delta])
    for pad in ("zeros", "reflection"):
        hand = torch.stack([_trilinear_by_hand(vol[n], grid[n], pad) for n in range(2)])
        fig = _clean(R.check_grid_sample3d(hand, vol, delta=delta, padding_mode=pad))    # another order of fp32 operations
        assert fig["max_ratio"] < 2 and fig["mean_ratio"] < 1.25
        swapped = torch.stack([_trilinear_by_hand(vol[n], grid[n], pad, swap=True) for n in range(2)])
        _caught(R.check_grid_sample3d(swapped, vol, delta=delta, padding_mode=pad))      # two corner weights exchanged
    border = F.grid_sample(vol, grid, padding_mode="border", align_corners=False)
    _caught(R.check_grid_sample3d(border, vol, delta=delta, padding_mode="reflection"))  # reflection replaced by border
    # the bank: sample n reads volume vol_index[n]; an index outside the bank gives zeros
    vol3, delta3, _ = _sampler_case(K=2, N=3)
    grid3 = torch.stack([R.delta_grid_f32(d) for d in delta3])
    index = torch.tensor([1, 0, 5], dtype=torch.int32)
    out = F.grid_sample(vol3[[1, 0, 0]], grid3, padding_mode="zeros", align_corners=False)
    out[2] = 0
    fig = _clean(R.check_grid_sample3d(out, vol3, delta=delta3, vol_index=index))
    assert fig["frames"] == [0, 1, 2]
    ignored = F.grid_sample(vol3[[0, 0, 0]], grid3, padding_mode="zeros", align_corners=False)
    ignored[2] = 0
    assert _caught(R.check_grid_sample3d(ignored, vol3, delta=delta3, vol_index=index))["worst_frame"] == 0
    out[2] = F.grid_sample(vol3[1:2], grid3[2:3], padding_mode="zeros", align_corners=False)[0]
    _caught(R.check_grid_sample3d(out, vol3, delta=delta3, vol_index=index))              # the bad index clamped, not zeroed
    # the theta form with the delta form's grid
    _caught(R.check_grid_sample3d(border, vol, theta=theta, padding_mode="border"))


# ---- conv2d_generic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", [9, 64, 70])
def test_unpack_generic_inverts_pack_generic_bit_for_bit(cout):
    from emoportraits_amd import pack
    w = torch.randn(cout, 5, 3, 2, generator=_g(20))
    w[0, 0, 0, 0], w[-1, -1, -1, -1] = -0.0, 2.0 ** -140                                  # a signed zero and a subnormal survive
    wt = pack.pack_generic(w)
    assert tuple(wt.shape) == (30, (cout + 63) // 64 * 64) and wt[:, cout:].abs().sum().item() == 0
    back = R.unpack_generic(wt, cout, 5, 3, 2)
    assert tuple(back.shape) == tuple(w.shape) and torch.equal(back.contiguous().view(torch.int32), w.view(torch.int32))
    with pytest.raises(ValueError):
        R.unpack_generic(wt, cout, 5, 3, 3)


def test_generic_splits_run_follows_the_launcher():
    """requests -> (chunks per split rounded up, empty splits dropped), as emo_conv2d_generic_f32 derives them"""
    assert R.generic_splits_run(576, 4) == 4            # 18 chunks: 5 + 5 + 5 + 3
    assert R.generic_splits_run(576, 7) == 6            # 3 per split: the seventh split would be empty
    assert R.generic_splits_run(4608, 32) == 29         # 144 chunks, 5 per split
    assert R.generic_splits_run(147, 64) == 5           # clamped to the 5 chunks (the last one ragged: 19 rows)
    assert R.generic_splits_run(288, 9) == 9 and R.generic_splits_run(288, 1) == 1 and R.generic_splits_run(31, 3) == 1


def _conv_case(N, Cin, H, W, Cout, k, stride, pad, seed, affine=True, bias=True, relu=True):
    from emoportraits_amd import pack
    g = _g(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) if bias else None
    sc = 1 + 0.3 * torch.randn(N, Cin, generator=g) if affine else None
    sh = 0.3 * torch.randn(N, Cin, generator=g) if affine else None
    return dict(x=x, w=w, wt=pack.pack_generic(w), geom=(Cout, k, k, stride, pad), bias=b, scale=sc, shift=sh,
                relu_in=relu and affine)


def _conv_by_hand(c, drop=None, bias_times=1, bias_roll=0, affine_of=None):
    """the operation in fp64 from the unpacked pieces, rounded once to fp32, with the faults to plant: `drop` = rows of the
    im2col matrix left out of the sum, the bias added `bias_times` times or rolled by `bias_roll` channels, sample n prepared
    with the affine of sample affine_of[n]"""
    Cout, k, _, stride, pad = c["geom"]
    N = c["x"].shape[0]
    outs = []
    for n in range(N):
        v = c["x"][n].double()
        if c["scale"] is not None:
            m = n if affine_of is None else affine_of[n]
            v = v * c["scale"][m].double()[:, None, None] + c["shift"][m].double()[:, None, None]
            if c["relu_in"]:
                v = v.clamp_min(0)
        cols = F.unfold(v[None], (k, k), padding=pad, stride=stride)[0]
        if drop is not None:
            cols[drop] = 0.0
        o = c["w"].double().reshape(Cout, -1) @ cols
        if c["bias"] is not None:
            o = o + bias_times * c["bias"].double().roll(bias_roll)[:, None]
        outs.append(o)
    Ho = (c["x"].shape[2] + 2 * pad - k) // stride + 1
    return torch.stack(outs).reshape(N, Cout, Ho, -1).float()


def _conv_check(c, out, splits=1):
    Cout, kh, kw, stride, pad = c["geom"]
    return R.check_conv2d_generic(out, c["x"], c["wt"], Cout, kh, kw, stride, pad, c["bias"], c["scale"], c["shift"], c["relu_in"], splits)


@pytest.mark.parametrize("case", [
    (3, 64, 8, 8, 64, 3, 1, 1, True, True),          # K = 576
    (3, 3, 16, 16, 16, 7, 2, 3, True, False),        # K = 147: the stem, affine without ReLU below
    (2, 40, 9, 7, 9, 3, 2, 1, False, True),          # odd sizes, no affine
    (2, 128, 4, 4, 9, 1, 2, 0, False, False),        # 1x1 stride 2: 2x2 outputs
])
def test_conv2d_generic_reference_equals_torch(case):
    N, Cin, H, W, Cout, k, stride, pad, affine, bias = case
    c = _conv_case(N, Cin, H, W, Cout, k, stride, pad, seed=21, affine=affine, bias=bias, relu=Cin != 3)
    ref = R.conv2d_generic_fp64(c["x"], c["wt"], Cout, k, k, stride, pad, c["bias"], c["scale"], c["shift"], c["relu_in"])
    xin = c["x"].double()
    if affine:
        xin = xin * c["scale"].double()[:, :, None, None] + c["shift"].double()[:, :, None, None]
        xin = F.relu(xin) if c["relu_in"] else xin
    own = F.conv2d(xin, c["w"].double(), None if c["bias"] is None else c["bias"].double(), stride=stride, padding=pad)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == tuple(own.shape)
    assert (ref - own).abs().max().item() <= 1e-13 * own.abs().max().item() * Cin * k * k
    fig = _clean(_conv_check(c, ref.float()))                                              # the rounded reference
    assert fig["frames"] == list(range(N)) and fig["worst"] <= 1 and len(fig["frame_rel"]) == N and 0 < fig["rms_rel"] < 1e-7
    assert torch.equal(_conv_by_hand(c), ref.float())
    _clean(_conv_check(c, F.conv2d(xin.float(), c["w"], c["bias"], stride=stride, padding=pad), splits=3))   # a plain fp32 evaluation


def test_conv_checker_reports_faults_in_the_k_loop():
    c = _conv_case(3, 64, 8, 8, 64, 3, 1, 1, seed=22)                                      # K = 576: 18 chunks
    _clean(_conv_check(c, _conv_by_hand(c), splits=4))
    fig = _caught(_conv_check(c, _conv_by_hand(c, drop=[100]), splits=4))                  # one K term of 576
    assert all(f > 1 for f in fig["frame_fig"])
    assert max(fig["frame_rel"]) > R.FP32_FRAME                                            # (the frame bound sees this one too)
    assert _conv_check(c, _conv_by_hand(c), splits=4)["splits_run"] == 4
    _caught(_conv_check(c, _conv_by_hand(c, drop=slice(15 * 32, 576)), splits=4))          # the last, uneven split: chunks 15..17
    stem = _conv_case(3, 3, 16, 16, 16, 7, 2, 3, seed=23, bias=False, relu=False)          # K = 147 = 4 chunks + 19 rows
    _clean(_conv_check(stem, _conv_by_hand(stem)))
    _caught(_conv_check(stem, _conv_by_hand(stem, drop=slice(128, 147))))                  # the ragged last chunk
    _caught(_conv_check(stem, _conv_by_hand(stem, drop=[146])))                            # its last row alone


def test_conv_checker_reports_faults_in_the_bias():
    c = _conv_case(3, 32, 4, 4, 70, 3, 1, 1, seed=24, affine=False)                        # K = 288: 9 chunks
    _clean(_conv_check(c, _conv_by_hand(c), splits=9))
    _caught(_conv_check(c, _conv_by_hand(c, bias_times=9), splits=9))                      # added by every split
    _caught(_conv_check(c, _conv_by_hand(c, bias_times=0), splits=9))                      # lost in the reduction
    fig = _caught(_conv_check(c, _conv_by_hand(c, bias_roll=1), splits=9))                 # the neighbouring channel's
    assert all(f > 1 for f in fig["frame_fig"])
    # in one channel with a small bias the wrong bias is far below the tensor's maximum: the bound is per output
    small = dict(c, bias=c["bias"].clone())
    small["bias"][5], small["bias"][4] = 3e-4, -2e-4
    out = _conv_by_hand(small)
    bad = out.clone()
    bad[:, 5] = _conv_by_hand(small, bias_roll=1)[:, 5]
    assert (bad - out).abs().max().item() < 2e-4 * out.abs().max().item()
    _caught(_conv_check(small, bad, splits=9))


def test_conv_checker_reports_faults_between_the_frames_of_one_tile():
    """N = 3 on a 4x4 map: 48 GEMM columns, all in one 64-column tile"""
    c = _conv_case(3, 32, 4, 4, 70, 3, 1, 1, seed=25, bias=False)
    out = _conv_by_hand(c)
    assert _clean(_conv_check(c, out))["frames"] == [0, 1, 2]
    fig = _caught(_conv_check(c, _conv_by_hand(c, affine_of=[0, 0, 2])))                   # frame 1 prepared with frame 0's affine
    assert fig["frame_fig"][0] <= 1 and fig["frame_fig"][2] <= 1 < fig["frame_fig"][1] and fig["worst_frame"] == 1
    fig = _caught(_conv_check(c, out[[0, 2, 1]]))                                          # frames 1 and 2 exchanged
    assert fig["frame_fig"][0] <= 1 and fig["frame_fig"][1] > 1 and fig["frame_fig"][2] > 1
    # a fault in one frame whose values are 1e-4 of the other frames': under 2e-5 of the tensor's maximum
    quiet = dict(c, x=c["x"] * torch.tensor([1.0, 1e-4, 1.0]).view(3, 1, 1, 1),
                 shift=c["shift"] * torch.tensor([1.0, 1e-4, 1.0]).view(3, 1))
    out = _conv_by_hand(quiet)
    bad = out.clone()
    bad[1] = _conv_by_hand(quiet, drop=[7])[1]
    assert (bad - out).abs().max().item() < 2e-5 * out.abs().max().item()
    assert _caught(_conv_check(quiet, bad))["worst_frame"] == 1


def _fma(x, s, t):
    """fl(x s + t) with ONE rounding, as the kernels' __fmaf_rn: the fp64 product of two fp32 values is exact"""
    return (x.double() * s.double()[:, :, None, None] + t.double()[:, :, None, None]).float()


# ---- maxpool2d -----------------------------------------------------------------------------------------------------------
def test_maxpool_reference_and_faults():
    g = _g(26)
    x = torch.randn(2, 5, 9, 7, generator=g) - 2.5                                        # mostly negative: the padding value shows
    sc, sh = torch.randn(2, 5, generator=g), torch.randn(2, 5, generator=g)               # negative scales included
    e = lambda t: t[:, :, None, None]
    plain = F.max_pool2d(x, 3, 2, 1)
    assert torch.equal(R.maxpool2d_fp64(x, 3, 2, 1), plain.double())
    assert _clean(R.check_maxpool2d(plain, x, 3, 2, 1))["worst"] == 0                     # bit-equal
    folded = F.max_pool2d(F.relu(x * e(sc) + e(sh)), 3, 2, 1)
    assert _same64(R.maxpool2d_fp64(x, 3, 2, 1, sc, sh, True), F.max_pool2d(F.relu(x.double() * e(sc).double() + e(sh).double()), 3, 2, 1))
    assert _same64(R.maxpool2d_fp64(x, 3, 2, 1, sc, sh, False), F.max_pool2d(x.double() * e(sc).double() + e(sh).double(), 3, 2, 1))
    _clean(R.check_maxpool2d(R.maxpool2d_fp64(x, 3, 2, 1, sc, sh, True).float(), x, 3, 2, 1, sc, sh, True))
    _clean(R.check_maxpool2d(F.max_pool2d(F.relu(_fma(x, sc, sh)), 3, 2, 1), x, 3, 2, 1, sc, sh, True))   # the kernel's arithmetic in fp32
    _caught(R.check_maxpool2d(folded, x, 3, 2, 1, sc, sh, True))        # product and sum rounded separately: outside one rounding
    ulp = plain.clone()
    ulp[1, 2, 3, 1] = torch.nextafter(ulp[1, 2, 3, 1], torch.tensor(9.0))
    assert _caught(R.check_maxpool2d(ulp, x, 3, 2, 1))["worst_frame"] == 1                # without a scale one ulp is a fault
    ninf = float("-inf")
    shifted = F.max_pool2d(F.pad(x, (1, 0, 0, 0), value=ninf)[..., :-1], 3, 2, 1)         # every window one column to the left
    _caught(R.check_maxpool2d(shifted, x, 3, 2, 1))
    zero_pad = F.max_pool2d(F.pad(x, (1, 1, 1, 1), value=0.0), 3, 2, 0)                   # 0 in place of -inf at the border
    assert torch.equal(zero_pad[:, :, 1:-1, 1:-1], plain[:, :, 1:-1, 1:-1]) and not torch.equal(zero_pad, plain)
    _caught(R.check_maxpool2d(zero_pad, x, 3, 2, 1))
    no_relu = F.max_pool2d(x * e(sc) + e(sh), 3, 2, 1)
    _caught(R.check_maxpool2d(no_relu, x, 3, 2, 1, sc, sh, True))


# ---- affine_add_relu -----------------------------------------------------------------------------------------------------
def test_affine_add_relu_reference_and_faults():
    g = _g(27)
    a, b = torch.randn(2, 6, 5, 3, generator=g), torch.randn(2, 6, 5, 3, generator=g)
    sa, ta, sb, tb = (torch.randn(2, 6, generator=g) for _ in range(4))
    e = lambda t: t[:, :, None, None]
    both = F.relu(a * e(sa) + e(ta) + (b * e(sb) + e(tb)))
    d = lambda t: e(t).double()
    assert _same64(R.affine_add_relu_fp64(a, sa, ta, b, sb, tb), F.relu(a.double() * d(sa) + d(ta) + (b.double() * d(sb) + d(tb))))
    assert _same64(R.affine_add_relu_fp64(a, sa, ta, b, sb, tb, relu=False), a.double() * d(sa) + d(ta) + (b.double() * d(sb) + d(tb)))
    _clean(R.check_affine_add_relu(F.relu(_fma(a, sa, ta) + _fma(b, sb, tb)), a, sa, ta, b, sb, tb))     # the kernel's arithmetic in fp32
    _clean(R.check_affine_add_relu(R.affine_add_relu_fp64(a, sa, ta, b, sb, tb).float(), a, sa, ta, b, sb, tb))
    skip = F.relu(a * e(sa) + e(ta) + b)                                                  # b = the block input: no affine
    assert _same64(R.affine_add_relu_fp64(a, sa, ta, b), F.relu(a.double() * d(sa) + d(ta) + b.double()))
    skip_fma = F.relu(_fma(a, sa, ta) + b)
    _clean(R.check_affine_add_relu(skip_fma, a, sa, ta, b))
    _caught(R.check_affine_add_relu(skip_fma, a, sa, ta, b, sb, tb))
    _caught(R.check_affine_add_relu(F.relu(a * e(sa) + e(ta) + (b * e(sa) + e(ta))), a, sa, ta, b, sb, tb))   # sb / tb taken from sa / ta
    _caught(R.check_affine_add_relu(a * e(sa) + e(ta) + b, a, sa, ta, b))                 # the ReLU left out
    rolled = F.relu(a * e(sa.roll(1, 1)) + e(ta.roll(1, 1)) + b)                          # the affine of the neighbouring channel
    _caught(R.check_affine_add_relu(rolled, a, sa, ta, b))
    # where A and B cancel the bound follows the operands, not the result: fp32 evaluation of a cancelling pair passes
    nb = -_fma(a, sa, ta) * 0.999
    _clean(R.check_affine_add_relu(F.relu(_fma(a, sa, ta) + nb), a, sa, ta, nb))


# ---- grid_sample2d -------------------------------------------------------------------------------------------------------
def _sampler2d_case():
    g = _g(28)
    smooth = F.interpolate(torch.randn(3, 4, 4, 5, generator=g), size=(21, 29), mode="bilinear", align_corners=True)
    img = (smooth + 0.05 * torch.randn(3, 4, 21, 29, generator=g)).contiguous()
    grid = torch.rand(3, 11, 13, 2, generator=g) * 2.8 - 1.4                              # reaches past the border
    theta = torch.tensor([[0.9, 0.2, 0.1], [-0.15, 1.1, -0.3]]).repeat(3, 1, 1) + 0.1 * torch.randn(3, 2, 3, generator=g)
    return img, grid, theta


def test_grid_sample2d_reference_and_faults():
    img, grid, theta = _sampler2d_case()
    S = 16
    out = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    assert _same64(R.grid_sample2d_fp64(img, grid=grid),
                   F.grid_sample(img.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=False))
    fig = _clean(R.check_grid_sample2d(out, img, grid=grid, warp=grid.clone()))
    assert fig["max_ratio"] == fig["mean_ratio"] == 1.0 and fig["warp_worst"] == 0 and fig["frames"] == [0, 1, 2]
    _clean(R.check_grid_sample2d(R.grid_sample2d_fp64(img, grid=grid).float(), img, grid=grid))
    with pytest.raises(ValueError, match="frame 0: output"):
        R.check_grid_sample2d(out[:, :, :-1], img, grid=grid)
    border = F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)
    _caught(R.check_grid_sample2d(border, img, grid=grid))                                # the corners outside the image not zeroed
    _caught(R.check_grid_sample2d(out, img, grid=grid, warp=grid.flip(-1)))
    # the theta form: the lattice of ExpressionEmbed, the grid the reference code builds
    g32 = torch.stack([R.theta_grid2d_f32(t, S) for t in theta])
    g64 = torch.stack([R.theta_grid2d_fp64(t, S) for t in theta])
    lin = torch.linspace(-1, 1, S)
    assert _close(g64, g32, 2.4e-7) and _close(g64[..., 0], theta[:, 0, 0].view(3, 1, 1) * lin.view(1, 1, S)
                                               + theta[:, 0, 1].view(3, 1, 1) * lin.view(1, S, 1) + theta[:, 0, 2].view(3, 1, 1), 2.4e-7)
    aligned = F.grid_sample(img, g32, align_corners=False)
    assert _same64(R.grid_sample2d_fp64(img, theta=theta, size=S), F.grid_sample(img.double(), g64, align_corners=False))
    assert _close(R.grid_sample2d_fp64(img, theta=theta, size=S), aligned, 2e-5)          # (and near the fp32 bmm grid's result)
    fig = _clean(R.check_grid_sample2d(aligned, img, theta=theta, size=S, warp=g64.float()))
    assert fig["max_ratio"] == 1.0 and fig["warp_worst"] <= 1
    swapped = theta[:, [1, 0]]                                                            # x and y of theta exchanged
    gs = torch.stack([R.theta_grid2d_f32(t, S) for t in swapped])
    _caught(R.check_grid_sample2d(F.grid_sample(img, gs, align_corners=False), img, theta=theta, size=S))
    fig = R.check_grid_sample2d(aligned, img, theta=theta, size=S, warp=gs)              # ... in the returned warp alone
    assert fig["failures"] and fig["warp_worst"] > 1 and fig["max_ratio"] == 1.0
    off = g64.float().clone()
    off[2, 5, 7, 1] = off[2, 5, 7, 1] + 4 * 2.0 ** -23 * off[2, 5, 7, 1].abs()           # four ulps in one coordinate
    _caught(R.check_grid_sample2d(aligned, img, theta=theta, size=S, warp=off))
    frame0_theta = F.grid_sample(img, g32[[0, 0, 2]], align_corners=False)                # frame 1 warped by frame 0's theta
    assert _caught(R.check_grid_sample2d(frame0_theta, img, theta=theta, size=S))["worst_frame"] == 1


# ---- resize2d ------------------------------------------------------------------------------------------------------------
def test_resize2d_reference_and_faults():
    x = torch.rand(2, 3, 24, 20, generator=_g(29))
    for size in ((12, 10), (6, 5), (9, 7)):
        out = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
        assert _same64(R.resize2d_fp64(x, size), F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False))
        fig = _clean(R.check_resize2d(out, x, size))
        assert fig["frames"] == [0, 1] and fig["max_ratio"] in (0.0, 1.0)
        _caught(R.check_resize2d(F.interpolate(x, size=size, mode="bilinear", align_corners=True), x, size))
        _caught(R.check_resize2d(F.interpolate(x, size=size, mode="nearest"), x, size))
    _caught(R.check_resize2d(F.interpolate(x, size=(9, 7), mode="bilinear", antialias=True), x, (9, 7)))


def _bicubic(x, window, size, A=-0.75, clamp_into="window"):
    """the bicubic resize of a window, written out (fp64 sums of the 4 x 4 taps, rounded once): source index s = scale (o + 0.5) -
    0.5, taps floor(s) - 1 ... floor(s) + 2, cubic-convolution weights with parameter A; a tap that leaves the window is clamped
    into the window -- or, the planted fault, into the frame, where it reads the pixels next to the window"""
    x0, y0, w, h = window
    H, W = x.shape[-2:]

    def axis(n_out, n_in, off, full):
        s = (n_in / n_out) * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5
        f = s.floor()
        t = s - f
        idx = f.long()[:, None] + torch.arange(-1, 3)[None]
        idx = idx.clamp(0, n_in - 1) + off if clamp_into == "window" else (idx + off).clamp(0, full - 1)
        c1 = lambda v: ((A + 2) * v - (A + 3)) * v * v + 1
        c2 = lambda v: ((A * v - 5 * A) * v + 8 * A) * v - 4 * A
        return idx, torch.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], 1)

    (iy, wy), (ix, wx) = axis(size[0], h, y0, H), axis(size[1], w, x0, W)
    v = x.double()[:, :, iy][..., ix]                                                     # [N, C, Ho, 4, Wo, 4]
    return (v * wy[None, None, :, :, None, None] * wx[None, None, None, None]).sum((3, 5)).float()


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_resize2d_windows_modes_and_clamp(mode):
    x = torch.rand(2, 3, 24, 32, generator=_g(31)) * 1.4 - 0.2                            # values in [-0.2, 1.2]
    for window, size in (((5, 3, 14, 12), (30, 28)), ((0, 0, 16, 10), (7, 9)), ((18, 14, 14, 10), (10, 14)), (None, (12, 16))):
        sl = x if window is None else x[:, :, window[1]:window[1] + window[3], window[0]:window[0] + window[2]]
        for clamp01 in (False, True):
            own = F.interpolate(sl.double(), size=size, mode=mode, align_corners=False)
            assert _same64(R.resize2d_fp64(x, size, mode, window, clamp01), own.clamp(0, 1) if clamp01 else own)
            out = F.interpolate(sl.contiguous(), size=size, mode=mode, align_corners=False)
            fig = _clean(R.check_resize2d(out.clamp(0, 1) if clamp01 else out, x, size, mode, window, clamp01))
            assert fig["max_ratio"] in (0.0, 1.0) and fig["exact_bad"] == 0
    # the clamp dropped: an overshoot (bicubic) or an input outside [0, 1] (both modes) survives
    out = F.interpolate(x[:, :, 3:15, 5:19].contiguous(), size=(30, 28), mode=mode, align_corners=False)
    assert out.min() < 0 and out.max() > 1
    assert _caught(R.check_resize2d(out, x, (30, 28), mode, (5, 3, 14, 12), True))["exact_bad"] > 0
    # equal size: the input's bits, in both modes; one ulp on one element is no longer the input
    same = x[:, :, 3:15, 5:19].contiguous()
    _clean(R.check_resize2d(same, x, (12, 14), mode, (5, 3, 14, 12)))
    _clean(R.check_resize2d(same.clamp(0, 1), x, (12, 14), mode, (5, 3, 14, 12), True))
    off = same.clone()
    off[1, 2, 5, 6] = torch.nextafter(off[1, 2, 5, 6], torch.tensor(9.0))
    assert _caught(R.check_resize2d(off, x, (12, 14), mode, (5, 3, 14, 12)))["exact_bad"] == 1
    with pytest.raises(ValueError):
        R.check_resize2d(same, x, (12, 14), mode, (20, 3, 14, 12))                        # a window that leaves the frame


def test_resize2d_bicubic_taps_and_parameter():
    """the written-out bicubic is the reference (so the plants below differ from it in what they plant alone); taps clamped into
    the frame read the pixels next to the window, A = -0.5 is the antialiased filter's parameter, not this one's"""
    x = torch.rand(2, 3, 24, 32, generator=_g(32))
    window, size = (6, 5, 12, 10), (40, 36)                                               # interior, upscaled: the border taps leave it
    _clean(R.check_resize2d(_bicubic(x, window, size), x, size, "bicubic", window))
    frame = _bicubic(x, window, size, clamp_into="frame")
    assert torch.equal(frame[:, :, 8:-8, 8:-8], _bicubic(x, window, size)[:, :, 8:-8, 8:-8])      # (the interior is untouched)
    _caught(R.check_resize2d(frame, x, size, "bicubic", window))
    _caught(R.check_resize2d(_bicubic(x, window, size, A=-0.5), x, size, "bicubic", window))
    # a window at the frame's corner has nothing beyond two of its edges, and the other two are caught all the same
    _caught(R.check_resize2d(_bicubic(x, (0, 0, 12, 10), size, clamp_into="frame"), x, size, "bicubic", (0, 0, 12, 10)))


# ---- mul_mask / stage2_compose -------------------------------------------------------------------------------------------
def _wrong_sample(mask, N, C):
    """[N, C, H, W]: the mask a kernel reads that computes the sample as i / HW, without the channels: plane n C + c (here
    modulo N, where the kernel would leave the tensor)"""
    planes = (torch.arange(N)[:, None] * C + torch.arange(C)[None]) % N
    return mask[:, 0][planes]


def test_mul_mask_reference_and_mask_of_the_wrong_sample():
    g = _g(33)
    img, mask = torch.randn(2, 3, 5, 7, generator=g), torch.rand(2, 1, 5, 7, generator=g)
    out = img * mask
    assert torch.equal(R.mul_mask_fp64(img, mask).float(), out) and R.mul_mask_fp64(img, mask).dtype == torch.float64
    assert _clean(R.check_mul_mask(out, img, mask))["worst"] == 0
    fig = _caught(R.check_mul_mask(img * _wrong_sample(mask, 2, 3), img, mask))
    assert fig["frame_fig"] == [35.0, 35.0]               # planes 0 1 0 | 1 0 1 where the masks are 0 0 0 | 1 1 1: channel 1 of each
    off = out.clone()
    off[1, 0, 2, 3] = torch.nextafter(off[1, 0, 2, 3], torch.tensor(9.0))
    assert _caught(R.check_mul_mask(off, img, mask))["frame_fig"] == [0.0, 1.0]
    zero = torch.zeros_like(img)
    _caught(R.check_mul_mask(zero, -img.abs(), torch.zeros_like(mask)))                   # -x * 0 is -0: the sign is part of the bits


def test_stage2_compose_reference_and_faults():
    g = _g(34)
    img, add = torch.rand(2, 3, 6, 9, generator=g), 2.0 * torch.randn(2, 3, 6, 9, generator=g)
    mask, face = torch.rand(2, 1, 6, 9, generator=g), (torch.rand(2, 1, 6, 9, generator=g) > 0.3).float()
    raw = img + add * (mask * face)
    out = raw.clamp(0, 1)
    assert (raw < 0).any() and (raw > 1).any()                                            # both clamps act
    assert _close(R.stage2_compose_fp64(img, add, mask, face), out, 2.4e-7)
    assert _clean(R.check_stage2_compose(out, img, add, mask, face))["worst"] <= 1
    fused = (img.double() + add.double() * (mask * face).double()).float().clamp(0, 1)    # the contracted form: one rounding fewer
    _clean(R.check_stage2_compose(fused, img, add, mask, face))
    _caught(R.check_stage2_compose(raw, img, add, mask, face))                            # the clamp dropped
    wrong = (img + add * (_wrong_sample(mask, 2, 3) * face)).clamp(0, 1)
    _caught(R.check_stage2_compose(wrong, img, add, mask, face))
    _caught(R.check_stage2_compose((img + add * mask).clamp(0, 1), img, add, mask, face))             # face_mask not applied
    # an output the clamp decides is exactly 1: one ulp below is inside any error bound and still wrong
    i = (raw > 1.5).flatten().nonzero()[0].item()
    off = out.clone()
    off.view(-1)[i] = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    _caught(R.check_stage2_compose(off, img, add, mask, face))
    # four ulps on an output inside (0, 1)
    j = ((raw > 0.4) & (raw < 0.6)).flatten().nonzero()[0].item()
    off = out.clone()
    off.view(-1)[j] = out.view(-1)[j] * (1 + 8 * 2.0 ** -23)
    _caught(R.check_stage2_compose(off, img, add, mask, face))


# ---- pack_rgb8 / unpack_rgb8 ---------------------------------------------------------------------------------------------
def test_pack_rgb8_reference_and_rounding_instead_of_truncation():
    img = torch.cat([R.rgb8_edge_image(), torch.rand(1, 3, 4, 193, generator=_g(35)) * 1.4 - 0.2])
    want = img.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1)
    assert torch.equal(R.pack_rgb8_ref(img), want)
    assert _clean(R.check_pack_rgb8(want.contiguous(), img))["frames"] == [0, 1]
    rounded = img.clamp(0, 1).mul(255).round().byte().permute(0, 2, 3, 1)
    assert _caught(R.check_pack_rgb8(rounded, img))["frame_fig"][1] > 100                 # about half of a random image
    _caught(R.check_pack_rgb8(img.mul(255).byte().permute(0, 2, 3, 1), img))              # the clamp dropped: bytes wrap
    _caught(R.check_pack_rgb8(want.flip(-1), img))                                        # BGR
    with pytest.raises(ValueError):
        R.check_pack_rgb8(want.permute(0, 3, 1, 2), img)


def test_unpack_rgb8_reference_and_multiplication_by_the_reciprocal():
    b = torch.arange(256, dtype=torch.uint8)
    frames = torch.stack([b, b.flip(0), b.roll(50)], -1).reshape(1, 16, 16, 3)
    want = frames.float().div(255).permute(0, 3, 1, 2)
    # the fp64 quotient rounded to fp32 is the fp32 quotient, for every byte
    assert torch.equal(R.unpack_rgb8_fp64(frames).float(), want) and R.unpack_rgb8_fp64(frames).dtype == torch.float64
    _clean(R.check_unpack_rgb8(want.contiguous(), frames))
    recip = frames.float().mul(torch.tensor(1.0 / 255)).permute(0, 3, 1, 2)
    assert 0 < (recip != want).sum() and (recip - want).abs().max() <= 2.0 ** -24        # one ulp, on some bytes
    _caught(R.check_unpack_rgb8(recip.contiguous(), frames))
    _caught(R.check_unpack_rgb8(want.flip(1).contiguous(), frames))                       # channels reversed
    # the round trip the video path relies on: every byte comes back
    assert torch.equal(R.pack_rgb8_ref(want), frames)
    assert torch.equal(R.pack_rgb8_ref(R.unpack_rgb8_fp64(frames).float()), frames)


# ---- pose_theta ----------------------------------------------------------------------------------------------------------
def test_pose_theta_reference_and_faults():
    g = _g(30)
    s, r, t = 1 + 0.1 * torch.randn(5, 3, generator=g), 0.5 * torch.randn(5, 3, generator=g), 0.1 * torch.randn(5, 3, generator=g)
    O = R._restate()
    out = O.get_transform_matrix(s, r, t)
    ref = R.pose_theta_fp64(s, r, t)
    assert _same64(ref, O.get_transform_matrix(s.double(), r.double(), t.double())) and _close(ref, out, 2.4e-7)
    assert _clean(R.check_pose_theta(out, s, r, t))["max_ratio"] == 1.0
    _clean(R.check_pose_theta(ref.float(), s, r, t))
    _caught(R.check_pose_theta(O.get_transform_matrix(s, r[:, [1, 0, 2]], t), s, r, t))   # yaw and pitch exchanged
    t_not_scaled = out.clone()
    t_not_scaled[:, :3, 3] = torch.einsum("bij,bj->bi", out[:, :3, :3] / s[:, :, None], t)
    _caught(R.check_pose_theta(t_not_scaled, s, r, t))                                    # the translation column without the scale
