"""The fp64 references and launch checkers of tests/ops_reference.py, on the CPU: each reference equals the plain fp32 torch
composition of its operation, each checker passes an output that carries only fp32 rounding noise, and each checker reports
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
