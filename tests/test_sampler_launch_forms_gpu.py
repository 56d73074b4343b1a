"""Every launch form and coordinate edge of the 3-D sampler and of the repack kernels, held to ATen on the device.

The cases are tests/sampler_launch_forms.py's, read from the launchers' decision functions (direct_form in csrc/grid_sample3d.hip,
tile_form in gs3d_tile_launch.h).  Each case first asks the library (emo_grid_sample3d_launch_form, ABI 29) and asserts the form
and the plan it is named for, then runs through emoportraits_amd.ops on poisoned, guarded outputs and is compared BIT FOR BIT, as
int32 views, with torch's CPU F.grid_sample(align_corners=False) -- theta mode against the sampling of the materialised grid.
The FMA forms are held to the bound the project derives (8 * 2^-24 * max|vol|: the eight skipped product roundings) and, where the
block order is ORDER 3, to bit equality with the same call on per-sample copies of the volume, which takes ORDER 1.

Inputs are laid out with torch permutes on the host, not with the repack kernels, which have their own tests below.  The run_*
functions take the device, so tests/test_sampler_launch_forms_emul.py runs the direct-form cases on the host-compiled library.
"""
import os
import re
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import c_oracle  # noqa: E402

import sampler_launch_forms as L  # noqa: E402
from emoportraits_amd import hip, ops  # noqa: E402
from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]

DEV = "cuda:0"
PADS = ("zeros", "border", "reflection")
MODES = ("grid", "theta", "delta")
FMA_BOUND = 8 * 2.0 ** -24          # x max|vol|: csrc/grid_sample3d.hip, gather_quad<true>
GUARD = 4096                        # NaN floats on either side of a bank


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want, what):
    """bit equality of two float32 tensors, with the first difference in the message"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = bits(got) != bits(want)
    if bool(ne.any()):
        i = tuple(int(v) for v in ne.nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at {i}: got {got[i].item()!r}, "
                             f"want {want[i].item()!r}")


def to_layout(v, layout):
    """[N,C,D,H,W] on the host -> the layout's tensor (a permute: independent of the repack kernels)"""
    N, C, D, H, W = v.shape
    if layout == "ndhwc":
        return v.permute(0, 2, 3, 4, 1).contiguous()
    if layout == "p4":
        return v.view(N, C // 4, 4, D, H, W).permute(0, 1, 3, 4, 5, 2).contiguous()
    return v.clone(memory_format=torch.contiguous_format)       # (a copy: a slice of a host tensor need not be 16-byte aligned)


def from_layout(o, layout):
    o = o.cpu()
    if layout == "ndhwc":
        return o.permute(0, 4, 1, 2, 3).contiguous()
    if layout == "p4":
        N, Q, D, H, W, _ = o.shape
        return o.permute(0, 1, 5, 2, 3, 4).reshape(N, 4 * Q, D, H, W).contiguous()
    return o


def lattice(dims):
    return [torch.linspace(-1, 1, n) for n in dims]


def coordinates(N, out, mode, gen):
    """(kwargs of ops.grid_sample3d on the host, the materialised grid [N,Do,Ho,Wo,3]): a near-identity lattice + 0.6 tanh(randn),
    so a good share of the corners lie outside the volume"""
    Do, Ho, Wo = out
    lz, ly, lx = lattice(out)
    if mode == "theta":
        a = torch.rand(N, generator=gen) - 0.5
        theta = torch.eye(4)[None, :3].repeat(N, 1, 1)
        theta[:, 0, 0], theta[:, 0, 1], theta[:, 1, 0], theta[:, 1, 1] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a)
        theta = theta * (1 + 0.3 * torch.tanh(torch.randn(N, 1, 1, generator=gen)))
        theta[:, :, 3] = 0.6 * torch.tanh(torch.randn(N, 3, generator=gen))
        grid = torch.from_numpy(c_oracle.affine_grid3d(theta.numpy(), lx.numpy(), ly.numpy(), lz.numpy()))
        return dict(theta=theta), grid
    zz, yy, xx = torch.meshgrid(lz, ly, lx, indexing="ij")
    ident = torch.stack([xx, yy, zz], 0)[None]                                     # [1,3,Do,Ho,Wo]
    delta = 0.6 * torch.tanh(torch.randn(N, 3, Do, Ho, Wo, generator=gen))
    grid = (ident + delta).permute(0, 2, 3, 4, 1).contiguous()
    return (dict(delta=delta) if mode == "delta" else dict(grid=grid)), grid


def expect_form(c, mode, vol_addr, out_addr):
    """the library reports the form and the plan the case names"""
    rc, plan = hip.sampler_launch_form(vol_addr, out_addr, c["N"], c["C"], L.vol_dims(c, mode), c["out"], "zeros", c["in_layout"],
                                       c["out_layout"], c["variant"], mode, c["shared"], c["index"] is not None)
    assert rc == 0 and plan["form"] == c["form"], (c["id"], mode, rc, plan)
    got = {k: plan[k] for k in c["plan"]}
    assert got == c["plan"], (c["id"], mode, got, plan)
    L.plan_edges(plan, c)
    return plan


def sample(vols, c, pm, dev, kw, index=None, **over):
    """one ops.grid_sample3d call of case c on host volumes [Nv,C,D,H,W]; returns NCDHW on the host"""
    a = dict(in_layout=c["in_layout"], out_layout=c["out_layout"], variant=c["variant"])
    a.update(over)
    v = to_layout(vols, a["in_layout"]).to(dev)
    k = {n: t.to(dev) for n, t in kw.items()}
    if index is not None:
        k["vol_index"] = torch.tensor(index, dtype=torch.int32).to(dev)
    o = ops.grid_sample3d(v, padding_mode=pm, **a, **k)
    return from_layout(o, a["out_layout"])


def run_case(c, pm, mode, dev):
    """query, launch, compare with ATen; returns the FMA error as a fraction of its bound (None: a bit-exact form)"""
    gen = _gen(c["id"], pm, mode)
    N, C = c["N"], c["C"]
    Nv = c["K"] if c["index"] is not None else 1 if c["shared"] else N
    vols = torch.randn(Nv, C, *L.vol_dims(c, mode), generator=gen)
    kw, grid = coordinates(N, c["out"], mode, gen)
    probe = to_layout(vols[:1], c["in_layout"]).to(dev)
    plan = expect_form(c, mode, probe.data_ptr(), probe.data_ptr())
    per_sample = vols[c["index"]] if c["index"] is not None else vols.expand(N, -1, -1, -1, -1) if c["shared"] else vols
    ref = F.grid_sample(per_sample, grid, padding_mode=pm, align_corners=False)
    got = sample(vols, c, pm, dev, kw, c["index"])
    what = f"{c['id']} {pm} {mode}"
    if not plan["fma"]:
        same_bits(got, ref, what)
        return None
    # FMA: the taps are ATen's, the values differ by the skipped product roundings
    assert not torch.isnan(got).any(), f"{what}: poison left in the output"
    err = (got - ref).abs().max().item() / (FMA_BOUND * vols.abs().max().item())
    print(f"PARITY sampler form [{what}]: FMA error {err:.3f} of the bound, order {plan['order']}")
    assert err <= 1.0, (what, err)
    if plan["order"] == 3:
        # the same FMA call on per-sample copies of the volume takes ORDER 1: the block order is the only difference
        own = dict(c, shared=False)
        assert expect_form(dict(own, plan=dict(order=1, fma=1)), mode, probe.data_ptr(), probe.data_ptr())["order"] == 1
        same_bits(got, sample(per_sample.contiguous(), own, pm, dev, kw), what + " against ORDER 1")
    return err


def run_family(family, pm, mode, dev, skip_slow=False):
    worst = None
    for c in L.FAMILIES[family]:
        if skip_slow and c["slow"]:
            continue
        if mode == "theta" and c["form"] == "tile_planar" and c["out"][2] % 4:
            continue
        e = run_case(c, pm, mode, dev)
        worst = e if worst is None or (e is not None and e > worst) else worst
    if worst is not None:
        print(f"PARITY sampler family {family} {pm} {mode}: worst FMA error {worst:.3f} of 8 * 2^-24 * max|vol|")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pm", PADS)
@pytest.mark.parametrize("family", list(L.FAMILIES))
def test_form_cases(family, pm, mode):
    run_family(family, pm, mode, DEV)


def run_refusals(dev, refused=None):
    for c, code in L.REFUSED if refused is None else refused:
        q = hip.sampler_launch_form(4096, 4096, c["N"], c["C"], c["vol"], c["out"], "zeros", c["in_layout"], c["out_layout"], c["variant"],
                                    "grid", c["shared"], c["index"] is not None)
        assert q == (code, None), (c["id"], q)
        if c["index"] is not None:
            continue                                            # (ops raises a ValueError of its own for a bank in these layouts)
        gen = _gen(c["id"])
        vols = torch.randn(c["N"], c["C"], *c["vol"], generator=gen)
        kw, _ = coordinates(c["N"], c["out"], "grid", gen)
        with pytest.raises(RuntimeError, match="BAD_ARG" if code == L.BAD_ARG else "UNSUPPORTED"):
            sample(vols, c, "zeros", dev, kw)


def test_refused_cases_are_reported_and_refused(guarded_outputs):
    run_refusals(DEV)


# ---- the bank: frames against the plain entry, indices out of range ------------------------------------------------------------
BANKED = [c for cs in L.FAMILIES.values() for c in cs if c["index"] is not None]
OUT_OF_RANGE = [-1, 1, 3, L.INT32_MIN, 0, L.INT32_MAX]          # K = 3


def guarded_bank(vols, layout, dev):
    """the bank [K,...] in `layout` between two runs of GUARD NaN floats in one device buffer: (whole buffer, bank view)"""
    b = to_layout(vols, layout)
    whole = torch.full((2 * GUARD + b.numel(),), float("nan"))
    whole[GUARD:GUARD + b.numel()] = b.reshape(-1)
    whole = whole.to(dev)
    return whole, whole[GUARD:GUARD + b.numel()].view(b.shape)


def run_bank(c, pm, dev):
    gen = _gen("bank", c["id"], pm)
    K, C = c["K"], c["C"]
    vols = torch.randn(K, C, *c["vol"], generator=gen)
    a = dict(padding_mode=pm, in_layout=c["in_layout"], out_layout=c["out_layout"], variant=c["variant"])
    for index in (c["index"], OUT_OF_RANGE):
        N = len(index)
        kw, grid = coordinates(N, c["out"], "delta", gen)
        whole, bank = guarded_bank(vols, c["in_layout"], dev)
        delta = kw["delta"].to(dev)
        got = ops.grid_sample3d(bank, delta=delta, vol_index=torch.tensor(index, dtype=torch.int32).to(dev), **a).cpu()
        for n, i in enumerate(index):
            if 0 <= i < K:      # the plain entry on the frame's own volume: bit for bit (and with it ATen, or the FMA bound)
                one = ops.grid_sample3d(to_layout(vols[i:i + 1], c["in_layout"]).to(dev), delta=delta[n:n + 1].contiguous(), **a).cpu()
                same_bits(got[n:n + 1], one, f"{c['id']} {pm} frame {n} of volume {i}")
                ref = F.grid_sample(vols[i:i + 1], grid[n:n + 1], padding_mode=pm, align_corners=False)
                o = from_layout(one, c["out_layout"])
                if c["variant"] & 4 and c["form"] != "brick":
                    assert (o - ref).abs().max().item() <= FMA_BOUND * vols.abs().max().item()
                else:
                    same_bits(o, ref, f"{c['id']} {pm} frame {n} against ATen")
            else:
                same_bits(got[n], torch.zeros_like(got[n]), f"{c['id']} {pm} frame {n} of index {i}: all zero")
        w = whole.cpu()
        assert torch.isnan(w[:GUARD]).all() and torch.isnan(w[-GUARD:]).all()
        assert not torch.isnan(got).any(), "a read of the guards (or poison) reached the output"


@pytest.mark.parametrize("pm", PADS)
@pytest.mark.parametrize("c", BANKED, ids=L.ids(BANKED))
def test_banked_forms_frame_by_frame_and_out_of_range_indices(c, pm):
    run_bank(c, pm, DEV)


# ---- coordinate edges --------------------------------------------------------------------------------------------------------
EDGE_VALUES = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 5e9, -5e9, 3e9, -3e9, 1e4, -1e4, 7.3, -7.3, 3.0, -3.0, 1.0, -1.0,
               0.75, -0.75, 2.0 ** -140, -0.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24)]
EDGE_VOLUMES = [(2, 3, 4), (1, 1, 1), (1, 5, 8)]
EDGE_OUT = (4, 8, 8)                # 256 points (a lattice of bricks): 69 with one planted axis, 69 with two, the rest random
# one call of every family: (in_layout, out_layout, variant)
EDGE_CALLS = [("planar", "ncdhw", "ncdhw", 0), ("rows", "ndhwc", "ndhwc", 0), ("rows_ncdhw", "ndhwc", "ncdhw", 0),
              ("brick", "ndhwc", "ndhwc", 1), ("tile_p4", "p4", "p4", 0), ("tile_planar", "ncdhw", "ncdhw", L.TILE)]


def edge_grid(gen):
    """[1, 4, 8, 8, 3]: random coordinates in [-1.3, 1.3] with every edge value planted on each axis alone and on each pair of axes
    (the second axis takes the next value of the list)"""
    g = (torch.rand(256, 3, generator=gen) * 2.6 - 1.3)
    v = torch.tensor(EDGE_VALUES, dtype=torch.float32)
    assert v[-3].item() == 0.0 and np.signbit(v[-3].numpy()) and v[-4].item() == 2.0 ** -140     # -0.0 and the subnormal survive
    p = 0
    for axis in range(3):
        for i in range(len(v)):
            g[p, axis] = v[i]
            p += 1
    for a, b in ((0, 1), (1, 2), (0, 2)):
        for i in range(len(v)):
            g[p, a], g[p, b] = v[i], v[(i + 1) % len(v)]
            p += 1
    assert p == 138
    return g.view(1, *EDGE_OUT, 3)


def run_edges(dims, pm, dev, calls=EDGE_CALLS):
    gen = _gen("edges", dims, pm)
    vol = torch.randn(1, 4, *dims, generator=gen)
    grid = edge_grid(gen)
    ref = F.grid_sample(vol, grid, padding_mode=pm, align_corners=False)
    assert not torch.isnan(ref).any()                           # (ATen's CPU kernel on this list: checked, and deterministic)
    D, H, W = dims
    for form, il, ol, variant in calls:
        rc, plan = hip.sampler_launch_form(4096, 4096, 1, 4, dims, EDGE_OUT, pm, il, ol, variant, "grid")
        want = "planar" if form == "tile_planar" and W % 4 else form          # (rows of W floats must be 16-byte multiples)
        assert rc == 0 and plan["form"] == want, (form, dims, rc, plan)
        got = from_layout(ops.grid_sample3d(to_layout(vol, il).to(dev), grid.to(dev), padding_mode=pm, in_layout=il, out_layout=ol,
                                            variant=variant), ol)
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{form} {dims} {pm}: NaN mask"
        same_bits(got, ref, f"{form} {dims} {pm} coordinate edges")


@pytest.mark.parametrize("pm", PADS)
@pytest.mark.parametrize("dims", EDGE_VOLUMES, ids=lambda d: "x".join(map(str, d)))
def test_coordinate_edges(dims, pm):
    """non-finite, absurd, multiply reflected, boundary, subnormal and signed-zero coordinates sample what ATen samples.  Reflection
    at |g| >= 2^32 (5e9, 1e30): the number of flips passes 2^31 and its parity must not come from a saturating conversion"""
    run_edges(dims, pm, DEV)


# ---- repack kernels and affine_grid3d ----------------------------------------------------------------------------------------
def planted(shape, gen):
    """random floats with NaN payloads, -0.0, subnormals, infinities and the poison's own pattern planted: a repack moves bits"""
    x = torch.randn(*shape, generator=gen)
    special = torch.tensor([0x7fc00001, 0x7f800123, -0x00000001, -0x80000000, 0x00000001, -0x7fffffff, 0x7f800000, -0x00800000, 0x007fffff],
                           dtype=torch.int32)
    flat = bits(x).view(-1)
    pos = torch.randperm(flat.numel(), generator=gen)[:min(flat.numel(), 4 * len(special))]
    flat[pos] = special.repeat(4)[:len(pos)]
    return flat.view(torch.float32).view(shape)


def repack_query(c, a=4096):
    return hip.repack_launch_form(a, a, c["N"], c["C"], c["DHW"], c["to_channels_last"], c["indexed"])


def run_repack(c, dev):
    gen = _gen("repack", c["id"])
    N, C, S, d = c["N"], c["C"], c["DHW"], c["direction"]
    rc, plan = repack_query(c)
    assert rc == 0 and plan == dict(c["plan"], direction=d), (c["id"], rc, plan)
    x = planted((N, C, 1, 1, S), gen)                           # NCDHW, D = H = 1
    if d == "to_channels_last":
        got, want = ops.volume_to_channels_last(x.to(dev)), to_layout(x, "ndhwc")
    elif d == "from_channels_last":
        got, want = ops.volume_to_channels_first(to_layout(x, "ndhwc").to(dev)), x
    elif d == "to_p4":
        got, want = ops.volume_to_p4(x.to(dev)), to_layout(x, "p4")
    elif d == "from_p4":
        got, want = ops.volume_from_p4(to_layout(x, "p4").to(dev)), x
    else:
        # indexed: K = 4 rows pre-filled; volumes 0 and 2 land in rows 3 and 1, volume 1 names a row outside [0, 4)
        for rows in ([3, -1, 1], [3, 4, 1], [3, L.INT32_MIN, 1], [3, L.INT32_MAX, 1]):
            fill = planted((4, 1, 1, S, C), gen)
            bank = ops.torch.empty((4, 1, 1, S, C), device=dev, dtype=torch.float32).copy_(fill)
            ops.volume_to_channels_last_indexed(x.to(dev), bank, torch.tensor(rows, dtype=torch.int32).to(dev))
            want = fill.clone()
            want[3], want[1] = to_layout(x[0:1], "ndhwc")[0], to_layout(x[2:3], "ndhwc")[0]
            same_bits(bank.cpu(), want, f"{c['id']} rows {rows}")
        return
    same_bits(got.cpu(), want, c["id"])


@pytest.mark.parametrize("c", L.REPACK, ids=L.ids(L.REPACK))
def test_repack_is_the_exact_permutation(c):
    run_repack(c, DEV)


def run_repack_refusals(dev, refused=None, launch_limit=1 << 20):
    """the query refuses, and so does the entry, before any launch: the poisoned output keeps its poison"""
    lib = hip.load()
    for c, code in L.REPACK_REFUSED if refused is None else refused:
        assert repack_query(c) == (code, None), c["id"]
        n = c["N"] * c["C"] * c["DHW"]
        x = torch.zeros(min(n, launch_limit)).to(dev)           # (refused from the integers alone: nothing is read or written)
        out = ops.torch.empty(min(n, launch_limit), device=dev, dtype=torch.float32)
        if c["indexed"]:
            rc = lib.emo_volume_repack_indexed_f32(hip.ptr(x), hip.ptr(out), hip.ptr(torch.zeros(1, dtype=torch.int32).to(dev)), c["N"], c["C"],
                                                   c["DHW"], 1, hip.current_stream())
        else:
            rc = lib.emo_volume_repack_f32(hip.ptr(x), hip.ptr(out), c["N"], c["C"], c["DHW"], c["to_channels_last"], hip.current_stream())
        assert rc == code, (c["id"], rc)
        assert torch.isnan(out).all(), c["id"]


def test_repack_refusals_launch_nothing():
    run_repack_refusals(DEV)
    # one tile row short of the refusal runs: 65535 tiles of rows
    c = L.REPACK_LAST_ROW_TILE
    rc, plan = repack_query(c)
    assert rc == 0 and plan["grid_y"] == 65535, (rc, plan)
    x = torch.randn(1, c["DHW"], 1, 1, c["C"], generator=_gen("last row tile"))       # [N, D, H, W, C] with C = 1
    same_bits(ops.volume_to_channels_first(x.to(DEV)).cpu(), x.permute(0, 4, 1, 2, 3).contiguous(), c["id"])


@pytest.mark.parametrize("size", [(3, 5, 7), (3, 10, 11), (1, 1, 1)], ids=lambda d: "x".join(map(str, d)))
def test_affine_grid3d_equals_the_oracle_bit_for_bit(size):
    run_affine_grid(size, DEV)


def run_affine_grid(size, dev):
    """N = 3; 105 and 330 voxels are no multiples of the block's 256, 330 spans two blocks"""
    kw, grid = coordinates(3, size, "theta", _gen("affine", size))
    same_bits(ops.affine_grid3d(kw["theta"].to(dev), size).cpu(), grid, f"affine_grid3d {size}")


# ---- the redirect of ops.grid_sample3d -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,dims,path", [(232, (5, 30, 32), "rows_ncdhw"), (236, (5, 30, 32), "planar"), (12, (16, 74, 74), "planar")])
def test_reference_call_shape_redirect(C, dims, path, monkeypatch):
    """grid_sample3d(NCDHW, grid) -> NCDHW on a volume of 2^20 elements or more goes through the channels-last kernel where that
    kernel takes it: C = 232 is the last channel count whose transposition tile fits the LDS; C = 236 and C = 12 (< 16) run the
    planar gather.  Bit-exact either way"""
    gen = _gen("redirect", C)
    assert C * dims[0] * dims[1] * dims[2] >= 1 << 20
    vol = torch.randn(1, C, *dims, generator=gen)
    kw, grid = coordinates(1, (3, 9, 11), "grid", gen)
    a = 4096
    rc_cl, plan_cl = hip.sampler_launch_form(a, a, 1, C, dims, (3, 9, 11), "zeros", "ndhwc", "ncdhw", 0, "grid")
    rc_pl, plan_pl = hip.sampler_launch_form(a, a, 1, C, dims, (3, 9, 11), "zeros", "ncdhw", "ncdhw", 0, "grid")
    assert rc_pl == 0 and plan_pl["form"] == "planar"
    assert (rc_cl, plan_cl and plan_cl["form"]) == ((0, "rows_ncdhw") if C != 236 else (L.UNSUPPORTED, None))
    forms, lib = [], hip.load()

    class Spy:
        """the library, recording what the sampler entry is asked for: the query's answer for the call's own arguments"""
        def __getattr__(self, name):
            return getattr(lib, name)

        def emo_grid_sample3d_f32(self, *args):
            layouts = {hip.LAYOUT_NCDHW: "ncdhw", hip.LAYOUT_NDHWC: "ndhwc"}
            q = hip.sampler_launch_form(args[0].value, args[6].value, args[7], args[8], args[9:12], args[12:15], "zeros", layouts[args[17]],
                                        layouts[args[18]], args[19], "grid", shared=args[15] == 0)
            forms.append(q[1]["form"])
            return lib.emo_grid_sample3d_f32(*args)
    monkeypatch.setattr(hip, "load", lambda: Spy())
    got = ops.grid_sample3d(vol.to(DEV), grid.to(DEV)).cpu()
    assert forms == [path], forms
    same_bits(got, F.grid_sample(vol, grid, align_corners=False), f"redirect C {C}")


# ---- the lists against the C enums and the plan edges --------------------------------------------------------------------------
def coverage(a=4096):
    """every form of the C enum and every required edge has a case, every case reports the form and plan it declares, every
    refusal is reported; the repack cases reach every direction with every required size in rows and in columns"""
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    found = re.findall(r"EMO_GS3D_FORM_([A-Z0-9_]+) = (\d+)", hdr)
    names = tuple(n.lower() for n, v in sorted(found, key=lambda nv: int(nv[1])) if n != "COUNT")
    assert names == hip.GS3D_FORMS and dict(found)["COUNT"] == str(len(names)), "hip.GS3D_FORMS out of step with include/emo_hip.h"
    edges = set()
    for family, cases in L.FAMILIES.items():
        for c in cases:
            for mode in MODES:
                if mode == "theta" and c["form"] == "tile_planar" and c["out"][2] % 4:
                    continue
                edges |= L.plan_edges(expect_form(c, mode, a, a), c)
    want = L.REQUIRED_EDGES | {"form " + f for f in names}
    assert want <= edges, f"no case for {sorted(want - edges)}"
    assert {e for e in edges if e.startswith("form ")} <= {"form " + f for f in names}
    for c, code in L.REFUSED:
        q = hip.sampler_launch_form(a, a, c["N"], c["C"], c["vol"], c["out"], "zeros", c["in_layout"], c["out_layout"], c["variant"], "grid",
                                    c["shared"], c["index"] is not None)
        assert q == (code, None), (c["id"], q)
    assert L.REQUIRED_REFUSALS <= {c["id"] for c, _ in L.REFUSED}
    assert hip.sampler_launch_form(a + 4, a, 2, 4, L.VOL, (2, 5, 7)) == (-3, None) and hip.sampler_launch_form(None, a, 2, 4, L.VOL, (2, 5, 7))[0] == -1
    return sorted(edges)


def repack_coverage():
    dirs = set()
    for c in L.REPACK:
        rc, plan = repack_query(c)
        assert rc == 0 and plan == dict(c["plan"], direction=c["direction"]), (c["id"], rc, plan)
        dirs.add(c["direction"])
    assert dirs == set(hip.REPACK_DIRECTIONS), dirs
    for d in ("to_channels_last", "from_channels_last", "to_channels_last_indexed"):
        for key in ("C", "DHW"):
            assert {c[key] for c in L.REPACK if c["direction"] == d} >= L.REPACK_REQUIRED_SIZES, (d, key)
        assert all(c["N"] > 1 for c in L.REPACK)
    for c, code in L.REPACK_REFUSED:
        assert repack_query(c) == (code, None), c["id"]
    assert any(not c["indexed"] and c["to_channels_last"] == 0 and -(-c["DHW"] // 64) > 65535 for c, _ in L.REPACK_REFUSED)
    return sorted(dirs)


def test_cases_cover_every_form_and_every_required_edge(guarded_outputs):
    guarded_outputs.may_serve_nothing("asks the two launch-form entry points about every case; nothing is launched")
    print("PARITY sampler launch form coverage:", coverage(), repack_coverage())
