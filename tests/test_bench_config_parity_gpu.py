"""GPU parity on the EXACT configuration bench.py times (BASELINE.json headline: R512, 16 driver frames per step) and on
the other R512 graphs that only existed at R256 in the round-1 tests:

  * R512 driver pass at B = 16 (the launch plan -- block config and K split, pack.plan_launch -- depends on the batch, so
    the kernels BENCH times are these and not the B = 1 ones): frames 0, 7, 15 of the batch against the oracle run
    frame by frame, end to end and stage-wise;
  * R512 source pass (LocalEncoder with from_rgb_512px + 3 encoder blocks: a different graph from R256,
    networks/volumetric_avatar/local_encoder.py:48-125);
  * stage 2 at 512^2 (notebooks/infer_s2.py:351-376);
  * the fused head-pose warp (theta applied in-kernel) against the reference's identity_grid.bmm(theta^T) grid on the
    SURVEY.md section 8(d) theta distribution: how far the coordinates differ, how many lattice points change floor(), and
    what that does to the sampled volume.

Tolerances are the ones of tests/test_nets_gpu.py (stage-wise 5e-5 of max / image 5e-4 abs; end to end 1e-3 / 5e-3 abs);
measured values are printed as PARITY lines and collected into profiles/r<round>_parity.txt (tools/collect_profiles.py).
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import restate as O  # noqa: E402

from emoportraits_amd import nets, ops, stage2  # noqa: E402
from test_nets_gpu import _full_size, rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_driver_pass_R512_B16_bench_configuration_vs_oracle():
    B, frames = 16, (0, 7, 15)
    cfg, sd, x = _full_size(512, B, seed=512)
    hp = nets.HotPath(sd, cfg, DEV, with_source=False)
    d = lambda t: t.to(DEV)
    ccl = hp.prepare_canonical(d(x["canonical"]))
    got = hp.driver_pass(ccl, d(x["idt"]), d(x["pose_t"]), d(x["th_t"]), keep=True)
    torch.cuda.synchronize()
    # stage-wise at B = 16: the decoder fed with the HIP path's own `aligned` batch; the oracle decodes the same rows
    dimg, dfeat, dimgf = hp.decoder(got["aligned"].view(B, -1, 64, 64))
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    worst = {}
    for i in frames:
        with torch.no_grad():
            ref = O.driver_pass(sd, cfg, x["canonical"], x["idt"], x["pose_t"][i:i + 1], x["th_t"][i:i + 1])
            r_img, r_feat, r_imgf = O.decoder(sd, "decoder_nw", got["aligned"][i:i + 1].cpu().reshape(1, -1, 64, 64), cfg)
        e = dict(warp_embed=rel(got["warp_embed"][i:i + 1], ref["warp_embed"]),
                 delta_abs=(got["delta_uv"][i:i + 1].cpu() - ref["delta_uv"]).abs().max().item(),
                 aligned=rel(got["aligned"][i:i + 1], ref["aligned"]), deep_f=rel(got["deep_f"][i:i + 1], ref["deep_f"]),
                 img_f=rel(got["img_f"][i:i + 1], ref["img_f"]),
                 img_abs=(got["img"][i:i + 1].cpu() - ref["img"]).abs().max().item(),
                 sw_deep_f=rel(dfeat[i:i + 1], r_feat), sw_img_f=rel(dimgf[i:i + 1], r_imgf),
                 sw_img_abs=(dimg[i:i + 1].cpu() - r_img).abs().max().item())
        print(f"PARITY R512 B=16 (bench configuration) frame {i}:", {k: f"{v:.2e}" for k, v in e.items()})
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert worst["warp_embed"] <= 1e-5 and worst["delta_abs"] <= 1e-4, worst
    assert worst["sw_deep_f"] <= 5e-5 and worst["sw_img_f"] <= 5e-5 and worst["sw_img_abs"] <= 5e-4, worst
    assert worst["aligned"] <= 1e-3 and worst["deep_f"] <= 1e-3 and worst["img_f"] <= 1e-3 and worst["img_abs"] <= 5e-3, worst
    # the stage-wise decoder call and the one inside driver_pass are the same launches on the same input
    assert torch.equal(dimg, got["img"])


def test_driver_pass_R256_B32_bench_configuration_vs_oracle():
    """bench.py also times the R256 driver pass, at 32 frames per call (r256_fps): a launch plan of its own (the plan is a function
    of size and batch; the decoder runs 256 / 160 / 96 channels there).  Frames 0 and 31 of the batch against the oracle run
    frame by frame, with the structure and the bounds of the R512 test above."""
    B, frames = 32, (0, 31)
    cfg, sd, x = _full_size(256, B, seed=256)
    hp = nets.HotPath(sd, cfg, DEV, with_source=False)
    d = lambda t: t.to(DEV)
    ccl = hp.prepare_canonical(d(x["canonical"]))
    got = hp.driver_pass(ccl, d(x["idt"]), d(x["pose_t"]), d(x["th_t"]), keep=True)
    torch.cuda.synchronize()
    dimg, dfeat, dimgf = hp.decoder(got["aligned"].view(B, -1, 64, 64))
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    worst = {}
    for i in frames:
        with torch.no_grad():
            ref = O.driver_pass(sd, cfg, x["canonical"], x["idt"], x["pose_t"][i:i + 1], x["th_t"][i:i + 1])
            r_img, r_feat, r_imgf = O.decoder(sd, "decoder_nw", got["aligned"][i:i + 1].cpu().reshape(1, -1, 64, 64), cfg)
        e = dict(warp_embed=rel(got["warp_embed"][i:i + 1], ref["warp_embed"]),
                 delta_abs=(got["delta_uv"][i:i + 1].cpu() - ref["delta_uv"]).abs().max().item(),
                 aligned=rel(got["aligned"][i:i + 1], ref["aligned"]), deep_f=rel(got["deep_f"][i:i + 1], ref["deep_f"]),
                 img_f=rel(got["img_f"][i:i + 1], ref["img_f"]),
                 img_abs=(got["img"][i:i + 1].cpu() - ref["img"]).abs().max().item(),
                 sw_deep_f=rel(dfeat[i:i + 1], r_feat), sw_img_f=rel(dimgf[i:i + 1], r_imgf),
                 sw_img_abs=(dimg[i:i + 1].cpu() - r_img).abs().max().item())
        print(f"PARITY R256 B=32 (bench configuration) frame {i}:", {k: f"{v:.2e}" for k, v in e.items()})
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert worst["warp_embed"] <= 1e-5 and worst["delta_abs"] <= 1e-4, worst
    assert worst["sw_deep_f"] <= 5e-5 and worst["sw_img_f"] <= 5e-5 and worst["sw_img_abs"] <= 5e-4, worst
    assert worst["aligned"] <= 1e-3 and worst["deep_f"] <= 1e-3 and worst["img_f"] <= 1e-3 and worst["img_abs"] <= 5e-3, worst
    assert torch.equal(dimg, got["img"])


def test_driver_pass_R512_B16_trained_like_checkpoint_vs_oracle():
    """The bench's own checkpoint (random_init.trained_like_state_dict: spectral norms ~1, predicted warp within one voxel of
    the identity, unsaturated image -- the released weights are not obtainable) at the bench's launch plan (B = 16): frames
    0 / 7 / 15 end to end against the oracle, as fp32 images and as the uint8 frames the wrapper hands out, and the same
    frames through batch-1 calls (a different launch plan: K split, tile choice)."""
    from emoportraits_amd import config, random_init
    B, frames = 16, (0, 7, 15)
    cfg = config.hot_path_config(overrides={"image_size": 512})
    sd = random_init.trained_like_state_dict(cfg, seed=0, with_source=False)
    _, _, x = _full_size(512, B, seed=512)
    d = lambda t: t.to(DEV)
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    refs = {}
    for i in frames:
        with torch.no_grad():
            refs[i] = O.driver_pass(sd, cfg, x["canonical"], x["idt"], x["pose_t"][i:i + 1], x["th_t"][i:i + 1])
    # every fp32 conv mode is held to the same bound: the default (f16x2: the device-checked two-term fp16 split), the exact
    # three-term bf16 split, and the exact-fp32 MFMA kernel everywhere
    for mode in (None, "bf16x3", "f32"):
        hp = nets.HotPath(sd, cfg, DEV, with_source=False, precision=mode)
        ccl = hp.prepare_canonical(d(x["canonical"]))
        got = hp.driver_pass(ccl, d(x["idt"]), d(x["pose_t"]), d(x["th_t"]), keep=True)
        u8 = ops.pack_rgb8(got["img"]).cpu()
        worst = dict(img_abs=0.0, u8_same=1.0, batch1_abs=0.0, delta_vox=0.0, saturated=0.0)
        for i in frames:
            ref = refs[i]
            one = hp.driver_pass(ccl, d(x["idt"]), d(x["pose_t"][i:i + 1]), d(x["th_t"][i:i + 1]))
            ref_u8 = (ref["img"].clamp(0, 1) * 255.0).round().to(torch.uint8)        # ToPILImage's mul(255).byte() after clamp
            ref_u8_trunc = (ref["img"].clamp(0, 1) * 255.0).to(torch.uint8)
            mine = u8[i:i + 1]
            mine = mine if mine.shape == ref_u8.shape else mine.permute(0, 3, 1, 2)
            same = max((mine == ref_u8).float().mean().item(), (mine == ref_u8_trunc).float().mean().item())
            e = dict(img_abs=(got["img"][i:i + 1].cpu() - ref["img"]).abs().max().item(), u8_same=same,
                     batch1_abs=(one - got["img"][i:i + 1]).abs().max().item(),
                     delta_vox=(ref["delta_uv"].abs().amax(dim=(0, 2, 3, 4)) * torch.tensor([32.0, 32.0, 8.0])).max().item(),
                     saturated=((ref["img"] < 0.02) | (ref["img"] > 0.98)).float().mean().item())
            print(f"PARITY R512 B=16 trained-like checkpoint [{hp.precision}] frame {i}:", {k: f"{v:.3e}" for k, v in e.items()})
            for k in ("img_abs", "batch1_abs", "delta_vox", "saturated"):
                worst[k] = max(worst[k], e[k])
            worst["u8_same"] = min(worst["u8_same"], e["u8_same"])
        assert worst["delta_vox"] < 1.5 and worst["saturated"] < 0.05, worst      # the checkpoint is what it claims to be
        assert worst["img_abs"] <= 2e-4 and worst["batch1_abs"] <= 2e-4 and worst["u8_same"] >= 0.999, (hp.precision, worst)
        if hp.precision == "f16x2":
            assert hp.overflow_events() == {}, "the trained-like checkpoint tripped the fp16 split's range check"
        if mode is not None:
            del hp
    # the opt-in fp16-operand mode (BASELINE configs[4]) on the same checkpoint, same launch plan, against the ORACLE's frames
    # (round 5 compared it with the HIP path's fp32 output): its stated tolerance is 2e-3 mean / 2e-2 worst pixel of the
    # [0, 1] image (decoder operands carry 11 significand bits, accumulation is fp32; the WarpGenerators -- geometry -- run
    # the fp32-accurate fp16 split, nets.HotPath)
    hp16 = nets.HotPath(sd, cfg, DEV, with_source=False, precision="f16")
    assert hp16.warp_precision == os.environ.get("EMO_WARP_PRECISION", "f16x2")
    got16 = hp16.driver_pass(hp16.prepare_canonical(d(x["canonical"])), d(x["idt"]), d(x["pose_t"]), d(x["th_t"]), keep=True)
    img16 = got16["img"].cpu()
    worst16 = dict(max=0.0, mean=0.0, delta_abs=0.0)
    for i in frames:
        e16 = (img16[i:i + 1] - refs[i]["img"]).abs()
        worst16["max"] = max(worst16["max"], e16.max().item())
        worst16["mean"] = max(worst16["mean"], e16.mean().item())
        worst16["delta_abs"] = max(worst16["delta_abs"], (got16["delta_uv"][i:i + 1].cpu() - refs[i]["delta_uv"]).abs().max().item())
    print(f"PARITY R512 B=16 trained-like checkpoint, fp16 operands vs oracle: image worst {worst16['max']:.3e} mean "
          f"{worst16['mean']:.3e}, deltas (fp16 split) {worst16['delta_abs']:.2e}")
    assert worst16["max"] <= 2e-2 and worst16["mean"] <= 2e-3 and worst16["delta_abs"] <= 1e-4, worst16
    assert hp16.overflow_events() == {}, "the WarpGenerators' fp16 split tripped its range check"


def test_source_pass_R512_vs_oracle():
    cfg, sd, x = _full_size(512, 1, seed=21)
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    with torch.no_grad():
        ref = O.source_pass(sd, cfg, x["img"], x["idt"], x["pose_s"], x["th_s"])
    hp = nets.HotPath(sd, cfg, DEV)
    assert len(hp.local_encoder.blocks) == 3 and hp.local_encoder.from_rgb.name.endswith("from_rgb_512px")
    d = lambda t: t.to(DEV)
    got = hp.source_pass(d(x["img"]), d(x["idt"]), d(x["pose_s"]), d(x["th_s"]), keep=True)
    e = dict(latents=rel(got["latents"], ref["latents"]), source_volume=rel(got["source_volume"], ref["source_volume"]),
             pre_canonical=rel(got["pre_canonical"], ref["pre_canonical"]), canonical=rel(got["canonical"], ref["canonical"]))
    # stage-wise: Unet3D alone on the oracle's input
    e["sw_canonical"] = rel(hp.volume_process(d(ref["pre_canonical"])), ref["canonical"])
    print("PARITY source pass R512:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["latents"] <= 1e-4 and e["source_volume"] <= 1e-4 and e["sw_canonical"] <= 1e-4, e
    assert e["pre_canonical"] <= 1e-3 and e["canonical"] <= 1e-3, e


@pytest.mark.parametrize("variant", ["bn", "gn_ws"])
def test_stage2_R512_vs_oracle(variant):
    over = dict(output_size_s2=512)
    if variant == "gn_ws":
        over.update(norm_layer_type="gn", use_ws=True)
    cfg = stage2.stage2_config(overrides=over)
    sd = stage2.random_state_dict(cfg, seed=5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand(1, 3, 512, 512, generator=g)
    mask = (torch.rand(1, 1, 512, 512, generator=g) > 0.1).float()
    face = (torch.rand(1, 1, 512, 512, generator=g) > 0.3).float()
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    with torch.no_grad():
        ref = O.stage2_forward(sd, cfg, img, mask, face)
    s2 = stage2.Stage2(sd, cfg, DEV)
    d = lambda t: t.to(DEV)
    got = s2.refine(d(img), d(mask), d(face), keep=True)
    e = {k: rel(got[k], ref[k]) for k in ("latents", "add")}
    e["out_abs"] = (got["out"].cpu() - ref["out"]).abs().max().item()
    print(f"PARITY stage2 R512 {variant}:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["latents"] <= 5e-5 and e["add"] <= 5e-4 and e["out_abs"] <= 5e-4, e


def test_fused_head_pose_warp_vs_reference_bmm_grid():
    """a2: the reference builds the rotation warp with a GEMM, `identity_grid_3d.bmm(theta[:, :3].transpose(1, 2))`
    (notebooks/infer.py:583-588); here theta is applied inside the sampler (fma chain u*t0 + v*t1 + w*t2 + t3).  With
    identical coordinates the index arithmetic is bit-exact (tests/test_grid_sample_gpu.py); this test bounds what the
    different summation order of the CPU GEMM does to the coordinates on the SURVEY.md section 8(d) theta distribution."""
    N, dd, ss = 64, 16, 64
    g = torch.Generator().manual_seed(3)
    th = O.get_transform_matrix(1 + 0.05 * torch.randn(N, 3, generator=g), 0.3 * torch.randn(N, 3, generator=g),
                                0.05 * torch.randn(N, 3, generator=g))
    ident = O.identity_grid_3d(dd, ss)                                        # [1, d*s*s, 4]
    ref_grid = ident.expand(N, -1, -1).bmm(th[:, :3].transpose(1, 2)).view(N, dd, ss, ss, 3)
    got_grid = ops.affine_grid3d(th.to(DEV), (dd, ss, ss)).cpu()
    # (1) coordinate distance.  |coordinate| <= ~1.7 here, so one ulp of a coordinate is at most 2^-23 = 1.2e-7 (it is smaller
    # near zero, where ulps of the VALUE would say nothing about the sampling position)
    abs_diff = (got_grid.double() - ref_grid.double()).abs().max().item()
    frac_identical = (got_grid == ref_grid).float().mean().item()
    # (2) lattice points whose floor() of the unnormalised index changes on any axis
    size = torch.tensor([ss, ss, dd], dtype=torch.float32)
    unnorm = lambda gr: ((gr + 1) * size - 1) / 2
    flips = (torch.floor(unnorm(got_grid)) != torch.floor(unnorm(ref_grid))).any(-1)
    n_flip = int(flips.sum())
    # (3) what it does to the sampled volume: explicit reference grid vs fused theta, same kernel family
    vol = torch.randn(1, 96, dd, ss, ss, generator=g)
    n_s = 8
    vcl = ops.volume_to_channels_last(vol.to(DEV))
    a = ops.grid_sample3d(vcl, grid=ref_grid[:n_s].contiguous().to(DEV), in_layout="ndhwc", out_layout="ncdhw")
    b = ops.grid_sample3d(vcl, theta=th[:n_s].to(DEV), in_layout="ndhwc", out_layout="ncdhw")
    out_abs = (a - b).abs().max().item()
    cpu = F.grid_sample(vol.expand(n_s, -1, -1, -1, -1), ref_grid[:n_s], align_corners=False)
    assert torch.equal(a.cpu(), cpu), "explicit-grid sampling must stay bit-exact vs ATen"
    print(f"PARITY fused theta warp vs reference bmm grid: {N} thetas x {dd * ss * ss} lattice points: identical coords "
          f"{frac_identical:.4f}, max |diff| {abs_diff:.2e} ({abs_diff / 2.0 ** -23:.2f} x 2^-23), floor() changed at {n_flip} points "
          f"({n_flip / flips.numel():.2e} of all), sampled-output max abs diff {out_abs:.2e} (max|vol| {vol.abs().max().item():.2f})")
    assert abs_diff <= 2.5 * 2.0 ** -23
    assert n_flip <= 1e-4 * flips.numel()
    # a floor() flip moves a sample by <= 2 ulp across a cell boundary, where the trilinear weights are continuous
    assert out_abs <= 1e-4 * vol.abs().max().item()
