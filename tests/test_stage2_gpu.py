"""GPU parity of the stage-2 refinement path against the golden outputs of the real reference
(BatchNorm default flags) and against the oracle (GroupNorm + weight-standardisation variant, R256)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import restate as O  # noqa: E402

from emoportraits_amd import ops, stage2  # noqa: E402
import ops_reference as R  # noqa: E402

from guarded_outputs import guarded_outputs  # noqa: E402,F401  (every output ops allocates: poisoned, between guards)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
DEV = "cuda:0"


def rel(got, ref):
    return (got.detach().cpu().double() - ref.double()).abs().max().item() / (ref.double().abs().max().item() + 1e-30)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return torch.load(os.path.join(golden_dir, "tiny_stage2.pt"), weights_only=False)


def test_compose_kernels():
    g = torch.Generator().manual_seed(0)
    img, add = torch.rand(2, 3, 8, 12, generator=g), torch.randn(2, 3, 8, 12, generator=g)
    m, f = torch.rand(2, 1, 8, 12, generator=g), (torch.rand(2, 1, 8, 12, generator=g) > 0.5).float()
    d = lambda t: t.to(DEV)
    assert R.check_mul_mask(ops.mul_mask(d(img), d(m)), d(img), d(m))["failures"] == []
    assert R.check_stage2_compose(ops.stage2_compose(d(img), d(add), d(m), d(f)), d(img), d(add), d(m), d(f))["failures"] == []


def test_stage2_batchnorm_default_flags_vs_reference_golden(tiny):
    cfg = stage2.stage2_config(tiny["cfg"])
    s2 = stage2.Stage2(tiny["state_dict"], cfg, DEV)
    d = lambda t: t.to(DEV)
    got = s2.refine(d(tiny["img"]), d(tiny["mask"]), d(tiny["face_mask"]), keep=True)
    e = {k: rel(got[k], tiny[k]) for k in ("latents", "add")}
    e["out_abs"] = (got["out"].cpu() - tiny["out"]).abs().max().item()
    print("PARITY stage2 tiny golden (bn):", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["latents"] <= 5e-5 and e["add"] <= 2e-4 and e["out_abs"] <= 2e-4, e


@pytest.mark.parametrize("variant", ["gn_ws", "bn"])
def test_stage2_r256_vs_oracle(variant):
    over = dict(output_size_s2=256)
    if variant == "gn_ws":
        over.update(norm_layer_type="gn", use_ws=True)
    cfg = stage2.stage2_config(overrides=over)
    sd = stage2.random_state_dict(cfg, seed=3)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 256, 256, generator=g)
    mask = (torch.rand(2, 1, 256, 256, generator=g) > 0.1).float()
    face = (torch.rand(2, 1, 256, 256, generator=g) > 0.3).float()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        ref = O.stage2_forward(sd, cfg, img, mask, face)
    s2 = stage2.Stage2(sd, cfg, DEV)
    d = lambda t: t.to(DEV)
    got = s2.refine(d(img), d(mask), d(face), keep=True)
    e = {k: rel(got[k], ref[k]) for k in ("latents", "add")}
    e["out_abs"] = (got["out"].cpu() - ref["out"]).abs().max().item()
    print(f"PARITY stage2 R256 {variant}:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["latents"] <= 5e-5 and e["add"] <= 5e-4 and e["out_abs"] <= 5e-4, e


@pytest.mark.parametrize("variant", ["bn", "gn_ws"])
def test_stage2_fp16_operand_mode_vs_oracle(variant):
    """BASELINE.json configs[4]: stage-2 refinement with fp16 MFMA convs (opt-in `precision="f16"`: fp16 operands, fp32
    accumulation, fp32 tensors).  Measured against the fp32 oracle on seeded random weights -- the worst case for this
    mode: nothing in a random network damps the 2^-11 operand rounding, and the weight-standardised layers amplify it
    (the fp32 path shows the same gain on its 1e-7 rounding noise).  BatchNorm (the stage-2 default flags): residual
    1.2e-3 of max, refined image 5.3e-4 worst pixel / 5.6e-5 mean; GroupNorm + WS variant: 5.7e-2 worst pixel / 6.6e-4 mean.
    Bounds below are those measurements with margin."""
    over = dict(output_size_s2=256)
    if variant == "gn_ws":
        over.update(norm_layer_type="gn", use_ws=True)
    cfg = stage2.stage2_config(overrides=over)
    sd = stage2.random_state_dict(cfg, seed=3)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 256, 256, generator=g)
    mask = (torch.rand(2, 1, 256, 256, generator=g) > 0.1).float()
    face = (torch.rand(2, 1, 256, 256, generator=g) > 0.3).float()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        ref = O.stage2_forward(sd, cfg, img, mask, face)
    s2 = stage2.Stage2(sd, cfg, DEV, precision="f16")
    assert s2.decoder.trunk[0].conv1.precision == "f16" and s2.decoder.head.precision == "f32"   # 3-channel head stays fp32
    d = lambda t: t.to(DEV)
    got = s2.refine(d(img), d(mask), d(face), keep=True)
    e = {k: rel(got[k], ref[k]) for k in ("latents", "add")}
    e["out_abs"] = (got["out"].cpu() - ref["out"]).abs().max().item()
    e["out_mean_abs"] = (got["out"].cpu() - ref["out"]).abs().mean().item()
    print(f"PARITY stage2 R256 {variant} fp16 operands:", {k: f"{v:.2e}" for k, v in e.items()})
    bound = dict(bn=(5e-3, 5e-4), gn_ws=(2e-1, 5e-3))[variant]
    assert e["latents"] <= 5e-3 and e["out_abs"] <= bound[0] and e["out_mean_abs"] <= bound[1], e


def test_stage2_wrapper_and_strict_loading(tmp_path, tiny):
    from notebooks.infer_s2 import InferenceWrapper
    exp = tmp_path / "logs_s2" / "exp2"
    (exp / "checkpoints").mkdir(parents=True)
    with open(exp / "args.txt", "wt") as f:
        for k, v in tiny["cfg"].items():
            f.write(f"{k}: {v}\n")
    torch.save(tiny["state_dict"], exp / "checkpoints" / "m.pth")
    w = InferenceWrapper(experiment_name="exp2", model_file_name="m.pth", project_dir=str(tmp_path))
    a, b, ffhq, mask = w.forward(tiny["img"], mask=tiny["mask"], face_mask=tiny["face_mask"])
    assert ffhq.dtype == torch.uint8 and ffhq.shape == (2, 64, 64, 3)
    want = tiny["out"].clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1)
    assert (ffhq.cpu().int() - want.int()).abs().max().item() <= 1
    with pytest.raises(RuntimeError, match="matte"):
        w.forward(tiny["img"])
    bad = dict(tiny["state_dict"])
    bad.pop("decoder.res_decoder.0.weight_u")
    with pytest.raises(KeyError, match="missing"):
        InferenceWrapper(experiment_name="exp2", model_file_name="m.pth", project_dir=str(tmp_path), state_dict=bad)
