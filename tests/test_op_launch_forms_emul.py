"""The launch forms of the pointwise and resampling ops without a GPU: the cases of tests/op_launch_forms.py, run by the same
functions as tests/test_op_launch_forms_gpu.py, through emoportraits_amd.ops on CPU tensors with the host-compiled stream libraries
(tests/emul/emulibs.py: the product's csrc/{resample,embed_ops,smallops,groupnorm}.hip against the stand-in runtime) in the
library's place.  The barrier-free kernels run in the sequential library; the block reductions -- GroupNorm's own pass, the sums
of the upsampling kernel, the wave-reduced small_gemm -- in the threaded one.  Left out: the cases marked `wrap` (two million
work items thread by thread) and, of the threaded ones, the capped upsampling plan at N = 2 (256 blocks of 256 OS threads).

What this checks is what decides a form and what a form computes -- the launcher's conditions, the work decomposition of every
kernel, the order of its fp32 operations (-ffp-contract=off, as the product is built) -- under the same checkers and the same
bounds as on the device.  emo_op_launch_form is the same source, so the coverage test at the end needs no device either.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))
import emulibs  # noqa: E402
import op_launch_forms as L  # noqa: E402
import test_op_launch_forms_gpu as G  # noqa: E402
from emoportraits_amd import hip, ops  # noqa: E402

DEV = "cpu"
# the entry points whose kernels meet at a barrier or exchange between lanes
THREADED = ("emo_groupnorm_affine_f32", "emo_groupnorm_affine_from_sums_f32", "emo_upsample_trilinear_gn_sums_f32", "emo_small_gemm_f32")


class StreamLibraries:
    """libemoportraits_hip.so as ops sees it, served by the two host-compiled stream libraries; argument and result types from
    hip.SIGNATURES"""

    def __init__(self):
        self._seq, self._thr = emulibs.stream(False), emulibs.stream(True)
        self._cache = {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name not in self._cache:
            fn = getattr(self._thr if name in THREADED else self._seq, name)
            fn.argtypes = hip.SIGNATURES[name]
            fn.restype = hip._RESTYPES.get(name, ctypes.c_int)
            self._cache[name] = fn
        return self._cache[name]


@pytest.fixture(scope="module")
def libs():
    return StreamLibraries()


@pytest.fixture(autouse=True)
def on_the_host(libs, monkeypatch):
    """ops on CPU tensors: the library, and the three places of hip / ops that ask for a device"""
    monkeypatch.setattr(hip, "load", lambda: libs)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    monkeypatch.setattr(ops, "_lattice", lambda n, idx: torch.linspace(-1, 1, n))
    return libs


def unpack_rgb8(frames):
    """ops.unpack_rgb8 without its device check"""
    N, H, W, _ = frames.shape
    out = torch.full((N, 3, H, W), float("nan"))
    assert hip.load().emo_unpack_rgb8(hip.ptr(frames), hip.ptr(out), N, H, W, None) == 0
    return out


def no_wrap(cases):
    keep = [c for c in cases if not c["wrap"]]
    return dict(argvalues=keep, ids=L.ids(keep))


@pytest.mark.parametrize("c", **no_wrap(L.UPSAMPLE))
def test_upsample_trilinear(c):
    G.run_upsample(c, DEV)


@pytest.mark.parametrize("c", **no_wrap([c for c in L.UPSAMPLE_GN if c["plan"]["runs"] * c["plan"]["split"] <= 64]))
def test_upsample_trilinear_with_groupnorm_sums(c):
    G.run_upsample_gn(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.AVGPOOL))
def test_avgpool(c):
    G.run_avgpool(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.AVGPOOL_REFUSED))
def test_avgpool_refuses_before_any_launch(c):
    G.run_avgpool_refused(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.ADD))
def test_add(c):
    G.run_add(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.ADD_ROWS))
def test_add_rows_indexed(c):
    G.run_add_rows(c, DEV)


def test_add_rows_indexed_refuses_65536_rows():
    G.run_add_rows_refused(DEV)


@pytest.mark.parametrize("c", **no_wrap(L.GROUPNORM))
def test_groupnorm_affine(c):
    G.run_groupnorm(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.SMALL_GEMM))
def test_small_gemm(c):
    G.run_small_gemm(c, DEV)


def test_small_gemm_refuses_other_widths_and_65536_batches():
    G.run_small_gemm_refused(DEV)


@pytest.mark.parametrize("c", **no_wrap(L.PROJECTOR))
def test_projector_finalize(c):
    G.run_projector(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.COMPOSE))
def test_mul_mask_and_stage2_compose(c):
    G.run_compose(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.RGB8))
def test_pack_and_unpack_rgb8(c):
    G.run_rgb8(c, DEV, unpack=unpack_rgb8)


@pytest.mark.parametrize("c", **no_wrap(L.RESIZE))
def test_resize2d(c):
    G.run_resize(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.MAXPOOL))
def test_maxpool2d(c):
    G.run_maxpool(c, DEV)


@pytest.mark.parametrize("c", **no_wrap(L.AFFINE_ADD))
def test_affine_add_relu(c):
    G.run_affine_add(c, DEV)


def test_affine_add_relu_refuses_an_affine_without_its_operand():
    G.run_affine_add_refused(DEV)


@pytest.mark.parametrize("c", **no_wrap(L.GRID_SAMPLE2D))
def test_grid_sample2d(c):
    G.run_grid_sample2d(c, DEV)


def test_grid_sample2d_refuses_theta_on_a_lattice_that_is_not_square():
    G.run_grid_sample2d_refused(DEV)


def test_grid_sample2d_non_finite_grid_values_as_aten():
    G.run_grid_sample2d_non_finite(DEV)


def test_cases_cover_every_form_and_every_plan_edge():
    """every form of the C enums and every plan edge has a case; a form added to an enum fails here until it has one"""
    seen = G.coverage()
    assert "form x4_w1" in seen["avgpool"] and "ragged slice" in seen["upsample_trilinear"], seen


def test_a_form_or_an_edge_without_a_case_is_reported(monkeypatch):
    """the coverage test is not vacuous: without the ragged case, or without the cases of one kernel, it fails and says what for"""
    with monkeypatch.context() as mp:
        mp.setitem(L.BY_OP, "upsample_trilinear", [c for c in L.UPSAMPLE if c["id"] != "block split 2 ragged"])
        with pytest.raises(AssertionError, match="upsample_trilinear: no case for .*ragged slice"):
            G.coverage()
    with monkeypatch.context() as mp:
        mp.setitem(L.BY_OP, "avgpool", [c for c in L.AVGPOOL if c["form"] != "x4_w1"])
        with pytest.raises(AssertionError, match="avgpool: no case for .*form x4_w1"):
            G.coverage()
