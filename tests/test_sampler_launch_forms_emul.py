"""The launch forms of the 3-D sampler without a GPU: the direct-form cases of tests/sampler_launch_forms.py, run by the same
functions as tests/test_sampler_launch_forms_gpu.py, through emoportraits_amd.ops on CPU tensors with the host-compiled sampler
library (tests/emul/emulibs.py: the product's csrc/grid_sample3d.hip against the stand-in runtime, a block = 256 OS threads) in
the library's place.  Left out: the tile family and the packed-4 repack (another translation unit: stubs that refuse in that
library, whose query therefore reports the direct forms only) and the cases marked `slow` (hundreds of blocks).  One ORDER 3 case
runs, once, in a test of its own.

What this checks is what decides a form and what a form computes -- the launchers' conditions, block_to_work, the item walk, the
bank's zero fill, the coordinate arithmetic of gs3d_coord.h compiled for the host (-ffp-contract=off) -- under the same comparisons
as on the device.  In emulation readfirstlane is a stand-in and a float -> int conversion is x86's, so the device's saturating
conversion (the reflection parity at |g| >= 2^32) is invisible here: only the GPU test sees it.  The coverage test at the end asks
the product library, which answers without a device.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))
import emulibs  # noqa: E402
import sampler_launch_forms as L  # noqa: E402
import test_sampler_launch_forms_gpu as G  # noqa: E402
from emoportraits_amd import hip, ops  # noqa: E402
from guarded_outputs import guarded_outputs  # noqa: E402,F401

DEV = "cpu"
pytestmark = pytest.mark.skipif(not os.path.exists(emulibs.CLANG), reason="ROCm clang++ not installed")
DIRECT = ("planar", "rows", "brick")


class SamplerLibrary:
    """libemoportraits_hip.so as ops sees it, served by the host-compiled sampler library; types from hip.SIGNATURES"""

    def __init__(self):
        self._lib, self._cache = emulibs.sampler(), {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name not in self._cache:
            fn = getattr(self._lib, name)
            fn.argtypes = hip.SIGNATURES[name]
            fn.restype = hip._RESTYPES.get(name, ctypes.c_int)
            self._cache[name] = fn
        return self._cache[name]


@pytest.fixture(scope="module")
def lib():
    return SamplerLibrary()


@pytest.fixture
def on_the_host(lib, monkeypatch, guarded_outputs):
    """ops on CPU tensors: the library, and the places of hip / ops that ask for a device; outputs poisoned and guarded"""
    monkeypatch.setattr(hip, "load", lambda: lib)
    monkeypatch.setattr(hip, "require_cuda_f32", lambda *a, **k: None)
    monkeypatch.setattr(hip, "current_stream", lambda: None)
    # (cached, as the product's is: ops.affine_grid3d passes the lattices' addresses without holding the tensors)
    monkeypatch.setattr(ops, "_lattice", functools.lru_cache(maxsize=None)(lambda n, idx: torch.linspace(-1, 1, n)))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    return lib


# every (padding, mode) pair once over the three families would be 27 runs of ~25 launches of OS threads: the paddings and the
# modes each meet every family (a Latin square), and the arithmetic they select is shared by all kernels (gs3d_coord.h)
SQUARE = [(f, G.PADS[(i + j) % 3], G.MODES[j]) for i, f in enumerate(DIRECT) for j in range(3)]


@pytest.mark.parametrize("family,pm,mode", SQUARE)
def test_form_cases(family, pm, mode, on_the_host):
    G.run_family(family, pm, mode, DEV, skip_slow=True)


def test_order_3_taken_with_fma(on_the_host):
    """the N = 16 case whose sample interleave can go wrong (two samples per XCD), FMA and both outputs: 2 x 256 blocks, and the
    ORDER 1 call it must equal bit for bit"""
    for c in L.ROWS:
        if c["id"].startswith("order 3 fma to"):
            assert G.run_case(c, "reflection", "delta", DEV) is not None


def test_refused_cases(on_the_host):
    refused = [(c, code) for c, code in L.REFUSED if c["in_layout"] != "p4"]
    assert refused
    G.run_refusals(DEV, refused)


@pytest.mark.parametrize("c", [c for c in G.BANKED], ids=L.ids(G.BANKED))
def test_banked_forms_frame_by_frame_and_out_of_range_indices(c, on_the_host):
    G.run_bank(c, G.PADS[G.BANKED.index(c) % 3], DEV)


@pytest.mark.parametrize("pm", G.PADS)
@pytest.mark.parametrize("dims", G.EDGE_VOLUMES, ids=lambda d: "x".join(map(str, d)))
def test_coordinate_edges(dims, pm, on_the_host):
    G.run_edges(dims, pm, DEV, [e for e in G.EDGE_CALLS if not e[0].startswith("tile")])


@pytest.mark.parametrize("c", [c for c in L.REPACK if not c["direction"].endswith("p4")],
                         ids=L.ids([c for c in L.REPACK if not c["direction"].endswith("p4")]))
def test_repack_is_the_exact_permutation(c, on_the_host):
    G.run_repack(c, DEV)


def test_repack_refusals_launch_nothing(on_the_host):
    G.run_repack_refusals(DEV, [(c, code) for c, code in L.REPACK_REFUSED if c["to_channels_last"] < 4])


@pytest.mark.parametrize("size", [(3, 5, 7), (3, 10, 11)], ids=lambda d: "x".join(map(str, d)))
def test_affine_grid3d_equals_the_oracle_bit_for_bit(size, on_the_host):
    G.run_affine_grid(size, DEV)


def test_cases_cover_every_form_and_every_required_edge():
    """the product library answers without a device: every form of the C enum, the tile forms included, and every required edge"""
    print("PARITY sampler launch form coverage:", G.coverage(), G.repack_coverage())
