"""Batched enrolment of source identities without a GPU:
  * emo_volume_repack_indexed_f32 (csrc/grid_sample3d.hip, ABI 14) compiled for the host from the product's own source
    (tests/emul/emulibs.py): every written bank row is bit for bit the emo_volume_repack_f32 repack of its volume, rows it does
    not name keep their sentinel, an out-of-range row writes nothing -- on shapes that are not multiples of the 64x64 tile and on
    the R512 volume shape;
  * hostglue.enrolment_plan, the host-side planning of InferenceWrapper.enrol_identities as a pure function: slot choice, the
    ValueErrors, and chunk ownership for 1, 2 and 8 ranks (the chunks themselves do not depend on the number of ranks).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "emul"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SENTINEL = np.float32(-7.25)


@pytest.fixture(scope="module")
def sampler():
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not installed")
    import emulibs
    return emulibs.sampler()


def _aligned(n, fill):
    raw = np.empty(n + 16, np.float32)
    off = (-(raw.ctypes.data // 4)) % 4
    out = raw[off:off + n]
    out[...] = fill
    return out


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _repack_one(sampler, vol):
    """emo_volume_repack_f32(..., 1) of one NCDHW volume [C,D,H,W] -> [D,H,W,C]"""
    C, D, H, W = vol.shape
    src = _aligned(vol.size, 0)
    src[...] = vol.reshape(-1)
    out = _aligned(vol.size, np.nan)
    assert sampler.emo_volume_repack_f32(_p(src), _p(out), 1, C, D * H * W, 1, None) == 0
    return out.reshape(D, H, W, C)


def _indexed(sampler, vols, rows, num_rows):
    """emo_volume_repack_indexed_f32 of vols [N,C,D,H,W] into a sentinel-filled bank of num_rows rows"""
    N, C, D, H, W = vols.shape
    src = _aligned(vols.size, 0)
    src[...] = vols.reshape(-1)
    bank = _aligned(num_rows * vols[0].size, SENTINEL)
    row = np.ascontiguousarray(rows, dtype=np.int32)
    rc = sampler.emo_volume_repack_indexed_f32(_p(src), _p(bank), _p(row), N, C, D * H * W, num_rows, None)
    return rc, bank.reshape(num_rows, D, H, W, C)


@pytest.mark.parametrize("shape,rows,num_rows", [
    ((5, 3, 7, 9), [3, 0, 5], 7),            # C and D*H*W below one tile, rows out of order
    ((70, 2, 5, 13), [1, 4], 5),             # C = 64 + 6, D*H*W = 2 * 64 + 2: partial tiles in both directions
    ((96, 16, 64, 64), [1], 2),              # the R512 canonical volume: c = 96, d = 16, s = 64
])
def test_indexed_repack_rows_equal_the_plain_repack(sampler, shape, rows, num_rows):
    g = torch.Generator().manual_seed(len(rows) * 31 + shape[0])
    vols = torch.randn((len(rows),) + shape, generator=g).numpy()
    rc, bank = _indexed(sampler, vols, rows, num_rows)
    assert rc == 0
    for n, r in enumerate(rows):
        want = _repack_one(sampler, vols[n])
        assert np.array_equal(bank[r].view(np.uint32), want.view(np.uint32)), (shape, n, r)
    for r in set(range(num_rows)) - set(rows):
        assert np.array_equal(bank[r].view(np.uint32), np.full(bank[r].shape, SENTINEL).view(np.uint32)), (shape, r)


def test_out_of_range_rows_write_nothing(sampler):
    g = torch.Generator().manual_seed(3)
    vols = torch.randn(4, 6, 3, 5, 7, generator=g).numpy()
    rc, bank = _indexed(sampler, vols, [-1, 2, 3, 0], 3)            # -1 and num_rows are skipped
    assert rc == 0
    assert np.array_equal(bank[2].view(np.uint32), _repack_one(sampler, vols[1]).view(np.uint32))
    assert np.array_equal(bank[0].view(np.uint32), _repack_one(sampler, vols[3]).view(np.uint32))
    assert np.array_equal(bank[1].view(np.uint32), np.full(bank[1].shape, SENTINEL).view(np.uint32))


def test_indexed_repack_refuses_bad_arguments(sampler):
    src, bank, row = _aligned(32, 0), _aligned(32, 0), np.zeros(1, np.int32)
    for num_rows in (0, -1):
        assert sampler.emo_volume_repack_indexed_f32(_p(src), _p(bank), _p(row), 1, 4, 8, num_rows, None) == -1
    assert sampler.emo_volume_repack_indexed_f32(_p(src), _p(bank), None, 1, 4, 8, 1, None) == -1
    assert sampler.emo_volume_repack_indexed_f32(_p(src), _p(bank), _p(row), 0, 4, 8, 1, None) == -1
    assert sampler.emo_volume_repack_indexed_f32(_p(src), _p(bank), _p(row), 70000, 4, 8, 1, None) == -2


def test_indexed_repack_is_in_the_abi_table():
    from emoportraits_amd import hip
    hdr = open(os.path.join(ROOT, "include", "emo_hip.h")).read()
    assert "int emo_volume_repack_indexed_f32(" in hdr
    assert len(hip.SIGNATURES["emo_volume_repack_indexed_f32"]) == 8


# ---- host-side planning ----------------------------------------------------------------------------------------------------
def test_plan_takes_the_lowest_free_slots_and_explicit_ones():
    from emoportraits_amd.hostglue import enrolment_plan
    used = [False, True, False, False, True, False]
    slots, chunks, owners = enrolment_plan(used, 3, batch_size=2)
    assert slots == [0, 2, 3] and chunks == [(0, 2), (2, 3)] and owners == [0, 0]
    slots, _, _ = enrolment_plan(used, 4, slots=[4, 1, 5, 0], batch_size=8)        # occupied slots may be overwritten
    assert slots == [4, 1, 5, 0]
    slots, _, _ = enrolment_plan(used, 2, slots=torch.tensor([5, 2]))
    assert slots == [5, 2]


@pytest.mark.parametrize("kw,msg", [
    (dict(used=[], n_sources=1), "no identity bank"),
    (dict(used=[False] * 3, n_sources=0), "no sources"),
    (dict(used=[False, True, False], n_sources=3), "free identity slots"),
    (dict(used=[False] * 3, n_sources=2, slots=[1, 1]), "twice"),
    (dict(used=[False] * 3, n_sources=2, slots=[0, 3]), "not in"),
    (dict(used=[False] * 3, n_sources=2, slots=[-1, 0]), "not in"),
    (dict(used=[False] * 3, n_sources=2, slots=[0, True]), "not in"),
    (dict(used=[False] * 3, n_sources=2, slots=[0, 1.0]), "not in"),
    (dict(used=[False] * 3, n_sources=2, slots=[0]), "slots for"),
    (dict(used=[False] * 3, n_sources=2, batch_size=0), "batch_size"),
])
def test_plan_refusals(kw, msg):
    from emoportraits_amd.hostglue import enrolment_plan
    with pytest.raises(ValueError, match=msg):
        enrolment_plan(**kw)


@pytest.mark.parametrize("K,bs", [(5, 2), (16, 4), (16, 8), (3, 8), (17, 1)])
def test_chunks_do_not_depend_on_the_world_and_ranks_own_contiguous_ranges(K, bs):
    from emoportraits_amd.hostglue import enrolment_plan
    from emoportraits_amd.parallel import shard_range
    used = [False] * 20
    plans = {w: enrolment_plan(used, K, batch_size=bs, world=w) for w in (1, 2, 8)}
    ref_slots, ref_chunks, _ = plans[1]
    assert ref_chunks == [(j * bs, min((j + 1) * bs, K)) for j in range(-(-K // bs))]
    for w, (slots, chunks, owners) in plans.items():
        assert slots == ref_slots and chunks == ref_chunks, w
        assert owners == sorted(owners) and len(owners) == len(chunks)          # contiguous, in rank order
        for r in range(w):
            lo, hi = shard_range(len(chunks), r, w)
            assert [j for j, o in enumerate(owners) if o == r] == list(range(lo, hi)), (w, r)
    assert plans[2][2] == [0] * (-(-len(ref_chunks) // 2)) + [1] * (len(ref_chunks) // 2)
