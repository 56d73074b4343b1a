"""tests/guarded_outputs.py on CPU tensors, with a toy module standing in for emoportraits_amd.ops; and the source guard that keeps
every allocation of ops.py / frames.py one the proxy serves."""
import ast
import functools
import os
import types

import pytest
import torch

import guarded_outputs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOY_SOURCE = '''
import functools
import torch


def add_one(x, skip_last=False):
    out = torch.empty_like(x)
    flat, src = out.view(-1), x.reshape(-1)
    n = src.numel() - (1 if skip_last else 0)
    flat[:n] = src[:n] + 1
    return out


def _workspace(n):
    return torch.empty(n, dtype=torch.uint8)


def writes_before(x):
    ws = _workspace(64)
    ws.fill_(0)
    torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1).fill_(7)
    return ws


def writes_after(x):
    out = torch.empty((2, 3), dtype=torch.float64, device=x.device)
    out.fill_(0)
    torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
    return out


def call_shapes(x):
    new = functools.partial(torch.empty, device=x.device, dtype=torch.float32)
    return [new((2, 3)), torch.empty(2, 3), torch.empty(6, device="cpu", dtype=torch.int32), torch.empty(0, device=x.device),
            torch.empty_like(x), torch.empty_like(x, dtype=torch.int64), torch.empty((4,) + tuple(x.shape[1:]), dtype=x.dtype),
            torch.empty(torch.Size((1, 2)), dtype=torch.uint16)]
'''


@pytest.fixture
def toy(monkeypatch):
    """(toy module, proxy): the module's name `torch` is the proxy, as the guarded_outputs fixture makes it for ops and frames"""
    mod = types.ModuleType("toy_ops")
    exec(compile(TOY_SOURCE, "toy_ops.py", "exec"), mod.__dict__)
    proxy = G.GuardedTorch(site_files=("toy_ops.py",))
    monkeypatch.setattr(mod, "torch", proxy)
    return mod, proxy


def test_an_unwritten_last_element_is_caught(toy):
    mod, proxy = toy
    x = torch.arange(12, dtype=torch.float32).view(3, 4)
    good = mod.add_one(x)
    G.assert_written(good, "add_one")
    assert torch.equal(good, x + 1)
    bad = mod.add_one(x, skip_last=True)                # (the same shape again: a plain allocator could hand `good`'s block back)
    assert not torch.equal(bad, x + 1)
    with pytest.raises(AssertionError, match=r"add_one: 1 of 12 elements were never written .* flat index 11"):
        G.assert_written(bad, "add_one")
    assert torch.equal(bad.view(-1)[:11], (x + 1).view(-1)[:11])
    proxy.check()                                       # (nothing was written outside)
    assert proxy.allocations == 2 and proxy.poisoned_bytes == 2 * 48
    with pytest.raises(TypeError):
        G.assert_written(torch.zeros(3, dtype=torch.int32), "ints")


def test_a_write_before_the_view_is_caught_with_the_site_named(toy):
    mod, proxy = toy
    mod.writes_before(torch.zeros(1))
    with pytest.raises(G.GuardError) as e:
        proxy.check()
    msg = str(e.value)
    assert "writes_before: front guard of the allocation at toy_ops.py:" in msg and "in _workspace" in msg, msg
    assert f"first at byte offset {G.GUARD_BYTES - 1} " in msg and "back guard" not in msg, msg


def test_a_write_after_the_view_is_caught_with_the_site_named(toy):
    mod, proxy = toy
    good = mod.add_one(torch.zeros(5))
    mod.writes_after(torch.zeros(1))
    with pytest.raises(G.GuardError) as e:
        proxy.check()
    msg = str(e.value)
    assert "1 of 2 guarded buffers" in msg, msg
    assert "writes_after: back guard of the allocation at toy_ops.py:" in msg and "in writes_after" in msg, msg
    assert "first at byte offset 0 " in msg and "(8 of 512 bytes" in msg and "front guard" not in msg, msg


def _ops_dtypes():
    """every dtype an allocation of ops.py / frames.py names (dtype=torch.<name>), and the ones they reach through a variable"""
    found = {torch.float32,                     # torch.empty(0, device=...): the default dtype
             torch.uint8, torch.uint16}         # ops.yuv420_dtype(frame_format), the batches of frames.HostRing
    for call in _empty_calls():
        for kw in call.keywords:
            if kw.arg == "dtype" and isinstance(kw.value, ast.Attribute) and isinstance(kw.value.value, ast.Name) \
                    and kw.value.value.id == "torch":
                found.add(getattr(torch, kw.value.attr))
    return found


def test_every_dtype_the_ops_allocate_has_a_poison():
    dtypes = _ops_dtypes()
    assert {torch.float32, torch.float64, torch.uint8, torch.uint16, torch.int32} <= dtypes <= set(G.POISONED_DTYPES)
    proxy = G.GuardedTorch()
    for dt in sorted(dtypes | {torch.int64}, key=str):          # (int64: the frame tables, should one be allocated empty)
        t = proxy.empty((3, 5), dtype=dt)
        if dt.is_floating_point:
            assert bool(torch.isnan(t).all()), dt
        else:
            want = G.int_poison(dt)
            assert want not in (0, -1, 1) and [int(v) for v in t.view(-1).tolist()] == [want] * 15, dt
    for dt in (torch.float16, torch.bfloat16, torch.bool, torch.int16, torch.complex64):
        with pytest.raises(TypeError, match="no poison"):
            proxy.empty(4, dtype=dt)
    with pytest.raises(TypeError):
        proxy.empty(4, requires_grad=True)              # a keyword the ops do not use is not silently dropped
    proxy.check()


def test_the_view_is_contiguous_has_the_shape_and_sits_one_guard_into_its_raw_buffer(toy):
    mod, proxy = toy
    x = torch.zeros(5, 7, 2)
    outs = mod.call_shapes(x.transpose(0, 1))           # (empty_like of a strided tensor: still a contiguous result)
    shapes = [(2, 3), (2, 3), (6,), (0,), (7, 5, 2), (7, 5, 2), (4, 5, 2), (1, 2)]
    dtypes = [torch.float32, torch.float32, torch.int32, torch.float32, torch.float32, torch.int64, torch.float32, torch.uint16]
    assert proxy.allocations == proxy.live == len(outs) == len(shapes)
    for out, shape, dt, rec in zip(outs, shapes, dtypes, proxy._live):
        assert tuple(out.shape) == shape and out.dtype == dt and out.is_contiguous() and out.device == x.device
        assert rec.raw.dim() == 1 and rec.raw.dtype == dt
        assert out.storage_offset() * out.element_size() == G.GUARD_BYTES == 512
        if out.numel():                                 # (torch gives an empty tensor the address 0)
            assert out.data_ptr() - rec.raw.data_ptr() == G.GUARD_BYTES
        assert rec.raw.numel() * rec.raw.element_size() == out.numel() * out.element_size() + 2 * G.GUARD_BYTES
        assert out.untyped_storage().data_ptr() == rec.raw.untyped_storage().data_ptr()
        assert bool((rec.front == G.GUARD_BYTE).all()) and bool((rec.back == G.GUARD_BYTE).all())
        assert rec.front.numel() == rec.back.numel() == G.GUARD_BYTES
    proxy.check()
    assert proxy.checked == len(outs)
    assert proxy.cat is torch.cat and proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor     # everything else: torch's


def test_the_budget_evicts_oldest_first_and_checks_before_dropping():
    assert G.BUDGET_BYTES == 2 << 30
    per = 1000 * 4 + 2 * G.GUARD_BYTES
    proxy = G.GuardedTorch(site_files=(os.path.basename(__file__),), budget=4 * per)
    held = [proxy.empty(1000, dtype=torch.float32) for _ in range(4)]
    raws = [r.raw for r in proxy._live]
    assert proxy.live == 4 and proxy.live_bytes == 4 * per and proxy.evicted == 0 and proxy.checked == 0
    held.append(proxy.empty(1000, dtype=torch.float32))         # over the budget: down to half of it, the oldest first
    assert proxy.evicted == 3 and proxy.checked == 3 and proxy.live == 2 and proxy.live_bytes == 2 * per
    assert [r.raw.data_ptr() for r in proxy._live] == [raws[3].data_ptr(), held[4].data_ptr() - G.GUARD_BYTES]
    # a damaged guard is reported by the eviction that would drop it, and the buffer stays until then
    torch.as_strided(held[3], (1,), (1,), held[3].storage_offset() + 1000).fill_(0.0)
    held += [proxy.empty(1000, dtype=torch.float32) for _ in range(2)]
    assert proxy.live == 4 and proxy.evicted == 3
    with pytest.raises(G.GuardError, match="back guard .* first at byte offset 0 "):
        proxy.empty(1000, dtype=torch.float32)
    # one allocation larger than the whole budget is not dropped before its kernel has run
    small = G.GuardedTorch(budget=1024)
    big = small.empty(4096, dtype=torch.uint8)
    assert small.live == 1 and small.evicted == 0
    torch.as_strided(big, (1,), (1,), big.storage_offset() - 3).fill_(0)
    with pytest.raises(G.GuardError, match=f"front guard .* first at byte offset {G.GUARD_BYTES - 3} "):
        small.check()


def test_the_fixture_fails_a_test_in_which_it_served_nothing():
    """the fixture's body (guarded_outputs.guarded), run by hand: ops and frames see the proxy while it is open, and its teardown
    raises when nothing was allocated"""
    from emoportraits_amd import frames, ops
    with pytest.MonkeyPatch.context() as mp:
        gen = G.guarded(mp)
        proxy = next(gen)
        assert ops.torch is proxy and frames.torch is proxy and ops.torch.empty.__self__ is proxy
        with pytest.raises(AssertionError, match="served no allocation"):
            next(gen)
    assert ops.torch is torch and frames.torch is torch
    with pytest.MonkeyPatch.context() as mp:            # a test that launches nothing has to say so, with a reason
        gen = G.guarded(mp)
        proxy = next(gen)
        with pytest.raises(ValueError):
            proxy.may_serve_nothing("")
        proxy.may_serve_nothing("only argument errors are provoked")
        with pytest.raises(StopIteration):
            next(gen)
    with pytest.MonkeyPatch.context() as mp:
        gen = G.guarded(mp)
        proxy = next(gen)
        assert functools.partial(ops.torch.empty, dtype=torch.float32)((2, 2)).shape == (2, 2)
        with pytest.raises(StopIteration):
            next(gen)
        assert proxy.allocations == 1 and proxy.live == 0


# ---- source guard: an allocation that would bypass the proxy fails here ---------------------------------------------------------
SOURCES = [os.path.join(ROOT, "emoportraits_amd", name) for name in ("ops.py", "frames.py")]


def _trees():
    for path in SOURCES:
        with open(path) as f:
            yield path, ast.parse(f.read(), path)


def _empty_calls():
    """every torch.empty(...) / torch.empty_like(...) call node of the two sources"""
    for _, tree in _trees():
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) \
                    and node.func.value.id == "torch" and node.func.attr in ("empty", "empty_like"):
                yield node


def test_every_allocation_of_ops_and_frames_goes_through_the_proxy():
    sites = {"ops.py": 0, "frames.py": 0}
    for path, tree in _trees():
        for node in ast.walk(tree):
            if not isinstance(node, ast.Attribute):
                continue
            where = f"{os.path.basename(path)}:{node.lineno}"
            # torch.<empty...>, as a call or handed on (functools.partial(torch.empty, ...)): only the two the proxy serves
            if isinstance(node.value, ast.Name) and node.value.id == "torch" and node.attr.startswith("empty"):
                assert node.attr in ("empty", "empty_like"), f"{where}: torch.{node.attr} bypasses tests/guarded_outputs.py"
                sites[os.path.basename(path)] += 1
            assert node.attr != "new_empty", f"{where}: .new_empty( bypasses tests/guarded_outputs.py"
            assert node.attr != "empty_strided", f"{where}: empty_strided bypasses tests/guarded_outputs.py"
        for node in ast.walk(tree):
            # `torch` is looked up in the module's globals at call time: no other name may hold the real module or its empty
            if isinstance(node, ast.ImportFrom) and node.module == "torch":
                assert not any(a.name.startswith("empty") for a in node.names), f"{path}:{node.lineno}: from torch import empty"
            if isinstance(node, ast.Import):
                assert all(a.asname in (None, a.name) for a in node.names if a.name == "torch"), f"{path}:{node.lineno}: torch under another name"
    assert sites["ops.py"] > 0 and sites["frames.py"] > 0, sites
    # the keywords those calls use are the ones the proxy takes
    for call in _empty_calls():
        assert {kw.arg for kw in call.keywords} <= {"dtype", "device", "pin_memory"}, ast.dump(call)
