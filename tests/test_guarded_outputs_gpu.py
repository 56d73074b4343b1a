"""tests/guarded_outputs.py bites on the device: a real kernel (emo_add_f32, through the C ABI) on buffers from the proxy, told to
write one element less than, exactly, and one element more than the view it was given.  No kernel is broken for this, and every
byte any launch touches belongs to a raw tensor the proxy allocated."""
import pytest
import torch

from emoportraits_amd import hip, ops
from guarded_outputs import GuardError, assert_written, guarded_outputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 4096


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(40)
    a, b = torch.randn(N, generator=g), torch.randn(N, generator=g)
    return a.to(DEV), b.to(DEV), ((a.double() + b.double()) * 0.5).float()      # (one fp32 add, one exact halving: bit for bit)


def _add(a, b, out, n):
    hip.check(hip.load().emo_add_f32(hip.ptr(a), hip.ptr(b), hip.ptr(out), n, n, 0.5, hip.current_stream()), "emo_add_f32")


def test_a_whole_launch_leaves_no_poison_and_no_guard_touched(operands, guarded_outputs):
    a, b, ref = operands
    out = ops.add(a, b, 0.5)                            # the wrapper's own torch.empty_like, through the proxy
    mine = guarded_outputs.empty(N, device=DEV, dtype=torch.float32)
    assert mine.data_ptr() % 512 == 0 and bool(torch.isnan(mine).all())
    _add(a, b, mine, N)
    for t in (out, mine):
        assert_written(t, "emo_add_f32")
        assert torch.equal(t.cpu(), ref)
    guarded_outputs.check()
    assert guarded_outputs.allocations == 2 and guarded_outputs.checked == 2


def test_an_element_the_launch_skips_is_still_poison(operands, guarded_outputs):
    a, b, ref = operands
    for _ in range(2):                                  # (twice: a plain allocator hands the second run the first one's block)
        out = guarded_outputs.empty(N, device=DEV, dtype=torch.float32)
        _add(a, b, out, N - 1)
        got = out.cpu()
        assert torch.equal(got[:N - 1], ref[:N - 1]) and bool(torch.isnan(got[N - 1]))
        assert not torch.equal(got, ref)
        with pytest.raises(AssertionError, match=f"1 of {N} elements were never written .* flat index {N - 1}"):
            assert_written(out, "emo_add_f32")
        del out
    guarded_outputs.check()


def test_a_store_one_element_past_the_view_is_reported(operands, guarded_outputs):
    a, b, ref = operands
    short = guarded_outputs.empty(N - 1, device=DEV, dtype=torch.float32)      # its back guard starts where element N - 1 would be
    _add(a, b, short, N)
    torch.cuda.synchronize()
    with pytest.raises(GuardError) as e:
        guarded_outputs.check()
    msg = str(e.value)
    assert "back guard" in msg and "first at byte offset 0 " in msg and "front guard" not in msg, msg
    assert "test_guarded_outputs_gpu.py" in msg and "(4 of 512 bytes" in msg, msg
    assert torch.equal(short.cpu(), ref[:N - 1])
    guarded_outputs.drop()                              # reported: the teardown's check would raise it again
