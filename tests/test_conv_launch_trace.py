"""The C-ABI calls of the convolution ops against the record of tests/golden/conv_launch_trace.json.

tools/conv_launch_trace.py runs ops.conv_igemm / conv_head / stage2_head on CPU tensors against a stub library and writes down
every call of a convolution entry point -- entry, integers, floats, pointers as role tokens -- over the plan lattice, pinned plans,
out= aliasing res, the driver passes and stage 2.  The fixture holds a digest per case, written by that tool at the commit that
added it; a change of the planner or of ops.conv_igemm that moves a launch, an argument or a buffer shows here, on the host,
as the first case whose record differs (`python tools/conv_launch_trace.py --dump <case>` prints it in full)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import convlib  # noqa: E402

needs_lib = pytest.mark.skipif(not convlib.available(), reason="needs ROCm clang++ and the built product library")


@needs_lib
def test_every_conv_launch_is_the_recorded_one():
    import conv_launch_trace as T
    with open(T.FIXTURE) as f:
        recorded = json.load(f)
    assert list(recorded) == list(T.CASES), ("the cases of the tool and of the fixture differ: only in the tool "
                                             f"{sorted(set(T.CASES) - set(recorded))[:10]}, only in the fixture "
                                             f"{sorted(set(recorded) - set(T.CASES))[:10]} (or their order)")
    digests = T.digests()
    differing = [key for key in T.CASES if digests[key] != recorded[key]]
    assert not differing, (f"{len(differing)} of {len(recorded)} cases make other C calls than recorded; the first is {differing[0]!r}: "
                           f"diff `python tools/conv_launch_trace.py --dump {differing[0]}` against the same at the fixture's commit")
