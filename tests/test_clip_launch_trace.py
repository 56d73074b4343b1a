"""What animate_frames, animate and animate_streams do between their checks and their yields, pinned on the CPU.

tools/clip_launch_trace.py runs a matrix of keyword combinations on the bare wrapper (tests/bare_wrapper.py: host-compiled kernels,
stand-ins for the networks, plain uploads) on one rank and on two (spawned processes, gloo), with the crop budget
EMO_SMOOTH_KEEP_GB at its default and at 0.  Per combination:
  a. the two ranks render disjoint rows whose union is the one-rank run's, every row's (pose, theta) as handed to the driver pass bit
     for bit the one-rank run's;
  b. every array of _bank_streams, _stream and _crop_streams is bit for bit the same on every rank and on the one-rank run;
  c. the C entries, the stand-ins' calls, the uploads and the gathers of every (combination, world, rank, budget), in call order,
     are those of tests/golden/clip_launch_trace.json, written by that tool at the commit that added it;
and what is yielded is the same frame by frame, the caller's frames untouched, a frame without a face as it went in."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import clip_launch_trace as T  # noqa: E402

SHARDED = [c for c in T.COMBOS if not T._combos()[c].get("local")]


@pytest.fixture(scope="module")
def runs():
    return T.run_all()


def _bits(a):
    return None if a is None else (a.dtype.str, a.shape, a.tobytes())


def _items(run):
    """{row or frame index: its yielded slice} of one run; animate_streams: {(stream, frame, face): ...}"""
    return {first + (i,) if isinstance(first, tuple) else first + i: out[i] for first, out in run["yields"] for i in range(out.shape[0])}


@pytest.mark.parametrize("keep", ["default", "0"])
@pytest.mark.parametrize("combo", SHARDED)
def test_two_ranks_render_the_rows_of_one(runs, combo, keep):
    one = runs[(1, "default", 0)][combo]
    n_rows = one["rows"][0].shape[0]
    assert T.expected_rows(combo, 1, 0) == list(range(n_rows))
    seen, items = [], {}
    for rank in range(2):
        run = runs[(2, keep, rank)][combo]
        rows = T.expected_rows(combo, 2, rank)
        assert run["rows"][0].shape[0] == len(rows), f"rank {rank} rendered {run['rows'][0].shape[0]} rows, its shards hold {len(rows)}"
        for got, want in zip(run["rows"], one["rows"]):
            assert _bits(got) == _bits(want[rows]), f"rank {rank}: a row's {'pose' if got is run['rows'][0] else 'theta'} differs"
        seen += rows
        assert not set(items) & set(_items(run))
        items.update(_items(run))
        assert run["untouched"]
    assert sorted(seen) == list(range(n_rows))                                   # disjoint, and their union is every row
    want = _items(one)
    assert sorted(items) == sorted(want) and all(_bits(items[i]) == _bits(want[i]) for i in want)


@pytest.mark.parametrize("combo", T.COMBOS)
def test_stream_states_are_the_same_on_every_rank(runs, combo):
    one = runs[(1, "default", 0)][combo]
    assert any(a is not None and a.any() for a in one["states"]), "the combination leaves no state behind"
    for (world, keep, rank), res in runs.items():
        if combo in res:
            got = res[combo]["states"]
            differing = [i for i, (g, w) in enumerate(zip(got, one["states"])) if _bits(g) != _bits(w)]
            assert not differing, f"world {world} rank {rank} keep {keep}: state arrays {differing} differ from the one-rank run's"


def test_the_budget_changes_no_result_on_one_rank(runs):
    for combo in T.COMBOS:
        a, b = runs[(1, "default", 0)][combo], runs[(1, "0", 0)][combo]
        assert all(_bits(x) == _bits(y) for x, y in zip(a["rows"], b["rows"])), combo
        assert sorted(_items(a)) == sorted(_items(b)) and all(_bits(v) == _bits(_items(b)[i]) for i, v in _items(a).items()), combo


def test_frames_without_a_face_come_back_as_they_went_in(runs):
    combo = next(c for c in T.COMBOS if c.startswith("8 "))
    clip = T._clip(T.N, T.HW, 80).numpy()
    frames = _items(runs[(1, "default", 0)][combo])
    assert sorted(frames) == list(range(T.N))
    for i, c in enumerate(T.FACE_COUNTS):
        assert np.array_equal(frames[i], clip[i]) == (c == 0), i                 # (a pasted frame differs: the driver pass is black)
    streams = next(c for c in T.COMBOS if c.startswith("13 "))
    assert len(runs[(1, "default", 0)][streams]["yields"]) == 8 and runs[(1, "default", 0)][streams]["untouched"]


def test_every_event_is_the_recorded_one(runs):
    with open(T.FIXTURE) as f:
        recorded = json.load(f)
    got = json.loads(T.dumps(T.traces(runs)))
    assert list(recorded) == list(got), "the keys of the tool and of the fixture differ (or their order)"
    differing = [k for k in got if got[k] != recorded[k]]
    assert not differing, (f"{len(differing)} of {len(got)} runs make other calls than recorded; the first is {differing[0]!r}: at event "
                           f"{next((i for i, (a, b) in enumerate(zip(got[differing[0]], recorded[differing[0]])) if a != b), 'the end')}")
