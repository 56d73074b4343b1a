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


def _batches(counts, world):
    """[(rank, first frame, last frame + 1)] of every batch of the clip whose frame i holds counts[i] rows, as the clip loop forms them"""
    from emoportraits_amd import frames as frames_mod
    from emoportraits_amd import parallel
    out, base = [], 0
    for n in T.CHUNKS:
        for rank in range(world):
            lo, hi = parallel.shard_range(n, rank, world)
            out += [(rank, base + a, base + b) for a, b in frames_mod.face_spans(counts[base:base + n], lo, hi, T.BATCH)]
        base += n
    return out


def test_the_cases_show_what_they_are_there_for():
    """the planted dropouts of the combinations 14 ... 17 leave, on one rank and on two, a batch without a kept row, a chunk whose shard
    on rank 1 has none, frames with one kept row and with two; the detections of 16 let a track die in such a batch, on one rank and
    on two, and bear a face into a slot a death freed"""
    from emoportraits_amd import hostglue, parallel
    kept = T.KEPT_COUNTS
    assert len(kept) == T.N == sum(T.CHUNKS) and 1 in kept and 2 in kept
    boxes = T._dropout_boxes()
    assert tuple(boxes.shape) == (T.N, 2, 4) and (2 - boxes.isnan().any(-1).sum(1)).tolist() == kept
    assert all(boxes[f, p].isnan().all() == (p in T.MISSING.get(f, ())) for f in range(T.N) for p in (0, 1))
    empty = {world: [(r, a, b) for r, a, b in _batches(kept, world) if not sum(kept[a:b])] for world in (1, 2)}
    assert (0, 3, 6) in empty[1] and (0, 3, 4) in empty[2]
    lo, hi = parallel.shard_range(T.CHUNKS[1], 1, 2)
    first = T.CHUNKS[0]
    assert sum(kept[first + lo:first + hi]) == 0 < sum(kept[first:first + lo])      # rank 1 of the second chunk: nobody, rank 0: somebody
    # detections=: hostglue's account of the association
    dets = T._detections().numpy()
    assert dets.shape == (T.N, 4, 4) and len({tuple(np.isfinite(dets[t, :, 0]).tolist()) for t in range(T.N)}) > 3  # (no stable order)
    ref, age = np.zeros((1, 2, 4)), np.full((1, 2), -1, np.int32)
    tracked, restart, _ = hostglue.track_assign(dets, None, ref, age, min_iou=0.3, max_missed=1)
    present = np.isfinite(tracked).all(-1)
    seen = T.SEEN_COUNTS
    assert present.sum(1).tolist() == seen == [sum(t in frames for frames, _ in T.SEEN.values()) for t in range(T.N)]
    assert seen[:T.CHUNKS[0]] == kept[:T.CHUNKS[0]]                             # (the first chunk's batches are those above)
    deaths = [(f, p) for f in range(T.N) for p in (0, 1) if restart[f, p] and not present[f, p]]
    births = [(f, p) for f in range(T.N) for p in (0, 1) if restart[f, p] and present[f, p]]
    assert deaths == [(3, 0), (4, 1)] and births == [(0, 0), (2, 1), (6, 0), (6, 1)]
    empty = {world: [(r, a, b) for r, a, b in _batches(seen, world) if not sum(seen[a:b])] for world in (1, 2)}
    assert empty == {1: [(0, 3, 6)], 2: [(0, 3, 4)]}
    for world in (1, 2):                                                         # a death in a batch that holds no kept row
        assert any(a <= f < b for f, _ in deaths for _, a, b in empty[world]), world
    assert any(fd < fb and pd == pb for fd, pd in deaths for fb, pb in births)   # a birth into a freed slot
    assert present[-1].all()                                                     # both tracks live at the end: the streams end with a state


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
