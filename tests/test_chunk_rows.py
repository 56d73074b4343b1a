"""frames.ChunkRows, the row arithmetic of one chunk of the clip loop, against a plain loop written here; and InferenceWrapper._control,
the one way a control is launched over a batch's rows, against the sequence it stands for.  Host integers and CPU tensors: no GPU."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

from emoportraits_amd import frames as F  # noqa: E402
from emoportraits_amd import parallel  # noqa: E402

BATCH = 3
FACE_COUNTS = [1, 2, 0, 0, 0, 0, 1, 2, 1, 0, 1, 2, 1]                            # (tools/clip_launch_trace.FACE_COUNTS)
# skip: present[i] = the tracks of frame i that have a face, of P = 2
PRESENT = {"dropouts": [(0,), (1,), (0,), (), (), (), (0, 1), (0, 1), (1,), (0, 1), (), (), ()],      # a span with none, a shard with none
           "nobody": [(), (), (), ()],
           "few": [(1,)]}                                                         # n smaller than the world


def _cases():
    """(name, n, per, P, present or None)"""
    out = [("one row per frame", 7, None, None, None), ("one row per frame, one frame", 1, None, None, None),
           ("faces", len(FACE_COUNTS), FACE_COUNTS, None, None), ("two tracks", 7, [2] * 7, 2, None),
           ("no frame", 0, None, None, None), ("skip, no frame", 0, [], 2, [])]
    for name, present in PRESENT.items():
        out.append((f"skip, {name}", len(present), [len(p) for p in present], 2, present))
    return out


CASES = _cases()


def test_the_cases_show_what_they_are_there_for():
    import clip_launch_trace as T
    assert FACE_COUNTS == T.FACE_COUNTS
    per = [len(p) for p in PRESENT["dropouts"]]
    rows = F.ChunkRows(len(per), per, 1, 2, BATCH, 0, P=2, row_of=torch.zeros(sum(per), dtype=torch.int64))
    assert any(rows.off[a] == rows.off[b] for a, b in rows.spans) and rows.with_rows                # a span without a kept row
    tail = F.ChunkRows(6, per[7:], 1, 2, BATCH, 0, P=2, row_of=torch.zeros(sum(per[7:]), dtype=torch.int64))
    assert tail.m_lo == tail.m_hi and tail.spans and not tail.with_rows and sum(tail.counts) > 0    # a shard without one
    assert len(PRESENT["few"]) < 2 and not any(PRESENT["nobody"])


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chunk_rows_is_the_plain_loop(case, world):
    _, n, per, P, present = case
    row0, full0 = 5, 8
    skip = present is not None
    counts = [1] * n if per is None else per
    # the plain account: every row of the chunk as (frame, its index in the call, its full row in the call)
    table, r = [], row0
    for i in range(n):
        which = present[i] if skip else range(counts[i])
        for p in which:
            table.append((i, r, full0 + i * P + p if skip else r))
            r += 1
    total = r - row0
    n_full = n * P if skip else total
    ids = torch.arange(100, 100 + (full0 + n_full if skip else row0 + total))                        # slot of full row k (of row k): 100 + k
    row_of = torch.tensor([f - full0 for _, _, f in table], dtype=torch.int64) if skip else None
    seen = []
    for rank in range(world):
        rows = F.ChunkRows(n, per, rank, world, BATCH, row0, ids, torch.device("cpu"), P, full0 if skip else 0, row_of)
        lo, hi = parallel.shard_range(n, rank, world)
        mine = [t for t in table if lo <= t[0] < hi]
        assert (rows.lo, rows.hi, rows.r0, rows.r1) == (lo, hi, row0, row0 + total)
        assert (rows.m_lo, rows.m_hi) == ((mine[0][1], mine[-1][1] + 1) if mine else (rows.m_lo, rows.m_lo))
        assert rows.m_hi - rows.m_lo == len(mine) and rows.ident.tolist() == [100 + f for _, _, f in mine]
        assert rows.spans == F.face_spans(counts, lo, hi, BATCH)
        assert rows.with_rows == [(a, b) for a, b in rows.spans if any(a <= t[0] < b for t in table)]
        if skip and not total:
            assert rows.counts is None                                           # nothing to gather: every rank knows
        else:
            assert rows.counts == [sum(a <= t[0] < b for t in table) for a, b in (parallel.shard_range(n, k, world) for k in range(world))]
        tags = [f"row {t[1]}" for t in mine]                                     # one entry per row of the shard
        assert rows.shard([f"row {t[1]}" for t in table]) == tags
        for b0, b1 in rows.spans:
            span = [t for t in mine if b0 <= t[0] < b1]
            a, b = rows.rows(b0, b1)
            assert list(range(a, b)) == [t[1] for t in span]
            assert rows.frame_of(b0, b1) == (None if per is None else [t[0] - b0 for t in span])
            assert rows.part(tags, b0, b1) == [f"row {t[1]}" for t in span] and rows.part(None, b0, b1) is None
            at = rows.where(b0, b1)
            assert at.ident.tolist() == [100 + t[2] for t in span]
            if not skip:
                assert at.at is None and (at.r0, at.n) == (a, b - a) and at.slots is at.ident
            else:
                assert (at.r0, at.n) == (full0 + b0 * P, (b1 - b0) * P) and at.slots.tolist() == [100 + at.r0 + k for k in range(at.n)]
                assert at.at.dtype == torch.int64 and at.at.tolist() == [t[2] - at.r0 for t in span]
            seen += [t[1] for t in span]
        whole = rows.where_chunk()
        assert whole.ident is rows.ident and whole.slots.tolist() == [100 + (full0 if skip else row0) + k for k in range(n_full)]
        assert (whole.r0, whole.n) == ((full0, n * P) if skip else (row0, total))
        assert whole.at is row_of if skip else whole.at is None
    assert seen == [t[1] for t in table]                                         # the spans of all ranks tile the chunk's rows, once, in order


def test_without_identities_there_are_no_slots():
    rows = F.ChunkRows(4, None, 0, 1, BATCH, 0)
    at, whole = rows.where(0, 3), rows.where_chunk()
    assert at == F.RowsAt(None, 0, 3, None, None) and whole == F.RowsAt(None, 0, 4, None, None)
    rows = F.ChunkRows(2, [1, 1], 0, 1, BATCH, 0, P=2, full0=6, row_of=torch.tensor([1, 2]))
    at = rows.where(1, 2)
    assert at.ident is None and at.slots is None and (at.r0, at.n, at.at.tolist()) == (8, 2, [0])


# ---- InferenceWrapper._control ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def wrapper(monkeypatch):
    import bare_wrapper
    return bare_wrapper.bare_wrapper(monkeypatch, None, 0)


def test_control_hands_full_rows_on_as_they_came(wrapper):
    a, b, slots = torch.randn(3, 2).double(), torch.arange(3), torch.tensor([2, 0, 1])                # (not even a cast)
    got = []
    result = (torch.zeros(3), torch.ones(3))

    def fn(*args):
        got.append(args)
        return result
    out = wrapper._control(F.RowsAt("ident", 7, 3, slots, None), fn, a, b)
    assert out is result and len(got) == 1 and len(got[0]) == 4
    assert got[0][0] is a and got[0][1] is b and got[0][2] is slots and got[0][3] == 7
    single = torch.zeros(3, 4)
    assert wrapper._control(F.RowsAt(None, 0, 3, None, None), lambda v, s, r: single, a) is single


@pytest.mark.parametrize("kept", [[1, 2, 5], []], ids=["three of six", "none of six"])
def test_control_over_kept_rows_is_scatter_call_gather(wrapper, kept):
    g = torch.Generator().manual_seed(3)
    at = torch.tensor(kept, dtype=torch.int64)
    a, b = torch.randn(len(kept), 3, generator=g), torch.randn(len(kept), 2, 2, generator=g)
    slots = torch.arange(6)
    seen = []

    def pair(x, y, s, r):
        seen.append((x.clone(), y.clone(), s, r))
        return x * 2 + 1, y.flatten(1).sum(1) + r                                # (an absent row's result is not zero)

    def one(x, s, r):
        return x.sum(1) + s
    where = F.RowsAt("ident", 40, 6, slots, at)
    got = wrapper._control(where, pair, a, b)
    # today's semantics, written out: zeros, index_copy_, the call over the full rows, index_select
    wide = [torch.zeros((6,) + tuple(t.shape[1:])).index_copy_(0, at, t) for t in (a, b)]
    want = tuple(t.index_select(0, at) for t in pair(*wide, slots, 40))
    assert isinstance(got, tuple) and len(got) == 2 and all(torch.equal(x, y) for x, y in zip(got, want))
    assert torch.equal(seen[0][0], wide[0]) and torch.equal(seen[0][1], wide[1]) and seen[0][2] is slots and seen[0][3] == 40
    assert not seen[0][0][[i for i in range(6) if i not in kept]].any()          # an absent row reads zeros
    got = wrapper._control(where, one, a)
    assert isinstance(got, torch.Tensor) and torch.equal(got, one(wide[0], slots, 40).index_select(0, at)) and got.shape[0] == len(kept)
