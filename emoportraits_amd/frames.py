"""The frame plumbing of InferenceWrapper.animate_frames / animate_streams / paste_back / enrol_identities that touches no
wrapper state: crop windows and the faces of a frame, uint8 frames -> fp32 crops (crops_of) and rendered crops -> frames
(paste_into), the upload-ahead of a host chunk and the pinned ring that takes finished batches back to the host."""
import collections
import itertools

import torch

from . import ops, parallel


def square_windows(windows):
    """(x_lo, y_lo, side) per frame, as animate_frames takes them (a fourth entry must repeat the side) -> (x0, y0, s, s)"""
    out = []
    for w in windows:
        w = [int(v) for v in w]
        if len(w) not in (3, 4) or (len(w) == 4 and w[3] != w[2]):
            raise ValueError(f"window {tuple(w)}: expected (x_lo, y_lo, side)")
        out.append((w[0], w[1], w[2], w[2]))
    return out


def flatten_faces(faces):
    """faces[i] = the (x_lo, y_lo, side) windows of frame i in paste order, [] for a frame without a face, as animate_frames
    takes them -> (the windows of every face as (x0, y0, s, s) in frame order, the number of faces of every frame)"""
    flat, counts = [], []
    for of_frame in faces:
        wins = square_windows(of_frame)
        flat += wins
        counts.append(len(wins))
    return flat, counts


def face_offsets(counts):
    """[0, c0, c0 + c1, ...]: entry i = the faces in front of frame i"""
    return [0] + list(itertools.accumulate(counts))


def face_spans(counts, lo, hi, batch_size):
    """The batches of the frames [lo, hi) of a clip whose frame i has counts[i] faces: [(b0, b1), ...], whole frames taken
    greedily while a batch holds at most batch_size faces (the rows of the networks' batch) and at most batch_size frames (the
    rows of a pinned ring slot).  Batches are not padded: a clip with the same number of faces in every frame gets batches of
    one shape.  A frame with more than batch_size faces fits no batch: ValueError."""
    spans, b0, n_faces = [], lo, 0
    for i in range(lo, hi):
        if counts[i] > batch_size:
            raise ValueError(f"frame {i} has {counts[i]} faces: more than batch_size={batch_size}")
        if i > b0 and (n_faces + counts[i] > batch_size or i - b0 >= batch_size):
            spans.append((b0, i))
            b0, n_faces = i, 0
        n_faces += counts[i]
    if hi > b0:
        spans.append((b0, hi))
    return spans


# What a control launch needs to know about the rows of a batch (ChunkRows.where) or of a chunk (where_chunk).  ident: the slots of
# the rows as the loop sees them (device tensor, None: the current identity) -- what mix and the render take.  The controls run over
# the FULL rows these were taken from: r0 = the first full row's index in the call, n their number, slots their slots; at = None
# where the loop's rows ARE the full rows, else int64 [rows] on the device: where each of the loop's rows lies among the n.
RowsAt = collections.namedtuple("RowsAt", "ident r0 n slots at")


class ChunkRows:
    """The row arithmetic of one chunk of the clip loop (InferenceWrapper._animate_clip), host integers but for the tensors it hands on.
    n frames, the chunk's frame i holding per[i] rows (per None: one row each -- windows=, boxes [N,4], whole frames), the first row
    the call's row `row0`; `rank` of `world` takes the frames [lo, hi) (parallel.shard_range) in batches of whole frames with at most
    batch_size rows and frames (face_spans).  ids: the slot of every row of the call (host tensor) or None, moved to `device` where
    a launch takes them.
    Under tracking skip_absent=True the rows are the KEPT rows: per[i] = the faces of frame i, row_of int64 [T] on the device = the row
    among the chunk's n * P full rows that each kept row is, full0 = the chunk's first full row in the call, and ids are indexed
    by the full rows.
    Fields: off (the rows in front of every frame, n + 1), r0, r1 (the chunk's rows in the call), lo, hi, m_lo, m_hi (the shard's
    frames and rows), spans and with_rows (the shard's batches, and those that hold a row), ident (the slots of the shard's rows, on
    the device), counts (the rows of every rank's shard, as parallel.gather_rows takes them; None where the chunk holds no kept row
    and nothing is to be gathered)."""

    def __init__(self, n, per, rank, world, batch_size, row0, ids=None, device=None, P=None, full0=0, row_of=None):
        self.n, self.per, self.r0, self.P, self.full0, self.row_of, self._ids, self._device = n, per, row0, P, full0, row_of, ids, device
        counts = [1] * n if per is None else per
        self.off = face_offsets(counts)
        self.r1 = row0 + self.off[n]
        self.lo, self.hi = parallel.shard_range(n, rank, world)
        self.m_lo, self.m_hi = self.rows(self.lo, self.hi)
        self.spans = face_spans(counts, self.lo, self.hi, batch_size)
        self.with_rows = [sp for sp in self.spans if self.off[sp[0]] < self.off[sp[1]]]
        self.counts = None if row_of is not None and self.r1 == self.r0 else \
            [self.off[b] - self.off[a] for a, b in (parallel.shard_range(n, r, world) for r in range(world))]
        # (slots: under skip, the slots of the chunk's full rows)
        self.slots = None if ids is None or row_of is None else ids[full0:full0 + n * P].to(device)
        self.ident = None if ids is None else ids[self.m_lo:self.m_hi].to(device) if row_of is None else self.slots.index_select(0, self.shard(row_of))

    def rows(self, b0, b1):
        """the rows of the chunk's frames [b0, b1), as indices in the call"""
        return self.r0 + self.off[b0], self.r0 + self.off[b1]

    def frame_of(self, b0, b1):
        """the frame, counted from b0, of every row of the frames [b0, b1); None: one row per frame"""
        return None if self.per is None else [i - b0 for i in range(b0, b1) for _ in range(self.per[i])]

    def part(self, t, b0, b1):
        """of something that has one entry per row of the rank's shard of the chunk, the entries of the frames [b0, b1)"""
        return None if t is None else t[self.rows(b0, b1)[0] - self.m_lo:self.rows(b0, b1)[1] - self.m_lo]

    def shard(self, t):
        """of something that has one entry per row of the chunk, the entries of the rank's shard"""
        return t[self.m_lo - self.r0:self.m_hi - self.r0]

    def where(self, b0, b1):
        """the RowsAt of the frames [b0, b1) of the shard"""
        ident, (a, b) = self.part(self.ident, b0, b1), self.rows(b0, b1)
        if self.row_of is None:
            return RowsAt(ident, a, b - a, ident, None)
        f0, f1 = b0 * self.P, b1 * self.P                                   # (the frames' full rows, counted from the chunk's first)
        return RowsAt(ident, self.full0 + f0, f1 - f0, None if self.slots is None else self.slots[f0:f1], self.row_of[a - self.r0:b - self.r0] - f0)

    def where_chunk(self):
        """the RowsAt of the whole chunk, every rank's rows: what a pass over the gathered rows takes (its ident is the shard's)"""
        if self.row_of is None:
            return RowsAt(self.ident, self.r0, self.r1 - self.r0, None if self._ids is None else self._ids[self.r0:self.r1].to(self._device), None)
        return RowsAt(self.ident, self.full0, self.n * self.P, self.slots, self.row_of)


FORMATS = ("rgb8", "nv12", "yuv420p", "p010", "yuv420p10")     # packed RGB bytes, or YUV 4:2:0 under ffmpeg's pixel-format names
YUV420 = FORMATS[1:]


def check_format(frame_format, colorspace="bt709", what="frame_format"):
    if frame_format not in FORMATS:
        raise ValueError(f"{what}={frame_format!r}: one of {', '.join(repr(f) for f in FORMATS)}")
    if colorspace not in ops.NV12_MATRICES:
        raise ValueError(f"colorspace {colorspace!r}: 'bt709' or 'bt601'")


def check_frames(chunk, frame_format):
    """the shape and dtype of one chunk of frames: uint8 [N,H,W,3], or a YUV 4:2:0 format's [N, 3H/2, W] of its dtype with H and
    W even and the strides ops.yuv420_geometry asks for (the check the ops make, so it is refused before anything is launched)"""
    check_format(frame_format)
    if frame_format == "rgb8":
        if chunk.dtype != torch.uint8 or chunk.dim() != 4 or chunk.shape[-1] != 3:
            raise ValueError("frames must be uint8 [N,H,W,3]")
    else:
        if not isinstance(chunk, torch.Tensor) or chunk.dim() != 3:
            raise ValueError(f"{ops.yuv420_name(frame_format)} frames must be {str(ops.yuv420_dtype(frame_format)).replace('torch.', '')} "
                             f"[N, 3H/2, W] with H and W even, got {tuple(getattr(chunk, 'shape', ()))}")
        ops.yuv420_geometry(chunk, frame_format, "frames")


def frame_size(chunk, frame_format):
    """(H, W) of the frames of a chunk"""
    return (chunk.shape[1], chunk.shape[2]) if frame_format == "rgb8" else (chunk.shape[1] // 3 * 2, chunk.shape[2])


def crops_of(u8, size, windows=None, frame_format="rgb8", colorspace="bt709", full_range=False, frame_of=None):
    """uint8 frames [b,H,W,3] on the device -> fp32 crops [b,3,size,size]: byte -> fp32 CHW (emo_unpack_rgb8), then each frame's
    window (x0, y0, s, s) read in place and resized, the whole batch in one launch (a host list or an int32 [b,4] device
    tensor, ops.resize2d_windows), or without windows the whole frame, resized only where its size differs.
    frame_format 'nv12' | 'yuv420p' | 'p010' | 'yuv420p10': frames [b, 3H/2, W] of the format -> the same crops of the converted
    frames in ONE launch (ops.yuv420_windows: only the samples under the windows are read, no full-frame fp32 picture is written).
    frame_of: several faces per frame -- windows[m] is cut out of frame frame_of[m], still one launch, [len(windows),3,size,size]."""
    if frame_format != "rgb8":
        return ops.yuv420_windows(u8, frame_format, (size, size), windows, colorspace, full_range, frame_of=frame_of)
    x = ops.unpack_rgb8(u8)
    if windows is not None:
        return ops.resize2d_windows(x, (size, size), windows, "bicubic", clamp01=True, frame_of=frame_of)
    if x.shape[-2:] != (size, size):
        return ops.resize2d(x, (size, size), "bicubic")
    return x


def paste_into(full, img, wins, feather, matte, frame_format="rgb8", colorspace="bt709", full_range=False, frame_of=None):
    """The inverse of crops_of, IN PLACE and in one launch: the rendered fp32 img [M,3,S,S] goes into the device frames `full`
    (uint8 [b,H,W,3]: ops.paste_windows; a YUV 4:2:0 format's [b,3H/2,W]: ops.paste_windows_yuv420) where the windows were,
    blended with the feathered edge and the matte; frame_of as in crops_of.  Returns full."""
    if frame_format != "rgb8":
        return ops.paste_windows_yuv420(full, frame_format, img, wins, feather, matte, colorspace, full_range, frame_of=frame_of)
    return ops.paste_windows(full, img, wins, feather, matte, frame_of=frame_of)


def uploaded(chunk, spans, device, upload_stream):
    """(b0, b1, uint8 frames on the device) for every span, with the upload of span i + 1 enqueued on a copy stream BEFORE
    span i is handed out -- i.e. before its kernels are enqueued -- so that a host chunk's H2D copy (12.6 MB per 16 frames
    at 512^2: 0.25 ms) runs beside the previous batch's compute instead of in front of its own (on the compute stream the
    copy serialises with the kernels).  Device-resident chunks pass through."""
    ahead = None
    for span in list(spans) + [None]:
        nxt = None
        if span is not None:
            b0, b1 = span
            src = chunk[b0:b1]
            if src.is_cuda:
                nxt = (b0, b1, src if src.dim() == 3 else src.contiguous(), None)   # (NV12 ops take a padded view as it is)
            else:
                with torch.cuda.stream(upload_stream):
                    t = src.to(device, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(upload_stream)
                nxt = (b0, b1, t, ev)
        if ahead is not None:
            p0, p1, t, ev = ahead
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
                t.record_stream(torch.cuda.current_stream())
            yield p0, p1, t
        ahead = nxt


class HostRing:
    """Finished batches (uint8; uint16 for the 10-bit formats: a slot has its batch's dtype) go D2H into `ring` pinned buffers
    on a copy stream; a batch is handed out once ITS copy event has
    completed, i.e. the host only ever waits for a batch that is `ring - 1` batches behind the GPU.  What is handed out is a
    view of a ring slot, valid only until the next push()."""

    def __init__(self, device, ring, batch_size):
        self.ring, self.batch_size = ring, batch_size
        self.stream = torch.cuda.Stream(device=device)
        self.slots, self.pending, self.k = [], [], 0     # pinned buffers; (first index, slot, n frames, event) in flight

    def drain(self, keep=0):
        while len(self.pending) > keep:
            b0, slot, nb, ev = self.pending.pop(0)
            ev.synchronize()
            yield b0, self.slots[slot][:nb]

    def push(self, b0, out):
        """queue the copy of batch `out` (first frame b0) behind the compute stream; yields the batches now due"""
        if self.slots and (self.slots[0].shape[1:] != out.shape[1:] or self.slots[0].dtype != out.dtype):   # other frames: a new ring
            yield from self.drain()
            self.slots.clear()
            self.k = 0
        if len(self.slots) < self.ring:
            self.slots.append(torch.empty((self.batch_size,) + tuple(out.shape[1:]), dtype=out.dtype, pin_memory=True))
        slot = self.k % self.ring
        self.k += 1
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self.slots[slot][:out.shape[0]].copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        out.record_stream(self.stream)
        self.pending.append((b0, slot, out.shape[0], ev))
        yield from self.drain(self.ring - 1)


# ---- video streams of different frame sizes in one batch (InferenceWrapper.animate_streams) ------------------------------------
ARENA_ALIGN = 256


def interleave(lengths):
    """The frame order of several streams served together: tick t takes frame t of every stream that still has one, in stream
    order -> [(stream, frame index in the stream)]"""
    return [(s, t) for t in range(max(lengths, default=0)) for s, n in enumerate(lengths) if t < n]


def check_frame(frame, frame_format):
    """one frame of a mixed batch: uint8 [H,W,3], or YUV 4:2:0 [3H/2, W] of the format's dtype with H and W even"""
    check_frames(frame[None], frame_format)


def arena_layout(shapes, itemsize=1):
    """byte offsets of the frames of a batch (samples of `itemsize` bytes) in one byte buffer, each at a multiple of
    ARENA_ALIGN -> (offsets, total bytes)"""
    offsets, total = [], 0
    for shape in shapes:
        offsets.append(total)
        n = 1
        for d in shape:
            n *= d
        total += -(-n * itemsize // ARENA_ALIGN) * ARENA_ALIGN
    return offsets, total


def arena_views(buf, shapes, offsets, dtype=torch.uint8):
    """the frames of a batch as views of its byte buffer (device arena or pinned ring slot): the bytes viewed as `dtype`, not
    converted"""
    out, itemsize = [], torch.empty(0, dtype=dtype).element_size()
    for shape, off in zip(shapes, offsets):
        n = itemsize
        for d in shape:
            n *= d
        out.append(buf[off:off + n].view(dtype).view(tuple(shape)))
    return out


def _row_unit(frame):
    """a device frame the mixed ops take where it lies: stride 1 along a row (a row-pitch view included); else a packed copy"""
    unit = frame.stride(-1) == 1 and (frame.dim() == 2 or frame.stride(1) == 3)
    return frame if unit else frame.contiguous()


def uploaded_mixed(batches, device, upload_stream, copy_all):
    """(frames, arena) for every batch of `batches` (each a list of frame tensors of any sizes, host or device) -- frames the
    batch's frames on the device, arena the byte buffer that holds those of them that were copied (None: none was) -- with the
    upload of batch i + 1 enqueued on the copy stream BEFORE batch i is handed out, as `uploaded` does for uniform chunks.
    Every host frame goes into its place in the arena (offsets a multiple of ARENA_ALIGN) with its own asynchronous copy:
    no host-side staging copy of frame bytes.  A device frame is used where it lies, or, with copy_all (the batch is pasted
    into and the caller's frames stay untouched), copied into the arena too, on the compute stream when the batch is handed
    out.  frames[i] is then a view of the arena."""
    ahead = None
    for batch in itertools.chain(batches, [None]):                               # (lazily: a stream's chunks are read as they are due)
        nxt = None
        if batch is not None:
            inside = [copy_all or not f.is_cuda for f in batch]
            shapes = [tuple(f.shape) for f, a in zip(batch, inside) if a]
            dtype = batch[0].dtype if batch else torch.uint8
            offsets, total = arena_layout(shapes, batch[0].element_size() if batch else 1)
            arena, ev, views = None, None, []
            if total:
                with torch.cuda.stream(upload_stream):
                    arena = torch.empty(total, dtype=torch.uint8, device=device)
                    views = arena_views(arena, shapes, offsets, dtype)
                    for f, v in zip([f for f, a in zip(batch, inside) if a], views):
                        if not f.is_cuda:
                            v.copy_(f, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(upload_stream)
            nxt = (batch, inside, views, arena, ev)
        if ahead is not None:
            batch0, inside0, views0, arena0, ev0 = ahead
            if ev0 is not None:
                torch.cuda.current_stream().wait_event(ev0)
                arena0.record_stream(torch.cuda.current_stream())
            frames, k = [], 0
            for f, a in zip(batch0, inside0):
                if a:
                    if f.is_cuda:
                        views0[k].copy_(f)
                    frames.append(views0[k])
                    k += 1
                else:
                    frames.append(_row_unit(f))
            yield frames, arena0
        ahead = nxt


class ArenaRing(HostRing):
    """HostRing for the arenas of mixed batches: a finished batch goes to the host as ONE copy of its arena into a pinned slot.
    The slots are byte buffers; when a batch needs more than they hold, the ring is drained and re-made at that size."""

    def __init__(self, device, ring):
        super().__init__(device, ring, 0)

    def push(self, tag, arena):
        if self.slots and self.slots[0].numel() < arena.numel():
            yield from self.drain()
            self.slots.clear()
            self.k = 0
        if not self.slots:
            self.batch_size = max(self.batch_size, arena.numel())               # (the slots' size in bytes)
        yield from super().push(tag, arena)
