"""Poisoned, guarded outputs for the GPU tests (a plain module: test modules import the fixture by name).

Every wrapper of emoportraits_amd/ops.py (and three places of frames.py) allocates its outputs, statistics and workspaces with
torch.empty / torch.empty_like, and PyTorch's caching allocator hands a freed block back to the next request of the same size with
its contents intact.  A kernel that skips a tile edge, a channel tail or the rows of a wave that left early then finds the right
values of the previous run of the same shape in its output; a store just outside the output lands in a neighbouring block of the
same segment and faults nowhere.  Neither is visible to a comparison with a reference.

GuardedTorch stands in for the name `torch` in those modules.  It forwards every attribute to torch except `empty` and
`empty_like`, which allocate the requested elements plus GUARD_BYTES on each side in one raw 1-D tensor of the requested dtype
and device, fill the guards with a byte pattern and the inner range with a poison (NaN for float32 / float64, the byte POISON_BYTE
in every byte of the integer types), and return the inner range viewed to the requested shape.  check() asserts that every guard
still holds its pattern; assert_written() that no float element is still NaN.

    from guarded_outputs import guarded_outputs  # noqa: F401
    pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_outputs")]
"""
import os
import sys

import pytest
import torch

# The caching allocator's block alignment: the inner view keeps the alignment of a plain allocation (base + 512), so no launch
# form that asks for 16-byte alignment changes.  A condition of the design, not a measurement.
GUARD_BYTES = 512
# Raw buffers are held strongly so that their guards can be checked; beyond this many bytes the oldest are checked and dropped.
# A condition, not a measurement: it bounds what the per-launch checkers of a B = 16 pass keep alive until teardown.
BUDGET_BYTES = 2 << 30
# An eviction drops the oldest buffers until the total is at most this fraction of the budget: one batched guard read-back (one
# device synchronisation) per eviction round instead of one per allocation once the budget is reached.
EVICT_TO = 0.5

GUARD_BYTE = 0xC3           # every guard byte
POISON_BYTE = 0xA5          # every byte of an integer element: uint8 0xA5, uint16 0xA5A5, int32 -1515870811, int64 0xA5A5...A5
_FLOAT_POISON = (torch.float32, torch.float64)
_INT_POISON = (torch.uint8, torch.uint16, torch.int32, torch.int64)
POISONED_DTYPES = _FLOAT_POISON + _INT_POISON
SITE_FILES = ("ops.py", "frames.py")


class GuardError(AssertionError):
    pass


def int_poison(dtype):
    """the value an untouched element of an integer dtype holds"""
    if dtype not in _INT_POISON:
        raise TypeError(f"{dtype} has no integer poison")
    size = torch.empty(0, dtype=dtype).element_size()
    return int.from_bytes(bytes([POISON_BYTE]) * size, "little", signed=dtype in (torch.int32, torch.int64))


_ITEMSIZE = {dt: torch.empty(0, dtype=dt).element_size() for dt in POISONED_DTYPES}
# Outputs of at most this many bytes are cloned from a filled template of their (size, dtype, device), kept for the process: the
# controls, trackers and frame tables allocate thousands of tiny outputs per test, and three fill launches each would cost such a
# test more than its kernels do.  Larger ones are filled in place.
TEMPLATE_BYTES = 64 << 10
_TEMPLATES = {}


def _fill(raw, numel, g, dtype):
    raw[:g].view(torch.uint8).fill_(GUARD_BYTE)
    raw[g + numel:].view(torch.uint8).fill_(GUARD_BYTE)
    if dtype in _FLOAT_POISON:
        raw[g:g + numel].fill_(float("nan"))
    elif numel:
        raw[g:g + numel].view(torch.uint8).fill_(POISON_BYTE)


def _template(numel, g, dtype, device):
    key = (numel, dtype, device)
    t = _TEMPLATES.get(key)
    if t is None and len(_TEMPLATES) < 4096:
        t = torch.empty(numel + 2 * g, dtype=dtype)
        _fill(t, numel, g, dtype)
        t = _TEMPLATES[key] = t.to(device)          # (filled on the host, copied synchronously: ready on every stream)
    return t


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


class _Raw:
    """one live raw buffer: the tensor, its two guards as byte views, and where it was allocated"""
    __slots__ = ("raw", "front", "back", "nbytes", "op", "site")

    def __init__(self, raw, front, back, op, site):
        self.raw, self.front, self.back, self.op, self.site = raw, front, back, op, site
        self.nbytes = raw.numel() * raw.element_size()


class GuardedTorch:
    """`torch` with guarded, poisoned empty() and empty_like().  site_files: the base names of the source files whose frames name
    an allocation's op (outermost such frame) and site (innermost); budget: bytes of raw buffers held before the oldest go."""

    def __init__(self, site_files=SITE_FILES, budget=BUDGET_BYTES):
        self._site_files = tuple(site_files)
        self._budget = int(budget)
        self._code_files = {}       # code object -> base name of its file
        self._live = []             # _Raw, oldest first
        self._live_bytes = 0
        self._deferred = False      # a check() fell into a graph capture: the next one outside it runs
        self.allocations = 0
        self.poisoned_bytes = 0
        self.serves_nothing = None  # the reason a test gave for launching nothing through ops (may_serve_nothing)
        self.checked = 0            # raw buffers whose guards were read back
        self.evicted = 0

    def __getattr__(self, name):
        return getattr(torch, name)

    # ---- the two allocators ----------------------------------------------------------------------------------------------------
    def empty(self, *size, dtype=None, device=None, pin_memory=False):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(s) for s in size)
        if any(s < 0 for s in shape):
            raise ValueError(f"negative dimension in {shape}")
        dtype = torch.get_default_dtype() if dtype is None else dtype
        device = torch.device("cpu" if device is None else device)
        return self._allocate(shape, dtype, device, pin_memory)

    def empty_like(self, t, dtype=None, device=None):
        return self._allocate(tuple(t.shape), t.dtype if dtype is None else dtype, t.device if device is None else torch.device(device),
                              False)

    def _allocate(self, shape, dtype, device, pin_memory):
        if dtype not in POISONED_DTYPES:
            raise TypeError(f"guarded empty: no poison for {dtype}; add one to tests/guarded_outputs.py with the allocation")
        numel = 1
        for s in shape:
            numel *= s
        item = _ITEMSIZE[dtype]
        g = GUARD_BYTES // item
        capturing = _capturing(device)
        template = None
        if numel * item <= TEMPLATE_BYTES and not capturing and not pin_memory:
            template = _template(numel, g, dtype, device)
        if template is not None:
            raw = template.clone()                  # guards and poison in one copy: small outputs cost one launch, not three
        else:
            raw = torch.empty(numel + 2 * g, dtype=dtype, device=device, pin_memory=pin_memory)
            _fill(raw, numel, g, dtype)
        inner = raw[g:g + numel]
        front, back = raw[:g].view(torch.uint8), raw[g + numel:].view(torch.uint8)
        self.allocations += 1
        self.poisoned_bytes += numel * item
        if not capturing:
            # (inside a graph capture the fills above are captured like any kernel and nothing is held: a captured allocation
            # belongs to the graph's pool, and its guards hold their pattern only once the graph has been replayed)
            op, site = self._where()
            rec = _Raw(raw, front, back, op, site)
            self._live.append(rec)
            self._live_bytes += rec.nbytes
            if self._live_bytes > self._budget:
                self._evict()
        return inner.view(shape)

    def _where(self):
        """(op, site): the outermost and the innermost frame of the call stack that lie in one of the site files"""
        f, op, site, names = sys._getframe(2), None, None, self._code_files
        while f is not None and f.f_code.co_filename == __file__:
            f = f.f_back
        caller = f
        while f is not None:
            code = f.f_code
            name = names.get(code)
            if name is None:                        # (per code object: the walk runs for every allocation)
                name = names[code] = os.path.basename(code.co_filename)
            if name in self._site_files:
                if site is None:
                    site = f"{name}:{f.f_lineno} in {code.co_name}"
                op = code.co_name
            f = f.f_back
        if site is None and caller is not None:     # (a test that takes a buffer of its own from the proxy)
            op, site = caller.f_code.co_name, f"{os.path.basename(caller.f_code.co_filename)}:{caller.f_lineno} in {caller.f_code.co_name}"
        return op or "<unknown op>", site or "<unknown site>"

    # ---- checking --------------------------------------------------------------------------------------------------------------
    @property
    def live_bytes(self):
        return self._live_bytes

    @property
    def live(self):
        return len(self._live)

    def _evict(self):
        """over the budget: check the oldest buffers, then drop them, until EVICT_TO of the budget is left"""
        keep_bytes, n, total = self._budget * EVICT_TO, 0, self._live_bytes
        while n < len(self._live) - 1 and total > keep_bytes:      # (never the newest: its kernel has not run yet)
            total -= self._live[n].nbytes
            n += 1
        oldest = self._live[:n]
        self._check(oldest)
        del self._live[:n]
        self._live_bytes = total
        self.evicted += n

    def check(self):
        """every guard of every live raw buffer still holds its pattern (GuardError names op, site, side and byte offset)"""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            self._deferred = True
            return
        self._deferred = False
        self._check(self._live)

    def _check(self, records):
        if not records:
            return
        by_device = {}
        for r in records:
            by_device.setdefault(r.raw.device, []).append(r)
        for device, recs in by_device.items():
            if device.type == "cuda":
                torch.cuda.synchronize(device)      # (buffers filled or written on other streams, e.g. an upload stream)
            # one reduction and one read-back per device: [n, 2 * GUARD_BYTES] guard bytes against the pattern
            guards = torch.cat([v for r in recs for v in (r.front, r.back)]).view(len(recs), 2 * GUARD_BYTES)
            bad = (guards != GUARD_BYTE)
            self.checked += len(recs)
            if not bool(bad.any()):
                continue
            rows = bad.any(dim=1).nonzero().flatten().tolist()
            lines = []
            for i in rows:
                r, row = recs[i], bad[i].cpu()
                for side, part in (("front", row[:GUARD_BYTES]), ("back", row[GUARD_BYTES:])):
                    if bool(part.any()):
                        off = int(part.nonzero()[0])
                        lines.append(f"{r.op}: {side} guard of the allocation at {r.site} changed, first at byte offset {off} "
                                     f"({int(part.sum())} of {GUARD_BYTES} bytes; {r.raw.dtype}, {r.nbytes - 2 * GUARD_BYTES} bytes inside)")
            raise GuardError(f"{len(rows)} of {len(recs)} guarded buffers on {device} were written outside their view:\n" + "\n".join(lines))

    def may_serve_nothing(self, reason):
        """said by a test, in its body, that by construction may reach no allocation of ops / frames under the fixture -- it only
        provokes argument errors, skips, or reads results another test of the module computed and cached: the teardown then does
        not ask for an allocation.  Never silent: the reason is a sentence in the test"""
        if not reason or not isinstance(reason, str):
            raise ValueError("may_serve_nothing needs the reason")
        self.serves_nothing = reason

    def drop(self):
        """forget the live buffers (after check())"""
        self._live.clear()
        self._live_bytes = 0


def assert_written(t, what):
    """no element of the float tensor t is still NaN: for outputs of finite inputs.  (Integer outputs are compared exactly with
    their references, so a surviving pattern fails there.)"""
    if not t.is_floating_point():
        raise TypeError(f"assert_written({what}): {t.dtype} is no float type; compare integer outputs exactly")
    nan = torch.isnan(t)
    if bool(nan.any()):
        first = nan.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(nan.sum())} of {t.numel()} elements were never written (still NaN), first at flat index "
                             f"{first} of shape {tuple(t.shape)}")


def guarded(monkeypatch):
    """the body of the guarded_outputs fixture, as a generator"""
    from emoportraits_amd import frames, ops
    proxy = GuardedTorch()
    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setattr(frames, "torch", proxy)
    yield proxy
    try:
        proxy.check()
    finally:
        n, b = proxy.allocations, proxy.poisoned_bytes
        proxy.drop()
    print(f"GUARDED {n} allocations, {b} bytes poisoned")
    assert n > 0 or proxy.serves_nothing, ("the guarded_outputs fixture served no allocation: ops.torch was not the proxy when the test "
                                           "allocated (a test that launches nothing says so: guarded_outputs.may_serve_nothing(reason))")


@pytest.fixture
def guarded_outputs(monkeypatch):
    """ops and frames allocate through a GuardedTorch for the test; at teardown every guard is checked, and the fixture must have
    served at least one allocation (a module where it is silently inactive fails) unless the test itself has said, with its
    reason, that it launches nothing (GuardedTorch.may_serve_nothing)"""
    yield from guarded(monkeypatch)
