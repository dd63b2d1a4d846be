"""Red-zone / poison arena for the C-ABI tests (tests/test_abi_redzone_gpu.py, tests/test_abi_arena_cpu.py).

An Arena carves every buffer of one entry-point call out of ONE torch.uint8 allocation:

    [ leading guard | payload | trailing guard ] ... [ leading guard | payload | trailing guard ]

  - the whole allocation is filled with one byte (0x00, or 0xFF = NaN in fp32 / fp16 / bf16 and -1 in every integer type)
    before a case initialises its payloads, so whatever the case did not write is poison;
  - a payload starts on a 256-byte boundary (as torch's own allocations do) and its trailing guard starts at the payload's
    last byte plus one -- no rounding, a 4-byte overrun lands in the guard;
  - guards are GUARD (64 KiB) bytes on each side of every payload;
  - a buffer has a ROLE:
        "in"     the case initialises the logical window; nothing of it may change during the call
        "out"    nothing is initialised; the kernel may write the logical window only
        "inout"  the case initialises the logical window as the header demands; the kernel may write the window only
        "ws"     exactly the size the entry's size query returned, left at the fill; all of it is the kernel's
    and, for a 2-D buffer, a logical WINDOW of columns [col, col + width) inside rows of `ld` elements: the other columns
    (row-pitch pad, a neighbour's column block) belong to the caller.
  - seal() snapshots the arena after the case's initialisation; check() compares every byte the kernel was NOT given
    (guards, pad columns, neighbours, inputs) with the snapshot and returns the first byte that changed.

A stray store of a NaN / -1 is invisible under 0xFF and a stray store of a 0 is invisible under 0x00: that is why every case
runs under both fills.
"""
from dataclasses import dataclass

import torch

GUARD = 64 * 1024
ALIGN = 256
FILLS = (0x00, 0xFF)
WRITABLE_ROLES = ("out", "inout", "ws")
ROLES = ("in",) + WRITABLE_ROLES


@dataclass
class Violation:
    buffer: str        # name the case gave the buffer
    region: str        # "leading guard" | "trailing guard" | "outside window" | "input"
    offset: int        # trailing guard: bytes past the payload's end (0 = the first byte after it);
                       # leading guard: bytes before the payload's start (1 = the byte just before it);
                       # outside window / input: byte offset from the payload's start
    payload_offset: int  # byte offset from the payload's start (negative in the leading guard)
    row: int = -1      # outside window / input of a 2-D buffer: element row and column
    col: int = -1

    def __str__(self):
        where = f" (row {self.row}, column {self.col})" if self.row >= 0 else ""
        return (f"buffer '{self.buffer}': {self.region} byte {self.offset} was written"
                f" (payload byte {self.payload_offset}){where}")


class Buf:
    """one carved buffer: .t the physical tensor ([n] or [rows, ld]), .win the logical window, .ptr / .win_ptr their addresses"""

    def __init__(self, arena, name, role, dtype, shape, col, width, start, nbytes):
        self.arena, self.name, self.role, self.dtype = arena, name, role, dtype
        self.shape, self.col, self.width = shape, col, width
        self.start, self.nbytes = start, nbytes
        self.t = arena.mem[start:start + nbytes].view(dtype).view(*shape)
        self.win = self.t if len(shape) == 1 else self.t[:, col:col + width]
        self.extra = []                      # documented pad writes: (col_lo, col_hi) the kernel may also write

    @property
    def sealed(self):
        return self.start < self.arena.sealed_upto

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def win_ptr(self):
        return self.win.data_ptr()

    @property
    def ld(self):
        return self.shape[1] if len(self.shape) == 2 else self.shape[0]

    def allow(self, col_lo, col_hi):
        """columns [col_lo, col_hi) of every row are ALSO the kernel's (a pad the header says it writes)"""
        assert not self.sealed and len(self.shape) == 2 and 0 <= col_lo <= col_hi <= self.shape[1]
        self.extra.append((col_lo, col_hi))
        return self

    def set(self, value):
        """initialise the logical window (roles in / inout) from a tensor or scalar"""
        assert self.role in ("in", "inout"), f"{self.name}: a '{self.role}' buffer keeps the fill until the kernel writes"
        assert not self.sealed, f"{self.name}: initialise a buffer before the call that follows its creation"
        if torch.is_tensor(value):
            self.win.copy_(value.to(self.dtype).reshape(self.win.shape))
        else:
            self.win.fill_(value)
        return self

    def bits(self):
        """the logical window as an integer tensor (a copy): bit-for-bit comparisons"""
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.t.element_size()]
        return self.win.contiguous().view(it).clone()

    def first_nonfinite(self):
        """None, or (row, col) / (index,) of the first non-finite value of the logical window (floating types)"""
        if not self.dtype.is_floating_point:
            return None
        bad = (~torch.isfinite(self.win)).nonzero()
        return None if bad.numel() == 0 else tuple(int(v) for v in bad[0])


class Arena:
    def __init__(self, fill, device="cpu", capacity=8 << 20):
        assert fill in FILLS
        self.fill, self.device = fill, torch.device(device)
        self.raw = torch.empty(capacity + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.raw.data_ptr()) % ALIGN       # the arena proper starts on a 256-byte boundary
        self.mem = self.raw[self.base:self.base + capacity]
        self.mem.fill_(fill)
        self.cursor = 0
        self.bufs = []
        self.n_sealed = 0            # buffers covered by the snapshot
        self.sealed_upto = 0         # ... and the arena bytes below this offset
        self.snap = None
        self.writable = None
        self.pending = None          # first stray byte found while sealing again (see seal)

    @property
    def sealed(self):
        """every buffer carved so far is covered by the snapshot"""
        return self.snap is not None and self.n_sealed == len(self.bufs)

    # ---- carving -----------------------------------------------------------------------------------------------
    def new(self, name, role, dtype, shape, col=0, width=None):
        """shape: (n,) or (rows, ld) PHYSICAL elements; col / width: the logical column window of a 2-D buffer
        (default: all ld columns).  The payload is exactly prod(shape) elements."""
        assert role in ROLES
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        assert len(shape) in (1, 2) and all(s >= 0 for s in shape)
        if len(shape) == 2:
            width = shape[1] - col if width is None else width
            assert 0 <= col and col + width <= shape[1]
        else:
            assert col == 0 and width is None
        item = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * item
        start = (self.cursor + GUARD + ALIGN - 1) // ALIGN * ALIGN
        end = start + nbytes
        assert end + GUARD <= self.mem.numel(), f"arena too small for '{name}' ({nbytes} bytes): raise `capacity`"
        self.cursor = end + GUARD
        b = Buf(self, name, role, dtype, shape, col, width, start, nbytes)
        self.bufs.append(b)
        return b

    def ws(self, name, nbytes):
        """a workspace of EXACTLY nbytes bytes (what the size query returned), at the fill"""
        return self.new(name, "ws", torch.uint8, (int(nbytes),))

    # ---- sealing and checking ----------------------------------------------------------------------------------
    def seal(self):
        """call after the case initialised its inputs and before the kernel runs.  A case of several calls may carve further
        buffers between two calls (an output of the first that the second reads is simply a writable buffer): sealing again
        snapshots the bytes carved since and leaves the earlier snapshot as it is."""
        if self.snap is None:
            self.snap = self.mem.clone()
            self.writable = torch.zeros(self.mem.numel(), dtype=torch.bool, device=self.device)
        else:
            lo = self.sealed_upto
            # a store of an earlier call beyond everything carved at that time must not vanish into the new snapshot: what
            # changed there outside the new payloads (which the case has just initialised) is kept for check()
            diff = self.mem[lo:] != self.snap[lo:]
            for b in self.bufs[self.n_sealed:]:
                diff[b.start - lo:b.start - lo + b.nbytes] = False
            bad = diff.nonzero()
            if bad.numel() and self.pending is None:
                self.pending = lo + int(bad[0])
            self.snap[lo:self.cursor] = self.mem[lo:self.cursor]
        w = self.writable
        for b in self.bufs[self.n_sealed:]:
            if b.role not in WRITABLE_ROLES or b.nbytes == 0:
                continue
            if len(b.shape) == 1:
                w[b.start:b.start + b.nbytes] = True
                continue
            item = b.t.element_size()
            rows = w[b.start:b.start + b.nbytes].view(b.shape[0], b.shape[1] * item)
            for lo_c, hi_c in [(b.col, b.col + b.width)] + b.extra:
                rows[:, lo_c * item:hi_c * item] = True
        self.n_sealed = len(self.bufs)
        self.sealed_upto = self.cursor
        return self

    def check(self):
        """None if every byte outside the kernel's windows still holds what seal() saw, else the first Violation"""
        assert self.sealed, "seal() the arena (again) after carving buffers"
        if self.pending is not None:
            pos = self.pending
        else:
            bad = ((self.mem != self.snap) & ~self.writable).nonzero()
            if bad.numel() == 0:
                return None
            pos = int(bad[0])
        # owner: the buffer whose [start - GUARD, next buffer's start - GUARD) span holds the byte
        owner = self.bufs[0]
        for b in self.bufs:
            if pos >= b.start - GUARD:
                owner = b
        b = owner
        rel = pos - b.start
        if rel < 0:
            return Violation(b.name, "leading guard", -rel, rel)
        if rel >= b.nbytes:
            return Violation(b.name, "trailing guard", rel - b.nbytes, rel)
        region = "input" if b.role == "in" else "outside window"
        if len(b.shape) == 2:
            item = b.t.element_size()
            e = rel // item
            return Violation(b.name, region, rel, rel, e // b.shape[1], e % b.shape[1])
        return Violation(b.name, region, rel, rel)

    def nonfinite(self):
        """None, or (buffer name, index) of the first non-finite value in the logical window of a writable float buffer
        (workspaces excepted: their content is undefined)"""
        for b in self.bufs:
            if b.role in ("out", "inout"):
                at = b.first_nonfinite()
                if at is not None:
                    return b.name, at
        return None
