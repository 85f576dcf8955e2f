"""One guarded arena per kernel call: every operand of a call is carved out of ONE allocation, between margins the test owns, so that a store
past a buffer, a read past an input or a workspace element that no slice wrote shows up in memory the test can look at - not in whatever tensor
torch's caching allocator put next.  A helper module (not a conftest); it works on any torch device, so tests/test_buffer_guard_host.py runs it on
the CPU against stand-in "kernels" with known faults.

Layout, per operand: [margin >= `margin` bytes][payload at `offset` bytes into a 256-byte line][margin >= `margin` bytes].  No two operands share
a margin.  Fill patterns:
  inputs               the payload; 0xFF bytes in both margins (NaN as fp32 and as fp16: a margin element that enters a sum makes the result NaN)
  outputs, workspaces  0xFF (NaN) where the kernel is to write; 0xA5 bytes in both margins
  in-place operands    the payload; 0xA5 bytes in both margins
A workspace is handed over at exactly the byte count it was declared with (what the *_workspace_bytes query answered); its margin starts at the
next byte.

    g = Guard(device)                       # margin = 64 KiB: one 128-pixel x 128-channel fp32 tile
    g.input("x", x); g.output("out", shape); g.workspace("ws", nbytes)
    rc = g.run(lambda g: fn(g.ptr("x"), g.ptr("out"), g.ptr("ws"), g.nbytes("ws"), ...))
    assert g.verdict() == []                # plain sentences, empty when clean
    got = g.result("out")

run() makes the call once from NaN everywhere the kernel is to write; when the call has a workspace, a second time with the workspace at the finite
1e30 instead (the two outputs must be bit-equal: a kernel that reads a workspace element before any slice wrote it cannot pass both).  Only when
a NaN is found in an output does it call again: from another output fill (a NaN that is there again was computed; one that is not was never
written) and, for a computed NaN, once per input with that input's margins finite (the input whose margins make the NaN go away was read beyond)."""
import ctypes

import torch

LINE = 256
DEFAULT_MARGIN = 64 * 1024
IN_MARGIN = 0xFF            # NaN as fp32 / fp16
OUT_MARGIN = 0xA5
UNWRITTEN = 0xFF            # NaN where the kernel is to write
ALT_UNWRITTEN = 0x5A        # the second output fill: 0x5A5A5A5A = 1.54e16 as fp32, finite
WS_FINITE = 1e30
KINDS = ("in", "out", "ws", "inout")


def _round_up(n, m):
    return (n + m - 1) // m * m


def offsets16(n, start=0):
    """n distinct byte offsets inside a 256-byte line, multiples of 16 that are no multiples of 64 (12 of them exist; they repeat beyond that,
    rotated by `start`)."""
    pool = [o for o in range(16, LINE, 16) if o % 64]
    return [pool[(start + i) % len(pool)] for i in range(n)]


class _Op:
    __slots__ = ("name", "kind", "nbytes", "offset", "shape", "dtype", "payload", "lo", "start", "end", "hi")


class Guard:
    def __init__(self, device, margin=DEFAULT_MARGIN):
        assert isinstance(margin, int) and margin > 0 and margin % 16 == 0, f"margin {margin!r}: a positive multiple of 16 bytes"
        self.device, self.margin = torch.device(device), margin
        self.ops, self.mem, self._sentences, self._results, self.rcs = {}, None, [], {}, []

    # ------------------------------------------------------------------------------------------------------------- declaring operands
    def _add(self, name, kind, nbytes, offset, shape, dtype, payload):
        assert self.mem is None, "declare every operand before the first run()"
        assert name not in self.ops, f"operand {name!r} declared twice"
        assert isinstance(offset, int) and 0 <= offset < LINE and offset % 16 == 0, \
            f"operand {name!r}: offset {offset!r} is no multiple of 16 inside a {LINE}-byte line (the entry points promise 16-byte alignment)"
        assert nbytes >= 0
        op = _Op()
        op.name, op.kind, op.nbytes, op.offset, op.shape, op.dtype, op.payload = name, kind, int(nbytes), offset, shape, dtype, payload
        self.ops[name] = op
        return name

    @staticmethod
    def _bytes(t):
        t = t.detach().cpu().contiguous()
        return t.reshape(-1).view(torch.uint8).clone(), tuple(t.shape), t.dtype

    def input(self, name, tensor, offset=0):
        """A read-only operand: the tensor's bytes (any dtype, made contiguous) between 0xFF margins."""
        b, shape, dtype = self._bytes(tensor)
        return self._add(name, "in", b.numel(), offset, shape, dtype, b)

    def inout(self, name, tensor, offset=0):
        """An operand the kernel updates in place: the tensor's bytes between 0xA5 margins."""
        b, shape, dtype = self._bytes(tensor)
        return self._add(name, "inout", b.numel(), offset, shape, dtype, b)

    def output(self, name, shape, offset=0, dtype=torch.float32):
        """An operand the kernel is to write completely: 0xFF bytes (NaN as fp32; -1 as int32) between 0xA5 margins."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        return self._add(name, "out", torch.empty(0, dtype=dtype).element_size() * n, offset, shape, dtype, None)

    def workspace(self, name, nbytes, offset=0):
        """A workspace of exactly `nbytes` bytes (what the query answered; 0: the operand is NULL)."""
        assert nbytes >= 0 and nbytes % 4 == 0, f"workspace {name!r}: {nbytes} bytes (a negative answer of a query is its error code)"
        return self._add(name, "ws", nbytes, offset, (nbytes // 4,), torch.float32, None)

    # ------------------------------------------------------------------------------------------------------------- the arena
    def _allocate(self):
        cur = 0
        for op in self.ops.values():
            op.lo = cur
            op.start = _round_up(cur + self.margin, LINE) + op.offset
            op.end = op.start + op.nbytes
            op.hi = _round_up(op.end, LINE) + self.margin
            cur = op.hi
        self.total = cur
        self._buf = torch.empty(cur + LINE, dtype=torch.uint8, device=self.device)          # the ONE allocation of this call
        shift = -self._buf.data_ptr() % LINE
        self.mem = self._buf[shift:shift + cur]
        assert self.mem.data_ptr() % LINE == 0
        for op in self.ops.values():
            if op.payload is not None:
                op.payload = op.payload.to(self.device)
        self.check_layout()

    def check_layout(self):
        """The arithmetic the tests rely on: margins, placement and sizes."""
        prev = 0
        for op in self.ops.values():
            assert op.lo == prev and op.start - op.lo >= self.margin and op.hi - op.end >= self.margin, (op.name, op.lo, op.start, op.end, op.hi)
            assert (self.mem.data_ptr() + op.start) % LINE == op.offset and op.end - op.start == op.nbytes, (op.name, op.start, op.offset)
            prev = op.hi
        assert prev == self.total == self.mem.numel()

    def _fill(self, ws_fill, out_byte, finite_margins=()):
        if self.mem is None:
            self._allocate()
        m = self.mem
        for op in self.ops.values():
            edge = 0 if op.name in finite_margins else (IN_MARGIN if op.kind == "in" else OUT_MARGIN)
            m[op.lo:op.start].fill_(edge)
            m[op.end:op.hi].fill_(edge)
            if op.payload is not None:
                m[op.start:op.end].copy_(op.payload)
            elif op.kind == "out":
                m[op.start:op.end].fill_(out_byte)
            elif ws_fill is None:
                m[op.start:op.end].fill_(UNWRITTEN)
            elif op.nbytes:
                m[op.start:op.end].view(torch.float32).fill_(ws_fill)
        self._pristine = m.clone()

    def ptr(self, name):
        """The device address of the operand as a ctypes pointer; None (NULL) for an empty workspace."""
        op = self.ops[name]
        if self.mem is None:
            self._allocate()
        if op.kind == "ws" and op.nbytes == 0:
            return None
        return ctypes.c_void_p(self.mem.data_ptr() + op.start)

    def nbytes(self, name):
        return self.ops[name].nbytes

    def view(self, name):
        """The operand as a tensor view of the arena, in its own dtype and shape."""
        op = self.ops[name]
        if self.mem is None:
            self._allocate()
        return self.mem[op.start:op.end].view(op.dtype).view(op.shape)

    def window(self, name, before=0, after=0):
        """The operand with `before` / `after` ELEMENTS of its margins on either side, flat - what a stand-in kernel with an addressing fault
        sees.  (A real kernel gets ptr() and sees the same memory.)"""
        op = self.ops[name]
        if self.mem is None:
            self._allocate()
        sz = torch.empty(0, dtype=op.dtype).element_size()
        assert before * sz <= op.start - op.lo and after * sz <= op.hi - op.end
        return self.mem[op.start - before * sz:op.end + after * sz].view(op.dtype)

    # ------------------------------------------------------------------------------------------------------------- running and judging
    def _call(self, call, ws_fill, out_byte, finite_margins=()):
        self._fill(ws_fill, out_byte, finite_margins)
        rc = call(self)
        self.rcs.append(rc)
        return rc

    def _first(self, mask):
        return int(mask.reshape(-1).to(torch.uint8).argmax())

    def _inspect(self, when=""):
        """Sentences about inputs and margins that differ from what _fill() left."""
        changed = self.mem != self._pristine
        for op in self.ops.values():
            if op.kind != "in":
                changed[op.start:op.end] = False
        if not bool(changed.any()):
            return []
        out = []
        for op in self.ops.values():
            what = {"in": "input", "out": "output", "ws": "workspace", "inout": "in-place operand"}[op.kind]
            if op.kind == "in" and bool(changed[op.start:op.end].any()):
                i = self._first(changed[op.start:op.end])
                out.append(f"{what} {op.name!r} changed{when}: first at byte {i} of {op.nbytes} (element {i // self._esize(op)})")
            seg = changed[op.lo:op.start]
            if bool(seg.any()):
                n, last = int(seg.sum()), op.start - op.lo - 1 - self._first(seg.flip(0))
                out.append(f"margin BEFORE {what} {op.name!r} changed{when}: {n} bytes, the nearest {op.start - op.lo - last} bytes in front of its "
                           f"first byte, the farthest {op.start - op.lo - self._first(seg)}")
            seg = changed[op.end:op.hi]
            if bool(seg.any()):
                out.append(f"margin AFTER {what} {op.name!r} changed{when}: {int(seg.sum())} bytes, first at byte {self._first(seg)} past its end "
                           f"(its size: {op.nbytes} bytes)")
        return out

    @staticmethod
    def _esize(op):
        return torch.empty(0, dtype=op.dtype).element_size()

    def _snapshot(self):
        return {op.name: self.mem[op.start:op.end].clone() for op in self.ops.values() if op.kind in ("out", "inout")}

    def _index(self, op, flat):
        idx, rem = [], flat
        for s in reversed(op.shape):
            idx.append(rem % s)
            rem //= s
        return f"flat index {flat} = {tuple(reversed(idx))} of {op.shape}"

    def run(self, call, want=None):
        """call(guard) -> return code, made from NaN outputs (and NaN workspaces), then again as the module docstring says.  `want`: {output name:
        the expected tensor}, used only to say what a NaN should have been.  Returns the first call's return code; verdict() has the findings."""
        self._sentences, self.rcs = [], []
        rc = self._call(call, None, UNWRITTEN)
        self._sentences += self._inspect()
        first = self._snapshot()
        self._results = first
        has_ws = any(op.kind == "ws" and op.nbytes for op in self.ops.values())
        second = None
        if has_ws:
            rc2 = self._call(call, WS_FINITE, UNWRITTEN)
            if rc2 != rc:
                self._sentences.append(f"return code {rc} from a NaN workspace, {rc2} from a workspace of {WS_FINITE:g}")
            when = f" (workspace filled with {WS_FINITE:g})"
            self._sentences += [s for s in self._inspect(when) if s.replace(when, "") not in self._sentences]
            second = self._snapshot()
            for name, a in first.items():
                if not torch.equal(a, second[name]):
                    op = self.ops[name]
                    i = self._first(a != second[name]) // self._esize(op)
                    va, vb = a.view(op.dtype)[i].item(), second[name].view(op.dtype)[i].item()
                    self._sentences.append(f"output {name!r} depends on what the workspace held before the call (an element read before any slice "
                                           f"wrote it): {self._index(op, i)} is {va!r} from a NaN workspace and {vb!r} from a workspace of {WS_FINITE:g}")
        nan = {name: torch.isnan(a.view(torch.float32)) for name, a in first.items()
               if self.ops[name].kind == "out" and self.ops[name].dtype == torch.float32}
        if any(bool(m.any()) for m in nan.values()):
            self._call(call, None, ALT_UNWRITTEN)
            third = self._snapshot()
            fill = torch.full((1,), ALT_UNWRITTEN, dtype=torch.uint8).repeat(4).view(torch.float32).item()
            for name, m in nan.items():
                if not bool(m.any()):
                    continue
                op, t = self.ops[name], third[name].view(torch.float32)
                ref = ""
                unwritten = m & (t == fill)
                computed = m & torch.isnan(t)
                other = m & ~unwritten & ~computed
                for mask, text in ((unwritten, "left unwritten (they keep whatever the output held before the call)"),
                                   (other, "NaN from a NaN output but not from a finite one: the kernel reads its output before writing it")):
                    if bool(mask.any()):
                        i = self._first(mask)
                        if want is not None and name in want:
                            ref = f", where the reference has {want[name].reshape(-1)[i].item()!r}"
                        self._sentences.append(f"output {name!r}: {int(mask.sum())} of {m.numel()} elements {text}; first {self._index(op, i)}{ref}")
                if bool(computed.any()):
                    i = self._first(computed)
                    if want is not None and name in want:
                        ref = f", where the reference has the finite {want[name].reshape(-1)[i].item()!r}"
                    src = self._trace_nan(call, name, i, second)
                    self._sentences.append(f"output {name!r}: {int(computed.sum())} of {m.numel()} elements are NaN that the kernel computed (the same NaN "
                                           f"from another output fill); first {self._index(op, i)}{ref}; {src}")
        # leave the arena as the first run left it is not needed: result() serves the first run's copies
        return rc

    def _trace_nan(self, call, name, i, second):
        if second is not None and not bool(torch.isnan(second[name].view(torch.float32)[i])):
            return "it is finite from a finite workspace: a workspace element was read before it was written"
        found = []
        for op in self.ops.values():
            if op.kind != "in":
                continue
            self._call(call, None, UNWRITTEN, finite_margins=(op.name,))
            if not bool(torch.isnan(self._snapshot()[name].view(torch.float32)[i])):
                found.append(op.name)
        if found:
            return "it is finite when the margins of input " + " / ".join(repr(f) for f in found) + " are finite: the kernel reads beyond that input"
        return "no single input's margins account for it"

    def verdict(self):
        """The findings of the last run() as plain sentences; empty when clean."""
        return list(self._sentences)

    def result(self, name):
        """The operand as the FIRST call of the last run() left it (a copy), in its dtype and shape."""
        op = self.ops[name]
        return self._results[name].view(op.dtype).view(op.shape)


def first_difference(got, want, names="index"):
    """None if torch.equal, else a sentence naming the first differing index (the way trunk34_forms.first_difference does)."""
    if got.shape == want.shape and torch.equal(got, want):
        return None
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)}, wanted {tuple(want.shape)}"
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return f"{bad.shape[0]} of {got.numel()} outputs differ; first {names} = {i}: got {float(got[i])!r}, want {float(want[i])!r}"
