"""Guard-band buffers for the kernel bounds tests (tests/test_kernel_bounds_gpu.py, proven on CPU stand-ins by tests/test_guard_cpu.py).

Every buffer a kernel receives lives inside ONE flat byte tensor owned by the test:

    [front guard | payload: rows x cols elements, row pitch ld >= cols | back guard]

The payload starts on a 256-byte boundary and ends after the last column of the last row (the pitch padding of the last row already belongs
to the back guard).  Both guards are part of the allocation, so a kernel that strays into them corrupts test memory and cannot fault.  The
caller passes the guard size and says which tile it was sized for (`guard_bytes` gives the usual max(64 KiB, 256 rows of the pitch)).

  inputs    (`guard_in`)   guards and pitch padding are POISONED: NaN for fp32 / fp64 / bf16 / f16, f16 NaN in both halves for f16x2 operand
                           buffers (int32 storage, poison="nan16"), a caller-chosen illegal byte for uint8 / int32 data.  A stray read that
                           reaches an output then shows in the comparison with the reference / the plain call.
  outputs   (`guard_out`)  the whole allocation is filled with the byte 0xA5 before the call.
  workspace (`guard_ws`)   an output of exactly the bytes the matching uni_*_workspace_bytes function returns.

After the call (and a synchronise) `Guarded.check()` demands that every guard byte and every pitch-padding byte still holds what it held
before the call, and -- for outputs that the header documents as completely written -- that no aligned 4-byte word of the payload still
holds the fill pattern.  `check_equal` compares the payload bit for bit with the result of the plain call (contiguous, exact-size tensors).
Every failure is a `GuardError` that names the buffer and the byte offset relative to the payload start (negative: front guard).

What the method CANNOT see: a stray write beyond the guard width, and a stray read whose value is discarded (multiplied away by a select,
masked lanes, a prefetch that is never consumed).  It sees every stray write inside the guard width and every stray read whose value
reaches an output.

This is a plain module imported like tests/planted.py; it holds no fixture and changes no pytest setting."""
import json
import os
import time

import torch

FILL = 0xA5
ALIGN = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def results_dir():
    """The suite's results directory: the one tests/test_model_gpu.py::_dump writes parity_metrics.json into, which is the directory that
    .gitignore lists for results (its one plain `<name>_out/` entry).  Anything else -- no such entry, or more than one -- is an error:
    the report never moves somewhere else silently.  tests/test_guard_cpu.py holds the answer to _dump's own directory."""
    with open(os.path.join(ROOT, ".gitignore")) as f:
        found = [ln.strip().strip("/") for ln in f if ln.strip().endswith("_out/") and not set(ln) & set("*?[!#")]
    if len(found) != 1:
        raise RuntimeError("guard report: .gitignore must list exactly one results directory `<name>_out/`, found %r" % (found,))
    return os.path.join(ROOT, found[0])


def report_path():
    return os.path.join(results_dir(), "guard_report.json")


REPORT = None          # tests may set a path of their own; None: report_path(), resolved when the file is written
_SESSION_START = time.time()
_RECORDS = {}

_NAN_VIEW = {"nan16": torch.float16, "nanbf16": torch.bfloat16, "nan32": torch.float32, "nan64": torch.float64}
_DEFAULT_POISON = {torch.float16: "nan16", torch.bfloat16: "nanbf16", torch.float32: "nan32", torch.float64: "nan64"}


class GuardError(AssertionError):
    """a buffer contract was broken; .buffer and .offset (bytes from the payload start) locate it"""

    def __init__(self, buffer, offset, what):
        self.buffer, self.offset, self.what = buffer, int(offset), what
        AssertionError.__init__(self, "buffer '%s': %s at byte offset %d from the payload start" % (buffer, what, int(offset)))


def guard_bytes(ld, esize, floor=64 * 1024, rows=256):
    """the usual guard width: max(64 KiB, `rows` (the tallest tile: 256) x row pitch in bytes)"""
    return max(int(floor), int(rows) * int(ld) * int(esize))


def _first(mask):
    """index of the first set element of a flat boolean tensor (or -1)"""
    if not bool(mask.any()):
        return -1
    return int(mask.reshape(-1).to(torch.uint8).argmax())          # argmax returns the first of equal maxima


class Guarded:
    """one guarded buffer; .view is the (rows, cols) strided tensor of the payload, .ptr its device address"""

    def __init__(self, name, kind, rows, cols, dtype, ld, guard, device, poison):
        ld = cols if ld is None else int(ld)
        assert ld >= cols and rows >= 0 and cols >= 0 and guard >= 0
        self.name, self.kind, self.rows, self.cols, self.ld, self.dtype = name, kind, int(rows), int(cols), ld, dtype
        self.esize = torch.empty((), dtype=dtype).element_size()
        self.guard = int(guard)
        self.nbytes = ((self.rows - 1) * ld + self.cols) * self.esize if self.rows and self.cols else 0     # payload extent, pitch included
        front = -(-self.guard // ALIGN) * ALIGN
        total = front + -(-(self.nbytes + self.guard) // ALIGN) * ALIGN + ALIGN
        self.base = torch.empty(total, dtype=torch.uint8, device=device)
        self.off = front + (-self.base.data_ptr() - front) % ALIGN                  # payload start on a 256-byte boundary
        assert (self.base.data_ptr() + self.off) % ALIGN == 0 and self.off + self.nbytes + self.guard <= total
        if kind == "in":
            poison = _DEFAULT_POISON.get(dtype) if poison is None else poison
            assert poison is not None, "integer inputs need an explicit poison byte (a value that is not legal data)"
            if isinstance(poison, str):
                self.base.view(_NAN_VIEW[poison]).fill_(float("nan"))
            else:
                self.base.fill_(int(poison))
        else:
            self.base.fill_(FILL)
        self.poison = poison
        self._snap = None

    # -- views ---------------------------------------------------------------------------------------------------
    @property
    def ptr(self):
        return self.base.data_ptr() + self.off

    @property
    def view(self):
        flat = self.base[self.off:self.off + self.nbytes].view(self.dtype)
        return torch.as_strided(flat, (self.rows, self.cols), (self.ld, 1)) if self.nbytes else flat.reshape(self.rows, self.cols)

    def payload(self):
        """contiguous (rows, cols) copy of the payload"""
        return self.view.clone(memory_format=torch.contiguous_format)

    def _payload_mask(self):
        """bool per byte of the allocation: True inside the payload columns"""
        m = torch.zeros(self.base.numel(), dtype=torch.bool, device=self.base.device)
        if self.nbytes:
            body = m[self.off:self.off + self.nbytes]
            torch.as_strided(body, (self.rows, self.cols * self.esize), (self.ld * self.esize, 1)).fill_(True)
        return m

    def arm(self):
        """remember the allocation as it is handed to the kernel (call after the payload of an input / in-place buffer is set)"""
        self._snap = self.base.clone()
        return self

    # -- checks --------------------------------------------------------------------------------------------------
    def check(self, complete=None):
        """guards and pitch padding unchanged since arm(); complete=True: no aligned 4-byte payload word still holds the fill pattern
        (default: True for outputs / False for inputs and workspaces)"""
        assert self._snap is not None, "arm() the buffer before the call"
        changed = (self.base != self._snap) & ~self._payload_mask()
        i = _first(changed)
        if i >= 0:
            rel = i - self.off
            if rel < 0:
                where = "front guard"
            elif rel >= self.nbytes:
                where = "back guard"
            else:
                where = "row padding (row %d, byte %d of the pitch)" % (rel // (self.ld * self.esize), rel % (self.ld * self.esize))
            raise GuardError(self.name, rel, "%s changed (0x%02x -> 0x%02x)" % (where, int(self._snap[i]), int(self.base[i])))
        if complete is None:                     # byte-valued outputs: 0xA5 may be data, they are compared with the plain call instead
            complete = self.kind == "out" and self.esize > 1
        if complete and self.nbytes:
            # per aligned 4-byte word; rows whose byte count or pitch is no multiple of 4 (bf16 rows of odd width) per element
            unit = 4 if (self.cols * self.esize) % 4 == 0 and (self.ld * self.esize) % 4 == 0 else self.esize
            vt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[unit]
            words = torch.as_strided(self.base[self.off:self.off + self.nbytes].view(vt), (self.rows, self.cols * self.esize // unit),
                                     (self.ld * self.esize // unit, 1))
            pat = int.from_bytes(bytes([FILL] * unit), "little", signed=unit > 1)
            i = _first(words == pat)
            if i >= 0:
                wpr = self.cols * self.esize // unit
                raise GuardError(self.name, (i // wpr) * self.ld * self.esize + (i % wpr) * unit,
                                 "payload word never written (still 0x%s)" % ("A5" * unit))
        return self

    def check_equal(self, plain, what="the plain call"):
        """payload bit for bit equal to `plain` ((rows, cols) tensor of the same dtype)"""
        got = self.payload()
        plain = plain.reshape(self.rows, self.cols).contiguous()
        assert plain.dtype == self.dtype, (plain.dtype, self.dtype)
        gb = got.view(torch.uint8).reshape(self.rows, -1)
        pb = plain.to(got.device).view(torch.uint8).reshape(self.rows, -1)
        i = _first(gb != pb)
        if i >= 0:
            rb = self.cols * self.esize
            r, c = i // rb, i % rb
            e = c // self.esize
            raise GuardError(self.name, r * self.ld * self.esize + c,
                             "payload differs from %s (row %d, col %d: %r vs %r)" % (what, r, e, got[r, e].item(), plain[r, e].item()))
        return self


def guard_in(name, t, ld=None, guard=64 * 1024, poison=None):
    """input buffer around the 2-D (rows, cols) tensor `t` (1-D tensors are one row); armed"""
    t = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    g = Guarded(name, "in", t.shape[0], t.shape[1], t.dtype, ld, guard, t.device, poison)
    if g.nbytes:
        g.view.copy_(t)
    return g.arm()


def guard_out(name, rows, cols, dtype, device, ld=None, guard=64 * 1024, init=None):
    """output buffer filled with 0xA5 (init: a (rows, cols) tensor for in-place outputs, e.g. a residual that `out` aliases); armed"""
    g = Guarded(name, "out", rows, cols, dtype, ld, guard, device, None)
    if init is not None and g.nbytes:
        g.view.copy_(init.reshape(rows, cols))
    return g.arm()


def guard_ws(name, nbytes, device, guard=64 * 1024):
    """workspace of EXACTLY nbytes (what the size function returned) filled with 0xA5; armed"""
    g = Guarded(name, "ws", 1, int(nbytes), torch.uint8, None, guard, device, None)
    return g.arm()


def check_all(*bufs):
    for b in bufs:
        if b is not None:
            b.check()


# -- results file -----------------------------------------------------------------------------------------------------
def record(entry, variant, shape, strides, bufs, workspace_bytes=0, bitwise=True, note=""):
    """one record per case into guard_report.json in the results directory (merged into a file of this session, like tests/test_model_gpu.py::_dump)"""
    key = "%s | %s | %s" % (entry, variant, shape)
    _RECORDS[key] = {"entry": entry, "variant": variant, "shape": shape, "strides": strides,
                     "guard_bytes": {b.name: b.guard for b in bufs if b is not None}, "workspace_bytes": int(workspace_bytes),
                     "bitwise_vs_plain": bool(bitwise), "note": note}


def dump():
    path = REPORT or report_path()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    old = {}
    try:
        if os.path.getmtime(path) >= _SESSION_START - 1.0:
            old = json.load(open(path))
    except (OSError, ValueError):
        old = {}
    old.update(_RECORDS)
    with open(path, "w") as f:
        json.dump(old, f, indent=1)
