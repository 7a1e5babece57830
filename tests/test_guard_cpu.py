"""The guard-band checker (tests/guard.py) on CPU tensors with small Python stand-ins for a kernel: it must accept a correct stand-in and
name the buffer and the byte offset of each planted fault.  This is the only place where wrong behaviour is planted; no GPU kernel is ever
built or run out of bounds on purpose."""
import json
import os

import pytest
import torch

import guard as G

ROWS, COLS, LDX, LDO = 37, 20, 24, 28            # ragged payload, padded pitches (16-byte aligned rows like the launchers ask for)
WS_BYTES = 1000


def _kernel(x, ldx, out, ldo, ws, ws_bytes, rows, cols, fault=None):
    """out[r][c] = 2 x[r][c] + 1 with a row-sum scratch in ws; the stand-in works on FLAT element views that start at the payload, like
    a kernel that gets a pointer and a leading dimension.  Negative flat indices reach in front of the payload."""
    for r in range(rows):
        n = cols + 1 if fault == "read_padding" and r == 5 else cols
        row = x[r * ldx:r * ldx + n]
        val = row[:cols] * 2 + 1
        if fault == "read_padding" and r == 5:
            val[cols - 1] += row[cols]                       # a tail load that is not masked
        if fault == "skip" and r == 11:
            out[r * ldo:r * ldo + cols - 1] = val[:cols - 1]      # the last column of one row is never stored
        else:
            out[r * ldo:r * ldo + cols] = val
    ws[:ws_bytes] = 7                                        # the scratch the kernel really uses
    if fault == "past_end":
        out[(rows - 1) * ldo + cols] = 1.0                   # one element behind the last payload element
    if fault == "row_padding":
        out[3 * ldo + cols + 2] = 1.0                        # the third padding element of row 3
    if fault == "front":
        out[-1] = 1.0                                        # one element in front of the payload
    if fault == "ws_overrun":
        ws[ws_bytes] = 7                                     # the size function was one byte short


def _flat(g, dtype):
    """flat view of the allocation that starts at the payload (negative indices = front guard), the way a raw pointer sees it"""
    class Ptr:
        def __init__(self, base, off):
            self.t, self.o = base.view(dtype), off // torch.empty((), dtype=dtype).element_size()

        def _ix(self, k):
            if isinstance(k, slice):
                return slice(self.o + k.start if k.start is not None else self.o, self.o + k.stop)
            return self.o + k

        def __getitem__(self, k):
            return self.t[self._ix(k)].clone()

        def __setitem__(self, k, v):
            self.t[self._ix(k)] = v
    assert g.off % 8 == 0
    return Ptr(g.base, g.off)


def _run(fault):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(ROWS, COLS, generator=gen)
    gx = G.guard_in("x", x, ld=LDX, guard=G.guard_bytes(LDX, 4, floor=4096, rows=8))
    go = G.guard_out("out", ROWS, COLS, torch.float32, "cpu", ld=LDO, guard=G.guard_bytes(LDO, 4, floor=4096, rows=8))
    gw = G.guard_ws("workspace", WS_BYTES, "cpu", guard=4096)
    _kernel(_flat(gx, torch.float32), LDX, _flat(go, torch.float32), LDO, _flat(gw, torch.uint8), WS_BYTES, ROWS, COLS, fault)
    plain = x * 2 + 1                                        # "the same entry point called the ordinary way"
    G.check_all(gx, go, gw)
    go.check_equal(plain)
    return gx, go, gw


def test_layout_alignment_and_poison():
    gx, go, gw = _run(None)
    for g in (gx, go, gw):
        assert g.ptr % 256 == 0 and g.off >= g.guard
        assert g.base.numel() - g.off - g.nbytes >= g.guard
    assert gx.nbytes == ((ROWS - 1) * LDX + COLS) * 4          # the payload ends after the last column of the last row
    flat = gx.base.view(torch.float32)
    assert torch.isnan(flat[:gx.off // 4]).all() and torch.isnan(flat[(gx.off + gx.nbytes) // 4:]).all()
    pitch = torch.as_strided(flat[gx.off // 4:], (ROWS - 1, LDX - COLS), (LDX, 1), COLS)
    assert torch.isnan(pitch).all() and torch.isfinite(gx.view).all()
    assert (go.base[:go.off] == G.FILL).all() and (gw.base[gw.off + WS_BYTES:] == G.FILL).all()
    assert gw.nbytes == WS_BYTES
    # f16x2 operand buffers: int32 storage, f16 NaN in both halves of every word
    gh = G.guard_in("a_h2", torch.zeros(4, 16, dtype=torch.int32), ld=24, guard=1024, poison="nan16")
    assert torch.isnan(gh.base[:gh.off].view(torch.float16)).all() and (gh.view == 0).all()
    # integer inputs take a caller-chosen illegal byte
    gm = G.guard_in("mask", torch.ones(5, 7, dtype=torch.uint8), ld=16, guard=512, poison=0x7F)
    assert (gm.base[:gm.off] == 0x7F).all() and (gm.view == 1).all() and int(gm.base[gm.off + 7]) == 0x7F
    with pytest.raises(AssertionError):
        G.guard_in("ids", torch.ones(5, dtype=torch.int32), guard=512)          # no default poison for integers


def test_correct_kernel_is_accepted():
    _run(None)


@pytest.mark.parametrize("fault,buffer,offset", [
    ("past_end", "out", ((ROWS - 1) * LDO + COLS) * 4),          # first byte behind the payload
    ("row_padding", "out", (3 * LDO + COLS + 2) * 4),
    ("front", "out", -4),
    ("skip", "out", (11 * LDO + COLS - 1) * 4),
    ("read_padding", "out", (5 * LDO + COLS - 1) * 4),           # where the poisoned value surfaces
    ("ws_overrun", "workspace", WS_BYTES),
])
def test_planted_fault_is_named(fault, buffer, offset):
    with pytest.raises(G.GuardError) as e:
        _run(fault)
    assert e.value.buffer == buffer and e.value.offset == offset, str(e.value)
    assert ("'%s'" % buffer) in str(e.value) and ("byte offset %d" % offset) in str(e.value)


def test_fault_kinds_are_told_apart():
    what = {}
    for fault in ("past_end", "row_padding", "front", "skip", "read_padding", "ws_overrun"):
        with pytest.raises(G.GuardError) as e:
            _run(fault)
        what[fault] = e.value.what
    assert "back guard" in what["past_end"] and "back guard" in what["ws_overrun"] and "front guard" in what["front"]
    assert "row padding (row 3" in what["row_padding"] and "never written" in what["skip"] and "differs" in what["read_padding"]


def test_input_guard_write_and_inplace_output():
    """a kernel that scribbles into an INPUT's padding is caught too; an in-place output (out aliases the residual) starts from real data"""
    x = torch.randn(6, 8)
    gx = G.guard_in("x", x, ld=12, guard=256)
    gx.base.view(torch.float32)[gx.off // 4 + 9] = 0.0
    with pytest.raises(G.GuardError) as e:
        gx.check()
    assert e.value.buffer == "x" and e.value.offset == 38          # fp32 NaN is 00 00 c0 7f: the first byte that 0.0 changes is the third
    go = G.guard_out("out", 6, 8, torch.float32, "cpu", ld=12, guard=256, init=x)
    go.view.add_(1.0)
    go.check().check_equal(x + 1.0)


def test_report_merges(tmp_path, monkeypatch):
    monkeypatch.setattr(G, "REPORT", str(tmp_path / "out" / "guard_report.json"))
    monkeypatch.setattr(G, "_RECORDS", {})
    g = G.guard_ws("workspace", 10, "cpu", guard=256)
    G.record("uni_x", "cfg 0", "M=1", {"ld": 8}, [g], workspace_bytes=10, bitwise=True)
    G.dump()
    monkeypatch.setattr(G, "_RECORDS", {})
    G.record("uni_y", "cfg 1", "M=2", {"ld": 8}, [g], bitwise=False, note="fp64 atomics")
    G.dump()
    rep = json.load(open(G.REPORT))
    assert len(rep) == 2
    assert any(r["entry"] == "uni_y" and not r["bitwise_vs_plain"] and r["guard_bytes"] == {"workspace": 256} for r in rep.values())


def test_report_goes_where_the_model_tests_write():
    """the report's directory is the one tests/test_model_gpu.py::_dump uses for parity_metrics.json, by that function's own text"""
    d = G.results_dir()
    assert os.path.dirname(d) == G.ROOT and os.path.basename(G.report_path()) == "guard_report.json"
    with open(os.path.join(G.ROOT, "tests", "test_model_gpu.py")) as f:
        src = f.read()
    assert 'os.path.join(ROOT, "%s", "parity_metrics.json")' % os.path.basename(d) in src
