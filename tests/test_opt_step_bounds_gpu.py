"""Guard-band run of uni_opt_step on the ragged list (the method of tests/test_prop_loss_bounds_gpu.py): every array of every entry, both
tables and the four state words are tests/guard.py allocations [front guard | payload | back guard], NaN-poisoned around the payload (0xEE
bytes around integer data).  The payload of an array is its ENCLOSING storage (the entry may start 1 - 3 elements into it and ends 5 elements
before its end), the tables are exactly 64 n_tensors and 8 total_chunks bytes.  Guards must come back untouched and every payload BIT-EQUAL
to the plain call (ops.adamw_ema_step on exact-size tensors), which also shows that a stray read reached no output.  Then the error codes."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import opt_step_ref as R  # noqa: E402

DEV = "cuda"
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, d=0.9991, growth=2.0, backoff=0.5, interval=3)


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_opt_step_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def call(lib, L, table, table_bytes, bmap, map_bytes, N, vec_chunks, total, step, scale, tracker, found):
    h = HYPER
    return lib.uni_opt_step(table, table_bytes, bmap, map_bytes, N, vec_chunks, total, step, scale, tracker, found, h["lr"], h["beta1"], h["beta2"],
                            h["eps"], h["d"], h["growth"], h["backoff"], h["interval"], L.stream_ptr())


@pytest.mark.parametrize("scaler", [True, False])
def test_opt_step_stays_inside_its_buffers(L, scaler):
    from unicorn_amd import ops, optim
    lib = L.lib()
    ch = lib.uni_opt_chunk_elems()
    spec = R.ragged_spec(ch)
    cpu = R.ragged_draw(spec, 9, grad_scale=16.0 if scaler else 1.0)
    n = len(spec)
    lrf, wds = [0.1 if i % 4 == 0 else 1.0 for i in range(n)], [0.0 if i % 3 == 0 else 5e-4 for i in range(n)]

    # the plain call on exact-size tensors
    stor = {a: [None if t is None else t.to(DEV) for t in lst] for a, lst in cpu.items()}
    v = R.ragged_views(spec, stor)
    step = torch.full((), 7.0, device=DEV)
    words = (torch.full((), 16.0, device=DEV), torch.full((), 2, dtype=torch.int32, device=DEV), torch.ones((), device=DEV)) if scaler else None
    ops.adamw_ema_step(v["p"], v["g"], v["m"], v["v"], v["e"], step, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"],
                       weight_decay=wds, lr_factors=lrf, ema_decay=HYPER["d"], scaler=words, growth_factor=HYPER["growth"],
                       backoff_factor=HYPER["backoff"], growth_interval=HYPER["interval"])
    torch.cuda.synchronize()

    # the guarded call through the C-ABI
    gb = {a: [None if t is None else G.guard_in("%s[%d]" % (a, i), t.to(DEV), guard=G.guard_bytes(1, 4, floor=4096 if t.numel() < 64 else 65536))
              for i, t in enumerate(cpu[a])] for a in R.ARRAYS}
    cols = {a: [0 if g_ is None else g_.ptr + 4 * s["off"][j] for g_, s in zip(gb[a], spec)] for j, a in enumerate(R.ARRAYS)}
    cols.update(n=[s["n"] for s in spec], lr_factor=lrf, wd=wds, has_grad=[s["grad"] for s in spec])
    img, map_off, N, vec_chunks, total = optim.StepPlan.image(cols, ch, lib.uni_opt_table_bytes)
    assert N == n and 0 < vec_chunks < total
    gt = G.guard_in("table", torch.from_numpy(img[:N * 64].copy()).to(DEV), poison=0xEE)
    gm = G.guard_in("block_map", torch.from_numpy(img[map_off:map_off + total * 8].copy()).to(DEV), poison=0xEE)
    gs = G.guard_in("step", torch.full((1,), 7.0, device=DEV))
    gw = [G.guard_in("scale", torch.full((1,), 16.0, device=DEV)), G.guard_in("growth_tracker", torch.full((1,), 2, dtype=torch.int32, device=DEV), poison=0xEE),
          G.guard_in("found_inf", torch.ones(1, device=DEV))] if scaler else [None, None, None]
    P = lambda g_: None if g_ is None else C.c_void_p(g_.ptr)      # noqa: E731
    L.check(call(lib, L, P(gt), N * 64, P(gm), total * 8, N, vec_chunks, total, P(gs), P(gw[0]), P(gw[1]), P(gw[2])), "uni_opt_step")
    torch.cuda.synchronize()
    every = [g_ for a in R.ARRAYS for g_ in gb[a]] + [gt, gm, gs] + gw
    G.check_all(*every)
    for a in R.ARRAYS:
        for g_, plain in zip(gb[a], stor[a]):
            if g_ is not None:
                g_.check_equal(plain)
    gs.check_equal(step.reshape(1))
    assert float(step) == 8.0
    if scaler:
        for g_, w in zip(gw, words):
            g_.check_equal(w.reshape(1))
        assert float(words[0]) == 32.0 and int(words[1]) == 0 and float(words[2]) == 0.0          # the tracker reached growth_interval = 3
    changed = sum(1 for g_, t in zip(gb["p"], cpu["p"]) if not torch.equal(g_.payload().cpu().reshape(-1), t))
    assert changed == sum(1 for s in spec if s["grad"] and s["n"])                              # the step did run on every entry with a gradient
    G.record("uni_opt_step", "scaler=%d" % scaler, "ragged list: %d tensors, %d chunks (%d vec)" % (N, total, vec_chunks), {},
             [gt, gm, gs] + [g_ for g_ in gw if g_ is not None] + [gb["p"][8], gb["g"][8]], workspace_bytes=0)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(1 << 12, device=DEV)
    X = C.c_void_p(x.data_ptr())
    ok = dict(table=X, table_bytes=128, bmap=X, map_bytes=16, N=2, vec_chunks=1, total=2, step=X, scale=X, tracker=X, found=X)
    for change, what in (({"table": None}, "NULL"), ({"bmap": None}, "NULL"), ({"step": None}, "NULL"), ({"table_bytes": 127}, "too small"),
                         ({"map_bytes": 15}, "too small"), ({"N": -1}, "negative"), ({"total": -2, "vec_chunks": -2}, "negative"),
                         ({"vec_chunks": 3}, "vec_chunks"), ({"found": None}, "NULL"), ({"tracker": None}, "NULL")):
        a = dict(ok, **change)
        rc = call(lib, L, a["table"], a["table_bytes"], a["bmap"], a["map_bytes"], a["N"], a["vec_chunks"], a["total"], a["step"], a["scale"],
                  a["tracker"], a["found"])
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    torch.cuda.synchronize()
    assert not x.any()                                      # a refused call launches nothing
    assert lib.uni_opt_table_bytes(-1, 4) == 0 and lib.uni_opt_table_bytes(3, -1) == 0
