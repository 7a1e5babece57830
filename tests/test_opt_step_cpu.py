"""CPU side of the fused AdamW + loss-scale + EMA step (uni_opt_step, ops.adamw_ema_step, unicorn_amd.optim.FusedAdamWEMA): the per-element
restatement of tests/opt_step_ref.py reproduces the fixtures that torch.optim.AdamW, torch.amp.GradScaler and the reference's ModelEMA
produced (tests/golden/opt_step_*.npz) to 1e-12 of scale in fp64, and step / scale / growth_tracker exactly; the fixtures equal their
seeded draw and show the skipped step; the C-ABI symbols are declared, bound and exported; the table image is what the header states; the
Python surface refuses bad arguments before it touches the library; state_dict() has AdamW's keys."""
import os
import re

import numpy as np
import pytest
import torch

import opt_step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_opt_chunk_elems": 0, "uni_opt_table_bytes": 2, "uni_opt_step": 20}


@pytest.fixture(scope="module")
def cases():
    return {tag: R.load_case(tag) for tag in R.CASES}


@pytest.mark.parametrize("tag", list(R.CASES))
def test_restatement_reproduces_the_fixture_in_fp64(cases, tag):
    c = cases[tag]
    got = R.run_case(tag, c, torch.float64)
    for kind in R.FLOAT_RESULTS:
        den = max(float(np.abs(c["%s_%s" % (kind, n)]).max()) for n in got["names"])
        for n, t in zip(got["names"], got[kind]):
            ref = c["%s_%s" % (kind, n)]
            assert ref.dtype == np.float64 and t.dtype == torch.float64 and tuple(t.shape) == ref.shape, (tag, kind, n)
            err = float(np.abs(t.numpy() - ref).max()) / den
            assert err <= 1e-12, (tag, kind, n, err)
    assert got["step"] == float(c["step"])
    if R.CASES[tag]["scaler"]:
        assert got["scale"] == float(c["scale"]) and got["tracker"] == int(c["growth_tracker"])
        assert got["skipped"] == [k == R.CASES[tag]["bad_step"] for k in range(R.CASES[tag]["steps"])]
    else:
        assert not any(got["skipped"])


def test_fixtures_equal_their_seeded_draw_and_show_the_skipped_step(cases):
    for tag, c in cases.items():
        cfg = R.CASES[tag]
        ins = R.draw(tag, int(c["seed"]))
        assert len(c["scale_before"]) == cfg["steps"]
        for name, shape, kind in R.shapes(tag):
            assert np.array_equal(c["p0_" + name], ins["p0_" + name].numpy()) and c["p0_" + name].shape == tuple(shape), (tag, name)
            if kind == "ibuf":
                assert "e0_" + name not in c and "p_" + name not in c          # integer entries are not part of the operator's list
                continue
            assert np.array_equal(c["e0_" + name], ins["e0_" + name].numpy()) and c["e0_" + name].dtype == np.float32
            if kind != "param":
                assert "gs_" + name not in c and not c["m_" + name].any() and not c["v_" + name].any()
                assert np.array_equal(c["p_" + name], c["p0_" + name].astype(np.float64))       # EMA-only entries keep their parameter
                assert not np.array_equal(c["e_" + name], c["e0_" + name].astype(np.float64))
                continue
            for k in range(cfg["steps"]):
                exp = {"g_" + name: (ins["g_" + name][k] * float(c["scale_before"][k])).clone()}
                if cfg["bad_step"] == k:
                    full = {"g_" + n: torch.zeros(s) for n, s, kd in R.shapes(tag) if kd == "param"}
                    R.plant_bad(tag, full)
                    bad = ~torch.isfinite(full["g_" + name])
                    exp["g_" + name][bad] = full["g_" + name][bad]
                assert np.array_equal(c["gs_" + name][k], exp["g_" + name].numpy(), equal_nan=True), (tag, name, k)
        for kind in R.FLOAT_RESULTS:
            assert 1e-9 < float(c[kind + "_fp32_ref_err"]) < 1e-6, (tag, kind)
    sizes = [int(np.prod(s)) for _, s, _ in R.shapes("plain")]
    assert sizes[:12] == [1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 4099] and len(R.shapes("plain")[12][1]) == 4
    # the skipped step: 5 steps fed, 4 counted; the scale went 1024 -> 2048 -> (inf / NaN) 1024 -> 2048; the inf and the NaN sit in different tensors
    s = cases["scaled"]
    assert float(s["step"]) == 4.0 and s["scale_before"].tolist() == [1024.0, 1024.0, 2048.0, 1024.0, 1024.0] and float(s["scale"]) == 2048.0
    assert int(s["growth_tracker"]) == 0
    assert np.isinf(s["gs_t07"][2]).sum() == 1 and np.isnan(s["gs_t11"][2]).sum() == 1
    assert sum(int((~np.isfinite(s[k])).sum()) for k in s if k.startswith("gs_")) == 2
    # groups: two lr factors, weight decay 0 on some tensors
    n = len(R.shapes("groups"))
    assert {R.group_of("groups", i)[0] for i in range(n)} == {0.1, 1.0} and {R.group_of("groups", i)[1] for i in range(n)} == {0.0, 1.0}
    src = open(os.path.join(R.GOLDEN, "make_golden_opt_step.py")).read()
    assert "ModelEMA" in src and "torch.optim.AdamW" in src and "GradScaler" in src and "foreach=False" in src
    for tag in R.CASES:
        assert os.path.getsize(os.path.join(R.GOLDEN, "opt_step_%s.npz" % tag)) < 512 * 1024


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "trainer.py:260-275" in src and "UNI_OPT_HAS_GRAD" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s, arity in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, code)
        assert m, "%s is not declared in include/unicorn_hip.h" % s
        args = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == arity, (s, m.group(1))
        assert s in _lib.PROTOS, "%s is not bound in _lib.PROTOS" % s
        assert len(_lib.PROTOS[s][1]) == arity, (s, len(_lib.PROTOS[s][1]))
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert "opt_step" in open(os.path.join(ROOT, "unicorn_amd", "csrc", "build.sh")).read()


def test_table_sizes_and_image_layout():
    from unicorn_amd import _lib, optim
    lib = _lib.lib()
    ch = lib.uni_opt_chunk_elems()
    assert ch > 0 and ch % 4 == 0
    tb = lib.uni_opt_table_bytes
    assert tb(0, 0) == 0 and tb(1, 0) == 256 and tb(4, 0) == 256 and tb(5, 0) == 512 and tb(5, 1) == 768 and tb(5, 33) == 512 + 512
    assert tb(-1, 0) == 0 and tb(1, -1) == 0
    # three tensors: aligned (2 chunks + 3), EMA-only and empty, relatively misaligned (scalar form); the vec chunks come first in the map
    cols = dict(p=[0x1000, 0x9000, 0x20000, 0x30004], g=[0x2000, 0, 0, 0x31000], m=[0x3000, 0, 0, 0x32004], v=[0x4000, 0, 0, 0x33004],
                e=[0x5000, 0xA000, 0x21000, 0x34004], n=[2 * ch + 3, 7, 0, ch + 1], lr_factor=[1.0, 1.0, 1.0, 0.1], wd=[5e-4, 0.0, 0.0, 0.0],
                has_grad=[True, False, False, True])
    img, map_off, N, vec_chunks, total = optim.StepPlan.image(cols, ch, tb)
    assert (N, vec_chunks, total, map_off) == (4, 4, 6, 256) and img.size == tb(4, 6)
    tab = img[:N * 64].view(optim.ENTRY)
    assert tab["p"].tolist() == cols["p"] and tab["e"].tolist() == cols["e"] and tab["n"].tolist() == cols["n"]
    assert tab["flags"].tolist() == [1, 0, 0, 1] and tab["lr_factor"].tolist() == [1.0, 1.0, 1.0, 0.1] and tab["wd"][0] == np.float32(5e-4)
    bm = img[map_off:map_off + total * 8].view(optim.BLOCK)
    assert bm["tensor"].tolist() == [0, 0, 0, 1, 3, 3] and bm["chunk"].tolist() == [0, 1, 2, 0, 0, 1]
    # every element of every tensor is covered exactly once
    for t in range(N):
        got = sorted(int(c) for tt, c in zip(bm["tensor"], bm["chunk"]) if tt == t)
        assert got == list(range(-(-cols["n"][t] // ch)))


def _good(n=5):
    return [torch.zeros(n) for _ in range(5)]


def test_python_surface_refuses_bad_arguments_before_any_library_call(monkeypatch):
    from unicorn_amd import _lib, ops, optim

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    step = torch.zeros(())

    def call(p, g, m, v, e, match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.adamw_ema_step([p], [g], [m], [v], [e], kw.pop("step", step), lr=1e-3, ema_decay=0.99, **kw)
    p, g, m, v, e = _good()
    call(p.double(), g.double(), m.double(), v.double(), e.double(), "only fp32")
    call(p.half(), g.half(), m.half(), v.half(), e.half(), "only fp32")
    call(p, g.bfloat16(), m, v, e, "only fp32")
    call(p, g, m, v, e.to("meta"), "different devices")
    call(p, g, m, v, p, "listed twice")                                              # the EMA copy is the parameter itself
    big = torch.zeros(16)
    call(big[0:5], g, big[3:8], v, e, "listed twice")                                # overlapping views of one storage
    call(torch.zeros(4, 6)[:, :3], torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), "not dense")
    call(torch.zeros(10)[::2], g, m, v, e, "not dense")
    call(torch.zeros(1, 1).expand(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), "not dense")
    cl = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    call(cl, torch.zeros(2, 3, 4, 5), cl.clone(), cl.clone(), cl.clone(), "shape and strides of p")      # a contiguous gradient of a channels_last parameter
    call(p, torch.zeros(6), m, v, e, "shape and strides of p")
    call(p, g, None, v, e, "no moments")
    call(p, g, m, v, e, "one fp32 device word", step=torch.zeros((), dtype=torch.float64))
    call(p, g, m, v, e, "growth_tracker", scaler=(torch.ones(()), torch.zeros(()), torch.zeros(())))      # the tracker is int32
    with pytest.raises(ValueError, match="differ in length"):
        ops.adamw_ema_step([p], [g, g], [m], [v], [e], step, lr=1e-3, ema_decay=0.99)
    # every other check passed: the device check is the last (a channels_last entry with channels_last partners is acceptable)
    call(cl, cl.clone(), cl.clone(), cl.clone(), cl.clone(), "CPU tensor")
    call(p, None, None, None, e, "CPU tensor")
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="CPU tensor"):
        optim.FusedAdamWEMA(lin, torch.nn.Linear(3, 2))
    with pytest.raises(ValueError, match="only fp32"):
        optim.FusedAdamWEMA(torch.nn.Linear(3, 2).double(), torch.nn.Linear(3, 2).double())
    with pytest.raises(ValueError, match="pass model="):
        optim.FusedAdamWEMA(list(torch.nn.BatchNorm1d(3).parameters()), torch.nn.BatchNorm1d(3))
    with pytest.raises(ValueError, match="listed twice"):
        optim.FusedAdamWEMA([{"params": [lin.weight]}, {"params": [lin.weight, lin.bias]}], torch.nn.Linear(3, 2))


def test_state_dict_has_adamws_keys_and_param_groups_follow_the_trainer(monkeypatch):
    from unicorn_amd import optim
    monkeypatch.setattr(optim, "check_entries", lambda *a, **k: torch.device("cpu"))          # a CPU stand-in: no device, no library
    net, ema = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2)), torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    opt = optim.FusedAdamWEMA(net, ema, lr=2e-3, weight_decay=5e-4, scaler=dict(init_scale=128.0, growth_interval=7))
    ref = torch.optim.AdamW([{"params": [p for _, p in net.named_parameters()]}], lr=2e-3, weight_decay=5e-4)
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert set(sd) == set(rsd) == {"state", "param_groups"} and sd["state"] == {}
    assert len(sd["param_groups"]) == 1 and set(sd["param_groups"][0]) == set(rsd["param_groups"][0])
    assert sd["param_groups"][0]["params"] == rsd["param_groups"][0]["params"] == [0, 1, 2, 3]
    assert sd["param_groups"][0]["lr"] == 2e-3 and sd["param_groups"][0]["weight_decay"] == 5e-4
    ref.load_state_dict(sd)                                                                   # AdamW accepts it
    # entries: the four parameters get AdamW, the two float buffers the EMA only, num_batches_tracked (int64) is not listed
    assert len(opt._src) == 6 and [g >= 0 for g in opt._group] == [True, True, True, True, False, False]
    # the trainer's lr lines (trainer.py:277-282) work on param_groups
    for lr in (1e-3, 5e-4):
        for g in opt.param_groups:
            g["lr"] = lr * g["factor"] if "factor" in g else lr
        assert opt._lr_split() == (lr, (1.0,))
    two = optim.FusedAdamWEMA([{"params": [net[0].weight], "factor": 0.1}, {"params": [net[0].bias] + list(net[1].parameters())}], ema, lr=1e-3, model=net)
    for lr in (1e-3, 7e-4, 3e-5):
        for g in two.param_groups:
            g["lr"] = lr * g["factor"] if "factor" in g else lr
        base, f = two._lr_split()
        assert f == (0.1, 1.0) and abs(base - lr) <= 1e-15
    # a loaded AdamW state arrives in the moments and the step word
    ref.param_groups[0]["lr"] = 3e-3
    for p in ref.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    ref.step()
    ref.step()
    opt.load_state_dict(ref.state_dict())
    assert float(opt._step) == 2.0 and opt.param_groups[0]["lr"] == 3e-3
    assert torch.equal(opt._m[0], ref.state[net[0].weight]["exp_avg"]) and torch.equal(opt._v[1], ref.state[net[0].bias]["exp_avg_sq"])
    back = opt.state_dict()
    assert set(back["state"]) == {0, 1, 2, 3} and set(back["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(back["state"][0]["step"]) == 2.0
    torch.optim.AdamW([{"params": [p for _, p in net.named_parameters()]}]).load_state_dict(back)
    # ModelEMA-shaped object: .ema / .updates
    class E:
        pass
    obj = E()
    obj.ema, obj.updates = ema, 41
    assert optim.FusedAdamWEMA(net, obj).ema_updates == 41
    assert abs(optim.ema_decay_at(0.9998, 2000) - 0.9998 * (1 - np.exp(-1.0))) < 1e-15
