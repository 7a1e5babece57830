"""tests/train_scale.py without a GPU: every shape of tests/test_train_scale_gpu.py satisfies the rule it was chosen by (it passes its boundary
by at least 2^24 elements, is ragged in the tiled axes, has the plan class and the idle slots claimed -- answered by `train_plan_check --list`
through tests/train_plans.py --, gives a lane the claimed number of terms, is admitted by train_shape_ok / pw_shape_ok); the memory each case
states follows from its shape and stays under the cap; and the checking functions are sensitive: on maps of a few thousand rows with the
boundary moved down to 2^12 elements they pass the correct result, with a positive yardstick, and report a map whose rows behind the boundary
are rotated by one, a row left at NaN and a column sum that lacks one row."""
import pytest
import torch

import train_plans as P
import train_scale as S


def _lib():
    from unicorn_amd import _lib
    return _lib.lib()


def _ceil(a, b):
    return -(-a // b)


# ================================================================================================================ the shapes
@pytest.mark.parametrize("tag", sorted(S.PW_A))
def test_pw_mlp_scale_shapes(tag):
    dt, M, Hd, Co, boundary, forms = S.PW_A[tag]
    assert M * Hd >= boundary + S.BEHIND > (M - 1) * Hd and M < 2 ** 31                  # the smallest such M
    assert _lib().uni_pw_mlp_workspace_bytes(M, Hd, Co) == 4 * 256 * (Hd + Co)          # pw_shape_ok admits it
    for N, V in ((Hd, 8 if dt != "f32" else 4), (Co, 4)):
        cls, e = P.predicted("pw_mlp", "", dt, N), P.plan_extra("pw_mlp", "", dt, N)
        assert cls == "<%s,V=%d> L=8" % (dt, V) and e["gx"] > 1 and e["idle"] == {(520, 8): 7, (520, 4): 6, (68, 4): 7}[(N, V)], (N, cls, e)
        assert M % (256 // e["L"]), "M is a multiple of the rows of a block"
        assert _ceil(M, 256 // e["L"]) > 256                                             # more groups than rows of partials: the blocks loop
    assert (boundary == S.B32) == (forms == ("in",)) and set(forms) <= {"out", "in"}
    # the integer run stays exact: base 1 below 2^24 / 3 rows, base 0 (values 0, 1, 2) above
    assert (3 if 3 * M < 2 ** 24 else 2) * M < 2 ** 24
    assert S.TEMPS < S.pw_need(tag) <= S.CAP and S.pw_need(tag) >= 4 * M * Hd * S.ESIZE[dt] + M * Co * S.ESIZE[dt]


def test_pw_mlp_scale_shape_spot_values():
    assert S.PW_A["f16"][1] == S.PW_A["f32"][1] == 4162041 and S.PW_A["f16_2p32"][1] == 8291817
    assert [round(S.pw_need(t) / 2 ** 30, 1) for t in ("f16", "f32", "f16_2p32")] == [21.7, 37.3, 39.3]


@pytest.mark.parametrize("tag", sorted(S.PW_B))
def test_pw_mlp_long_sum_shapes(tag):
    dt, M, N, lanes, terms = S.PW_B[tag]
    e = P.plan_extra("pw_mlp", "", dt, N)
    rows = P.plan_list()[1]["PW_ROWS"]
    assert e["L"] == lanes and e["idle"] == 0
    groups = _ceil(M, 256 // lanes)
    assert _ceil(groups, rows) == terms == 1025 and groups // rows == 1024             # every lane adds 1024 or 1025 rows
    assert M * N in (2 ** 28 + 3 * 1024, 2 ** 28 + 9 * 32, 2 ** 29 + 3 * 2048, 2 ** 29 + 9 * 64)
    assert _lib().uni_pw_mlp_workspace_bytes(M, N, N) == 4 * 256 * 2 * N
    assert S.pw_b_need(tag) <= S.CAP


@pytest.mark.parametrize("tag", sorted(S.BT_A))
def test_block_tail_scale_shapes(tag):
    dt, nchw, shape = S.BT_A[tag]
    B, C, H, W = shape
    assert S.elements(shape) >= S.B31 + S.BEHIND and B == 3 and (H * W) % 64 and B * H * W < 2 ** 31
    assert S.BT_SCALE[1] == 0.0 == S.BT_SCALE_EXACT[1] and S.BT_SCALE[0] == S.BT_SCALE[2] != 0 and len(S.BT_SCALE) == B
    assert _lib().uni_block_tail_workspace_bytes(B, H, W, C) == 4 * 1024 * C           # train_shape_ok admits it
    layout = "nchw" if nchw else "cl"
    cls, e = P.bt_class(layout, dt, C), P.plan_extra("block_tail", layout, dt, C)
    if nchw:
        assert cls == "nchw<f16>" and C == 136 and _ceil(C, 64) == 3 and C % 64 == 8
    else:
        assert cls == "cl<f16,V=8>" and C == 200 and (e["PP"], e["block"]) == (20, 512) and e["block"] - e["PP"] * (C // 8) == 12
        assert (H * W) % (2 * e["PP"])                                                   # a chunk is two steps of PP pixels at V = 8
    assert _ceil(H * W, 64) * B > 1024                                                   # more units than blocks: the blocks loop
    assert S.bt_need(tag) <= S.CAP


@pytest.mark.parametrize("tag", sorted(S.LN_A))
def test_lncf_scale_shapes(tag):
    dt, nchw, shape, cls = S.LN_A[tag]
    B, C, H, W = shape
    assert S.elements(shape) >= S.B31 + S.BEHIND and B * H * W < 2 ** 31
    assert _lib().uni_lncf_train_workspace_bytes(B, H, W, C) == 4 * 1024 * 2 * C
    assert P.predicted("lncf", "nchw" if nchw else "cl", dt, C) == cls and cls in P.EXPECTED["lncf"]
    if nchw:
        assert (H * W) % 64 and C % 8 == 4
        assert {"regs16": C <= 128, "regs32": 128 < C <= 256, "stream8": C > 256 and _ceil(C, 8) % 8}[tag]
    else:
        nv, g = 3, 8
        assert cls == "cl<f16,V=8,NV=%d> G=%d" % (nv, g) and nv * g - C // 8 == 7 and (B * H * W) % (256 // g) == 6
    assert S.ln_need(tag) <= S.CAP


def test_dwln_scale_shape():
    B, C, H, W = S.DW_A
    assert S.elements(S.DW_A) >= S.B31 + S.BEHIND and B * H * W < 2 ** 31 and B == 2 and C == 68 and H % 2 and W % 2 and W > 128
    assert P.predicted("dwln", "", "f32", C) == S.DW_CLASS
    segs = _ceil(W, 8)
    assert W % 8 == 5 and segs == 687 and (B * H * segs) % 8                            # strips of 8 pixels, 8 strips per block
    segs_w = _ceil(W, 128)
    slen = _ceil(W, segs_w)
    assert (segs_w, slen, W - (segs_w - 1) * slen) == (43, 128, 117) and (B * H * segs_w) % 4
    assert _lib().uni_dwln_train_workspace_bytes(B, H, W, C) == S.dw_workspace(S.DW_A)
    assert S.dw_need() <= S.CAP
    bands = S.DwCase(S.DW_A).value_bands()
    assert [b[0] for b in bands] == ["first", "boundary", "last"] and bands[0][1:] == (0, 0, 8) and bands[2][1:] == (1, H - 8, H)
    _, n, r0, r1 = bands[1]
    assert (n * H + r0) * W * C < S.B31 < (n * H + r1) * W * C and r1 - r0 == 8           # the offset passes 2^31 inside the band


def test_the_memory_arithmetic():
    """each need is the sum of the buffers its docstring names plus the chunk temporaries, and the largest is below the cap"""
    E = S.elements(S.BT_A["cl"][2])
    assert S.bt_need("cl") == 2 * E + 3 * 4 * E + S.TEMPS
    E = S.elements(S.LN_A["cl"][2])
    assert S.ln_need("cl") == 3 * 2 * E + 2 * 4 * E + 8 * (E // 136) + S.TEMPS
    E = S.elements(S.DW_A)
    assert S.dw_need() == 12 * E + S.dw_workspace(S.DW_A) + 8 * (E // 68) + S.TEMPS and S.dw_workspace(S.DW_A) > 4 * E
    assert S.TEMPS == 4 * 2 ** 30 and S.CHUNK <= 1 << 26
    needs = [S.pw_need(t) for t in S.PW_A] + [S.pw_b_need(t) for t in S.PW_B] + [S.bt_need(t) for t in S.BT_A] + [S.ln_need(t) for t in S.LN_A] + [S.dw_need()]
    assert 30 * 2 ** 30 < max(needs) <= S.CAP == 40 * 2 ** 30


# ================================================================================================================ the checkers are sensitive
BOUNDARY = 2 ** 12
SMALL = 1 << 14                                  # elements of a chunk: several chunks per map


def _failures(rep):
    assert all(0 < y < 1e-5 for ys in rep.yard.values() for y in ys), rep.yard      # an fp32 deviation: neither zero nor a wrong reference
    return rep.failures()


def test_pw_mlp_checker_is_sensitive():
    case = S.PwCase("f32", 3001, 24, 12, chunk=SMALL)
    h, ga, gy = (case.fill(n, torch.empty(3001, N)) for n, N in (("h", 24), ("ga", 24), ("gy", 12)))
    ref = S.RP.act_maps(h.double(), ga.double())
    good = {"a_fwd": ref["a"].float(), "a": ref["a"].float(), "grad_h": ref["grad_h"].float(), "g_b1": ref["g_b1"].float(), "g_b2": gy.double().sum(0).float()}
    assert _failures(S.pw_check(case, good, BOUNDARY)) == []
    split = BOUNDARY // 24
    rot = dict(good, grad_h=torch.cat([good["grad_h"][:split], good["grad_h"][split:].roll(1, 0)]))
    bad = _failures(S.pw_check(case, rot, BOUNDARY))
    assert len(bad) == 1 and bad[0].startswith("grad_h: err") and S.pw_check(case, rot, BOUNDARY)["grad_h"][0] <= S.pw_check(case, rot, BOUNDARY)["grad_h"][2]
    hole = dict(good, a=good["a"].clone())
    hole["a"][2999] = float("nan")
    assert any(f == "a: 24 NaN left" for f in _failures(S.pw_check(case, hole, BOUNDARY)))
    short = dict(good, g_b1=(ref["g_b1"] - ref["grad_h"][1234]).float(), g_b2=(gy.double().sum(0) - gy[17].double()).float())
    assert [f.split(":")[0] for f in _failures(S.pw_check(case, short, BOUNDARY))] == ["g_b1", "g_b2"]
    # half maps: the rounded result passes with the half ulp it is given
    c16 = S.PwCase("f16", 1001, 24, 12, chunk=SMALL)
    h, ga = (c16.fill(n, torch.empty(1001, 24, dtype=torch.float16)) for n in ("h", "ga"))
    r16 = S.RP.act_maps(h.double(), ga.double())
    assert _failures(S.pw_check(c16, {"a": r16["a"].half(), "grad_h": r16["grad_h"].half(), "g_b1": r16["g_b1"].float()}, BOUNDARY)) == []


def test_pw_mlp_integer_checker_is_sensitive():
    for base in (1, 0):
        case = S.PwCase("f16", 1003, 24, 12, exact=base, chunk=SMALL)
        h, ga, gy = (case.fill(n, torch.empty(1003, N, dtype=torch.float16)) for n, N in (("h", 24), ("ga", 24), ("gy", 12)))
        if base == 1:
            ref = S.RP.exact_maps(1003, 24, 12, torch.float16)
            assert all(torch.equal(a, b) for a, b in zip((h, ga, gy), ref[:3]))           # the pattern of pw_mlp_ref.exact_maps, drawn per chunk
        good = {"a": h, "grad_h": ga, "g_b1": ga.double().sum(0).float(), "g_b2": gy.double().sum(0).float()}
        assert S.pw_check_exact(case, good).failures() == []
        assert S.pw_check_exact(case, dict(good, grad_h=ga.roll(1, 0))).failures() == ["grad_h: %d elements differ" % (1002 * 24)]      # 1002 = 0 (mod 3)
        assert S.pw_check_exact(case, dict(good, g_b1=good["g_b1"] - ga[5].float())).failures()[0].startswith("g_b1: ")


def _bt_good(case):
    M, C = case.M, case.C
    y = case.fill(case.y, torch.empty(M, C, dtype=case.dtype), 0)
    x = case.fill(case.x, torch.empty(M * C), 0)
    ins = (y.float().view(case.B, case.H, case.W, C), x.view(case.B, case.H, case.W, C).permute(0, 3, 1, 2), case.gamma, case.scale)
    r = S.RB.value_and_grads(*ins, ins[1], dtype=torch.float64)
    return {"out": r["out"].permute(0, 2, 3, 1).reshape(M, C).float(), "g_y": r["g_y"].reshape(M, C).to(case.dtype), "g_gamma": r["g_gamma"].float()}


@pytest.mark.parametrize("nchw", [0, 1])
def test_block_tail_checker_is_sensitive(nchw):
    """the chunked reference of a three-image map (chunks end inside an image) is the restatement on the whole map; the layout of x only
    matters to store / load"""
    case = S.BtCase("f16", nchw, (3, 8, 21, 23), chunk=1 << 10)
    good = _bt_good(case)
    assert _failures(S.bt_check(case, good, BOUNDARY)) == []
    assert float(good["g_y"][case.HW:2 * case.HW].abs().max()) == 0.0                    # the dropped sample
    split = BOUNDARY // 8
    rot = dict(good, out=torch.cat([good["out"][:split], good["out"][split:].roll(1, 0)]))
    assert [f.split(":")[0] for f in _failures(S.bt_check(case, rot, BOUNDARY))] == ["out"]
    hole = dict(good, g_y=good["g_y"].clone())
    hole["g_y"][1200] = float("nan")
    assert "g_y: 8 NaN left" in _failures(S.bt_check(case, hole, BOUNDARY))
    y = case.fill(case.y, torch.empty(case.M, 8, dtype=case.dtype), 0).double()
    x = case.fill(case.x, torch.empty(case.M * 8), 0).view(case.M, 8).double()
    short = dict(good, g_gamma=(good["g_gamma"].double() - x[5] * case.scale[0].double() * y[5]).float())
    assert [f.split(":")[0] for f in _failures(S.bt_check(case, short, BOUNDARY))] == ["g_gamma"]
    # the layouts: a chunk stored in NCHW memory and loaded again is the chunk
    buf = torch.zeros(case.M * 8)
    chunk = torch.randn(40, 8)
    case.store(buf, 1, 2, 100, 140, chunk)
    assert torch.equal(case.load(buf, 1, 2, 100, 140), chunk) and torch.equal(buf.view(3, 8, case.HW)[2, :, 100:140], chunk.t())
    # integers: to the last bit
    exact = S.BtCase("f16", nchw, (3, 8, 21, 23), exact=True, chunk=1 << 10)
    ge = _bt_good(exact)
    assert S.bt_check(exact, ge).failures() == []
    assert [f.split(":")[0] for f in S.bt_check(exact, dict(ge, out=ge["out"].roll(1, 0))).failures()] == ["out"]
    assert [f.split(":")[0] for f in S.bt_check(exact, dict(ge, g_gamma=ge["g_gamma"] - 2)).failures()] == ["g_gamma"]


@pytest.mark.parametrize("nchw", [0, 1])
def test_lncf_checker_is_sensitive(nchw):
    case = S.LnCase("f16", nchw, (2, 12, 19, 21), chunk=1 << 10)
    M, C, E = case.M, 12, case.M * 12
    x = case.fill(case.x, torch.empty(E, dtype=torch.float16), nchw)
    g = case.fill(case.gy, torch.empty(E), nchw)
    to4 = (lambda t: t.view(2, C, 19, 21)) if nchw else (lambda t: t.view(2, 19, 21, C).permute(0, 3, 1, 2))
    back = (lambda t: t.reshape(E)) if nchw else (lambda t: t.permute(0, 2, 3, 1).reshape(E))
    r = S.RL.value_and_grads(to4(x).float(), case.weight, case.bias, to4(g), dtype=torch.float64)
    xd = to4(x).double()
    u = xd.mean(1)
    rstd = 1 / torch.sqrt((xd - u[:, None]).pow(2).mean(1) + S.RL.EPS)
    good = {"y": back(r["y"]).float(), "g_x": back(r["g_x"]).half(), "stats": torch.stack([u.reshape(M), rstd.reshape(M)], 1).float(),
            "g_weight": r["g_weight"].float(), "g_bias": r["g_bias"].float()}
    assert _failures(S.ln_check(case, good, BOUNDARY, gy=g)) == []
    cl = (lambda t: t.view(2, C, 19 * 21).permute(0, 2, 1).reshape(M, C)) if nchw else (lambda t: t.view(M, C))
    uncl = (lambda t: t.view(2, 19 * 21, C).permute(0, 2, 1).reshape(E)) if nchw else (lambda t: t.reshape(E))
    split = BOUNDARY // C
    rows = cl(good["y"])
    rot = dict(good, y=uncl(torch.cat([rows[:split], rows[split:].roll(1, 0)])).contiguous())
    assert [f.split(":")[0] for f in _failures(S.ln_check(case, rot, BOUNDARY, gy=g))] == ["y"]
    hole = dict(good, stats=good["stats"].clone())
    hole["stats"][700] = float("nan")
    assert "stats: 2 NaN left" in _failures(S.ln_check(case, hole, BOUNDARY, gy=g))
    short = dict(good, g_bias=(r["g_bias"] - cl(g)[33].double()).float())
    assert [f.split(":")[0] for f in _failures(S.ln_check(case, short, BOUNDARY, gy=g))] == ["g_bias"]


def test_dwln_checkers_are_sensitive():
    """on a map of 2 x 8 x 37 x 21: the bands (with their halo of 6 rows) and the shifted multiply-adds give what dwln_train_ref gives on the
    whole map"""
    shape = (2, 8, 37, 21)
    B, C, H, W = shape
    case = S.DwCase(shape, band=5)
    x, g = case.fill(case.x, torch.empty(S.elements(shape))), case.fill(case.gy, torch.empty(S.elements(shape)))
    x4 = x.view(B, H, W, C).permute(0, 3, 1, 2)
    r = S.RD.value_and_grads(x4.double(), case.weight.double(), case.bias.double(), case.ln_weight.double(), case.ln_bias.double(), g.view(B, H, W, C).double())
    boundary = (H + 17) * W * C + 5                                                      # in row 17 of the second image
    assert [b[1:] for b in case.value_bands(boundary)] == [(0, 0, 8), (1, 13, 21), (1, 29, 37)]
    u = S.F.conv2d(x4.double(), case.weight.double(), case.bias.double(), padding=3, groups=C).permute(0, 2, 3, 1)
    m = u.mean(-1, keepdim=True)
    stats = torch.cat([m, 1 / torch.sqrt((u - m).pow(2).mean(-1, keepdim=True) + S.RD.EPS)], -1).reshape(-1, 2).float()
    good = {"y": r["y"].reshape(-1).float(), "stats": stats, "grad_x": r["gx"].permute(0, 2, 3, 1).reshape(-1).float()}
    rep = S.dw_band_check(case, x, g, good, boundary)
    assert _failures(rep) == [] and len(rep) == 9
    rot = dict(good, grad_x=good["grad_x"].view(B * H, W * C).roll(1, 0).reshape(-1))
    assert {f.split(":")[0] for f in _failures(S.dw_band_check(case, x, g, rot, boundary))} == {"grad_x first", "grad_x boundary", "grad_x last"}
    hole = dict(good, y=good["y"].clone())
    hole["y"][-3] = float("nan")
    assert "y: 1 NaN left" in _failures(S.dw_band_check(case, x, g, hole, boundary))
    params = {"grad_weight": r["gw"].reshape(C, 49).t().float(), "grad_bias": r["gb"].float(), "grad_ln_weight": r["ggamma"].float(),
              "grad_ln_bias": r["gbeta"].float()}
    rep = S.dw_param_check(case, x, g, params)
    assert _failures(rep) == [] and len(rep.notes) == 4 and set(rep) == set(params)
    ref = S.dw_param_reference(case, x, g)
    for k in params:
        assert S.sum_err(params[k].double(), ref[k]) < 1e-6, k
    short = dict(params, grad_ln_bias=(r["gbeta"] - g.view(-1, C)[100].double()).float())
    assert [f.split(":")[0] for f in _failures(S.dw_param_check(case, x, g, short))] == ["grad_ln_bias"]


def test_bit_comparisons_and_the_digest():
    a = torch.randn(1000)
    assert S.same_bits(a, a.clone(), chunk=64) and not S.same_bits(a, a.roll(1), chunk=64) and S.digest(a, chunk=64) == S.digest(a.clone(), chunk=64)
    b = a.clone()
    b[[3, 4]] = b[[4, 3]]                                                                # a swap keeps a plain sum, not the weighted one
    assert S.digest(b, chunk=64) != S.digest(a, chunk=64)
    n = torch.full((10,), float("nan"))
    assert not S.same_bits(n, n.clone()) and S.count_nan(torch.cat([a, n]), chunk=64) == 10
