"""Thin tensor-level wrappers over the C-ABI operators (torch only allocates and hands over pointers)."""
import ctypes as C

import torch

from . import _lib as L


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.UnicornHipError("unicorn_amd ops need HIP device tensors (got a CPU tensor); there is no CPU fallback")


def nhwc(t):
    """(1,C,H,W) tensor -> fp32 tensor whose memory is [H][W][C] (channels_last), no copy when already so."""
    t = t.float() if t.dtype != torch.float32 else t
    return t.contiguous(memory_format=torch.channels_last)


def empty_nhwc(c, h, w, device, b=1):
    return torch.empty((b, c, h, w), device=device, dtype=torch.float32, memory_format=torch.channels_last)


_F64_SFX = {torch.float32: "", torch.float64: "_f64"}      # the dtypes of the fp32 / fp64 operator pairs -> suffix of the exported name


def _entry(base, dtype, err=None):
    """(bound library function, exported name) of the fp32 / fp64 operator pair `base` for `dtype`; the name is what L.check reports.
    Any other dtype raises `err`, the caller's own message."""
    if dtype not in _F64_SFX:
        raise L.UnicornHipError(err or "%s: dtype %s unsupported (fp32 / fp64)" % (base, dtype))
    name = base + _F64_SFX[dtype]
    return getattr(L.lib(), name), name


def _ws_factor(dtype):
    """the workspace size functions count fp32 elements: the fp64 forms need twice that"""
    return torch.finfo(dtype).bits // 32


def _stream_scratch(cache, dev, need):
    """grow-only byte scratch of at least `need` bytes, one per (device, current stream), kept in the dict `cache`"""
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        ws = cache[key] = torch.empty(max(need, 1), device=dev, dtype=torch.uint8)
    return ws


def _msda_args(what, value, spatial_shapes, level_start_index, loc, attn, *more):
    """Common argument handling of the two MultiScaleDeformableAttention functions: device + dtype checks (fp32 / fp64, no mixing, as
    AT_DISPATCH_FLOATING_TYPES on value.type()), contiguous copies, the host int64 shape arrays and the sizes."""
    ts = (value, loc, attn) + more
    _need_cuda(*ts)
    _entry("uni_msda_fwd", value.dtype, "%s: dtype %s unsupported (fp32 / fp64, like the reference's dispatch)" % (what, value.dtype))
    if any(t.dtype != value.dtype for t in ts):
        raise L.UnicornHipError("%s: mixed dtypes %s (every floating tensor must have value's dtype)" % (what, [str(t.dtype) for t in ts]))
    if value.dim() != 4 or loc.dim() != 6 or attn.dim() != 5 or loc.shape[-1] != 2 or tuple(loc.shape[:5]) != tuple(attn.shape) \
            or loc.shape[0] != value.shape[0] or loc.shape[2] != value.shape[2]:
        raise L.UnicornHipError("%s: shapes value %s, sampling_locations %s, attention_weights %s do not fit (N,S,M,D), (N,Lq,M,L,P,2), "
                                "(N,Lq,M,L,P)" % (what, tuple(value.shape), tuple(loc.shape), tuple(attn.shape)))
    Ln = loc.shape[3]
    if spatial_shapes.numel() != 2 * Ln or level_start_index.numel() != Ln:
        raise L.UnicornHipError("%s: spatial_shapes / level_start_index do not describe %d levels" % (what, Ln))
    shp = (C.c_int64 * (2 * Ln))(*[int(v) for v in spatial_shapes.reshape(-1).tolist()])
    lsi = (C.c_int64 * Ln)(*[int(v) for v in level_start_index.reshape(-1).tolist()])
    return tuple(t.contiguous() for t in ts), shp, lsi


def msda_forward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=64):
    """Same signature as MultiScaleDeformableAttention.ms_deform_attn_forward (ops/src/vision.cpp:13-16); fp32 or fp64."""
    (value, loc, attn), shp, lsi = _msda_args("msda_forward", value, spatial_shapes, level_start_index, sampling_locations,
                                              attention_weights)
    N, S, M, D = value.shape
    _, Lq, _, Ln, P, _ = loc.shape
    out = torch.empty((N, Lq, M * D), device=value.device, dtype=value.dtype)
    if out.numel() == 0:
        return out
    fn, name = _entry("uni_msda_fwd", value.dtype)
    L.check(fn(L.ptr(value), shp, lsi, L.ptr(loc), L.ptr(attn), L.ptr(out), N, S, M, D, Lq, Ln, P, L.stream_ptr()), name)
    return out


def msda_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, grad_output, im2col_step=64):
    """Same signature as MultiScaleDeformableAttention.ms_deform_attn_backward (ops/src/vision.cpp:13-16); fp32 or fp64.
    Returns (grad_value, grad_sampling_loc, grad_attn_weight).  grad_value is summed with float atomics: its last bits depend on the
    arrival order, like the reference's; the other two are bitwise reproducible."""
    (value, loc, attn, gout), shp, lsi = _msda_args("msda_backward", value, spatial_shapes, level_start_index, sampling_locations,
                                                    attention_weights, grad_output)
    N, S, M, D = value.shape
    _, Lq, _, Ln, P, _ = loc.shape
    if gout.numel() != N * Lq * M * D:
        raise L.UnicornHipError("msda_backward: grad_output %s is not (N, Lq, M*D) = (%d, %d, %d)" % (tuple(gout.shape), N, Lq, M * D))
    gvalue, gloc, gattn = torch.empty_like(value), torch.empty_like(loc), torch.empty_like(attn)
    if value.numel() == 0 or attn.numel() == 0:       # no query / empty batch: nothing to scatter (empty tensors have no device pointer)
        return gvalue.zero_(), gloc, gattn
    fn, name = _entry("uni_msda_bwd", value.dtype)
    L.check(fn(L.ptr(value), shp, lsi, L.ptr(loc), L.ptr(attn), L.ptr(gout), L.ptr(gvalue), L.ptr(gloc), L.ptr(gattn), N, S, M, D, Lq, Ln, P,
               L.stream_ptr()), name)
    return gvalue, gloc, gattn


class MSDeformAttnFunction(torch.autograd.Function):
    """The reference's autograd function (ops/functions/ms_deform_attn_func.py:21-38) on the two HIP operators:
    apply(value, shapes, level_start_index, sampling_locations, attention_weights, im2col_step)."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step):
        ctx.im2col_step = im2col_step
        output = msda_forward(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights)
        return output

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        value, shapes, lsi, loc, attn = ctx.saved_tensors
        gv, gl, ga = msda_backward(value, shapes, lsi, loc, attn, grad_output.contiguous(), ctx.im2col_step)
        need = ctx.needs_input_grad
        return gv if need[0] else None, None, None, gl if need[3] else None, ga if need[4] else None, None


_corr_ws = {}


def corr_softmax_pv(embed_ref, embed_cur, values, precision=0):
    """embed_* : (C, HW) (any strides; an NHWC map viewed as (C,HW) needs no copy) ; values (K, HW_ref) -> (K, HW_cur).
    == values @ softmax(embed_ref^T @ embed_cur, dim=0)   (unicorn_sot.py:95-100)
    precision 0: exact fp32 MFMA; 1: fp32-equivalent "bf16x3" (operands split exactly into three bf16 pieces, six fp32-exact
    partial products accumulated in fp32; error at the fp32 rounding level, 2.7x less MFMA time); 2: fp32-equivalent "f16x2"
    (hi + lo f16 halves, three products: half the MFMA time of bf16x3, same error class for embeddings inside the f16 range);
    3: the arithmetic class of the reference driver itself, which casts keys / queries / values to fp16 (:95-97): f16-rounded
    operands, one product, f16-rounded scores (the `.half()` of the normalised softmax is not reproduced).  The trackers keep 2."""
    _need_cuda(embed_ref, embed_cur, values)
    er = embed_ref.float().t().contiguous()     # (HW, C) row-major
    ec = embed_cur.float().t().contiguous()
    v = values.float().contiguous()
    R, D = er.shape
    Q = ec.shape[0]
    K = v.shape[0]
    out = torch.empty((K, Q), device=er.device, dtype=torch.float32)
    ws = _stream_scratch(_corr_ws, er.device, L.lib().uni_corr_workspace_bytes(R, Q, K))
    L.check(L.lib().uni_corr_softmax_pv(L.ptr(er), L.ptr(ec), L.ptr(v), L.ptr(out), R, Q, D, K, precision, L.ptr(ws),
                                        ws.numel(), L.stream_ptr()), "uni_corr_softmax_pv")
    return out


def corr_softmax_pv_batched(embed_ref, embed_cur, values, precision=2, values_per_frame=False):
    """B frames in ONE launch (`uni_corr_softmax_pv_batched`): embed_* (B, C, HW) or (B, C, H, W) (channels_last maps need no copy),
    values (K, HW_ref) shared by the frames -- the SOT label map of the cached first frame -- or (B, K, HW_ref) with values_per_frame
    -> (B, K, HW_cur).  == torch.stack([corr_softmax_pv(embed_ref[b], embed_cur[b], values) for b in range(B)])."""
    _need_cuda(embed_ref, embed_cur, values)
    er = embed_ref.float().flatten(2).transpose(1, 2).contiguous()     # (B, HW, C)
    ec = embed_cur.float().flatten(2).transpose(1, 2).contiguous()
    v = values.float().contiguous()
    B, R, D = er.shape
    Q = ec.shape[1]
    K = v.shape[-2]
    if values_per_frame and (v.dim() != 3 or v.shape[0] != B):
        raise ValueError("values_per_frame needs values of shape (B, K, HW_ref)")
    if not values_per_frame and v.dim() != 2:
        raise ValueError("shared values must have shape (K, HW_ref)")
    if ec.shape[0] != B or v.shape[-1] != R:
        raise ValueError("corr_softmax_pv_batched: shape mismatch")
    out = torch.empty((B, K, Q), device=er.device, dtype=torch.float32)
    ws = _stream_scratch(_corr_ws, er.device, L.lib().uni_corr_workspace_bytes_batched(B, R, Q, K))
    L.check(L.lib().uni_corr_softmax_pv_batched(L.ptr(er), L.ptr(ec), L.ptr(v), L.ptr(out), B, R, Q, D, K, 1 if values_per_frame else 0,
                                                precision, L.ptr(ws), ws.numel(), L.stream_ptr()), "uni_corr_softmax_pv_batched")
    return out


def _corr_train_args(what, embed_ref, embed_cur, values, *more):
    """Argument handling of the differentiable correlation: shapes (B,R,D), (B,Q,D), (B,K,R) [+ (B,K,Q) tensors], one dtype (fp32 / fp64),
    device tensors; returns contiguous tensors."""
    ts = (embed_ref, embed_cur, values) + more
    if embed_ref.dim() != 3 or embed_cur.dim() != 3 or values.dim() != 3 or embed_ref.shape[0] != embed_cur.shape[0] \
            or values.shape[0] != embed_ref.shape[0] or embed_ref.shape[2] != embed_cur.shape[2] or values.shape[2] != embed_ref.shape[1] \
            or any(t.shape != (values.shape[0], values.shape[1], embed_cur.shape[1]) for t in more):
        raise L.UnicornHipError("%s: shapes %s do not fit embed_ref (B,R,D), embed_cur (B,Q,D), values (B,K,R)%s"
                                % (what, [tuple(t.shape) for t in ts], ", out / grad_out (B,K,Q)" if more else ""))
    if embed_ref.dtype not in (torch.float32, torch.float64) or any(t.dtype != embed_ref.dtype for t in ts):
        raise L.UnicornHipError("%s: dtypes %s unsupported (all fp32 or all fp64)" % (what, [str(t.dtype) for t in ts]))
    if min(embed_ref.shape + embed_cur.shape + values.shape) == 0:
        raise L.UnicornHipError("%s: empty problem %s" % (what, [tuple(t.shape) for t in ts]))
    _need_cuda(*ts)
    return tuple(t.contiguous() for t in ts)


def corr_softmax_pv_lse(embed_ref, embed_cur, values, precision=0):
    """The forward of the differentiable operator (`uni_corr_softmax_pv_lse`): embed_ref (B,R,128), embed_cur (B,Q,128) row-major, values (B,K,R)
    (or (K,R): rows shared by the frames) -> (out (B,K,Q), lse (B,Q)) with lse[b,q] = logsumexp_r <embed_ref[b,r], embed_cur[b,q]>.
    `out` is bitwise what corr_softmax_pv_batched returns for the same inputs and precision (the same kernels, one more store).
    fp64 tensors take the plain double-precision path (precision is ignored there)."""
    shared = values.dim() == 2
    er, ec, v = _corr_train_args("corr_softmax_pv_lse", embed_ref, embed_cur,
                                 values.unsqueeze(0).expand(embed_ref.shape[0], -1, -1) if shared and embed_ref.dim() == 3 else values)
    if shared:
        v = values.contiguous()
    B, R, D = er.shape
    Q, K = ec.shape[1], v.shape[-2]
    out = torch.empty((B, K, Q), device=er.device, dtype=er.dtype)
    lse = torch.empty((B, Q), device=er.device, dtype=er.dtype)
    with torch.cuda.device(er.device):
        if er.dtype == torch.float64:
            L.check(L.lib().uni_corr_softmax_pv_lse_f64(L.ptr(er), L.ptr(ec), L.ptr(v), L.ptr(out), L.ptr(lse), B, R, Q, D, K, 0 if shared else 1,
                                                        L.stream_ptr()), "uni_corr_softmax_pv_lse_f64")
        else:
            ws = _stream_scratch(_corr_ws, er.device, L.lib().uni_corr_bwd_workspace_bytes(B, R, Q, K))
            L.check(L.lib().uni_corr_softmax_pv_lse(L.ptr(er), L.ptr(ec), L.ptr(v), L.ptr(out), L.ptr(lse), B, R, Q, D, K, 0 if shared else 1,
                                                    int(precision), L.ptr(ws), ws.numel(), L.stream_ptr()), "uni_corr_softmax_pv_lse")
    return out, lse


def corr_softmax_pv_backward(embed_ref, embed_cur, values, out, lse, grad_out, need=(True, True, True), precision=0):
    """`uni_corr_softmax_pv_bwd`: (grad_embed_ref, grad_embed_cur, grad_values) for the tensors of corr_softmax_pv_lse; with shared (K,R)
    values grad_values is (K,R), summed over the frames.  An entry of `need` that is False is not computed (None).  One writer per output
    element: bitwise reproducible."""
    shared = values.dim() == 2
    er, ec, v, o, g = _corr_train_args("corr_softmax_pv_backward", embed_ref, embed_cur,
                                       values.unsqueeze(0).expand(embed_ref.shape[0], -1, -1) if shared and embed_ref.dim() == 3 else values,
                                       out, grad_out)
    if shared:
        v = values.contiguous()
    B, R, D = er.shape
    Q, K = ec.shape[1], v.shape[-2]
    if lse.shape != (B, Q) or lse.dtype != er.dtype:
        raise L.UnicornHipError("corr_softmax_pv_backward: lse %s %s is not (B,Q) = (%d, %d) %s" % (tuple(lse.shape), lse.dtype, B, Q, er.dtype))
    _need_cuda(lse)
    lse = lse.contiguous()
    ger = torch.empty_like(er) if need[0] else None
    gec = torch.empty_like(ec) if need[1] else None
    gv = torch.empty_like(v) if need[2] else None
    with torch.cuda.device(er.device):
        if er.dtype == torch.float64:
            L.check(L.lib().uni_corr_softmax_pv_bwd_f64(L.ptr(er), L.ptr(ec), L.ptr(v), L.ptr(o), L.ptr(lse), L.ptr(g), L.ptr(ger), L.ptr(gec),
                                                        L.ptr(gv), B, R, Q, D, K, 0 if shared else 1, L.stream_ptr()), "uni_corr_softmax_pv_bwd_f64")
        else:
            ws = _stream_scratch(_corr_ws, er.device, L.lib().uni_corr_bwd_workspace_bytes(B, R, Q, K))
            L.check(L.lib().uni_corr_softmax_pv_bwd(L.ptr(er), L.ptr(ec), L.ptr(v), L.ptr(o), L.ptr(lse), L.ptr(g), L.ptr(ger), L.ptr(gec),
                                                    L.ptr(gv), B, R, Q, D, K, 0 if shared else 1, int(precision), L.ptr(ws), ws.numel(), L.stream_ptr()),
                    "uni_corr_softmax_pv_bwd")
    return ger, gec, gv


class CorrSoftmaxPVFunction(torch.autograd.Function):
    """values @ softmax(embed_ref embed_cur^T, dim = reference axis) per frame, differentiable, in O(R + Q) memory:
    apply(embed_ref (B,R,128), embed_cur (B,Q,128), values (B,K,R), precision=0) -> (B,K,Q); fp32 or fp64 device tensors.
    The training form of unicorn/models/unicorn.py:321-326; saves `out` and `lse`, the backward recomputes the probabilities tile by tile."""

    @staticmethod
    def forward(ctx, embed_ref, embed_cur, values, precision=0):
        er, ec, v = _corr_train_args("CorrSoftmaxPVFunction", embed_ref, embed_cur, values)
        if precision != 0 and er.dtype == torch.float32 and any(ctx.needs_input_grad[:3]):
            raise L.UnicornHipError("CorrSoftmaxPVFunction: the backward exists in precision 0 (exact fp32) only, got precision %r" % (precision,))
        out, lse = corr_softmax_pv_lse(er, ec, v, precision)
        ctx.save_for_backward(er, ec, v, out, lse)
        ctx.precision = precision
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        er, ec, v, out, lse = ctx.saved_tensors
        ger, gec, gv = corr_softmax_pv_backward(er, ec, v, out, lse, grad_out.contiguous(), ctx.needs_input_grad[:3], ctx.precision)
        return ger, gec, gv, None


def propagate_labels(embed_0, embed_1, labels, precision=0):
    """The label propagation of the reference's training losses (unicorn/models/unicorn.py:321-326, 342-371) without the HW x HW matrices:
    embed_* (B, C, H, W) or (B, C, HW) (any strides), labels (B, K, HW_0) -> (B, K, HW_1), equal in value and in gradient to
        torch.bmm(labels, torch.softmax(torch.bmm(embed_0.flatten(-2).transpose(-1, -2), embed_1.flatten(-2)), dim=1)).
    The layout changes are ordinary torch ops, so autograd carries the gradients back to the callers' layouts."""
    if embed_0.dim() not in (3, 4) or embed_1.dim() not in (3, 4):
        raise L.UnicornHipError("propagate_labels: embeddings must be (B, C, H, W) or (B, C, HW), got %s, %s" % (tuple(embed_0.shape), tuple(embed_1.shape)))
    e0 = embed_0.flatten(2).transpose(1, 2)
    e1 = embed_1.flatten(2).transpose(1, 2)
    return CorrSoftmaxPVFunction.apply(e0, e1, labels, precision)


def prior_pyramid(coarse):
    """(1,K,H8,W8) -> (coarse, 1/2, 1/4) like unicorn_sot.py:103-105"""
    _need_cuda(coarse)
    c = coarse.float().contiguous()
    _, K, H8, W8 = c.shape
    p16 = torch.empty((1, K, H8 // 2, W8 // 2), device=c.device, dtype=torch.float32)
    p32 = torch.empty((1, K, H8 // 4, W8 // 4), device=c.device, dtype=torch.float32)
    L.check(L.lib().uni_prior_pyramid(L.ptr(c), L.ptr(p16), L.ptr(p32), K, H8, W8, L.stream_ptr()), "uni_prior_pyramid")
    return c, p16, p32


def label_map_s8(box_xyxy, H, W, device):
    b = torch.as_tensor(box_xyxy, dtype=torch.float32).reshape(4).to(device)
    out = torch.empty((1, (H // 8) * (W // 8)), device=device, dtype=torch.float32)
    L.check(L.lib().uni_label_map_s8(L.ptr(b), L.ptr(out), H, W, L.stream_ptr()), "uni_label_map_s8")
    return out


def sample_embeddings(embed, boxes_xyxy, stride=8.0):
    """embed (1,C,H8,W8); boxes (N,>=4) xyxy in input pixels -> (N,C)  (mot_evaluator.py:1024-1034)"""
    _need_cuda(embed, boxes_xyxy)
    e = nhwc(embed)
    _, Cc, H8, W8 = e.shape
    b = boxes_xyxy.float().contiguous()
    n = b.shape[0]
    out = torch.empty((n, Cc), device=e.device, dtype=torch.float32)
    if n:
        L.check(L.lib().uni_sample_embeddings(L.ptr(e), H8, W8, Cc, L.ptr(b), b.shape[1], n, float(stride), L.ptr(out),
                                              L.stream_ptr()), "uni_sample_embeddings")
    return out


def _condinst_inputs(mask_feats, up_masks, params, inst_loc, inst_lvl, up_rate):
    """what condinst_masks and condinst_masks_resized hand to the library: the NHWC maps, fp32 parameter rows, and for n > 0 instances
    their locations / int32 levels on the maps' device and the fp32 workspace -> (mf, um, p, loc, lvl, ws)"""
    _need_cuda(mask_feats, up_masks, params)
    mf, um = nhwc(mask_feats), nhwc(up_masks)
    p = params.float().contiguous()
    if p.shape[0] == 0:
        return mf, um, p, None, None, None
    loc = inst_loc.float().contiguous().to(mf.device)
    lvl = inst_lvl.to(device=mf.device, dtype=torch.int32).contiguous()
    ws = torch.empty(p.shape[0] * mf.shape[2] * mf.shape[3] * (1 + up_rate * up_rate), device=mf.device, dtype=torch.float32)
    return mf, um, p, loc, lvl, ws


def condinst_masks(mask_feats, up_masks, params, inst_loc, inst_lvl, up_rate, d_rate):
    """-> (N,1,d_rate*up_rate*H8, d_rate*up_rate*W8) sigmoid scores"""
    mf, um, p, loc, lvl, ws = _condinst_inputs(mask_feats, up_masks, params, inst_loc, inst_lvl, up_rate)
    (_, _, H8, W8), n = mf.shape, p.shape[0]
    out = torch.empty((n, 1, d_rate * up_rate * H8, d_rate * up_rate * W8), device=mf.device, dtype=torch.float32)
    if n:
        L.check(L.lib().uni_condinst_masks(L.ptr(mf), L.ptr(um), L.ptr(p), p.shape[1], L.ptr(loc), L.ptr(lvl), n, H8, W8,
                                           up_rate, d_rate, L.ptr(out), L.ptr(ws), ws.numel() * 4, L.stream_ptr()),
                "uni_condinst_masks")
    return out


def _condinst_loss_ws(dev, dtype, n, H8, W8, r):
    need = L.lib().uni_condinst_loss_workspace_bytes(n, H8, W8, r) * _ws_factor(dtype)
    return torch.empty(max(need, 8), device=dev, dtype=torch.uint8)


class CondInstDiceFunction(torch.autograd.Function):
    """The CondInst mask loss per instance (dynamic_mask_head.py:247-278) on the kernels' layouts, differentiable, in O(N H8 W8) memory:
    apply(mask_feats (H8,W8,8), up_masks (H8,W8,9 r r), params (N,169), inst_loc (N,2), inst_lvl (N,) int32, gt (N,r H8,r W8), up_rate)
    -> loss (N,); fp32 or fp64 contiguous device tensors (condinst_dice_loss checks and converts).  Saves the inputs and three sums per
    instance; the backward recomputes the sigmoid scores from the coarse logits.  One writer per gradient element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, mask_feats, up_masks, params, inst_loc, inst_lvl, gt, up_rate):
        H8, W8, _ = mask_feats.shape
        n, r = params.shape[0], int(up_rate)
        fn, fwd = _entry("uni_condinst_loss_fwd", params.dtype)
        loss = torch.empty((n,), device=params.device, dtype=params.dtype)
        sums = torch.empty((n, 3), device=params.device, dtype=params.dtype)
        with torch.cuda.device(params.device):
            ws = _condinst_loss_ws(params.device, params.dtype, n, H8, W8, r)
            L.check(fn(L.ptr(mask_feats), L.ptr(up_masks), L.ptr(params), params.stride(0), L.ptr(inst_loc), L.ptr(inst_lvl), L.ptr(gt), n, H8, W8, r,
                       L.ptr(loss), L.ptr(sums), L.ptr(ws), ws.numel(), L.stream_ptr()), fwd)
        ctx.save_for_backward(mask_feats, up_masks, params, inst_loc, inst_lvl, gt, sums)
        ctx.up_rate = r
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        mf, um, p, loc, lvl, gt, sums = ctx.saved_tensors
        H8, W8, _ = mf.shape
        n, r = p.shape[0], ctx.up_rate
        fn, bwd = _entry("uni_condinst_loss_bwd", p.dtype)
        g = grad_loss.contiguous()
        gmf = torch.empty_like(mf) if ctx.needs_input_grad[0] else None
        gum = torch.empty_like(um) if ctx.needs_input_grad[1] else None
        gp = torch.empty((n, p.stride(0)), device=p.device, dtype=p.dtype)[:, :169] if ctx.needs_input_grad[2] else None      # rows of pitch ldp, like params
        if gmf is not None or gum is not None or gp is not None:
            with torch.cuda.device(p.device):
                ws = _condinst_loss_ws(p.device, p.dtype, n, H8, W8, r)
                L.check(fn(L.ptr(mf), L.ptr(um), L.ptr(p), p.stride(0), L.ptr(loc), L.ptr(lvl), L.ptr(gt), L.ptr(sums), L.ptr(g), n, H8, W8, r,
                           L.ptr(gmf), L.ptr(gum), L.ptr(gp), L.ptr(ws), ws.numel(), L.stream_ptr()), bwd)
        return gmf, gum, gp, None, None, None, None


def condinst_dice_loss(mask_feats, up_masks, params, inst_loc, inst_lvl, gt_bitmasks, up_rate):
    """The training half of DynamicMaskHead.__call__ (dynamic_mask_head.py:247-278, fully supervised branch) in one call:
    mask_feats (1,8,H8,W8), up_masks (1,9 r r,H8,W8), params (N,169), inst_loc (N,2), inst_lvl (N,), gt_bitmasks (N,1,r H8,r W8) or
    (N,r H8,r W8) -> the (N,) per-instance dice losses; the reference's `loss_mask` is `.mean()` of it.  Equal in value and in gradient
    (mask_feats, up_masks, params) to dice_coefficient(mask_heads_forward_with_coords(...).sigmoid(), gt_bitmasks), without any
    (N, r H8, r W8) tensor.  All floating tensors fp32 or all fp64; the NCHW -> NHWC layout changes are ordinary torch ops, so autograd
    carries the gradients back to the callers' layouts."""
    ts = (mask_feats, up_masks, params, inst_loc, gt_bitmasks)
    r = int(up_rate)
    if mask_feats.dim() != 4 or up_masks.dim() != 4 or params.dim() != 2 or mask_feats.shape[0] != 1 or mask_feats.shape[1] != 8 \
            or r < 1 or r > 16 or tuple(up_masks.shape) != (1, 9 * r * r) + tuple(mask_feats.shape[2:]) or params.shape[1] != 169 \
            or tuple(inst_loc.shape) != (params.shape[0], 2) or tuple(inst_lvl.shape) != (params.shape[0],):
        raise L.UnicornHipError("condinst_dice_loss: shapes %s, inst_lvl %s, up_rate %r do not fit mask_feats (1,8,H8,W8), up_masks (1,9 r r,H8,W8), "
                                "params (N,169), inst_loc (N,2), inst_lvl (N,), up_rate 1..16"
                                % ([tuple(t.shape) for t in ts], tuple(inst_lvl.shape), up_rate))
    n, H8, W8 = params.shape[0], mask_feats.shape[2], mask_feats.shape[3]
    if tuple(gt_bitmasks.shape) not in ((n, 1, r * H8, r * W8), (n, r * H8, r * W8)):
        raise L.UnicornHipError("condinst_dice_loss: gt_bitmasks %s do not fit (N,1,r H8,r W8) = (%d, 1, %d, %d): the ground truth must be exactly "
                                "up_rate x the feature map" % (tuple(gt_bitmasks.shape), n, r * H8, r * W8))
    if params.dtype not in _F64_SFX or any(t.dtype != params.dtype for t in ts):
        raise L.UnicornHipError("condinst_dice_loss: dtypes %s unsupported (all fp32 or all fp64)" % [str(t.dtype) for t in ts])
    if inst_lvl.dtype.is_floating_point or inst_lvl.dtype == torch.bool:
        raise L.UnicornHipError("condinst_dice_loss: inst_lvl must be an integer tensor, got %s" % inst_lvl.dtype)
    _need_cuda(*ts, inst_lvl)
    if n == 0:
        return params.new_zeros((0,))
    if H8 == 0 or W8 == 0:
        raise L.UnicornHipError("condinst_dice_loss: empty feature map %s" % (tuple(mask_feats.shape),))
    mf = mask_feats[0].permute(1, 2, 0).contiguous()
    um = up_masks[0].permute(1, 2, 0).contiguous()
    p = params if params.stride(1) == 1 and params.stride(0) >= 169 else params.contiguous()      # a row pitch (ldp) is passed through
    return CondInstDiceFunction.apply(mf, um, p, inst_loc.detach().contiguous(), inst_lvl.to(torch.int32).contiguous(),
                                      gt_bitmasks.detach().reshape(n, r * H8, r * W8).contiguous(), r)


def _simota_1d(name, t, A):
    if t.dim() == 2 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 1 or t.shape[0] != A:
        raise ValueError("simota_assign: %s %s does not fit (1, A) or (A,) with A = %d" % (name, tuple(t.shape), A))
    return t


def _simota_check(ts, names):
    for n, t in zip(names, ts):
        if not isinstance(t, torch.Tensor):
            raise ValueError("simota_assign: %s is not a tensor" % n)
    for n, t in zip(names, ts):
        if t.dtype != torch.float32:
            raise ValueError("simota_assign: %s is %s; only fp32 is supported (no fp16 / autocast inputs)" % (n, t.dtype))


def _simota_dev(ts, names):
    for n, t in zip(names, ts):
        if not t.is_cuda:
            raise ValueError("simota_assign: %s is a CPU tensor; the operator needs HIP device tensors (there is no CPU fallback)" % n)
    if len({t.device for t in ts}) != 1:
        raise ValueError("simota_assign: tensors on different devices %s" % sorted({str(t.device) for t in ts}))


def _simota_img(img_size):
    try:
        h, w = int(img_size[0]), int(img_size[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError("simota_assign: img_size %r is not (height, width)" % (img_size,))
    if h <= 0 or w <= 0:
        raise ValueError("simota_assign: img_size %r is not positive" % (img_size,))
    return h, w


def _simota_call(outputs, labels, num_gt, xs, ys, st, h, w, C):
    """outputs (B, A, >= 5 + C) with unit column stride, labels (B, M, 5) contiguous, num_gt (B,) int32 on the device, xs / ys / st (A,)
    contiguous -> fg (B, A) uint8, matched (B, A) int32, iou (B, A) fp32, num_fg (B,) int32.  No host synchronisation."""
    B, A, M, dev = outputs.shape[0], outputs.shape[1], labels.shape[1], outputs.device
    lib = L.lib()
    need = lib.uni_simota_workspace_bytes(B, A, M, C)
    if need == 0:
        raise ValueError("simota_assign: shape B=%d A=%d M=%d C=%d is outside the limits of uni_simota_assign (include/unicorn_hip.h)"
                         % (B, A, M, C))
    fg = torch.empty((B, A), device=dev, dtype=torch.uint8)
    matched = torch.empty((B, A), device=dev, dtype=torch.int32)
    iou = torch.empty((B, A), device=dev, dtype=torch.float32)
    num_fg = torch.empty((B,), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        L.check(lib.uni_simota_assign(L.ptr(outputs), outputs.stride(1), L.ptr(labels), L.ptr(num_gt), M, L.ptr(xs), L.ptr(ys), L.ptr(st), B, A, C,
                                      h, w, L.ptr(fg), L.ptr(matched), L.ptr(iou), L.ptr(num_fg), L.ptr(ws), need, L.stream_ptr()),
                "uni_simota_assign")
    return fg, matched, iou, num_fg


def simota_assign_batch(outputs, labels, x_shifts, y_shifts, expanded_strides, img_size, num_classes):
    """The SimOTA label assignment of get_losses (unicorn_head_mask.py:571-645 with :754-983) for the WHOLE batch in one call and without a
    host synchronisation: outputs (B, A, 5 + C) = decoded cx, cy, w, h, objectness logit, class logits; labels (B, M, 5) = class, cx, cy, w, h,
    padded with zero rows (the number of boxes per image is (labels.sum(2) > 0).sum(1), computed on the device as the reference does);
    x_shifts / y_shifts / expanded_strides (1, A) or (A,); img_size (height, width); all tensors fp32 on one HIP device.
    -> fg_masks (B, A) bool, matched_gt_inds (B, A) int64 (-1 = background), matched_ious (B, A), num_fg (B,) int64 on the device.
    Ties, which PyTorch leaves open: the lower anchor index wins in both top-k passes, the lower box index in the arg-min."""
    names = ("outputs", "labels", "x_shifts", "y_shifts", "expanded_strides")
    ts = (outputs, labels, x_shifts, y_shifts, expanded_strides)
    _simota_check(ts, names)
    C = int(num_classes)
    if outputs.dim() != 3 or labels.dim() != 3 or C < 1 or outputs.shape[2] != 5 + C or labels.shape[2] != 5 or labels.shape[0] != outputs.shape[0]:
        raise ValueError("simota_assign_batch: outputs %s, labels %s do not fit (B, A, 5 + num_classes) and (B, M, 5) with num_classes = %r"
                         % (tuple(outputs.shape), tuple(labels.shape), num_classes))
    B, A, _ = outputs.shape
    xs, ys, st = (_simota_1d(n, t, A).contiguous() for n, t in zip(names[2:], ts[2:]))
    h, w = _simota_img(img_size)
    if B == 0 or A == 0:
        raise ValueError("simota_assign_batch: empty batch or no anchors, outputs %s" % (tuple(outputs.shape),))
    _simota_dev(ts, names)
    with torch.no_grad():
        out = outputs.detach()
        out = out if out.stride(2) == 1 and out.stride(0) == A * out.stride(1) and out.stride(1) >= 5 + C else out.contiguous()
        lab = labels.detach().contiguous()
        num_gt = (lab.sum(dim=2) > 0).sum(dim=1).to(torch.int32)
        fg, matched, iou, num_fg = _simota_call(out, lab, num_gt, xs, ys, st, h, w, C)
        return fg.bool(), matched.long(), iou, num_fg.long()


def simota_assign(bboxes_preds_per_image, obj_preds_b, cls_preds_b, gt_bboxes_per_image, gt_classes, x_shifts, y_shifts, expanded_strides,
                  img_size, num_classes):
    """Drop-in for the get_assignments call of one image (unicorn_head_mask.py:592-613): bboxes_preds_per_image (A, 4) decoded cx, cy, w, h,
    obj_preds_b (A, 1) and cls_preds_b (A, C) logits, gt_bboxes_per_image (G, 4) cx, cy, w, h, gt_classes (G,), shifts and strides (1, A) or
    (A,), img_size (height, width); all fp32 on one HIP device.  -> the reference's tuple (gt_matched_classes (num_fg,), fg_mask (A,) bool,
    pred_ious_this_matching (num_fg,), matched_gt_inds (num_fg,) int64 in ascending anchor order, num_fg int).  The one host synchronisation
    is the read of num_fg.  Ties: the lower anchor index wins in both top-k passes, the lower box index in the arg-min."""
    names = ("bboxes_preds_per_image", "obj_preds_b", "cls_preds_b", "gt_bboxes_per_image", "gt_classes", "x_shifts", "y_shifts",
             "expanded_strides")
    ts = (bboxes_preds_per_image, obj_preds_b, cls_preds_b, gt_bboxes_per_image, gt_classes, x_shifts, y_shifts, expanded_strides)
    _simota_check(ts, names)
    C = int(num_classes)
    box, obj, cls, gtb, gtc = ts[:5]
    if box.dim() != 2 or box.shape[1] != 4 or C < 1 or tuple(cls.shape) != (box.shape[0], C) or gtb.dim() != 2 or gtb.shape[1] != 4 \
            or tuple(gtc.shape) != (gtb.shape[0],) or obj.numel() != box.shape[0] or obj.dim() not in (1, 2):
        raise ValueError("simota_assign: shapes %s do not fit bboxes (A, 4), obj (A, 1), cls (A, num_classes = %r), gt boxes (G, 4), gt classes (G,)"
                         % ([tuple(t.shape) for t in ts[:5]], num_classes))
    A, G, dev = box.shape[0], gtb.shape[0], box.device
    xs, ys, st = (_simota_1d(n, t, A).contiguous() for n, t in zip(names[5:], ts[5:]))
    h, w = _simota_img(img_size)
    if A == 0:
        raise ValueError("simota_assign: no anchors")
    _simota_dev(ts, names)
    if G == 0:
        return (gtc.new_zeros((0,)), torch.zeros((A,), device=dev, dtype=torch.bool), box.new_zeros((0,)),
                torch.zeros((0,), device=dev, dtype=torch.int64), 0)
    with torch.no_grad():
        out = torch.cat([box.detach(), obj.detach().reshape(A, 1), cls.detach()], dim=1)[None]
        lab = torch.cat([gtc.detach()[:, None], gtb.detach()], dim=1)[None].contiguous()
        num_gt = torch.full((1,), G, device=dev, dtype=torch.int32)
        fg, matched, iou, num_fg = _simota_call(out, lab, num_gt, xs, ys, st, h, w, C)
        n = int(num_fg.item())                                     # the one host synchronisation
        fg = fg[0].bool()
        # compaction in ascending anchor order without a second synchronisation (a boolean index would read the count back again):
        # matched anchor a goes to slot (number of matched anchors before it); the others share a dump slot that is cut off.
        # scatter_ with duplicate indices is non-deterministic, but the duplicates all land in that discarded slot: slots < n have one writer
        slot = torch.where(fg, torch.cumsum(fg, 0) - 1, torch.full((), n, device=dev, dtype=torch.int64))
        anchors = torch.zeros((n + 1,), device=dev, dtype=torch.int64).scatter_(0, slot, torch.arange(A, device=dev))[:n]
        inds = matched[0].long()[anchors]
        return gtc[inds], fg, iou[0][anchors], inds, n


def _hl_ws(dev, B, A, Cn):
    need = L.lib().uni_head_loss_workspace_bytes(B, A, Cn)
    if need == 0:
        raise ValueError("head_det_loss: shape B=%d A=%d C=%d is outside the limits of uni_head_loss_fwd (include/unicorn_hip.h)" % (B, A, Cn))
    return torch.empty(need, device=dev, dtype=torch.uint8)


def _hl_rows(t, cols):
    """(B, A, cols) with unit column stride and one row pitch >= cols over the whole batch is passed through; anything else is copied"""
    return t if t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1) and t.stride(1) >= cols else t.contiguous()


class HeadLossFunction(torch.autograd.Function):
    """The four detection losses of get_losses (unicorn_head_mask.py:646-745) from the device-side assignment, differentiable in `outputs`
    and `origin_preds`: apply(outputs (B, A, 5 + C), origin_preds (B, A, 4) or None, labels (B, M, 5), fg (B, A) uint8, matched (B, A) int32,
    iou (B, A), num_fg (B,) int32, num_gt (B,) int32, xs, ys, st (A,), reg_weight) -> (5,) = reg_weight x iou, obj, cls, l1 losses and
    max(sum num_fg, 1) / max(sum num_gt, 1).  All floating-point tensors fp32, or all fp64; `outputs` may carry a row pitch (a view of a wider
    buffer).  Saves the inputs only; the backward recomputes.  No host synchronisation in either direction; one writer per gradient
    element and no atomic: bitwise reproducible."""

    @staticmethod
    def forward(ctx, outputs, origin_preds, labels, fg, matched, iou, num_fg, num_gt, xs, ys, st, reg_weight):
        B, A, Cn = outputs.shape[0], outputs.shape[1], outputs.shape[2] - 5
        M, dev = labels.shape[1], outputs.device
        out_ = _hl_rows(outputs.detach(), 5 + Cn)
        org_ = None if origin_preds is None else _hl_rows(origin_preds.detach(), 4)
        ins = (out_, org_, labels.contiguous(), fg.contiguous(), matched.contiguous(), iou.contiguous(), num_fg.contiguous(), num_gt.contiguous(),
               xs.contiguous(), ys.contiguous(), st.contiguous())
        ctx.save_for_backward(*ins)
        ctx.reg_weight, ctx.dims = float(reg_weight), (B, A, Cn, M)
        res = torch.empty((5,), device=dev, dtype=outputs.dtype)
        fn, fwd = _entry("uni_head_loss_fwd", outputs.dtype)
        with torch.cuda.device(dev):
            ws = _hl_ws(dev, B, A, Cn)
            L.check(fn(L.ptr(out_), out_.stride(1), L.ptr(org_), 0 if org_ is None else org_.stride(1), L.ptr(ins[2]), M, *map(L.ptr, ins[3:]), B, A,
                       Cn, ctx.reg_weight, L.ptr(res), L.ptr(ws), ws.numel(), L.stream_ptr()), fwd)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_res):
        ins = ctx.saved_tensors
        out_, org_ = ins[:2]
        B, A, Cn, M = ctx.dims
        # both are written completely by the call
        g_out = torch.empty((B, A, 5 + Cn), device=out_.device, dtype=out_.dtype) if ctx.needs_input_grad[0] else None
        g_org = torch.empty((B, A, 4), device=out_.device, dtype=out_.dtype) if org_ is not None and ctx.needs_input_grad[1] else None
        if g_out is not None or g_org is not None:
            fn, bwd = _entry("uni_head_loss_bwd", out_.dtype)
            g = grad_res[:4].contiguous()
            with torch.cuda.device(out_.device):
                ws = _hl_ws(out_.device, B, A, Cn)
                L.check(fn(L.ptr(out_), out_.stride(1), L.ptr(org_), 0 if org_ is None else org_.stride(1), L.ptr(ins[2]), M, *map(L.ptr, ins[3:]),
                           L.ptr(g), B, A, Cn, ctx.reg_weight, L.ptr(g_out), 5 + Cn, L.ptr(g_org), L.ptr(ws), ws.numel(), L.stream_ptr()), bwd)
        return (g_out, g_org) + (None,) * 10


def head_det_loss(outputs, origin_preds, labels, x_shifts, y_shifts, expanded_strides, img_size, num_classes, reg_weight=5.0, assignment=None):
    """The detection part of get_losses (unicorn_head_mask.py:571-745 without the CondInst lines :675-694; identically unicorn_head.py) for
    the WHOLE batch without a host synchronisation: the SimOTA assignment (simota_assign_batch's kernels, under no_grad) and then the four
    losses in one fused forward and one fused backward.  outputs (B, A, 5 + C) = decoded cx, cy, w, h, objectness logit, class logits;
    origin_preds (B, A, 4), a list of per-level (B, A_l, 4) tensors (concatenated as the reference does) or None (use_l1 False: l1_loss is an
    exact zero and carries no gradient); labels (B, M, 5) = class, cx, cy, w, h padded with zero rows; x_shifts / y_shifts /
    expanded_strides (1, A) or (A,); img_size (height, width); all tensors fp32 on one HIP device.  assignment: the 4-tuple that
    simota_assign_batch returned for these inputs (it is not computed again).
    -> (losses, assignment): losses = dict of 0-d device tensors iou_loss (already times reg_weight), conf_loss, cls_loss, l1_loss, num_fg
    (max(sum num_fg, 1) / max(sum num_gt, 1), the ratio the reference logs: 1.0 with no box at all) and total_loss = the sum of the four losses; assignment = (fg_masks bool,
    matched_gt_inds int64, matched_ious, num_fg int64) for the mask loss."""
    if isinstance(origin_preds, (list, tuple)):
        for k, t in enumerate(origin_preds):
            if not isinstance(t, torch.Tensor):
                raise ValueError("head_det_loss: origin_preds[%d] is not a tensor" % k)
            if t.dim() != 3 or t.shape[2] != 4 or t.shape[0] != origin_preds[0].shape[0] or t.dtype != origin_preds[0].dtype \
                    or t.device != origin_preds[0].device:
                raise ValueError("head_det_loss: origin_preds[%d] %s %s does not fit a list of (B, A_level, 4) tensors of one dtype and device"
                                 % (k, tuple(t.shape), t.dtype))
        if len(origin_preds) == 0:
            raise ValueError("head_det_loss: origin_preds is an empty list (pass None for use_l1 = False)")
        origin_preds = torch.cat(list(origin_preds), 1)
    names = ("outputs", "labels", "x_shifts", "y_shifts", "expanded_strides") + (() if origin_preds is None else ("origin_preds",))
    ts = (outputs, labels, x_shifts, y_shifts, expanded_strides) + (() if origin_preds is None else (origin_preds,))
    for n, t in zip(names, ts):
        if not isinstance(t, torch.Tensor):
            raise ValueError("head_det_loss: %s is not a tensor" % n)
    for n, t in zip(names, ts):
        if t.dtype != torch.float32:
            raise ValueError("head_det_loss: %s is %s; only fp32 is supported (no fp16 / bf16 / autocast inputs)" % (n, t.dtype))
    Cn = int(num_classes)
    if outputs.dim() != 3 or labels.dim() != 3 or Cn < 1 or outputs.shape[2] != 5 + Cn or labels.shape[2] != 5 or labels.shape[0] != outputs.shape[0]:
        raise ValueError("head_det_loss: outputs %s, labels %s do not fit (B, A, 5 + num_classes) and (B, M, 5) with num_classes = %r"
                         % (tuple(outputs.shape), tuple(labels.shape), num_classes))
    B, A, _ = outputs.shape
    if origin_preds is not None and tuple(origin_preds.shape) != (B, A, 4):
        raise ValueError("head_det_loss: origin_preds %s do not fit (B, A, 4) = (%d, %d, 4)" % (tuple(origin_preds.shape), B, A))
    xs, ys, st = (_simota_1d(n, t, A).contiguous() for n, t in zip(names[2:5], ts[2:5]))
    h, w = _simota_img(img_size)
    if B == 0 or A == 0:
        raise ValueError("head_det_loss: empty batch or no anchors, outputs %s" % (tuple(outputs.shape),))
    if assignment is not None:
        if not isinstance(assignment, (tuple, list)) or len(assignment) != 4 or not all(isinstance(t, torch.Tensor) for t in assignment) \
                or any(tuple(t.shape) != (B, A) for t in assignment[:3]) or tuple(assignment[3].shape) != (B,) \
                or assignment[2].dtype != torch.float32:
            raise ValueError("head_det_loss: assignment is not the (fg_masks (B, A), matched_gt_inds (B, A), matched_ious (B, A) fp32, num_fg (B,)) "
                             "tuple of simota_assign_batch")
        names, ts = names + ("assignment",) * 4, ts + tuple(assignment)
    _simota_dev(ts, names)
    with torch.no_grad():
        lab = labels.detach().contiguous()
        num_gt = (lab.sum(dim=2) > 0).sum(dim=1).to(torch.int32)
        if assignment is None:
            fg, matched, iou, num_fg = _simota_call(_hl_rows(outputs.detach(), 5 + Cn), lab, num_gt, xs, ys, st, h, w, Cn)
            assignment = (fg.bool(), matched.long(), iou, num_fg.long())
        else:
            fg, matched, iou, num_fg = (assignment[0].to(torch.uint8), assignment[1].to(torch.int32), assignment[2].detach(),
                                        assignment[3].to(torch.int32))
            assignment = tuple(assignment)
    res = HeadLossFunction.apply(outputs, origin_preds, lab, fg, matched, iou, num_fg, num_gt, xs, ys, st, float(reg_weight))
    l1 = res[3] if origin_preds is not None else res.new_zeros(())
    losses = {"total_loss": res[0] + res[1] + res[2] + l1, "iou_loss": res[0], "conf_loss": res[1], "cls_loss": res[2], "l1_loss": l1,
              "num_fg": res[4].detach()}
    return losses, assignment


HEAD_ASSEMBLE_MAX_LEVELS = 4
HEAD_ASSEMBLE_TILE = 64           # anchors of one level per block (HA_TILE of csrc/kernels.h): shapes around it are the ragged ones


def _ha_arrays(hs, ws, strides, layouts):
    n = len(hs)
    return ((C.c_int32 * n)(*hs), (C.c_int32 * n)(*ws), (C.c_double * n)(*strides), (C.c_int32 * n)(*layouts))


def _ha_ptrs(ts):
    """host array of the device pointers of `ts` (an entry None: NULL), or None for no list at all"""
    return None if ts is None else (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class HeadAssembleFunction(torch.autograd.Function):
    """The head-output assembly (unicorn_head_mask.py:339-366, :476-500, the cats :396-401 / :554-558) as one launch forward and one backward:
    apply(strides (tuple of L floats), use_l1, has_ctrl, *maps) with maps = the L reg maps (B, 4, h, w), the L obj maps (B, 1, h, w), the L cls
    maps (B, C, h, w) and, with has_ctrl, the L controller maps (B, P, h, w) -> (outputs (B, A, 5 + C), origin_preds (B, A, 4) or None,
    x_shifts, y_shifts, expanded_strides (1, A), dynamic_params (B, A, P) or None, fpn_levels (B, A) int32 or None).  Maps fp32 / fp16 / bf16
    -> results fp32, or all fp64 (ops.head_assemble checks).  NCHW-contiguous and channels-last memory are read in place per map, other
    strides are converted once.  Saves the reg maps only.  Gradients in the dtype and layout of their map, only those autograd asks for; an
    unused result costs no zero tensor.  The shifts, strides and levels are not differentiable.  No host synchronisation, no host-built
    tensor, one writer per element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, strides, use_l1, has_ctrl, *maps):
        ctx.set_materialize_grads(False)
        Ln = len(strides)
        laid = [_map_layout(m) for m in maps]
        roles = [[t for t, _ in laid[r * Ln:(r + 1) * Ln]] for r in range(4 if has_ctrl else 3)]
        reg, obj, cls = roles[:3]
        ctrl = roles[3] if has_ctrl else None
        layouts = [sum(laid[r * Ln + k][1] << r for r in range(len(roles))) for k in range(Ln)]
        B, Cn, P = reg[0].shape[0], cls[0].shape[1], ctrl[0].shape[1] if has_ctrl else 0
        hs, ws = [t.shape[2] for t in reg], [t.shape[3] for t in reg]
        A, dev, mdt = sum(h * w for h, w in zip(hs, ws)), reg[0].device, reg[0].dtype
        dt = torch.float64 if mdt == torch.float64 else torch.float32
        outputs = torch.empty((B, A, 5 + Cn), device=dev, dtype=dt)
        origin = torch.empty((B, A, 4), device=dev, dtype=dt) if use_l1 else None
        xs, ys, st = (torch.empty((1, A), device=dev, dtype=dt) for _ in range(3))
        params = torch.empty((B, A, P), device=dev, dtype=dt) if has_ctrl else None
        levels = torch.empty((B, A), device=dev, dtype=torch.int32) if has_ctrl else None
        ctx.geom = (hs, ws, tuple(strides), layouts, Ln, B, Cn, P, _STORE_DTYPE[mdt])
        ctx.shapes = [(t.shape, t.dtype) for r in roles for t in r]
        ctx.save_for_backward(*reg)
        fn, name = _entry("uni_head_assemble_fwd", dt)
        with torch.cuda.device(dev):
            L.check(fn(_ha_ptrs(reg), _ha_ptrs(obj), _ha_ptrs(cls), _ha_ptrs(ctrl), *_ha_arrays(hs, ws, strides, layouts), Ln, B, Cn, P,
                       _STORE_DTYPE[mdt], L.ptr(outputs), 5 + Cn, L.ptr(origin), L.ptr(xs), L.ptr(ys), L.ptr(st), L.ptr(params),
                       P, L.ptr(levels), L.stream_ptr()), name)
        ctx.mark_non_differentiable(*[t for t in (xs, ys, st, levels) if t is not None])
        return outputs, origin, xs, ys, st, params, levels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_org, _gx, _gy, _gs, g_par, _gl):
        hs, ws, strides, layouts, Ln, B, Cn, P, code = ctx.geom
        reg = ctx.saved_tensors
        nroles = len(ctx.shapes) // Ln
        need = ctx.needs_input_grad[3:]
        # a gradient that nobody sent is a zero: its maps get none (autograd reads None as zero), the others read a NULL pointer as zero
        live = (g_out is not None or g_org is not None, g_out is not None, g_out is not None, g_par is not None)
        grads = [None] * len(need)
        for r in range(nroles):
            for k in range(Ln):
                i = r * Ln + k
                if need[i] and live[r]:
                    shape, dtype = ctx.shapes[i]
                    grads[i] = torch.empty(shape, device=reg[0].device, dtype=dtype,
                                           memory_format=torch.contiguous_format if (layouts[k] >> r) & 1 else torch.channels_last)
        if any(g is not None for g in grads):
            dt = torch.float64 if reg[0].dtype == torch.float64 else torch.float32
            g_out = None if g_out is None else _hl_rows(g_out, 5 + Cn)
            g_org = None if g_org is None else g_org.contiguous()
            g_par = None if g_par is None else _hl_rows(g_par, P)
            fn, name = _entry("uni_head_assemble_bwd", dt)
            per_role = [grads[r * Ln:(r + 1) * Ln] for r in range(nroles)] + [None] * (4 - nroles)
            with torch.cuda.device(reg[0].device):
                L.check(fn(_ha_ptrs(list(reg)), *_ha_arrays(hs, ws, strides, layouts), Ln, B, Cn, P, code, L.ptr(g_out),
                           0 if g_out is None else g_out.stride(1), L.ptr(g_org), L.ptr(g_par), 0 if g_par is None else g_par.stride(1),
                           *[_ha_ptrs(p) if p is not None and any(t is not None for t in p) else None for p in per_role], L.stream_ptr()), name)
        return (None, None, None) + tuple(grads)


def head_assemble(reg_outputs, obj_outputs, cls_outputs, strides, controller_outputs=None, use_l1=True):
    """The training-time lines of the heads' forward between the prediction convolutions and get_losses (unicorn_head_mask.py:339-366 with
    get_output_and_grid :476-500 and the level cats :396-401 / :554-558; identically unicorn_head.py, yolo_head_det.py, yolo_head_det_mask.py)
    for all levels and the whole batch in one launch, differentiable in every map, n_anchors == 1.
      reg_outputs, obj_outputs, cls_outputs   lists of L <= 4 maps (B, 4, h_l, w_l), (B, 1, h_l, w_l), (B, C, h_l, w_l)
      controller_outputs                      None or a list of L maps (B, P, h_l, w_l) (P = 169 in the reference)
      strides                                 L positive numbers
    All maps of one call fp32, fp16 or bf16 (read as stored, decoded in fp32: wider than the reference's fp16 decode under autocast, whose
    exp overflows above 11.09) with fp32 results, or all fp64 with fp64 results.  NCHW-contiguous and channels-last memory are read in place,
    per map; other strides are converted once.  With anchor a = off_l + y w_l + x:
    -> (outputs (B, A, 5 + C) = (reg0 + x) s, (reg1 + y) s, exp(reg2) s, exp(reg3) s, obj, cls -- the fp32 bits of the eager lines in columns
        0, 1, 4 and up; origin_preds (B, A, 4) = reg, or None with use_l1 False; x_shifts, y_shifts, expanded_strides (1, A); dynamic_params
        (B, A, P) and fpn_levels (B, A) int32, or None, None without controller maps)
    as get_losses / ops.head_det_loss / ops.head_mask_loss take them.  Gradients reach every map that requires one, in its dtype and layout,
    rounded once; the shifts, strides and levels carry none.  Autograd keeps the reg maps and nothing else.  No host synchronisation, no
    host-to-device copy.  1 <= C <= 256, 1 <= P <= 1024, 1 <= B <= 65535, A < 2^24."""
    op = "head_assemble"
    names = ("reg_outputs", "obj_outputs", "cls_outputs") + (() if controller_outputs is None else ("controller_outputs",))
    lists = (reg_outputs, obj_outputs, cls_outputs) + (() if controller_outputs is None else (controller_outputs,))
    for n, ts in zip(names, lists):
        if not isinstance(ts, (list, tuple)):
            raise L.UnicornHipError("%s: %s is not a list of maps" % (op, n))
        _check_tensors(op, ["%s[%d]" % (n, k) for k in range(len(ts))], ts)
    Ln = len(reg_outputs)
    if not 1 <= Ln <= HEAD_ASSEMBLE_MAX_LEVELS or any(len(ts) != Ln for ts in lists):
        raise L.UnicornHipError("%s: %s maps per role do not fit 1 <= L <= %d levels, the same for every role"
                                % (op, " / ".join(str(len(ts)) for ts in lists), HEAD_ASSEMBLE_MAX_LEVELS))
    try:
        strides = tuple(float(s) for s in strides)
    except (TypeError, ValueError):
        raise L.UnicornHipError("%s: strides %r are not %d numbers" % (op, strides, Ln))
    if len(strides) != Ln or not all(0 < s < float("inf") for s in strides):
        raise L.UnicornHipError("%s: strides %r are not %d positive numbers" % (op, strides, Ln))
    for n, ts in zip(names, lists):
        for k, t in enumerate(ts):
            _check_map_dims(op, "%s[%d]" % (n, k), t)
    B, Cn = reg_outputs[0].shape[0], cls_outputs[0].shape[1]
    P = None if controller_outputs is None else controller_outputs[0].shape[1]
    chans = (4, 1, Cn) + (() if P is None else (P,))
    for n, ts, nc in zip(names, lists, chans):
        for k, t in enumerate(ts):
            if tuple(t.shape) != (B, nc) + tuple(reg_outputs[k].shape[2:]):
                raise L.UnicornHipError("%s: %s[%d] of shape %s is not (%d, %d, %d, %d): the level's size with the role's channels"
                                        % (op, n, k, tuple(t.shape), B, nc, reg_outputs[k].shape[2], reg_outputs[k].shape[3]))
    A = sum(t.shape[2] * t.shape[3] for t in reg_outputs)
    if not (1 <= B <= 65535 and 1 <= Cn <= 256 and (P is None or 1 <= P <= 1024) and all(t.shape[2] and t.shape[3] for t in reg_outputs)
            and A < 1 << 24):
        raise L.UnicornHipError("%s: shape B=%d C=%d P=%r levels %s is outside 1 <= B <= 65535, 1 <= C <= 256, 1 <= P <= 1024, non-empty levels "
                                "with fewer than 2^24 anchors" % (op, B, Cn, P, [tuple(t.shape[2:]) for t in reg_outputs]))
    every = [t for ts in lists for t in ts]
    if reg_outputs[0].dtype not in _STORE_DTYPE or any(t.dtype != reg_outputs[0].dtype for t in every):
        raise L.UnicornHipError("%s: dtypes %s unsupported (all maps fp32, fp16 or bf16, or all fp64)"
                                % (op, ", ".join(sorted({str(t.dtype) for t in every}))))
    _check_one_device(op, every)
    return HeadAssembleFunction.apply(strides, bool(use_l1), controller_outputs is not None, *every)


def _hm_ws(dev, dtype, B, A, H8, W8, r, cap):
    need = L.lib().uni_head_mask_loss_workspace_bytes(B, A, H8, W8, r, cap)
    if need == 0:
        raise L.UnicornHipError("head_mask_loss: shape B=%d A=%d H8=%d W8=%d up_rate=%d capacity=%d is outside the limits of "
                                "uni_head_mask_loss_fwd (include/unicorn_hip.h)" % (B, A, H8, W8, r, cap))
    return torch.empty(need * _ws_factor(dtype), device=dev, dtype=torch.uint8)


class HeadMaskLossFunction(torch.autograd.Function):
    """The CondInst mask loss of get_losses (unicorn_head_mask.py:568-569, :675-694, :731-732) for the whole batch from the device-side
    assignment, differentiable in the two maps and the parameters: apply(mask_feats (B, H8, W8, 8), up_masks (B, H8, W8, 9 r r),
    params (B, A, 169) rows of any pitch >= 169, fpn_levels (B, A) int32, masks (B, M, r H8, r W8), fg (B, A) uint8, matched (B, A) int32,
    xs, ys, st (A,), up_rate, capacity) -> (1 + B,) = loss_condinst, loss_mask per image.  All floating-point tensors fp32, or all fp64,
    contiguous (head_mask_loss checks and converts).  Saves the inputs and three sums per instance slot; the backward recomputes.  No host
    synchronisation in either direction: the instance table is built on the device, `capacity` only sizes the workspace and the grids.  One
    writer per gradient element: bitwise reproducible.  More foreground anchors than capacity: NaN losses and zero gradients."""

    @staticmethod
    def forward(ctx, mask_feats, up_masks, params, fpn_levels, masks, fg, matched, xs, ys, st, up_rate, capacity):
        B, H8, W8, _ = mask_feats.shape
        A, M, r, cap = params.shape[1], masks.shape[1], int(up_rate), int(capacity)
        dev, dt = params.device, params.dtype
        fn, fwd = _entry("uni_head_mask_loss_fwd", dt)
        out = torch.empty((1 + B,), device=dev, dtype=dt)
        sums = torch.empty((cap, 3), device=dev, dtype=dt)
        with torch.cuda.device(dev):
            ws = _hm_ws(dev, dt, B, A, H8, W8, r, cap)
            L.check(fn(L.ptr(mask_feats), L.ptr(up_masks), L.ptr(params), params.stride(1), L.ptr(fpn_levels), L.ptr(masks), M, L.ptr(fg),
                       L.ptr(matched), L.ptr(xs), L.ptr(ys), L.ptr(st), B, A, H8, W8, r, cap, L.ptr(out), L.ptr(sums), L.ptr(ws), ws.numel(),
                       L.stream_ptr()), fwd)
        ctx.save_for_backward(mask_feats, up_masks, params, fpn_levels, masks, fg, matched, xs, ys, st, sums)
        ctx.up_rate, ctx.capacity = r, cap
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        mf, um, p, lvl, masks, fg, matched, xs, ys, st, sums = ctx.saved_tensors
        B, H8, W8, _ = mf.shape
        A, M, r, cap = p.shape[1], masks.shape[1], ctx.up_rate, ctx.capacity
        fn, bwd = _entry("uni_head_mask_loss_bwd", p.dtype)
        # all three are written completely by the call
        gmf = torch.empty_like(mf) if ctx.needs_input_grad[0] else None
        gum = torch.empty_like(um) if ctx.needs_input_grad[1] else None
        gp = torch.empty((B, A, 169), device=p.device, dtype=p.dtype) if ctx.needs_input_grad[2] else None
        if gmf is not None or gum is not None or gp is not None:
            g = grad_out[:1].contiguous()                    # the per-image losses are returned detached
            with torch.cuda.device(p.device):
                ws = _hm_ws(p.device, p.dtype, B, A, H8, W8, r, cap)
                L.check(fn(L.ptr(mf), L.ptr(um), L.ptr(p), p.stride(1), L.ptr(lvl), L.ptr(masks), M, L.ptr(fg), L.ptr(matched), L.ptr(xs), L.ptr(ys),
                           L.ptr(st), B, A, H8, W8, r, cap, L.ptr(sums), L.ptr(g), L.ptr(gmf), L.ptr(gum), L.ptr(gp), 169, L.ptr(ws), ws.numel(),
                           L.stream_ptr()), bwd)
        return (gmf, gum, gp) + (None,) * 9


def head_mask_loss(mask_feats, up_masks, dynamic_params, fpn_levels, masks, assignment, x_shifts, y_shifts, expanded_strides, up_rate,
                   capacity=None):
    """The CondInst lines of get_losses (unicorn_head_mask.py:568-569, :675-694, :731-732) for the WHOLE batch without a host
    synchronisation, fed by what simota_assign_batch / head_det_loss leave on the device: mask_feats (B, 8, H8, W8), up_masks
    (B, 9 r r, H8, W8), dynamic_params (B, A, 169) (a view of wider rows is read in place), fpn_levels (B, A) integer, masks
    (B, M, r H8, r W8) floating 0 / 1 maps read in place through matched_gt_inds (no per-instance copy), assignment = (fg_masks,
    matched_gt_inds, matched_ious, num_fgs), x_shifts / y_shifts / expanded_strides (1, A) or (A,).  All floating tensors fp32, or all fp64.
    -> (loss_condinst, per_image): loss_condinst = sum_b loss_mask[b] / max(number of images with foreground, 1), differentiable in
    mask_feats, up_masks and dynamic_params (dense gradients; background rows and images without foreground get exact zeros); per_image =
    the detached (B,) loss_mask.  `masks is None` is the caller's business (no call, loss 0).
    capacity: the number of instance slots the workspace (O(capacity H8 W8), include/unicorn_hip.h) and the grids are sized for; default
    B * min(A, 10 M), which SimOTA cannot exceed.  A caller who knows the data passes less.  More foreground anchors than capacity: both
    results are NaN and the gradients zero -- visible in the logged loss, never a silent truncation, and no read-back to raise."""
    names = ("mask_feats", "up_masks", "dynamic_params", "masks", "x_shifts", "y_shifts", "expanded_strides", "fpn_levels")
    ts = (mask_feats, up_masks, dynamic_params, masks, x_shifts, y_shifts, expanded_strides, fpn_levels)
    for n, t in zip(names, ts):
        if not isinstance(t, torch.Tensor):
            raise L.UnicornHipError("head_mask_loss: %s is not a tensor" % n)
    if not isinstance(assignment, (tuple, list)) or len(assignment) != 4 or not all(isinstance(t, torch.Tensor) for t in assignment):
        raise L.UnicornHipError("head_mask_loss: assignment is not the (fg_masks, matched_gt_inds, matched_ious, num_fgs) tuple of "
                                "simota_assign_batch / head_det_loss")
    fg, matched = assignment[0], assignment[1]
    r = int(up_rate)
    if mask_feats.dim() != 4 or mask_feats.shape[1] != 8 or dynamic_params.dim() != 3 or dynamic_params.shape[2] != 169 or r < 1 or r > 16 \
            or dynamic_params.shape[0] != mask_feats.shape[0] or tuple(up_masks.shape) != (mask_feats.shape[0], 9 * r * r) + tuple(mask_feats.shape[2:]):
        raise L.UnicornHipError("head_mask_loss: shapes %s, up_rate %r do not fit mask_feats (B,8,H8,W8), up_masks (B,9 r r,H8,W8), "
                                "dynamic_params (B,A,169), up_rate 1..16" % ([tuple(t.shape) for t in ts[:3]], up_rate))
    B, _, H8, W8 = mask_feats.shape
    A = dynamic_params.shape[1]
    if masks.dim() != 4 or masks.shape[0] != B or tuple(masks.shape[2:]) != (r * H8, r * W8):
        raise L.UnicornHipError("head_mask_loss: masks %s do not fit (B, M, r H8, r W8) = (%d, M, %d, %d): the ground truth must be exactly "
                                "up_rate x the feature map" % (tuple(masks.shape), B, r * H8, r * W8))
    if tuple(fpn_levels.shape) != (B, A) or tuple(fg.shape) != (B, A) or tuple(matched.shape) != (B, A):
        raise L.UnicornHipError("head_mask_loss: fpn_levels %s, fg_masks %s, matched_gt_inds %s do not fit (B, A) = (%d, %d)"
                                % (tuple(fpn_levels.shape), tuple(fg.shape), tuple(matched.shape), B, A))
    dt = dynamic_params.dtype
    if dt not in _F64_SFX or any(t.dtype != dt for t in ts[:7]):
        raise L.UnicornHipError("head_mask_loss: dtypes %s unsupported (all fp32 or all fp64; no fp16 / bf16)" % [str(t.dtype) for t in ts[:7]])
    if fpn_levels.dtype.is_floating_point or fpn_levels.dtype == torch.bool or matched.dtype.is_floating_point or matched.dtype == torch.bool \
            or fg.dtype.is_floating_point:
        raise L.UnicornHipError("head_mask_loss: fpn_levels %s / matched_gt_inds %s must be integer tensors and fg_masks %s bool or integer"
                                % (fpn_levels.dtype, matched.dtype, fg.dtype))
    try:
        xs, ys, st = (_simota_1d(n, t, A) for n, t in zip(names[4:7], ts[4:7]))
    except ValueError as e:
        raise L.UnicornHipError(str(e).replace("simota_assign", "head_mask_loss"))
    M = masks.shape[1]
    if capacity is None:
        cap = max(B * min(A, 10 * M), 1)
    else:
        cap = int(capacity)
        if cap < 1:
            raise L.UnicornHipError("head_mask_loss: capacity %r must be a positive number of instance slots" % (capacity,))
    _need_cuda(*ts, fg, matched)
    if len({t.device for t in ts + (fg, matched)}) != 1:
        raise L.UnicornHipError("head_mask_loss: tensors on different devices")
    if B == 0 or A == 0:
        zero = (mask_feats.sum() + up_masks.sum() + dynamic_params.sum()) * 0.0
        return zero, dynamic_params.new_zeros((B,))
    if H8 == 0 or W8 == 0 or M == 0:
        raise L.UnicornHipError("head_mask_loss: empty feature map or no ground-truth rows, mask_feats %s, masks %s"
                                % (tuple(mask_feats.shape), tuple(masks.shape)))
    mf = mask_feats.permute(0, 2, 3, 1).contiguous()
    um = up_masks.permute(0, 2, 3, 1).contiguous()
    p = dynamic_params if dynamic_params.stride(2) == 1 and dynamic_params.stride(1) >= 169 \
        and dynamic_params.stride(0) == A * dynamic_params.stride(1) else dynamic_params.contiguous()      # a row pitch (ldp) is passed through
    out = HeadMaskLossFunction.apply(mf, um, p, fpn_levels.to(torch.int32).contiguous(), masks.detach().contiguous(),
                                     fg.to(torch.uint8).contiguous(), matched.to(torch.int32).contiguous(), xs.detach().contiguous(),
                                     ys.detach().contiguous(), st.detach().contiguous(), r, cap)
    return out[0], out[1:].detach()


def _mc_strides(t):
    return (C.c_int64 * 4)(*t.stride())


def _mc_ws(dev, dtype, B, M, Cc):
    need = L.lib().uni_mot_corr_workspace_bytes(B, M, Cc)
    if need == 0:
        raise L.UnicornHipError("mot_corr_loss: shape B=%d M=%d C=%d is outside the limits of uni_mot_corr_loss_fwd (include/unicorn_hip.h)"
                                % (B, M, Cc))
    return torch.empty(need * _ws_factor(dtype), device=dev, dtype=torch.uint8)


class MotCorrLossFunction(torch.autograd.Function):
    """The MOT instance-contrastive loss per sample (unicorn.py:407-466), differentiable in the two embedding maps:
    apply(embed_0 (B,C,H,W), embed_1 (B,C,H,W), targets (B,2,M,6) fp32 contiguous, s, flags) -> loss (B,); fp32 or fp64 device maps of any
    strides (mot_corr_loss checks).  Saves the inputs only; the backward recomputes.  No host synchronisation in either direction; one writer
    per gradient element: bitwise reproducible.  B == 0 or M == 0: no library call (NaN losses, zero gradients)."""

    @staticmethod
    def forward(ctx, embed_0, embed_1, targets, s, flags):
        B, Cc, H, W = embed_0.shape
        M = targets.shape[2]
        ctx.save_for_backward(embed_0, embed_1, targets)
        ctx.s, ctx.flags = float(s), int(flags)
        loss = torch.empty((B,), device=embed_0.device, dtype=embed_0.dtype)
        if B == 0 or M == 0:
            return loss.fill_(float("nan"))
        fn, fwd = _entry("uni_mot_corr_loss_fwd", embed_0.dtype)
        with torch.cuda.device(embed_0.device):
            ws = _mc_ws(embed_0.device, embed_0.dtype, B, M, Cc)
            L.check(fn(L.ptr(embed_0), _mc_strides(embed_0), L.ptr(embed_1), _mc_strides(embed_1), L.ptr(targets), B, Cc, H, W, M, ctx.s, ctx.flags,
                       L.ptr(loss), L.ptr(ws), ws.numel(), L.stream_ptr()), fwd)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        e0, e1, targets = ctx.saved_tensors
        B, Cc, H, W = e0.shape
        M = targets.shape[2]
        if B == 0 or M == 0:
            return (torch.zeros_like(e0) if ctx.needs_input_grad[0] else None, torch.zeros_like(e1) if ctx.needs_input_grad[1] else None, None,
                    None, None)
        # empty_like: a dense tensor in the map's own dimension order (NCHW, channels-last); the call writes it completely
        g0 = torch.empty_like(e0) if ctx.needs_input_grad[0] else None
        g1 = torch.empty_like(e1) if ctx.needs_input_grad[1] else None
        if g0 is not None or g1 is not None:
            fn, bwd = _entry("uni_mot_corr_loss_bwd", e0.dtype)
            g = grad_loss.contiguous()
            with torch.cuda.device(e0.device):
                ws = _mc_ws(e0.device, e0.dtype, B, M, Cc)
                L.check(fn(L.ptr(e0), _mc_strides(e0), L.ptr(e1), _mc_strides(e1), L.ptr(targets), L.ptr(g), B, Cc, H, W, M, ctx.s, ctx.flags,
                           L.ptr(g0), None if g0 is None else _mc_strides(g0), L.ptr(g1), None if g1 is None else _mc_strides(g1), L.ptr(ws),
                           ws.numel(), L.stream_ptr()), bwd)
        return g0, g1, None, None, None


def mot_corr_loss(embed_0, embed_1, targets, s=8, bidirect=True, grid_sample=True):
    """Unicorn.compute_loss_mot_corr (unicorn.py:407-466) for the whole batch in one call without a host synchronisation:
    embed_0, embed_1 (B, C, H_d, W_d) fp32 (or both fp64), NCHW or channels-last memory, read in place; targets (B, 2, M, 6) rows
    [cls, cx, cy, w, h, trackid], converted with .float() as the reference does -> the (B,) per-sample losses; the reference's value is
    `.mean()` of it.  Equal in value and in gradient (embed_0, embed_1) to the reference's loop, with its quirks: the first n rows of a frame
    are its instances (n = number of non-zero ids), a repeated id keeps the reference's overwrite order, the align_corners=True style grid is
    sampled with align_corners=False.  A sample without a matched pair gives NaN and a zero gradient like the reference; so does a sample
    without instances, where the reference raises.  fp16 / bf16 maps are refused: the reference computes them under autocast(enabled=False)."""
    for n, t in (("embed_0", embed_0), ("embed_1", embed_1), ("targets", targets)):
        if not isinstance(t, torch.Tensor):
            raise L.UnicornHipError("mot_corr_loss: %s is not a tensor" % n)
    if embed_0.dim() != 4 or embed_1.shape != embed_0.shape or targets.dim() != 4 or targets.shape[0] != embed_0.shape[0] \
            or targets.shape[1] != 2 or targets.shape[3] != 6:
        raise L.UnicornHipError("mot_corr_loss: shapes %s, %s, %s do not fit embed_0 (B,C,H,W), embed_1 (B,C,H,W), targets (B,2,M,6)"
                                % (tuple(embed_0.shape), tuple(embed_1.shape), tuple(targets.shape)))
    if embed_0.dtype not in _F64_SFX or embed_1.dtype != embed_0.dtype:
        raise L.UnicornHipError("mot_corr_loss: embedding dtypes %s / %s unsupported (both fp32 or both fp64; no fp16 / autocast input: the "
                                "reference computes the embeddings under autocast(enabled=False))" % (embed_0.dtype, embed_1.dtype))
    _need_cuda(embed_0, embed_1, targets)
    if len({t.device for t in (embed_0, embed_1, targets)}) != 1:
        raise L.UnicornHipError("mot_corr_loss: tensors on different devices")
    B, Cc, H, W = embed_0.shape
    M = targets.shape[2]
    if not float(s) > 0:
        raise L.UnicornHipError("mot_corr_loss: stride s = %r is not positive" % (s,))
    if B and M and (B > 65535 or H == 0 or W == 0 or not 1 <= Cc <= 1024 or M > 1024 or Cc * H * W >= 1 << 31):
        raise L.UnicornHipError("mot_corr_loss: shape B=%d C=%d H=%d W=%d M=%d is outside B <= 65535, 1 <= C <= 1024, M <= 1024, a non-empty map "
                                "with C H W < 2^31" % (B, Cc, H, W, M))
    flags = (1 if bidirect else 0) | (2 if grid_sample else 0)
    return MotCorrLossFunction.apply(embed_0, embed_1, targets.detach().float().contiguous(), float(s), flags)


# ---- what the three ConvNeXt training operators (dwconv7_ln, block_tail, layernorm_cf) share: their argument checks, in the order each calls them
TRAIN_MAX_C = 2048
DWLN_MAX_C = TRAIN_MAX_C          # the earlier name
_STORE_DTYPE = {torch.float32: 0, torch.float64: 0, torch.float16: 1, torch.bfloat16: 2}     # the y_dtype / x_dtype argument of the library


def _check_tensors(op, names, ts, optional=()):
    """every argument is a tensor; those named in `optional` may be None"""
    for n, t in zip(names, ts):
        if not isinstance(t, torch.Tensor) and (t is not None or n not in optional):
            raise L.UnicornHipError("%s: %s is not a tensor%s" % (op, n, " or None" if n in optional else ""))


def _check_map_dims(op, name, t):
    """-> N, C, H, W of the map `t`"""
    if t.dim() != 4:
        raise L.UnicornHipError("%s: %s of shape %s is not (N, C, H, W)" % (op, name, tuple(t.shape)))
    return t.shape


def _check_channel_vecs(op, names, ts, Cc):
    for n, t in zip(names, ts):
        if tuple(t.shape) != (Cc,):
            raise L.UnicornHipError("%s: %s of shape %s is not (%d,)" % (op, n, tuple(t.shape), Cc))


def _check_train_shape(op, N, Cc, H, W):
    if Cc % 4 or not 4 <= Cc <= TRAIN_MAX_C:
        raise L.UnicornHipError("%s: C = %d is outside C %% 4 == 0, 4 <= C <= %d" % (op, Cc, TRAIN_MAX_C))
    if N and (H == 0 or W == 0 or N * H * W >= 1 << 31):
        raise L.UnicornHipError("%s: shape N=%d H=%d W=%d is outside a non-empty map with N H W < 2^31" % (op, N, H, W))


def _check_eps(op, eps):
    if not float(eps) > 0:
        raise L.UnicornHipError("%s: eps = %r is not positive" % (op, eps))


def _check_one_device(op, ts):
    _need_cuda(*ts)
    if len({t.device for t in ts}) != 1:
        raise L.UnicornHipError("%s: tensors on different devices" % op)


def _train_ws(op, entry_name, dev, dtype, N, H, W, Cc):
    """the backward workspace that the library function `entry_name` (uni_*_workspace_bytes) sizes: uninitialised bytes on `dev`"""
    need = getattr(L.lib(), entry_name)(N, H, W, Cc)
    if need == 0:
        raise L.UnicornHipError("%s: shape N=%d C=%d H=%d W=%d is outside the limits of %s (include/unicorn_hip.h)"
                                % (op, N, Cc, H, W, entry_name.replace("workspace_bytes", "bwd")))
    return torch.empty(need * _ws_factor(dtype), device=dev, dtype=torch.uint8)


def _map_layout(t):
    """-> (t or a channels-last copy of it, nchw flag): NCHW-contiguous and channels-last memory are read in place"""
    if t.is_contiguous(memory_format=torch.channels_last):
        return t, 0
    if t.is_contiguous():
        return t, 1
    return t.contiguous(memory_format=torch.channels_last), 0


class DwConv7LNFunction(torch.autograd.Function):
    """The opening of a ConvNeXt block (convnext.py:43-45), differentiable in all five tensors:
    apply(x (N,C,H,W), weight (C,1,7,7), bias, ln_weight, ln_bias (C,), eps) -> y (N,H,W,C) contiguous; device tensors, all fp32 or all fp64
    (dwconv7_ln checks).  Channels-last memory of x is read in place, any other layout is converted once; grad_x is channels-last.  Saves x, the
    four parameters and the (N H W, 2) statistics; neither y nor the convolution output.  The backward recomputes the convolution and writes only
    the gradients autograd asks for.  No host synchronisation in either direction, one writer per gradient element: bitwise reproducible.
    Under autocast the inputs are cast to fp32 and y is fp32, as F.layer_norm's result is there; grad_x then has the dtype of x."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, weight, bias, ln_weight, ln_bias, eps):
        N, Cc, H, W = x.shape
        ctx.dims = (N, Cc, H, W)
        y = torch.empty((N, H, W, Cc), device=x.device, dtype=x.dtype)
        if N == 0:
            ctx.save_for_backward(x, weight, bias, ln_weight, ln_bias)
            return y
        xc = x.contiguous(memory_format=torch.channels_last)
        wt = weight.reshape(Cc, 49).t().contiguous()                      # [49][C], the layout of uni_dwconv7_ln_ex
        stats = torch.empty((N * H * W, 2), device=x.device, dtype=x.dtype)
        fn, name = _entry("uni_dwln_train_fwd", x.dtype)
        with torch.cuda.device(x.device):
            L.check(fn(L.ptr(xc), L.ptr(wt), L.ptr(bias.contiguous()), L.ptr(ln_weight.contiguous()), L.ptr(ln_bias.contiguous()), float(eps),
                       N, H, W, Cc, L.ptr(y), L.ptr(stats), L.stream_ptr()), name)
        ctx.save_for_backward(xc, weight, bias, ln_weight, ln_bias, stats)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y):
        N, Cc, H, W = ctx.dims
        need = ctx.needs_input_grad
        need_x, need_w, need_g = need[0], need[1] or need[2], need[3] or need[4]
        if N == 0:
            x, weight, bias, ln_weight, ln_bias = ctx.saved_tensors
            z = torch.zeros_like
            return (z(x) if need[0] else None, z(weight) if need[1] else None, z(bias) if need[2] else None, z(ln_weight) if need[3] else None,
                    z(ln_bias) if need[4] else None, None)
        xc, weight, bias, ln_weight, ln_bias, stats = ctx.saved_tensors
        gx = torch.empty_like(xc) if need_x else None                     # channels-last like xc; the call writes it completely
        gwt = torch.empty((49, Cc), device=xc.device, dtype=xc.dtype) if need_w else None
        gb = torch.empty_like(bias, memory_format=torch.contiguous_format) if need_w else None
        gg = torch.empty_like(ln_weight, memory_format=torch.contiguous_format) if need_g else None
        gbe = torch.empty_like(ln_bias, memory_format=torch.contiguous_format) if need_g else None
        if need_x or need_w or need_g:
            fn, name = _entry("uni_dwln_train_bwd", xc.dtype)
            g = grad_y.contiguous()
            wt = weight.reshape(Cc, 49).t().contiguous()
            with torch.cuda.device(xc.device):
                ws = _train_ws("dwconv7_ln", "uni_dwln_train_workspace_bytes", xc.device, xc.dtype, N, H, W, Cc)
                L.check(fn(L.ptr(xc), L.ptr(wt), L.ptr(bias.contiguous()), L.ptr(ln_weight.contiguous()), L.ptr(stats), L.ptr(g), N, H, W, Cc,
                           L.ptr(gx), L.ptr(gwt), L.ptr(gb), L.ptr(gg), L.ptr(gbe), L.ptr(ws), ws.numel(), L.stream_ptr()), name)
        gw = gwt.t().reshape(Cc, 1, 7, 7).contiguous() if need[1] else None
        return gx, gw, gb if need[2] else None, gg if need[3] else None, gbe if need[4] else None, None


def dwconv7_ln(x, weight, bias, ln_weight, ln_bias, eps=1e-6):
    """`norm(dwconv(x).permute(0, 2, 3, 1))` of a ConvNeXt block (convnext.py:32-33,43-45) as one operator, equal in value and in all five
    gradients: x (N, C, H, W), weight (C, 1, 7, 7) and bias (C,) of the depthwise Conv2d(C, C, 7, padding=3, groups=C), ln_weight / ln_bias
    (C,) and eps of the channels-last LayerNorm -> y (N, H, W, C), contiguous.  All tensors fp32, or all fp64 for checks; under
    torch.autocast("cuda") they are cast to fp32 and y is fp32 (what F.layer_norm returns there), x.grad keeps the dtype of x.  x in
    channels-last memory is read in place; any other layout (NCHW-contiguous included) is converted ONCE with
    .contiguous(memory_format=torch.channels_last), and x.grad comes back channels-last.  C % 4 == 0, 4 <= C <= 2048.  Autograd keeps x, the
    parameters and two numbers per pixel; neither y nor the convolution output.  N == 0 returns an empty tensor without a library call."""
    names = ("x", "weight", "bias", "ln_weight", "ln_bias")
    ts = (x, weight, bias, ln_weight, ln_bias)
    _check_tensors("dwconv7_ln", names, ts)
    N, Cc, H, W = _check_map_dims("dwconv7_ln", "x", x)
    if tuple(weight.shape) != (Cc, 1, 7, 7):
        raise L.UnicornHipError("dwconv7_ln: weight of shape %s is not the depthwise 7x7 weight (%d, 1, 7, 7) of x's %d channels"
                                % (tuple(weight.shape), Cc, Cc))
    _check_channel_vecs("dwconv7_ln", names[2:], ts[2:], Cc)
    _check_train_shape("dwconv7_ln", N, Cc, H, W)
    _check_eps("dwconv7_ln", eps)
    autocast = x.is_cuda and torch.is_autocast_enabled("cuda")
    if autocast:
        if not all(t.is_floating_point() for t in ts):
            raise L.UnicornHipError("dwconv7_ln: dtypes %s: floating-point tensors are needed" % ", ".join(str(t.dtype) for t in ts))
    elif x.dtype not in _F64_SFX or any(t.dtype != x.dtype for t in ts):
        raise L.UnicornHipError("dwconv7_ln: dtypes %s unsupported (all fp32 or all fp64; half inputs only under torch.autocast)"
                                % ", ".join(str(t.dtype) for t in ts))
    _check_one_device("dwconv7_ln", ts)
    return DwConv7LNFunction.apply(x, weight, bias, ln_weight, ln_bias, float(eps))


class BlockTailFunction(torch.autograd.Function):
    """The close of a ConvNeXt block (convnext.py:49-53): apply(y (N,H,W,C) contiguous, residual (N,C,H,W), gamma (C,) or None, scale (N,) or
    None) -> out (N,C,H,W) in channels-last memory, in the dtype of residual (fp32 / fp64; ops.block_tail checks).  y may be fp16 / bf16 next
    to an fp32 residual.  residual and grad_out are read in place in NCHW-contiguous or channels-last memory, anything else is converted once.
    Saves y, gamma and scale, never out.  The gradient of residual is grad_out itself, that of y a contiguous (N,H,W,C) tensor of y's dtype,
    that of gamma (C,); only what autograd asks for is computed.  No host synchronisation, one writer per element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, y, residual, gamma, scale):
        N, Cc, H, W = residual.shape
        ctx.dims = (N, Cc, H, W)
        ctx.save_for_backward(y, gamma, scale)
        out = torch.empty((N, Cc, H, W), device=residual.device, dtype=residual.dtype, memory_format=torch.channels_last)
        if N == 0:
            return out
        res, nchw = _map_layout(residual)
        fn, name = _entry("uni_block_tail_fwd", residual.dtype)
        with torch.cuda.device(residual.device):
            L.check(fn(L.ptr(y), _STORE_DTYPE[y.dtype], L.ptr(res), nchw, L.ptr(gamma), L.ptr(scale), N, H, W, Cc, L.ptr(out), L.stream_ptr()), name)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        N, Cc, H, W = ctx.dims
        y, gamma, scale = ctx.saved_tensors
        need_y, need_res, need_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and gamma is not None
        gy = torch.empty_like(y) if need_y else None
        gg = torch.empty_like(gamma) if need_g else None
        if N == 0:
            return gy, grad_out if need_res else None, gg.zero_() if need_g else None, None
        if need_y or need_g:
            g, nchw = _map_layout(grad_out)
            fn, name = _entry("uni_block_tail_bwd", g.dtype)
            with torch.cuda.device(g.device):
                ws = _train_ws("block_tail", "uni_block_tail_workspace_bytes", g.device, g.dtype, N, H, W, Cc) if need_g else None
                L.check(fn(L.ptr(y), _STORE_DTYPE[y.dtype], L.ptr(g), nchw, L.ptr(gamma), L.ptr(scale), N, H, W, Cc, L.ptr(gy), L.ptr(gg),
                           L.ptr(ws), ws.numel() if need_g else 0, L.stream_ptr()), name)
        return gy, grad_out if need_res else None, gg, None


def block_tail(y, residual, gamma=None, scale=None):
    """`input + drop_path((gamma * x).permute(0, 3, 1, 2))` of a ConvNeXt block (convnext.py:49-53) as one operator with the drop-path factor
    given per sample: out[n, c, h, w] = residual[n, c, h, w] + scale[n] * gamma[c] * y[n, h, w, c].
      y         (N, H, W, C), the output of pwconv2: fp32, or fp16 / bf16 (what pwconv2 returns under autocast); made contiguous if it is not
      residual  (N, C, H, W) fp32; a half residual is cast with .float(), as type promotion does in the eager lines.  NCHW-contiguous and
                channels-last memory are read in place, any other strides are converted once to channels-last
      gamma     (C,) fp32 or None (= 1)
      scale     (N,) or (N, 1, 1, 1) fp32 without gradient, or None (= 1): 0 or 1 / keep of the sample
    All four fp64 is accepted for checks.  Returns out (N, C, H, W) fp32 (fp64) with out.is_contiguous(memory_format=torch.channels_last).
    Gradients: residual receives grad_out itself (no copy), y a contiguous (N, H, W, C) tensor of its own dtype, gamma (C,); grad_out is read in
    place in either of the two layouts.  Autograd keeps y, gamma and scale, never out.  C % 4 == 0, 4 <= C <= 2048.  The one deliberate
    difference to the eager lines: a sample with scale 0 is not read, so its grad_y is 0 and it adds 0 to grad_gamma even where y holds Inf
    or NaN (eager gives NaN).  N == 0 returns an empty tensor without a library call."""
    _check_tensors("block_tail", ("y", "residual", "gamma", "scale"), (y, residual, gamma, scale), optional=("gamma", "scale"))
    N, Cc, H, W = _check_map_dims("block_tail", "residual", residual)
    if tuple(y.shape) != (N, H, W, Cc):
        raise L.UnicornHipError("block_tail: y of shape %s is not (N, H, W, C) = (%d, %d, %d, %d) of residual" % (tuple(y.shape), N, H, W, Cc))
    if gamma is not None:
        _check_channel_vecs("block_tail", ("gamma",), (gamma,), Cc)
    if scale is not None and tuple(scale.shape) not in ((N,), (N, 1, 1, 1)):
        raise L.UnicornHipError("block_tail: scale of shape %s is not (%d,) or (%d, 1, 1, 1)" % (tuple(scale.shape), N, N))
    _check_train_shape("block_tail", N, Cc, H, W)
    if scale is not None and scale.requires_grad:
        raise L.UnicornHipError("block_tail: scale requires a gradient; it is a constant of the step")
    ts = [t for t in (y, residual, gamma, scale) if t is not None]
    if y.dtype == torch.float64:
        ok = all(t.dtype == torch.float64 for t in ts)
    else:
        ok = (y.dtype in _STORE_DTYPE and residual.dtype in (torch.float32, torch.float16, torch.bfloat16)
              and all(t.dtype == torch.float32 for t in (gamma, scale) if t is not None))
    if not ok:
        raise L.UnicornHipError("block_tail: dtypes %s unsupported (y fp32 / fp16 / bf16 with residual fp32 or half and gamma, scale fp32; or "
                                "all fp64)" % ", ".join(str(t.dtype) for t in ts))
    _check_one_device("block_tail", ts)
    if residual.dtype in (torch.float16, torch.bfloat16):
        residual = residual.float()
    if scale is not None:
        scale = scale.detach().reshape(N).contiguous()
    return BlockTailFunction.apply(y.contiguous(), residual, None if gamma is None else gamma.contiguous(), scale)


def _lncf_like(t, nchw, dtype):
    """an uninitialised tensor of the shape of `t` in the memory layout `nchw` names"""
    return torch.empty(t.shape, device=t.device, dtype=dtype, memory_format=torch.contiguous_format if nchw else torch.channels_last)


class LayerNormCFFunction(torch.autograd.Function):
    """The channels-first LayerNorm of the ConvNeXt backbone (convnext.py:160-184): apply(x (N,C,H,W), weight (C,), bias (C,), eps) -> y
    (N,C,H,W) in the memory layout of x; x fp32 / fp16 / bf16 with fp32 weight and bias -> y fp32, or all fp64 (ops.layernorm_cf checks).
    Channels-last and NCHW-contiguous memory of x are read in place, anything else is converted once to channels-last; grad_out is read in place
    when it has the layout of x.  Saves x, weight and the (N H W, 2) statistics, never y or the normalised map.  x.grad has the dtype and layout
    of x; only what autograd asks for is computed.  No host synchronisation, one writer per element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        N, Cc, H, W = x.shape
        ctx.dims = (N, Cc, H, W)
        out_dtype = torch.promote_types(x.dtype, weight.dtype)
        xc, nchw = _map_layout(x)
        ctx.nchw = nchw
        y = _lncf_like(xc, nchw, out_dtype)
        if N == 0:
            ctx.save_for_backward(xc, weight)
            return y
        stats = torch.empty((N * H * W, 2), device=x.device, dtype=out_dtype)
        fn, name = _entry("uni_lncf_train_fwd", out_dtype)
        with torch.cuda.device(x.device):
            L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], nchw, L.ptr(weight), L.ptr(bias), float(eps), N, H, W, Cc, L.ptr(y), L.ptr(stats),
                       L.stream_ptr()), name)
        ctx.save_for_backward(xc, weight, stats)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        N, Cc, H, W = ctx.dims
        nchw = ctx.nchw
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        xc, weight = ctx.saved_tensors[:2]
        gx = _lncf_like(xc, nchw, xc.dtype) if need_x else None
        gw = torch.empty_like(weight) if need_p else None
        gb = torch.empty_like(weight) if need_p else None
        if N == 0:
            if need_p:
                gw.zero_(), gb.zero_()
        elif need_x or need_p:
            stats = ctx.saved_tensors[2]
            g = grad_out.contiguous() if nchw else grad_out.contiguous(memory_format=torch.channels_last)       # no copy in the layout of x
            fn, name = _entry("uni_lncf_train_bwd", weight.dtype)
            with torch.cuda.device(xc.device):
                ws = _train_ws("layernorm_cf", "uni_lncf_train_workspace_bytes", xc.device, weight.dtype, N, H, W, Cc) if need_p else None
                L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], nchw, L.ptr(weight), L.ptr(stats), L.ptr(g), N, H, W, Cc, L.ptr(gx), L.ptr(gw),
                           L.ptr(gb), L.ptr(ws), ws.numel() if need_p else 0, L.stream_ptr()), name)
        return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None


def layernorm_cf(x, weight, bias, eps=1e-6):
    """The reference's LayerNorm(C, data_format="channels_first") (convnext.py:160-184) as one operator, equal in value and in all three
    gradients: y[n, c, h, w] = weight[c] * (x[n, c, h, w] - u) / sqrt(s + eps) + bias[c] with u and s the mean and the biased variance over
    the C channels of the pixel.
      x             (N, C, H, W) fp32, fp16 or bf16; read in the dtype it has (no cast under autocast).  Channels-last memory (what
                    ops.block_tail returns) and NCHW-contiguous memory (what a convolution returns) are read in place, any other strides are
                    converted once to channels-last
      weight, bias  (C,) fp32
    All three fp64 is accepted for checks.  Returns y of the shape of x in the MEMORY LAYOUT of x (of its channels-last copy for other
    strides), dtype torch.promote_types(x.dtype, weight.dtype): fp32 (fp64), what the eager lines return with or without autocast.
    Gradients: x.grad in the dtype and layout of x, weight.grad and bias.grad (C,); grad_out is read in place when it has the layout of x,
    otherwise it is converted once.  Autograd keeps x, weight and two numbers per pixel, neither y nor the normalised map.
    C % 4 == 0, 4 <= C <= 2048.  N == 0 returns an empty tensor without a library call."""
    names = ("x", "weight", "bias")
    ts = (x, weight, bias)
    _check_tensors("layernorm_cf", names, ts)
    N, Cc, H, W = _check_map_dims("layernorm_cf", "x", x)
    _check_channel_vecs("layernorm_cf", names[1:], ts[1:], Cc)
    _check_train_shape("layernorm_cf", N, Cc, H, W)
    _check_eps("layernorm_cf", eps)
    if x.dtype == torch.float64:
        ok = weight.dtype == bias.dtype == torch.float64
    else:
        ok = x.dtype in _STORE_DTYPE and weight.dtype == bias.dtype == torch.float32
    if not ok:
        raise L.UnicornHipError("layernorm_cf: dtypes %s unsupported (x fp32 / fp16 / bf16 with weight, bias fp32; or all fp64)"
                                % ", ".join(str(t.dtype) for t in ts))
    _check_one_device("layernorm_cf", ts)
    return LayerNormCFFunction.apply(x, weight.contiguous(), bias.contiguous(), float(eps))


GN_ACT = {"none": 0, "relu": 1, "silu": 3}       # the activation codes of the engine


class GroupNormActFunction(torch.autograd.Function):
    """GroupNorm followed by an activation (network_blocks.py:29-51 after convert_bn_model_to_gn): apply(x (N,C,H,W), weight (C,), bias (C,),
    num_groups, eps, act code) -> y (N,C,H,W) in the memory layout of x; x fp32 / fp16 / bf16 with fp32 weight and bias -> y fp32, or all fp64
    (ops.group_norm_act checks).  Channels-last and NCHW-contiguous memory of x are read in place, anything else is converted once to
    channels-last; grad_out is read in place when it has the layout of x.  Saves x, weight, bias and the (N G, 2) statistics, never y or a
    normalised map: the backward recomputes xhat, z and act'(z).  x.grad has the dtype and layout of x; only what autograd asks for is computed.
    No host synchronisation, one writer per element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, act):
        N, Cc, H, W = x.shape
        ctx.dims = (N, Cc, H, W, num_groups, act)
        out_dtype = torch.promote_types(x.dtype, weight.dtype)
        xc, nchw = _map_layout(x)
        ctx.nchw = nchw
        y = _lncf_like(xc, nchw, out_dtype)
        if N == 0:
            ctx.save_for_backward(xc, weight, bias)
            return y
        stats = torch.empty((N * num_groups, 2), device=x.device, dtype=out_dtype)
        fn, name = _entry("uni_gn_act_train_fwd", out_dtype)
        with torch.cuda.device(x.device):
            L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], nchw, L.ptr(weight), L.ptr(bias), float(eps), act, N, H, W, Cc, num_groups, L.ptr(y),
                       L.ptr(stats), L.stream_ptr()), name)
        ctx.save_for_backward(xc, weight, bias, stats)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        N, Cc, H, W, G, act = ctx.dims
        nchw = ctx.nchw
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        xc, weight, bias = ctx.saved_tensors[:3]
        gx = _lncf_like(xc, nchw, xc.dtype) if need_x else None
        gw = torch.empty_like(weight) if need_p else None
        gb = torch.empty_like(weight) if need_p else None
        if N == 0:
            if need_p:
                gw.zero_(), gb.zero_()
        elif need_x or need_p:
            stats = ctx.saved_tensors[3]
            g = grad_out.contiguous() if nchw else grad_out.contiguous(memory_format=torch.channels_last)       # no copy in the layout of x
            fn, name = _entry("uni_gn_act_train_bwd", weight.dtype)
            with torch.cuda.device(xc.device):
                need = L.lib().uni_gn_act_train_workspace_bytes(N, H, W, Cc, G)
                if need == 0:
                    raise L.UnicornHipError("group_norm_act: shape N=%d C=%d H=%d W=%d G=%d is outside the limits of uni_gn_act_train_bwd "
                                            "(include/unicorn_hip.h)" % (N, Cc, H, W, G))
                ws = torch.empty(need * _ws_factor(weight.dtype), device=xc.device, dtype=torch.uint8)
                L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], nchw, L.ptr(weight), L.ptr(bias), L.ptr(stats), L.ptr(g), act, N, H, W, Cc, G, L.ptr(gx),
                           L.ptr(gw), L.ptr(gb), L.ptr(ws), ws.numel(), L.stream_ptr()), name)
        return gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None, None, None


def group_norm_act(x, num_groups, weight, bias, eps=1e-5, act="silu"):
    """act(F.group_norm(x, num_groups, weight, bias, eps)) as one operator, equal in value and in all three gradients: mean and biased
    variance over the (C / num_groups) H W elements of every (sample, group), z = (x - mean) / sqrt(var + eps) * weight[c] + bias[c], y = z
    (act="none"), max(z, 0) ("relu") or z * sigmoid(z) ("silu").
      x             (N, C, H, W) fp32, fp16 or bf16; read in the dtype it has (no cast under autocast).  Channels-last memory and
                    NCHW-contiguous memory (what a convolution returns) are read in place, any other strides are converted once to channels-last
      num_groups    1 <= num_groups <= C, C % num_groups == 0; C / num_groups need not be a multiple of 4
      weight, bias  (C,) fp32
    All three fp64 is accepted for checks.  Returns y of the shape of x in the MEMORY LAYOUT of x (of its channels-last copy for other
    strides), dtype torch.promote_types(x.dtype, weight.dtype): fp32 (fp64), what the eager lines return with or without autocast.
    Gradients: x.grad in the dtype and layout of x, weight.grad and bias.grad (C,); grad_out is read in place when it has the layout of x,
    otherwise it is converted once.  Autograd keeps x, weight, bias and two numbers per (sample, group), neither y nor a normalised map.
    C % 4 == 0, 4 <= C <= 2048.  N == 0 returns an empty tensor without a library call."""
    names = ("x", "weight", "bias")
    ts = (x, weight, bias)
    _check_tensors("group_norm_act", names, ts)
    N, Cc, H, W = _check_map_dims("group_norm_act", "x", x)
    _check_channel_vecs("group_norm_act", names[1:], ts[1:], Cc)
    _check_train_shape("group_norm_act", N, Cc, H, W)
    if isinstance(num_groups, bool) or not isinstance(num_groups, int) or not 1 <= num_groups <= Cc or Cc % num_groups:
        raise L.UnicornHipError("group_norm_act: num_groups = %r is not an integer in [1, C] that divides C = %d" % (num_groups, Cc))
    _check_eps("group_norm_act", eps)
    if act not in GN_ACT:
        raise L.UnicornHipError("group_norm_act: act = %r is not one of %s" % (act, ", ".join(repr(k) for k in GN_ACT)))
    if x.dtype == torch.float64:
        ok = weight.dtype == bias.dtype == torch.float64
    else:
        ok = x.dtype in _STORE_DTYPE and weight.dtype == bias.dtype == torch.float32
    if not ok:
        raise L.UnicornHipError("group_norm_act: dtypes %s unsupported (x fp32 / fp16 / bf16 with weight, bias fp32; or all fp64)"
                                % ", ".join(str(t.dtype) for t in ts))
    _check_one_device("group_norm_act", ts)
    return GroupNormActFunction.apply(x, weight.contiguous(), bias.contiguous(), num_groups, float(eps), GN_ACT[act])


PW_MLP_MAX_H = 4 * TRAIN_MAX_C
PW_MLP_KEEP = ("hidden", "input")


def _pw_sum_dtype(cd):
    """the dtype of the bias sums, which names the library form: fp64 for fp64 maps, fp32 for fp32 and half maps"""
    return torch.float64 if cd == torch.float64 else torch.float32


def _pw_act_bwd(dev, cd, M, Hd, Co, h, grad_a, a, grad_h, grad_b1, grad_y, grad_b2):
    """uni_pw_mlp_act_bwd on (M, Hd) / (M, Co) maps of the dtype `cd` on the current device `dev`; every tensor may be None"""
    fn, name = _entry("uni_pw_mlp_act_bwd", _pw_sum_dtype(cd))
    ws, nws = None, 0
    if grad_b1 is not None or grad_b2 is not None:
        nws = L.lib().uni_pw_mlp_workspace_bytes(M, Hd, Co) * _ws_factor(_pw_sum_dtype(cd))
        if nws == 0:
            raise L.UnicornHipError("pw_mlp: shape M=%d Hd=%d Co=%d is outside the limits of uni_pw_mlp_act_bwd (include/unicorn_hip.h)" % (M, Hd, Co))
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    L.check(fn(L.ptr(h), _STORE_DTYPE[cd], L.ptr(grad_a), M, Hd, L.ptr(a), L.ptr(grad_h), L.ptr(grad_b1), L.ptr(grad_y), Co, L.ptr(grad_b2),
               L.ptr(ws), nws, L.stream_ptr()), name)


class PwMlpFunction(torch.autograd.Function):
    """`pwconv2(act(pwconv1(t)))` of a ConvNeXt block (convnext.py:46-48) with the GELU in HIP and the hidden maps rebuilt in the backward:
    apply(t (..., C), w1 (Hd, C), b1 (Hd,), w2 (Co, Hd), b2 (Co,), keep) -> y (..., Co); ops.pw_mlp checks the arguments.  The two GEMMs of the
    forward are the addmm calls F.linear makes.  The compute dtype is fp64 for fp64 tensors, else fp32, and under torch.autocast("cuda") the
    autocast dtype: t and the parameters are cast to it here and autocast is switched off for the Function's own lines, so forward and
    backward use the same dtypes.
      keep == "hidden"  saves t (the cast copy under autocast), w1, w2 and h = pwconv1(t); a = gelu(h) is a temporary of the forward and is
                        rebuilt by the backward into a temporary.  h is never written.
      keep == "input"   a is written over h, nothing of M x Hd elements survives the forward; saves t, w1, b1 and w2.  The backward repeats the
                        first addmm and works in place on its own buffers.
    Only what autograd asks for is computed.  No host synchronisation, one writer per element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, t, w1, b1, w2, b2, keep):
        Hd, Cc = w1.shape
        Co = w2.shape[0]
        if torch.is_autocast_enabled("cuda"):
            cd = torch.get_autocast_dtype("cuda")
        else:
            cd = torch.float64 if t.dtype == torch.float64 else torch.float32
        M = t.numel() // Cc
        ctx.keep, ctx.cd, ctx.t_shape, ctx.t_dtype, ctx.empty = keep, cd, t.shape, t.dtype, M == 0
        if M == 0:
            ctx.save_for_backward(w1, b1, w2, b2)
            return torch.empty(t.shape[:-1] + (Co,), device=t.device, dtype=cd)
        with torch.autocast("cuda", enabled=False), torch.cuda.device(t.device):
            t2 = t.detach().reshape(M, Cc).to(cd).contiguous()
            h = torch.addmm(b1.detach().to(cd), t2, w1.detach().to(cd).t())
            a = h if keep == "input" else torch.empty_like(h)
            fn, name = _entry("uni_pw_mlp_act_fwd", _pw_sum_dtype(cd))
            L.check(fn(L.ptr(h), _STORE_DTYPE[cd], M, Hd, L.ptr(a), L.stream_ptr()), name)
            y = torch.addmm(b2.detach().to(cd), a, w2.detach().to(cd).t())
        if keep == "input":
            ctx.save_for_backward(t2, w1, b1, w2)
        else:
            ctx.save_for_backward(t2, w1, w2, h)
        ctx.b_dtypes = (b1.dtype, b2.dtype)
        return y.reshape(t.shape[:-1] + (Co,))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        need = ctx.needs_input_grad
        cd = ctx.cd
        if ctx.empty:
            w1, b1, w2, b2 = ctx.saved_tensors
            z = torch.zeros_like
            return (torch.zeros(ctx.t_shape, device=w1.device, dtype=ctx.t_dtype) if need[0] else None, z(w1) if need[1] else None,
                    z(b1) if need[2] else None, z(w2) if need[3] else None, z(b2) if need[4] else None, None)
        if ctx.keep == "input":
            t2, w1, b1, w2 = ctx.saved_tensors
            h = None
        else:
            t2, w1, w2, h = ctx.saved_tensors
        M, Hd, Co, dev = t2.shape[0], w1.shape[0], w2.shape[0], t2.device
        need_ga, need_gh = need[0] or need[1] or need[2], need[0] or need[1]
        g_t = g_w1 = g_b1 = g_w2 = g_b2 = a = ga = None
        with torch.autocast("cuda", enabled=False), torch.cuda.device(dev):
            gy = grad_y.reshape(M, Co).to(cd).contiguous()
            if need_ga or need[3]:
                if h is None:                                                # keep == "input": h again, and a over it
                    h = torch.addmm(b1.detach().to(cd), t2, w1.detach().to(cd).t())
                    a = h if need[3] else None
                elif need[3]:
                    a = torch.empty_like(h)                                  # keep == "hidden": h is a saved tensor and is not written
            else:
                h = None
            if need_ga:
                ga = torch.mm(gy, w2.detach().to(cd))
            gh = ga if need_gh else None                                     # grad_h over grad_a, a buffer of this call
            if need[2]:
                g_b1 = torch.empty(Hd, device=dev, dtype=_pw_sum_dtype(cd))
            if need[4]:
                g_b2 = torch.empty(Co, device=dev, dtype=_pw_sum_dtype(cd))
            _pw_act_bwd(dev, cd, M, Hd, Co, h, ga, a, gh, g_b1, gy if need[4] else None, g_b2)
            if need[3]:
                g_w2 = torch.mm(gy.t(), a).to(w2.dtype)
            if need[1]:
                g_w1 = torch.mm(gh.t(), t2).to(w1.dtype)
            if need[0]:
                g_t = torch.mm(gh, w1.detach().to(cd)).reshape(ctx.t_shape).to(ctx.t_dtype)
            if need[2]:
                g_b1 = g_b1.to(ctx.b_dtypes[0])
            if need[4]:
                g_b2 = g_b2.to(ctx.b_dtypes[1])
        return g_t, g_w1, g_b1, g_w2, g_b2, None


def pw_mlp(t, w1, b1, w2, b2, keep="hidden"):
    """`pwconv2(act(pwconv1(t)))` of a ConvNeXt block (convnext.py:46-48) as one operator, equal in value and in all five gradients to
    F.linear(F.gelu(F.linear(t, w1, b1)), w2, b2) (the exact erf GELU, nn.GELU()'s default):
      t        (..., C)
      w1, b1   (Hd, C), (Hd,): pwconv1;  w2, b2  (Co, Hd), (Co,): pwconv2.  Hd % 4 == 0, 4 <= Hd <= 8192, the same for Co
    All five fp32, or all fp64 for checks; under torch.autocast("cuda") any floating-point dtypes: t and the parameters are cast to the
    autocast dtype as F.linear casts them, and y is half as it is in eager.  Returns y (..., Co) in the compute dtype.  Gradients come back in
    the dtypes of their tensors.  The GEMMs are the vendor library's (the very addmm calls of F.linear, so h has eager's bits); the GELU, its
    derivative and both bias sums are HIP (uni_pw_mlp_act_fwd / _bwd).
      keep="hidden"  autograd keeps t (the half copy under autocast), w1, w2 and h: one (M, Hd) map instead of eager's two (h and gelu(h)).
                     The backward rebuilds gelu(h) in one point-wise pass.
      keep="input"   autograd keeps t, w1, b1 and w2: NO (M, Hd) map.  The backward repeats the first GEMM.
    An empty t returns an empty result (zero parameter gradients) without a library call.  No host synchronisation."""
    names = ("t", "w1", "b1", "w2", "b2")
    ts = (t, w1, b1, w2, b2)
    _check_tensors("pw_mlp", names, ts)
    if keep not in PW_MLP_KEEP:
        raise L.UnicornHipError("pw_mlp: keep = %r is not one of %s" % (keep, ", ".join(repr(k) for k in PW_MLP_KEEP)))
    if t.dim() < 1 or w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != t.shape[-1] or w2.shape[1] != w1.shape[0]:
        raise L.UnicornHipError("pw_mlp: shapes %s, %s, %s do not fit t (..., C), w1 (Hd, C), w2 (Co, Hd)"
                                % (tuple(t.shape), tuple(w1.shape), tuple(w2.shape)))
    Hd, Co = w1.shape[0], w2.shape[0]
    _check_channel_vecs("pw_mlp", ("b1",), (b1,), Hd)
    _check_channel_vecs("pw_mlp", ("b2",), (b2,), Co)
    for n, v in (("Hd", Hd), ("Co", Co)):
        if v % 4 or not 4 <= v <= PW_MLP_MAX_H:
            raise L.UnicornHipError("pw_mlp: %s = %d is outside %s %% 4 == 0, 4 <= %s <= %d" % (n, v, n, n, PW_MLP_MAX_H))
    if t.shape[-1] == 0 or t.numel() // max(t.shape[-1], 1) >= 1 << 31:
        raise L.UnicornHipError("pw_mlp: t of shape %s is outside C >= 1 with fewer than 2^31 rows" % (tuple(t.shape),))
    if t.is_cuda and torch.is_autocast_enabled("cuda"):
        if not all(x.is_floating_point() for x in ts):
            raise L.UnicornHipError("pw_mlp: dtypes %s: floating-point tensors are needed" % ", ".join(str(x.dtype) for x in ts))
    elif t.dtype not in _F64_SFX or any(x.dtype != t.dtype for x in ts):
        raise L.UnicornHipError("pw_mlp: dtypes %s unsupported (all fp32 or all fp64; half tensors only under torch.autocast)"
                                % ", ".join(str(x.dtype) for x in ts))
    _check_one_device("pw_mlp", ts)
    return PwMlpFunction.apply(t, w1, b1, w2, b2, keep)


def _patch_compute_dtype(x):
    """the compute dtype of the two downsample operators, PwMlpFunction's rule"""
    if torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def _col_sum(dev, cd, gy):
    """the column sums of gy (M, Co) in the sum dtype of `cd`: the grad_y / grad_b2 path of uni_pw_mlp_act_bwd alone, which its header allows"""
    M, Co = gy.shape
    out = torch.empty(Co, device=dev, dtype=_pw_sum_dtype(cd))
    _pw_act_bwd(dev, cd, M, Co, Co, None, None, None, None, None, gy, out)
    return out


WGRAD_ROWS = 1024


def _wgrad_mm(gy, A):
    """gy.t() @ A for gy (M, Co), A (M, K): the weight gradient of a patch convolution, a sum over the M output pixels.  One mm adds
    the M terms of an element in fp32 in the order the vendor kernel takes them, and at training maps (M of 10^4 .. 10^5) its error is
    several times that of the eager convolution's weight gradient.  So fp32 maps of at least 2 WGRAD_ROWS rows are multiplied in slices of
    WGRAD_ROWS rows by ONE bmm, and the slices (and the mm of the rows left over) are added in ascending order in fp64: a fixed order, the
    error of a 1024-term sum.  Half maps keep the single mm (fp32 accumulation, one rounding), fp64 maps too."""
    M = gy.shape[0]
    S = M // WGRAD_ROWS
    if gy.dtype != torch.float32 or S < 2:
        return torch.mm(gy.t(), A)
    head = S * WGRAD_ROWS
    part = torch.bmm(gy[:head].view(S, WGRAD_ROWS, -1).transpose(1, 2), A[:head].view(S, WGRAD_ROWS, -1))
    out = part.sum(0, dtype=torch.float64)
    if head < M:
        out += torch.mm(gy[head:].t(), A[head:])
    return out.to(torch.float32)


class DownsampleLNFunction(torch.autograd.Function):
    """A downsample layer of the ConvNeXt backbone (convnext.py:83-87: channels-first LayerNorm, then Conv2d(C, Co, 2, stride=2)):
    apply(x (N,C,H,W), ln_weight (C,), ln_bias (C,), weight (Co,C,2,2), bias (Co,), eps) -> y (N,Co,H//2,W//2) in channels-last memory, in the
    compute dtype; ops.downsample_ln checks the arguments.  The compute dtype is fp64 for fp64 tensors, else fp32, and under
    torch.autocast("cuda") the autocast dtype; autocast is switched off for the Function's own lines, so forward and backward use the same
    dtypes.  The HIP forward (uni_down_train_fwd) reads x in the dtype it has and writes the LayerNorm output straight into the patch matrix
    A (M, 4C) of the convolution, which is then the addmm F.linear would make.  Saves x, the two LayerNorm vectors, weight and the (N H W, 2)
    statistics: neither A nor the LayerNorm output.  The backward rebuilds A only when weight.grad is asked for (gy.t() @ A, in row slices:
    _wgrad_mm) and computes only what autograd asks for.  No host synchronisation, one writer per element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, x, ln_weight, ln_bias, weight, bias, eps):
        N, Cc, H, W = x.shape
        Co, Ho, Wo = weight.shape[0], H // 2, W // 2
        cd = _patch_compute_dtype(x)
        sd = _pw_sum_dtype(cd)
        ctx.dims, ctx.cd, ctx.eps, ctx.x_dtype = (N, Cc, H, W, Co), cd, eps, x.dtype
        if N == 0:
            ctx.save_for_backward(x, ln_weight, ln_bias, weight)
            ctx.b_dtype = bias.dtype
            return torch.empty((N, Co, Ho, Wo), device=x.device, dtype=cd, memory_format=torch.channels_last)
        M = N * Ho * Wo
        with torch.autocast("cuda", enabled=False), torch.cuda.device(x.device):
            xc = x.detach().contiguous(memory_format=torch.channels_last)
            A = torch.empty((M, 4 * Cc), device=x.device, dtype=cd)
            stats = torch.empty((N * H * W, 2), device=x.device, dtype=sd)
            fn, name = _entry("uni_down_train_fwd", sd)
            L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], L.ptr(ln_weight.detach().to(sd).contiguous()), L.ptr(ln_bias.detach().to(sd).contiguous()),
                       eps, N, H, W, Cc, 0, L.ptr(A), _STORE_DTYPE[cd], L.ptr(stats), L.stream_ptr()), name)
            W2 = weight.detach().permute(0, 2, 3, 1).reshape(Co, 4 * Cc).to(cd)
            y = torch.addmm(bias.detach().to(cd), A, W2.t())
        ctx.save_for_backward(xc, ln_weight, ln_bias, weight, stats)
        ctx.b_dtype = bias.dtype
        return y.view(N, Ho, Wo, Co).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        need = ctx.needs_input_grad
        N, Cc, H, W, Co = ctx.dims
        cd = ctx.cd
        sd = _pw_sum_dtype(cd)
        if N == 0:
            x, ln_weight, ln_bias, weight = ctx.saved_tensors
            z = torch.zeros_like
            return (z(x) if need[0] else None, z(ln_weight) if need[1] else None, z(ln_bias) if need[2] else None, z(weight) if need[3] else None,
                    torch.zeros(Co, device=x.device, dtype=ctx.b_dtype) if need[4] else None, None)
        xc, ln_weight, ln_bias, weight, stats = ctx.saved_tensors
        dev, Ho, Wo = xc.device, H // 2, W // 2
        M = N * Ho * Wo
        need_ln = need[1] or need[2]
        g_x = g_lw = g_lb = g_w = g_b = None
        with torch.autocast("cuda", enabled=False), torch.cuda.device(dev):
            gy = grad_y.permute(0, 2, 3, 1).reshape(M, Co).to(cd).contiguous()
            lw = ln_weight.detach().to(sd).contiguous()
            if need[4]:
                g_b = _col_sum(dev, cd, gy).to(ctx.b_dtype)
            if need[3]:                                                      # A again, with the forward's bits
                A = torch.empty((M, 4 * Cc), device=dev, dtype=cd)
                fn, name = _entry("uni_down_train_fwd", sd)
                L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], L.ptr(lw), L.ptr(ln_bias.detach().to(sd).contiguous()), ctx.eps, N, H, W, Cc, 1,
                           L.ptr(A), _STORE_DTYPE[cd], L.ptr(stats), L.stream_ptr()), name)
                g_w = _wgrad_mm(gy, A).view(Co, 2, 2, Cc).permute(0, 3, 1, 2).to(weight.dtype).contiguous()
                del A
            if need[0] or need_ln:
                W2 = weight.detach().permute(0, 2, 3, 1).reshape(Co, 4 * Cc).to(cd)
                gA = torch.mm(gy, W2)
                g_x = torch.empty_like(xc) if need[0] else None              # channels-last like xc; the call writes it completely
                g_lw = torch.empty(Cc, device=dev, dtype=sd) if need_ln else None
                g_lb = torch.empty(Cc, device=dev, dtype=sd) if need_ln else None
                ws = _train_ws("downsample_ln", "uni_down_train_workspace_bytes", dev, sd, N, H, W, Cc) if need_ln else None
                fn, name = _entry("uni_down_train_bwd", sd)
                L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], L.ptr(lw), L.ptr(stats), L.ptr(gA), _STORE_DTYPE[cd], N, H, W, Cc, L.ptr(g_x),
                           L.ptr(g_lw), L.ptr(g_lb), L.ptr(ws), ws.numel() if need_ln else 0, L.stream_ptr()), name)
        return (g_x, g_lw.to(ln_weight.dtype) if need[1] else None, g_lb.to(ln_bias.dtype) if need[2] else None, g_w, g_b, None)


def _check_patch_conv(op, x, weight, bias, k):
    """the checks the two downsample operators share on the map and the convolution's parameters -> N, C, H, W, Co"""
    N, Cc, H, W = _check_map_dims(op, "x", x)
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (Cc, k, k):
        raise L.UnicornHipError("%s: weight of shape %s is not (Co, %d, %d, %d): a %dx%d / stride-%d convolution of x's %d channels"
                                % (op, tuple(weight.shape), Cc, k, k, k, k, k, Cc))
    Co = weight.shape[0]
    _check_channel_vecs(op, ("bias",), (bias,), Co)
    if Co % 4 or not 4 <= Co <= PW_MLP_MAX_H:
        raise L.UnicornHipError("%s: Co = %d is outside Co %% 4 == 0, 4 <= Co <= %d" % (op, Co, PW_MLP_MAX_H))
    if H < k or W < k:
        raise L.UnicornHipError("%s: map of H=%d W=%d is smaller than the %dx%d kernel" % (op, H, W, k, k))
    if N * H * W >= 1 << 31:
        raise L.UnicornHipError("%s: shape N=%d H=%d W=%d is outside N H W < 2^31" % (op, N, H, W))
    return N, Cc, H, W, Co


def _check_patch_dtypes(op, x, params, autocast):
    ts = (x,) + tuple(params)
    if x.dtype == torch.float64:
        ok = not autocast and all(t.dtype == torch.float64 for t in params)
    elif autocast:
        ok = x.dtype in _STORE_DTYPE and all(t.is_floating_point() and t.dtype != torch.float64 for t in params)
    else:
        ok = x.dtype in _STORE_DTYPE and all(t.dtype == torch.float32 for t in params)
    if not ok:
        raise L.UnicornHipError("%s: dtypes %s unsupported (x fp32 / fp16 / bf16 with fp32 parameters, or all fp64; half parameters only under "
                                "torch.autocast)" % (op, ", ".join(str(t.dtype) for t in ts)))


def downsample_ln(x, ln_weight, ln_bias, weight, bias, eps=1e-6):
    """A downsample layer of the ConvNeXt backbone (convnext.py:83-87) as one operator, equal in value and in all five gradients to
    Conv2d(C, Co, 2, stride=2)(LayerNorm(C, data_format="channels_first")(x)):
      x                  (N, C, H, W) fp32, fp16 or bf16, read in the dtype it has.  Channels-last memory (what ops.block_tail returns) is read
                         in place; any other layout (NCHW-contiguous included) is converted ONCE with
                         .contiguous(memory_format=torch.channels_last), and x.grad comes back channels-last
      ln_weight, ln_bias (C,): the LayerNorm;  weight (Co, C, 2, 2), bias (Co,): the convolution.  fp32
    All five fp64 is accepted for checks.  The compute dtype is fp64 for fp64 tensors, else fp32, and under torch.autocast("cuda") the
    autocast dtype (the parameters are cast to it as F.conv2d casts them; the LayerNorm itself is computed in fp32 and rounded once).  Returns
    y (N, Co, H // 2, W // 2) in the compute dtype with y.is_contiguous(memory_format=torch.channels_last): what the next block's
    ops.dwconv7_ln reads in place.  A last row or column that an odd H or W leaves over is dropped, as the convolution drops it: its x.grad is
    exact zeros.  The GEMMs are the vendor library's (addmm / mm); the LayerNorm, the patch layout and the LayerNorm backward are HIP
    (uni_down_train_fwd / _bwd), the bias gradient is the column sum of uni_pw_mlp_act_bwd.  Autograd keeps x, ln_weight, ln_bias, weight and
    two numbers per pixel: neither the LayerNorm output nor the patch matrix, which the backward rebuilds only for weight.grad.
    C % 4 == 0, 4 <= C <= 2048, Co % 4 == 0, 4 <= Co <= 8192, H, W >= 2.  N == 0 returns an empty tensor without a library call."""
    op = "downsample_ln"
    names = ("x", "ln_weight", "ln_bias", "weight", "bias")
    ts = (x, ln_weight, ln_bias, weight, bias)
    _check_tensors(op, names, ts)
    autocast = x.is_cuda and torch.is_autocast_enabled("cuda")
    N, Cc, H, W, Co = _check_patch_conv(op, x, weight, bias, 2)
    _check_channel_vecs(op, names[1:3], ts[1:3], Cc)
    _check_train_shape(op, N, Cc, H, W)
    _check_eps(op, eps)
    _check_patch_dtypes(op, x, ts[1:], autocast)
    _check_one_device(op, ts)
    return DownsampleLNFunction.apply(x, ln_weight, ln_bias, weight, bias, float(eps))


class StemConvFunction(torch.autograd.Function):
    """The stem convolution of the ConvNeXt backbone (convnext.py:77-80: Conv2d(in_chans, C0, 4, stride=4)): apply(x (N,Cin,H,W), weight
    (Co,Cin,4,4), bias (Co,)) -> y (N,Co,H//4,W//4) in channels-last memory, in the compute dtype of DownsampleLNFunction; ops.stem_conv checks
    the arguments.  uni_patch4_gather writes the patch matrix A (M, 16 Cin), the GEMM is the addmm F.linear would make.  Saves x and weight; A
    is gathered again for weight.grad, and x.grad (an image normally has none) is a mm and uni_patch4_scatter."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        N, Cin, H, W = x.shape
        Co, Ho, Wo = weight.shape[0], H // 4, W // 4
        cd = _patch_compute_dtype(x)
        ctx.dims, ctx.cd, ctx.b_dtype = (N, Cin, H, W, Co), cd, bias.dtype
        if N == 0:
            ctx.save_for_backward(x, weight)
            return torch.empty((N, Co, Ho, Wo), device=x.device, dtype=cd, memory_format=torch.channels_last)
        M = N * Ho * Wo
        with torch.autocast("cuda", enabled=False), torch.cuda.device(x.device):
            xc = x.detach().contiguous()
            A = torch.empty((M, 16 * Cin), device=x.device, dtype=cd)
            fn, name = _entry("uni_patch4_gather", _pw_sum_dtype(cd))
            L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], N, Cin, H, W, L.ptr(A), _STORE_DTYPE[cd], L.stream_ptr()), name)
            y = torch.addmm(bias.detach().to(cd), A, weight.detach().reshape(Co, 16 * Cin).to(cd).t())
        ctx.save_for_backward(xc, weight)
        return y.view(N, Ho, Wo, Co).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        need = ctx.needs_input_grad
        N, Cin, H, W, Co = ctx.dims
        cd = ctx.cd
        xc, weight = ctx.saved_tensors
        if N == 0:
            return (torch.zeros_like(xc) if need[0] else None, torch.zeros_like(weight) if need[1] else None,
                    torch.zeros(Co, device=xc.device, dtype=ctx.b_dtype) if need[2] else None)
        dev, Ho, Wo = xc.device, H // 4, W // 4
        M = N * Ho * Wo
        g_x = g_w = g_b = None
        with torch.autocast("cuda", enabled=False), torch.cuda.device(dev):
            gy = grad_y.permute(0, 2, 3, 1).reshape(M, Co).to(cd).contiguous()
            if need[2]:
                g_b = _col_sum(dev, cd, gy).to(ctx.b_dtype)
            if need[1]:
                A = torch.empty((M, 16 * Cin), device=dev, dtype=cd)
                fn, name = _entry("uni_patch4_gather", _pw_sum_dtype(cd))
                L.check(fn(L.ptr(xc), _STORE_DTYPE[xc.dtype], N, Cin, H, W, L.ptr(A), _STORE_DTYPE[cd], L.stream_ptr()), name)
                g_w = _wgrad_mm(gy, A).view(Co, Cin, 4, 4).to(weight.dtype)
                del A
            if need[0]:
                gA = torch.mm(gy, weight.detach().reshape(Co, 16 * Cin).to(cd))
                g_x = torch.empty_like(xc)                                   # NCHW-contiguous like xc; the call writes it completely
                fn, name = _entry("uni_patch4_scatter", _pw_sum_dtype(cd))
                L.check(fn(L.ptr(gA), _STORE_DTYPE[cd], N, Cin, H, W, L.ptr(g_x), _STORE_DTYPE[xc.dtype], L.stream_ptr()), name)
        return g_x, g_w, g_b


STEM_MAX_CIN = 4


def stem_conv(x, weight, bias):
    """The stem convolution of the ConvNeXt backbone (convnext.py:77-80) as one operator, equal in value and in all three gradients to
    Conv2d(Cin, Co, 4, stride=4)(x): x (N, Cin, H, W) fp32, fp16 or bf16 (any strides but NCHW-contiguous are converted once with
    .contiguous()), weight (Co, Cin, 4, 4) and bias (Co,) fp32; or all fp64 for checks.  Compute dtype, autocast and the layout of the result are
    those of ops.downsample_ln: y (N, Co, H // 4, W // 4) in channels-last memory, which ops.layernorm_cf reads in place.  The margin that
    H % 4 or W % 4 leaves over is dropped, as the convolution drops it: its x.grad is zero.  The GEMMs are the vendor library's; the patch
    gather and scatter are HIP (uni_patch4_gather / _scatter), the bias gradient is the column sum of uni_pw_mlp_act_bwd.  Autograd keeps x
    and weight; x.grad is computed only when x requires a gradient.  1 <= Cin <= 4, Co % 4 == 0, 4 <= Co <= 8192, H, W >= 4.  N == 0 returns
    an empty tensor without a library call."""
    op = "stem_conv"
    ts = (x, weight, bias)
    _check_tensors(op, ("x", "weight", "bias"), ts)
    autocast = x.is_cuda and torch.is_autocast_enabled("cuda")
    N, Cin, H, W, Co = _check_patch_conv(op, x, weight, bias, 4)
    if not 1 <= Cin <= STEM_MAX_CIN:
        raise L.UnicornHipError("%s: Cin = %d is outside 1 <= Cin <= %d" % (op, Cin, STEM_MAX_CIN))
    _check_patch_dtypes(op, x, ts[1:], autocast)
    _check_one_device(op, ts)
    return StemConvFunction.apply(x, weight, bias)


def _prop_ws(dev, B, Kc, Q):
    need = L.lib().uni_prop_workspace_bytes(B, Kc, Q)
    if need == 0:
        raise L.UnicornHipError("prop_loss: shape B=%d Kc=%d Q=%d is outside the limits of uni_prop_dice_pyramid_fwd (include/unicorn_hip.h)" % (B, Kc, Q))
    return torch.empty(need, device=dev, dtype=torch.uint8)


def prop_labels(targets, H8, W8, Kc, dtype=torch.float32, masks=None, sot=False):
    """`uni_prop_labels`: targets (B, 2, M, 6) fp32 contiguous device rows [cls, cx, cy, w, h, trackid] (+ masks (B, 2, M, r H8, r W8) fp32 / uint8
    contiguous, r = 1, 2, 4) -> matched (B, Kc, 2) int32, num_matched (B,) int32, gt0, gt1 (B, Kc, H8 W8) of `dtype`: the match table of
    compute_loss_vos (unicorn.py:352-361; sot: row 0 of both frames) and the stride-8 label rows of both frames, from boxes
    (F.interpolate(get_label_map(..), 1/8)) or from the masks (init_with_mask).  Not differentiable, no host synchronisation."""
    B, M, dev = targets.shape[0], targets.shape[2], targets.device
    matched = torch.empty((B, Kc, 2), device=dev, dtype=torch.int32)
    num = torch.empty((B,), device=dev, dtype=torch.int32)
    gt0 = torch.empty((B, Kc, H8 * W8), device=dev, dtype=dtype)
    gt1 = torch.empty_like(gt0)
    r = 0 if masks is None else masks.shape[3] // H8
    fn, name = _entry("uni_prop_labels", dtype)
    with torch.cuda.device(dev):
        L.check(fn(L.ptr(targets), L.ptr(masks), 1 if masks is not None and masks.dtype == torch.uint8 else 0, B, M, Kc, 1 if sot else 0, H8, W8, r,
                   L.ptr(matched), L.ptr(num), L.ptr(gt0), L.ptr(gt1), L.stream_ptr()), name)
    return matched, num, gt0, gt1


class PropDiceFunction(torch.autograd.Function):
    """The Dice loss and the prior pyramid behind the label propagation (unicorn.py:329-334, :372-379, :509-519) in one forward pass and ONE
    backward kernel: apply(pred (B, Kc, H8, W8), gt1 (B, Kc, H8 W8), num_matched (B,) int32 or None) -> (loss, p8, p16, p32).
    p8 is `pred` itself; p16 / p32 = F.interpolate(pred, 1/2 and 1/4, bilinear).  num_matched given: loss (B, Kc), one Dice per slot, zero
    behind num_matched[b]; None: ONE Dice over the batch (the SOT branch).  Differentiable in pred; the upstream gradients of all four
    outputs are honoured, and one that is None costs nothing.  Saves pred, gt1 and three sums per Dice.  No host synchronisation; one
    writer per gradient element: bitwise reproducible."""

    @staticmethod
    def forward(ctx, pred, gt1, num_matched):
        B, Kc, H8, W8 = pred.shape
        dev, dt = pred.device, pred.dtype
        pred_, gt_ = pred.detach().contiguous(), gt1.contiguous()
        groups = 1 if num_matched is None else B * Kc
        p16 = torch.empty((B, Kc, H8 // 2, W8 // 2), device=dev, dtype=dt)
        p32 = torch.empty((B, Kc, H8 // 4, W8 // 4), device=dev, dtype=dt)
        loss = torch.empty(() if num_matched is None else (B, Kc), device=dev, dtype=dt)
        sums = torch.empty((groups, 3), device=dev, dtype=torch.float64)
        fn, name = _entry("uni_prop_dice_pyramid_fwd", dt)
        with torch.cuda.device(dev):
            ws = _prop_ws(dev, B, Kc, H8 * W8)
            L.check(fn(L.ptr(pred_), L.ptr(gt_), L.ptr(num_matched), B, Kc, H8, W8, L.ptr(p16), L.ptr(p32), L.ptr(loss), L.ptr(sums), L.ptr(ws),
                       ws.numel(), L.stream_ptr()), name)
        ctx.save_for_backward(pred_, gt_, num_matched, sums)
        ctx.set_materialize_grads(False)
        return loss, pred, p16, p32

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_p8, g_p16, g_p32):
        pred, gt1, num_matched, sums = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_loss is None and g_p8 is None and g_p16 is None and g_p32 is None):
            return None, None, None
        B, Kc, H8, W8 = pred.shape
        gs = [None if g is None else g.contiguous() for g in (g_p8, g_p16, g_p32, g_loss)]
        g_pred = torch.empty_like(pred)                   # written completely by the call
        fn, name = _entry("uni_prop_dice_pyramid_bwd", pred.dtype)
        with torch.cuda.device(pred.device):
            L.check(fn(L.ptr(pred), L.ptr(gt1), L.ptr(num_matched), L.ptr(sums), *map(L.ptr, gs), B, Kc, H8, W8, L.ptr(g_pred), L.stream_ptr()), name)
        return g_pred, None, None


def _prop_args(what, embed_0, embed_1, targets, img_size):
    """the checks the two label-propagation losses share -> (B, C, H8, W8, M)"""
    for n, t in (("embed_0", embed_0), ("embed_1", embed_1), ("targets", targets)):
        if not isinstance(t, torch.Tensor):
            raise L.UnicornHipError("%s: %s is not a tensor" % (what, n))
    if embed_0.dim() != 4 or embed_1.shape != embed_0.shape or targets.dim() != 4 or targets.shape[0] != embed_0.shape[0] \
            or targets.shape[1] != 2 or targets.shape[3] != 6 or targets.shape[2] < 1 or embed_0.shape[0] < 1:
        raise L.UnicornHipError("%s: shapes %s, %s, %s do not fit embed_0 (B,C,H8,W8), embed_1 (B,C,H8,W8), targets (B,2,M,6) with B, M >= 1"
                                % (what, tuple(embed_0.shape), tuple(embed_1.shape), tuple(targets.shape)))
    try:
        H, W = int(img_size[0]), int(img_size[1])
    except (TypeError, IndexError, ValueError):
        raise L.UnicornHipError("%s: img_size %r is not (height, width)" % (what, img_size))
    B, Cc, H8, W8 = embed_0.shape
    if H != 8 * H8 or W != 8 * W8 or H8 < 4 or W8 < 4:
        raise L.UnicornHipError("%s: img_size (%d, %d) is not 8 x the %d x %d maps, or a map side is below 4" % (what, H, W, H8, W8))
    if embed_0.dtype not in _F64_SFX or embed_1.dtype != embed_0.dtype:
        raise L.UnicornHipError("%s: embedding dtypes %s / %s unsupported (both fp32 or both fp64; no fp16 / autocast input: the reference "
                                "computes the embeddings under autocast(enabled=False))" % (what, embed_0.dtype, embed_1.dtype))
    if Cc > 128 or (embed_0.dtype == torch.float32 and Cc != 128):
        raise L.UnicornHipError("%s: C = %d channels unsupported: fp32 maps need C == 128, the limit of uni_corr_softmax_pv_lse (precision 0); "
                                "fp64 maps C <= 128" % (what, Cc))
    if targets.shape[2] > 1024:
        raise L.UnicornHipError("%s: M = %d rows per frame is outside M <= 1024" % (what, targets.shape[2]))
    return B, Cc, H8, W8, targets.shape[2]


def _prop_propagate(embed_0, embed_1, gt0):
    """propagate_labels on (B, C, H8, W8) maps; fp64 maps of fewer than 128 channels are padded with zero channels (the fp64 kernels are
    written for 128 too; a zero channel adds an exact zero to every dot product)"""
    e0, e1 = embed_0.flatten(2).transpose(1, 2), embed_1.flatten(2).transpose(1, 2)
    if e0.shape[2] < 128:
        e0, e1 = torch.nn.functional.pad(e0, (0, 128 - e0.shape[2])), torch.nn.functional.pad(e1, (0, 128 - e1.shape[2]))
    return CorrSoftmaxPVFunction.apply(e0, e1, gt0, 0)


def sot_prop_loss(embed_0, embed_1, targets, img_size):
    """The label-propagation part of Unicorn.compute_loss_sot (unicorn.py:321-334, propagate=True) for the whole batch without a host
    synchronisation: embed_0, embed_1 (B, 128, H8, W8) fp32 (or both fp64, C <= 128), NCHW or channels-last; targets (B, 2, M, 6) rows
    [cls, cx, cy, w, h, trackid], converted with .detach().float(); img_size (H, W) = (8 H8, 8 W8).  Row 0 of each frame is the object.
    -> corr_loss (0-d: ONE Dice over the batch, as the reference flattens it), (p8 (B,1,H8,W8), p16, p32) = pred_lbs1_ms for the head.
    The label maps are built on the device without the full-resolution map (get_label_map's .tolist() is a synchronisation per sample);
    the HW x HW matrix is never formed (propagate_labels); Dice and pyramid are one pass, their backward one kernel.  corr_loss and the three
    priors are differentiable in both embeddings."""
    B, Cc, H8, W8, M = _prop_args("sot_prop_loss", embed_0, embed_1, targets, img_size)
    _need_cuda(embed_0, embed_1, targets)
    if len({t.device for t in (embed_0, embed_1, targets)}) != 1:
        raise L.UnicornHipError("sot_prop_loss: tensors on different devices")
    t = targets.detach().float().contiguous()
    _, _, gt0, gt1 = prop_labels(t, H8, W8, 1, embed_0.dtype, None, sot=True)
    pred = _prop_propagate(embed_0, embed_1, gt0).view(B, 1, H8, W8)
    loss, p8, p16, p32 = PropDiceFunction.apply(pred, gt1, None)
    return loss, (p8, p16, p32)


def vos_prop_loss(embed_0, embed_1, targets, img_size, masks=None, max_inst=None):
    """The label-propagation part of Unicorn.compute_loss_vos (unicorn.py:342-379 without the head call) for the whole batch and ALL matched
    instances at once, without a host synchronisation: embeddings, targets, img_size as in sot_prop_loss; masks (B, 2, M, r H8, r W8) fp32 or
    uint8 with r = 1, 2, 4 = init_with_mask with scale_factor 1 / r (labels from the masks instead of the boxes); max_inst = the
    reference's max_matched_inst.  Kc = min(M, max_inst or M) slots per sample, filled in the reference's order: i = 0 .. M-1 with
    id_r[i] != 0 and the first j with id_c[j] != 0 and id_c[j] == id_r[i] (fp32 compare).
    -> corr_loss (B, Kc) one Dice per slot, (p8 (B,Kc,H8,W8), p16, p32) the priors of every instance, matched (B, Kc, 2) int32 = (i, j),
    num_matched (B,) int32.  Slots >= num_matched[b] hold -1, zero loss, zero priors and carry exactly zero gradient.  The reference's
    average_dict is corr_loss.sum() / num_matched.sum().clamp(min=1) on the device.  All instances of a sample are value rows of ONE
    propagation; the backward of the correlation walks them in chunks of 8 rows (KMAX in csrc/corr_bwd.hip), each chunk one more recompute
    pass over the HW x HW tiles."""
    B, Cc, H8, W8, M = _prop_args("vos_prop_loss", embed_0, embed_1, targets, img_size)
    if max_inst is not None and int(max_inst) < 1:
        raise L.UnicornHipError("vos_prop_loss: max_inst = %r is not positive" % (max_inst,))
    Kc = M if max_inst is None else min(M, int(max_inst))
    if masks is not None:
        if not isinstance(masks, torch.Tensor) or masks.dim() != 5 or tuple(masks.shape[:3]) != (B, 2, M) \
                or not any(tuple(masks.shape[3:]) == (r * H8, r * W8) for r in (1, 2, 4)):
            raise L.UnicornHipError("vos_prop_loss: masks %s do not fit (B, 2, M, r H8, r W8) = (%d, 2, %d, r x %d, r x %d) with r = 1, 2 or 4"
                                    % (None if not isinstance(masks, torch.Tensor) else tuple(masks.shape), B, M, H8, W8))
        if masks.dtype not in (torch.float32, torch.uint8):
            raise L.UnicornHipError("vos_prop_loss: masks of dtype %s unsupported (fp32 or uint8)" % masks.dtype)
    _need_cuda(embed_0, embed_1, targets, masks)
    if len({t.device for t in (embed_0, embed_1, targets) + (() if masks is None else (masks,))}) != 1:
        raise L.UnicornHipError("vos_prop_loss: tensors on different devices")
    if B * Kc > 32767:
        raise L.UnicornHipError("vos_prop_loss: B x Kc = %d x %d slots is outside B Kc <= 32767" % (B, Kc))
    t = targets.detach().float().contiguous()
    matched, num, gt0, gt1 = prop_labels(t, H8, W8, Kc, embed_0.dtype, None if masks is None else masks.detach().contiguous())
    pred = _prop_propagate(embed_0, embed_1, gt0).view(B, Kc, H8, W8)
    loss, p8, p16, p32 = PropDiceFunction.apply(pred, gt1, num)
    return loss, (p8, p16, p32), matched, num


def condinst_masks_resized(mask_feats, up_masks, params, inst_loc, inst_lvl, up_rate, d_rate, r, H, W, thr=None):
    """condinst_masks + mask_resize in ONE call (uni_condinst_masks_u8): the CondInst scores of `params` resized by 1/r and pasted into
    (N, H, W) maps -- `> thr` bytes (mot_evaluator.py:804-805) or, with thr=None, fp32 probabilities (unicorn_vos.py:141-152) -- without the
    (N, 1, Hn, Wn) network-size maps ever reaching HBM.  Bit-identical to mask_resize(condinst_masks(...)[:, 0], r, H, W, thr)."""
    mf, um, p, loc, lvl, ws = _condinst_inputs(mask_feats, up_masks, params, inst_loc, inst_lvl, up_rate)
    (_, _, H8, W8), n = mf.shape, p.shape[0]
    out = torch.empty((n, int(H), int(W)), device=mf.device, dtype=torch.float32 if thr is None else torch.uint8)
    if n:
        L.check(L.lib().uni_condinst_masks_u8(L.ptr(mf), L.ptr(um), L.ptr(p), p.shape[1], L.ptr(loc), L.ptr(lvl), n, H8, W8, up_rate, d_rate,
                                              float(r), int(H), int(W), 0.0 if thr is None else float(thr), L.ptr(out) if thr is None else None,
                                              None if thr is None else L.ptr(out), L.ptr(ws), ws.numel() * 4, L.stream_ptr()),
                "uni_condinst_masks_u8")
    return out


_post_ws = {}


class PostTicket:
    """uni_postprocess in flight: device buffers + the row count on its way to pinned host memory + the event that says it arrived"""
    __slots__ = ("det", "keep", "n_dev", "n_host", "event", "A")


def postprocess_launch(image_pred, num_classes, conf_thre, nms_thre, class_agnostic=False, precornered=False):
    """Enqueue unicorn/utils/boxes.py:33-77 for ONE image (uni_postprocess) WITHOUT a host sync: the survivor count goes to pinned
    host memory by an async copy and an event is recorded behind it.  `postprocess_collect(ticket)` waits for THAT event only, so
    work enqueued later on the same stream (the next frame of a pipelined tracker loop) does not delay the read-back."""
    _need_cuda(image_pred)
    if image_pred.dtype != torch.float32 or image_pred.stride(-1) != 1:
        raise L.UnicornHipError("postprocess_image: needs a float32 (A, 5+nc) tensor with unit inner stride")
    A, ld = image_pred.shape[0], image_pred.stride(0) if image_pred.shape[0] > 1 else image_pred.shape[1]
    dev = image_pred.device
    ws = _stream_scratch(_post_ws, dev, L.lib().uni_postprocess_workspace_bytes(A))
    t = PostTicket()
    t.A = A
    t.det = torch.empty((max(A, 1), 7), device=dev, dtype=torch.float32)
    t.keep = torch.empty((max(A, 1),), device=dev, dtype=torch.int32)
    t.n_dev = torch.zeros((1,), device=dev, dtype=torch.int32)
    L.check(L.lib().uni_postprocess(L.ptr(image_pred), A, ld, num_classes, float(conf_thre), float(nms_thre),
                                    int(bool(class_agnostic)) | (2 if precornered else 0), A, L.ptr(t.det), L.ptr(t.keep), L.ptr(t.n_dev), L.ptr(ws), ws.numel(), L.stream_ptr()), "uni_postprocess")
    t.n_host = torch.empty((1,), dtype=torch.int32).pin_memory()
    t.n_host.copy_(t.n_dev, non_blocking=True)
    t.event = torch.cuda.Event()
    t.event.record()
    return t


def postprocess_collect(t):
    """-> (det (M,7), anchor indices (M,) int64) or (None, None); blocks on the ticket's own event only"""
    t.event.synchronize()
    m = int(t.n_host[0])
    if m == 0:
        return None, None
    return t.det[:m], t.keep[:m].long()


def postprocess_image(image_pred, num_classes, conf_thre, nms_thre, class_agnostic=False, precornered=False):
    """unicorn/utils/boxes.py:33-77 for ONE image on the device (uni_postprocess): image_pred (A, 5+nc) decoded cxcywh fp32,
    converted to corners in place (precornered=True: boxes are already xyxy).  Returns (det (M,7), anchor indices (M,) int64) or (None, None).  The only host sync is
    the read-back of M (the output shape is data dependent)."""
    return postprocess_collect(postprocess_launch(image_pred, num_classes, conf_thre, nms_thre, class_agnostic, precornered))


def letterbox(image, input_size, swap_rb=True, device=None):
    """PreprocessorX.process (unicorn_sot.py:111-123, swap_rb=True) / preproc (data_augment.py:194-214, swap_rb=False) on the
    device: image (h, w, 3) uint8 (numpy array or cuda tensor) -> ((1, 3, H, W) float32 cuda tensor, r)."""
    import ctypes as C
    if not torch.is_tensor(image):
        import numpy as np
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise L.UnicornHipError("letterbox: needs an (h, w, 3) uint8 image")
    if not image.is_cuda:
        image = image.to(device if device is not None else "cuda", non_blocking=True)
    image = image.contiguous()
    H, W = int(input_size[0]), int(input_size[1])
    out = torch.empty((1, 3, H, W), device=image.device, dtype=torch.float32)
    r = C.c_double(0.0)
    with torch.cuda.device(image.device):
        L.check(L.lib().uni_letterbox(L.ptr(image), image.shape[0], image.shape[1], int(bool(swap_rb)), H, W, L.ptr(out), C.byref(r),
                                      L.stream_ptr()), "uni_letterbox")
    return out, r.value


# ---------------------------------------------------------------------------------------------------------------------
# mask post-processing of the VOS / MOTS drivers on the device (csrc/mask_post.hip)
# ---------------------------------------------------------------------------------------------------------------------
def mask_resize(masks, r, H, W, thr=None):
    """masks (N, Hn, Wn) fp32 cuda -> F.interpolate(masks[:, None], scale_factor=1/r, bilinear)[:, 0, :H, :W] pasted into zero
    (N, H, W) maps (unicorn_vos.py:146-150); with thr: the `> thr` byte masks of mot_evaluator.py:804-805 instead."""
    _need_cuda(masks)
    m = masks.float().contiguous()
    N, Hn, Wn = m.shape
    if N == 0:
        return torch.empty((0, H, W), device=m.device, dtype=torch.float32 if thr is None else torch.uint8)
    if thr is None:
        out = torch.empty((N, H, W), device=m.device, dtype=torch.float32)
        L.check(L.lib().uni_mask_resize(L.ptr(m), N, Hn, Wn, float(r), H, W, 0.0, L.ptr(out), None, L.stream_ptr()), "uni_mask_resize")
    else:
        out = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
        L.check(L.lib().uni_mask_resize(L.ptr(m), N, Hn, Wn, float(r), H, W, float(thr), None, L.ptr(out), L.stream_ptr()), "uni_mask_resize")
    return out


def vos_merge(probs, prob_ids, r, H, W, init_masks=None, init_ids=()):
    """soft aggregation of unicorn_vos.py:99-120 fused with the 1/r resize: probs (K1, Hn, Wn) network-resolution mask
    probabilities of the tracked objects (ids prob_ids, cur_obj_ids order), init_masks (K2, H, W) of objects introduced in
    this frame -> (H, W) uint8 id map on the device."""
    dev = probs.device if probs is not None else init_masks.device
    K1 = 0 if probs is None else probs.shape[0]
    K2 = len(init_ids)
    out = torch.empty((H, W), device=dev, dtype=torch.uint8)
    p = probs.float().contiguous() if K1 else None
    pid = torch.tensor([int(k) for k in prob_ids], dtype=torch.int32, device=dev) if K1 else None
    im = init_masks.to(torch.uint8).contiguous() if K2 else None
    iid = torch.tensor([int(k) for k in init_ids], dtype=torch.int32, device=dev) if K2 else None
    Hn, Wn = (p.shape[1], p.shape[2]) if K1 else (0, 0)
    L.check(L.lib().uni_vos_merge(L.ptr(p), L.ptr(pid), K1, Hn, Wn, float(r), L.ptr(im), L.ptr(iid), K2, H, W, L.ptr(out),
                                  L.stream_ptr()), "uni_vos_merge")
    return out


def mots_overlap_free(masks):
    """mot_evaluator.py:860-865: (N, H, W) bool/uint8 masks in track order -> earlier tracks keep overlapping pixels"""
    _need_cuda(masks)
    m = masks.to(torch.uint8).contiguous()
    out = torch.empty_like(m)
    if m.shape[0]:
        L.check(L.lib().uni_mots_overlap_free(L.ptr(m), m.shape[0], m.shape[1], m.shape[2], L.ptr(out), L.stream_ptr()), "uni_mots_overlap_free")
    return out


def _rle_call(m, max_runs):
    """one uni_rle_encode over (N, H, W) uint8 masks -> (chars (N, max_chars) uint8, lens (N,) int32) on the device; a length < 0 = more than
    max_runs runs"""
    N, H, W = m.shape
    max_chars = 6 * (max_runs + 1)
    ws = torch.empty(L.lib().uni_rle_workspace_bytes(N, H, W, max_runs), device=m.device, dtype=torch.uint8)
    chars = torch.empty((N, max_chars), device=m.device, dtype=torch.uint8)
    lens = torch.empty((N,), device=m.device, dtype=torch.int32)
    L.check(L.lib().uni_rle_encode(L.ptr(m), N, H, W, max_runs, max_chars, L.ptr(chars), L.ptr(lens), None, None, L.ptr(ws),
                                   ws.numel(), L.stream_ptr()), "uni_rle_encode")
    return chars, lens


def rle_encode_launch(masks, max_runs=1 << 14):
    """enqueue uni_rle_encode + async copies of the string lengths and characters into pinned host memory; -> ticket"""
    _need_cuda(masks)
    m = masks.to(torch.uint8).contiguous()
    N = m.shape[0]
    if N == 0:
        return {"N": 0}
    chars, lens = _rle_call(m, max_runs)
    # the strings of real masks are short (a few hundred characters): the first `head` characters of every row travel with the
    # lengths; a longer string (or an overflow of max_runs, length < 0) is fetched / re-encoded by rle_encode_collect
    head = min(chars.shape[1], 4096)
    lens_h = torch.empty((N,), dtype=torch.int32).pin_memory()
    chars_h = torch.empty((N, head), dtype=torch.uint8).pin_memory()
    lens_h.copy_(lens, non_blocking=True)
    chars_h.copy_(chars[:, :head], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return {"N": N, "m": m, "chars": chars, "lens_h": lens_h, "chars_h": chars_h, "head": head, "event": ev, "max_runs": max_runs}


def rle_encode_collect(t):
    if t["N"] == 0:
        return []
    t["event"].synchronize()
    ln = t["lens_h"].tolist()
    if min(ln) < 0:                          # a mask with more runs than expected: synchronous retry with larger bounds
        return rle_encode(t["m"], max_runs=t["max_runs"] * 4)
    if max(ln) > t["head"]:
        host = t["chars"][:, :max(ln)].cpu().numpy()
    else:
        host = t["chars_h"].numpy()
    return [host[i, :ln[i]].tobytes() for i in range(t["N"])]


def rle_encode(masks, max_runs=1 << 14):
    """pycocotools.mask.encode(np.asfortranarray(mask))["counts"] for every (H, W) mask of an (N, H, W) {0,1} cuda tensor
    (mot_evaluator.py:889-892) -> list of bytes objects.  Runs are found and the strings are written on the device; one
    read-back of lengths + chars."""
    _need_cuda(masks)
    m = masks.to(torch.uint8).contiguous()
    N = m.shape[0]
    if N == 0:
        return []
    while True:
        chars, lens = _rle_call(m, max_runs)
        ln = lens.cpu().tolist()
        if min(ln) >= 0:
            break
        max_runs *= 4                      # a mask with more runs than expected: retry with larger bounds
    top = max(ln)
    host = chars[:, :top].cpu().numpy()
    return [host[i, :ln[i]].tobytes() for i in range(N)]


def adamw_ema_step(params, grads, exp_avgs, exp_avg_sqs, emas, step, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, lr_factors=None,
                   ema_decay, scaler=None, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, plan=None):
    """`uni_opt_step`, the functional form of unicorn_amd.optim.FusedAdamWEMA over lists of fp32 device tensors, all updated IN PLACE:
    GradScaler.step (unscale, non-finite check, skip) + torch.optim.AdamW's single-tensor update + GradScaler.update + ModelEMA.update
    (trainer.py:260-275, utils/ema.py:50-63) in at most three launches and without a host read-back.

    params[i], emas[i]                  parameter (or float buffer) and its EMA copy
    grads[i], exp_avgs[i], exp_avg_sqs[i]   None = no gradient: the entry gets the EMA update only
    step                                one fp32 device word (t - 1); incremented unless the step is skipped
    lr, lr_factors[i], weight_decay     the entry's learning rate is lr * lr_factors[i]; weight_decay a float or one per entry
    ema_decay                           d of `e = e * d + (1 - d) * p` (ModelEMA: decay * (1 - exp(-updates / 2000)), a host scalar)
    scaler                              None or (scale fp32, growth_tracker int32, found_inf fp32) device words; found_inf is cleared by the call
    plan                                the StepPlan a previous call returned: while the addresses and per-entry scalars stay the same, nothing
                                        is uploaded.  -> the plan

    The gradients are left scaled.  Entries must be dense with identical strides (a channels_last parameter with channels_last partners is
    updated in storage order); bad arguments raise ValueError before the library is touched."""
    from . import optim
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(emas) == n):
        raise ValueError("adamw_ema_step: the five lists differ in length")
    wds = [float(weight_decay)] * n if not hasattr(weight_decay, "__len__") else [float(w) for w in weight_decay]
    lrf = [1.0] * n if lr_factors is None else [float(f) for f in lr_factors]
    if len(wds) != n or len(lrf) != n:
        raise ValueError("adamw_ema_step: lr_factors / weight_decay need one value per entry")
    entries = [(p, g, m if g is not None else None, v if g is not None else None, e) for p, g, m, v, e in zip(params, grads, exp_avgs, exp_avg_sqs, emas)]
    dev = optim.check_entries(entries, device_check=False)
    optim.check_state_words(step, scaler, dev)
    optim.need_cuda(dev)
    if dev is None:
        raise ValueError("adamw_ema_step: empty list")
    addr = [[0 if t is None else t.data_ptr() for t in ent] for ent in entries]
    key = (addr, lrf, wds)
    plan = plan or optim.StepPlan()
    if plan.key != key:
        cols = {k: [a[j] for a in addr] for j, k in enumerate(("p", "g", "m", "v", "e"))}
        cols.update(n=[ent[0].numel() for ent in entries], lr_factor=lrf, wd=wds, has_grad=[ent[1] is not None for ent in entries])
        plan.upload(key, cols, dev)
    plan.launch(step, scaler, lr, betas, eps, ema_decay, growth_factor, backoff_factor, growth_interval)
    return plan
