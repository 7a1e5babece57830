// Fused CondInst mask loss for TRAINING (condinst/dynamic_mask_head.py:138-170 mask_heads_forward / upsample_preds, :172-225
// mask_heads_forward_with_coords, :247-278 the dice loss of __call__; dice_coefficient :50-58), forward and a recomputing backward.
//
//   in = [rel_x, rel_y, mask_feats(8)]   h0 = relu(W0 in + b0)   h1 = relu(W1 h0 + b1)   L = W2 h1 + b2        (per instance, per coarse pixel)
//   u[n, r y + i, r x + j] = sum_t w_t[y, x, i, j] Lpad[n, (y, x) + delta_t],  w = softmax_t(up_masks)           (convex upsample x r)
//   s = sigmoid(u)   I = sum s g   U = sum s^2 + sum g^2 + 1e-5   loss_n = 1 - 2 I / U
//
// Nothing of size n x rH x rW is ever stored: the forward keeps three sums per instance, the backward recomputes s from the coarse logits.
// Every output element has ONE writer and every sum a fixed order (no float atomics): results are bitwise reproducible.
//
//   forward   cl_mlp_kernel      logits[n][HW]                                         thread = (instance, coarse pixel)
//             cl_dice_kernel     block partials of (sum s g, sum s^2, sum g^2)         thread = fine pixel x CL_IC instances (tap weights once)
//             cl_dice_final      partials -> sums[n][3], loss[n]                       block = instance, fixed-order tree
//   backward  cl_mlp_kernel      logits again (the workspace is scratch between calls)
//             per chunk of CL_CH instances, in stream order:
//               cl_du_kernel     du = gout (-2 g / U + 4 I s / U^2) s (1 - s) per fine pixel; d up_masks += du w_t (L_t - u) (the thread owns its
//                                element over ALL instances: chunk c adds to what chunk c - 1 left); A[k][p][t] = sum_sub w_t du  (LDS, fixed order)
//               cl_gather_kernel dL[n][q] = sum_t A[k][q - delta_t][t]                    the 9 x r r contributions that read q, one writer
//             cl_dparams_kernel  recompute h0 / h1, one half of the 169 accumulators per thread over its pixels (blockIdx.z), wave + block
//                                reduction -> partials
//             cl_dparams_final   partials -> grad_params[n][169]
//             cl_dfeat_kernel    thread = coarse pixel, loops the instances of a chunk -> partials;  cl_dfeat_final adds the chunks in order
//
// The chunked A buffer (CL_CH x HW x 9) keeps the workspace at O(n HW) with a small constant instead of 9 x the logits.
//
// The kernels here are shells: the arithmetic and every summation order live in condinst_dev.h (the cl_* bodies), which
// head_mask_loss.hip calls too.  A shell picks the instance (compacted index) and the rows it reads.
#include "condinst_dev.h"

namespace {

constexpr int CL_CH = 16;      // backward: instances per chunk launch

template <typename T>
__global__ __launch_bounds__(256) void cl_mlp_kernel(const T* __restrict__ mask_feats, const T* __restrict__ params, int ldp,
                                                     const T* __restrict__ inst_loc, const int* __restrict__ inst_lvl, int HWc, int W,
                                                     T* __restrict__ logits) {
    __shared__ T prm[CL_NP];
    const int inst = blockIdx.y;
    for (int i = threadIdx.x; i < CL_NP; i += blockDim.x) prm[i] = params[(size_t)inst * ldp + i];
    __syncthreads();
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= HWc) return;
    T in[10], h0[8], h1[8];
    cl_inputs(mask_feats, inst_loc, inst_lvl, inst, pix, W, in);
    logits[(size_t)inst * HWc + pix] = cl_mlp(prm, in, h0, h1);
}

template <typename T>
__global__ __launch_bounds__(256) void cl_dice_kernel(const T* __restrict__ up_masks, const T* __restrict__ logits, const T* __restrict__ gt,
                                                      T* __restrict__ part, int n, int H, int W, int r, int PX, int nblk) {
    __shared__ T red[4][3 * CL_IC];
    const int rr = r * r, HWc = H * W;
    int pix, i, j, xl;
    bool valid;
    cl_map(r, PX, HWc, pix, i, j, xl, valid);
    T wt[9];
    int off[9];
    cl_taps(up_masks, pix, i * r + j, rr, H, W, valid, wt, off);
    const int y = pix / W, x = pix - y * W;
    const size_t fine = (size_t)(r * y + i) * (r * W) + r * x + j, fsz = (size_t)HWc * rr;
    const int i0 = blockIdx.y * CL_IC, cnt = min(n - i0, CL_IC);
    const auto g_at = [=](int inst) { return gt[(size_t)inst * fsz + fine]; };
    for (int k = 0; k < cnt; ++k) cl_dice_accum(wt, off, valid, logits, HWc, g_at, i0 + k, red, k);
    cl_dice_combine(i0, cnt, red, part, nblk);
}

template <typename T>
__global__ __launch_bounds__(256) void cl_dice_final(const T* __restrict__ part, int nblk, T* __restrict__ sums, T* __restrict__ loss) {
    __shared__ T red[3][256];
    T a[3];
    cl_dice_partial(part, blockIdx.x, nblk, a);
    cl_dice_finish(a, red, blockIdx.x, sums, loss);
}

template <typename T>
__global__ __launch_bounds__(256) void cl_du_kernel(const T* __restrict__ up_masks, const T* __restrict__ logits, const T* __restrict__ gt,
                                                    const T* __restrict__ sums, const T* __restrict__ gout, T* __restrict__ A,
                                                    T* __restrict__ grad_um, int c0, int cnt, int H, int W, int r, int PX, int want_dl) {
    __shared__ T cs[9][256];
    const int rr = r * r, HWc = H * W;
    int pix, i, j, xl;
    bool valid;
    cl_map(r, PX, HWc, pix, i, j, xl, valid);
    T wt[9], acc[9];
    int off[9];
    cl_taps(up_masks, pix, i * r + j, rr, H, W, valid, wt, off);
    const int y = pix / W, x = pix - y * W;
    const size_t fine = (size_t)(r * y + i) * (r * W) + r * x + j, fsz = (size_t)HWc * rr;
    T* gum = grad_um ? grad_um + (size_t)pix * 9 * rr + i * r + j : nullptr;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = (gum && valid && c0 > 0) ? gum[t * rr] : (T)0;
    const auto g_at = [=](int inst) { return gt[(size_t)inst * fsz + fine]; };
    for (int k = 0; k < cnt; ++k) {
        T c[9];
        cl_du_instance(sums, gout[c0 + k], wt, off, valid, logits, HWc, g_at, c0 + k, c, acc);
        if (want_dl) cl_stage_taps(c, cs, A, k, r, PX, HWc);
    }
    if (gum && valid) {
#pragma unroll
        for (int t = 0; t < 9; ++t) gum[t * rr] = acc[t];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cl_gather_kernel(const T* __restrict__ A, T* __restrict__ dL, int c0, int H, int W) {
    const int HWc = H * W, q = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (q >= HWc) return;
    const int y = q / W, x = q - y * W;
    dL[(size_t)(c0 + k) * HWc + q] = cl_gather_pixel(A, k, y, x, H, W);
}

template <typename T>
__global__ __launch_bounds__(256) void cl_dparams_kernel(const T* __restrict__ mask_feats, const T* __restrict__ params, int ldp,
                                                         const T* __restrict__ inst_loc, const int* __restrict__ inst_lvl,
                                                         const T* __restrict__ dL, int HWc, int W, T* __restrict__ part, int nblk) {
    __shared__ T prm[CL_NP];
    __shared__ T red[4][CL_NP];
    for (int i = threadIdx.x; i < CL_NP; i += 256) prm[i] = params[(size_t)blockIdx.y * ldp + i];
    __syncthreads();
    if (blockIdx.z == 0) cl_dparams_half<T, 0>(prm, red, mask_feats, inst_loc, inst_lvl, dL, blockIdx.y, HWc, W, part, nblk);
    else cl_dparams_half<T, 1>(prm, red, mask_feats, inst_loc, inst_lvl, dL, blockIdx.y, HWc, W, part, nblk);
}

template <typename T>
__global__ __launch_bounds__(256) void cl_dparams_final(const T* __restrict__ part, int nblk, T* __restrict__ grad_params, int ldp) {
    const int inst = blockIdx.x, tid = threadIdx.x;
    if (tid >= CL_NP) return;
    T s = (T)0;
    for (int b = 0; b < nblk; ++b) s += part[((size_t)inst * nblk + b) * CL_NP + tid];
    grad_params[(size_t)inst * ldp + tid] = s;
}

template <typename T>
__global__ __launch_bounds__(CL_FB) void cl_dfeat_kernel(const T* __restrict__ mask_feats, const T* __restrict__ params, int ldp,
                                                          const T* __restrict__ inst_loc, const int* __restrict__ inst_lvl,
                                                          const T* __restrict__ dL, int n, int HWc, int W, T* __restrict__ part) {
    __shared__ T prm[CL_NP];
    const int pix = blockIdx.x * CL_FB + threadIdx.x, c0 = blockIdx.y * CL_CH, cnt = min(n - c0, CL_CH);
    const bool valid = pix < HWc;
    T dmf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dmf[c] = (T)0;
    for (int inst = c0; inst < c0 + cnt; ++inst)
        cl_dfeat_instance(prm, params + (size_t)inst * ldp, mask_feats, inst_loc, inst_lvl, dL, inst, pix, valid, HWc, W, dmf);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 8; ++c) part[((size_t)blockIdx.y * HWc + pix) * 8 + c] = dmf[c];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cl_dfeat_final(const T* __restrict__ part, int nchunk, int HWc, T* __restrict__ grad_mf) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= HWc * 8) return;
    T s = (T)0;
    for (int c = 0; c < nchunk; ++c) s += part[(size_t)c * HWc * 8 + e];
    grad_mf[e] = s;
}

// workspace layout, in elements of T
struct CLLayout {
    size_t logits, dL, dice, A, pp, pf, total;
    int PX, nblk_d, nblk_p, nchunk;
};
CLLayout cl_layout(int n, int H, int W, int r) {
    CLLayout l;
    const size_t hw = (size_t)H * W;
    l.PX = 256 / (r * r);
    l.nblk_d = cdiv(H * W, l.PX);
    l.nblk_p = cdiv(H * W, 256 * CL_PPT);
    l.nchunk = cdiv(n, CL_CH);
    size_t o = 0;
    l.logits = o; o += (size_t)n * hw;
    l.dL = o;     o += (size_t)n * hw;
    l.dice = o;   o += (size_t)n * l.nblk_d * 3;
    l.A = o;      o += (size_t)(n < CL_CH ? n : CL_CH) * hw * 9;
    l.pp = o;     o += (size_t)n * l.nblk_p * CL_NP;
    l.pf = o;     o += (size_t)l.nchunk * hw * 8;
    l.total = o;
    return l;
}

template <typename T>
int cl_check(const char* what, const ClArgs<T>& a) {
    UNI_REQUIRE(a.n > 0 && a.H > 0 && a.W > 0, "%s: empty problem n=%d H8=%d W8=%d", what, a.n, a.H, a.W);
    UNI_REQUIRE(a.r >= 1 && a.r <= 16, "%s: up_rate %d unsupported (1..16)", what, a.r);
    UNI_REQUIRE(a.ldp >= CL_NP, "%s: ldp %d < 169", what, a.ldp);
    UNI_REQUIRE(a.n <= 65535, "%s: more than 65535 instances", what);
    UNI_REQUIRE((size_t)a.H * a.W * a.r * a.r < (size_t)1 << 30, "%s: map too large", what);
    const size_t need = cl_layout(a.n, a.H, a.W, a.r).total * sizeof(T);
    UNI_REQUIRE(a.ws && ((uintptr_t)a.ws & 7) == 0 && a.ws_bytes >= need, "%s: workspace %zu < %zu bytes or misaligned", what, a.ws_bytes, need);
    return 0;
}

}  // namespace

size_t condinst_loss_workspace_bytes(int n, int H, int W, int r) {
    if (n <= 0 || H <= 0 || W <= 0 || r < 1 || r > 16 || n > 65535) return 0;
    if ((size_t)H * W * r * r >= (size_t)1 << 30) return 0;          // the shapes cl_check refuses: H * W stays inside int below
    return cl_layout(n, H, W, r).total * sizeof(float);
}

template <typename T>
int launch_condinst_loss_fwd(const ClArgs<T>& a, T* loss, T* sums, hipStream_t s) {
    if (int rc = cl_check("condinst_loss_fwd", a)) return rc;
    const CLLayout l = cl_layout(a.n, a.H, a.W, a.r);
    T* ws = reinterpret_cast<T*>(a.ws);
    const int hw = a.H * a.W;
    hipLaunchKernelGGL(cl_mlp_kernel<T>, dim3(cdiv(hw, 256), a.n), dim3(256), 0, s, a.mf, a.params, a.ldp, a.loc, a.lvl, hw, a.W, ws + l.logits);
    hipLaunchKernelGGL(cl_dice_kernel<T>, dim3(l.nblk_d, cdiv(a.n, CL_IC)), dim3(256), 0, s, a.um, ws + l.logits, a.gt, ws + l.dice, a.n, a.H, a.W,
                       a.r, l.PX, l.nblk_d);
    hipLaunchKernelGGL(cl_dice_final<T>, dim3(a.n), dim3(256), 0, s, ws + l.dice, l.nblk_d, sums, loss);
    return 0;
}

template <typename T>
int launch_condinst_loss_bwd(const ClArgs<T>& a, const T* sums, const T* gout, T* gmf, T* gum, T* gpar, hipStream_t s) {
    if (int rc = cl_check("condinst_loss_bwd", a)) return rc;
    if (!gmf && !gum && !gpar) return 0;
    const CLLayout l = cl_layout(a.n, a.H, a.W, a.r);
    T* ws = reinterpret_cast<T*>(a.ws);
    const int n = a.n, hw = a.H * a.W, want_dl = (gmf || gpar) ? 1 : 0;
    hipLaunchKernelGGL(cl_mlp_kernel<T>, dim3(cdiv(hw, 256), n), dim3(256), 0, s, a.mf, a.params, a.ldp, a.loc, a.lvl, hw, a.W, ws + l.logits);
    for (int c0 = 0; c0 < n; c0 += CL_CH) {
        const int cnt = n - c0 < CL_CH ? n - c0 : CL_CH;
        hipLaunchKernelGGL(cl_du_kernel<T>, dim3(l.nblk_d), dim3(256), 0, s, a.um, ws + l.logits, a.gt, sums, gout, ws + l.A, gum, c0, cnt, a.H, a.W,
                           a.r, l.PX, want_dl);
        if (want_dl) hipLaunchKernelGGL(cl_gather_kernel<T>, dim3(cdiv(hw, 256), cnt), dim3(256), 0, s, ws + l.A, ws + l.dL, c0, a.H, a.W);
    }
    if (gpar) {
        hipLaunchKernelGGL(cl_dparams_kernel<T>, dim3(l.nblk_p, n, 2), dim3(256), 0, s, a.mf, a.params, a.ldp, a.loc, a.lvl, ws + l.dL, hw, a.W,
                           ws + l.pp, l.nblk_p);
        hipLaunchKernelGGL(cl_dparams_final<T>, dim3(n), dim3(256), 0, s, ws + l.pp, l.nblk_p, gpar, a.ldp);
    }
    if (gmf) {
        hipLaunchKernelGGL(cl_dfeat_kernel<T>, dim3(cdiv(hw, CL_FB), l.nchunk), dim3(CL_FB), 0, s, a.mf, a.params, a.ldp, a.loc, a.lvl, ws + l.dL, n,
                           hw, a.W, ws + l.pf);
        hipLaunchKernelGGL(cl_dfeat_final<T>, dim3(cdiv(hw * 8, 256)), dim3(256), 0, s, ws + l.pf, l.nchunk, hw, gmf);
    }
    return 0;
}

template int launch_condinst_loss_fwd<float>(const ClArgs<float>&, float*, float*, hipStream_t);
template int launch_condinst_loss_fwd<double>(const ClArgs<double>&, double*, double*, hipStream_t);
template int launch_condinst_loss_bwd<float>(const ClArgs<float>&, const float*, const float*, float*, float*, float*, hipStream_t);
template int launch_condinst_loss_bwd<double>(const ClArgs<double>&, const double*, const double*, double*, double*, double*, hipStream_t);
