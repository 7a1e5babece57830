// The four detection losses of the head (unicorn/models/unicorn_head_mask.py:646-745 of get_losses, identically unicorn_head.py:484-681,
// with IOUloss of unicorn/models/losses.py:15-36, loss_type "iou") for a whole batch, forward and backward, fp32 and fp64, fed by the
// device-side results of uni_simota_assign: two launches each way whatever B, A, M, C and the foreground counts, no host read.
//
//   obj   sum over ALL anchors        bce(obj_logit, fg)
//   iou   sum over fg anchors         1 - iou(pred, gt[matched])^2;  edges = centre -+ size / 2, tl = max, br = min, en = (tl < br) on both
//                                     axes, area_i = (br - tl).prod * en, iou = area_i / (area_p + area_g - area_i + 1e-16)
//   cls   sum over fg anchors x C     bce(cls_logit_c, c == class ? matched_iou : 0)
//   l1    sum over fg anchors x 4     |origin - t|,  t = (gx / s - x_shift, gy / s - y_shift, log(gw / s + 1e-8), log(gh / s + 1e-8))
//   bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|));  every sum / max(sum_b num_fg[b], 1), the iou one times reg_weight.
//
//   hl_fwd_kernel     block = 256 anchors of one image, thread = anchor: the objectness term of every anchor, the box and L1 terms of a
//                     foreground anchor (these two in double in both precisions: the foreground is sparse).  The class term: the wave ballots its foreground lanes and spreads the classes of each such anchor
//                     over its 64 lanes (coalesced reads of the class logits; a wave without foreground reads none).  The four sums are
//                     accumulated in double in both precisions and leave the block as one partial each, summed in a fixed tree.
//   hl_final_kernel   one block: the partials in a fixed order, sum num_fg, sum num_gt -> out[5] (the last one n / max(sum num_gt, 1))
//   hl_count_kernel   one block: n = max(sum num_fg, 1) into the workspace (the backward keeps nothing from the forward)
//   hl_bwd_kernel     block = 256 anchors, thread = anchor: the five leading gradient columns and grad_origin of its anchor (recomputed from
//                     the inputs); the columns go through LDS, and the block then writes its 256 x (5 + C) tile of grad_outputs row by row
//                     with consecutive lanes on consecutive addresses -- zeros for the class columns of background anchors, which read
//                     nothing.  One writer per element.
//
// No atomics at all; two runs give the same bits.  The file is compiled without FMA contraction so that the fp64 form rounds like the
// reference's separate tensor operations.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int HL_TB = 256;

bool hl_shape_ok(int B, int A, int M, int C) {
    return B >= 1 && B <= 65535 && A >= 1 && A < (1 << 24) && M >= 0 && M <= 1024 && C >= 1 && C <= 256;
}
size_t hl_ws_bytes(int B, int A) {      // [B][ceil(A / 256)][4] double partial sums; the backward uses the first 8 bytes
    return (((size_t)B * cdiv(A, HL_TB) * 4 * sizeof(double)) + 255) & ~(size_t)255;
}

__device__ __forceinline__ float hl_exp(float x) { return expf(x); }
__device__ __forceinline__ double hl_exp(double x) { return exp(x); }
__device__ __forceinline__ float hl_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double hl_log1p(double x) { return log1p(x); }
template <typename T>
__device__ __forceinline__ T hl_abs(T x) { return x < 0 ? -x : x; }
template <typename T>
__device__ __forceinline__ T hl_bce(T x, T t) { return (x > 0 ? x : (T)0) - x * t + hl_log1p(hl_exp(-hl_abs(x))); }
template <typename T>
__device__ __forceinline__ T hl_sigmoid(T x) { return (T)1 / ((T)1 + hl_exp(-x)); }

// the matched box of a foreground anchor: a matched_gt outside 0..M-1 and a class outside 0..C-1 are clamped
// The box, IoU and L1 lines of a foreground anchor run in double in both precisions: the foreground is sparse (at most ten anchors per
// box), so this costs nothing, and the fp32 form then carries only the rounding of its inputs and of its results.
struct HlBox { double gx, gy, gw, gh; int cls; };
template <typename T>
__device__ __forceinline__ HlBox hl_box(const T* __restrict__ labels, int b, int M, int g, int C) {
    const T* lab = labels + ((size_t)b * M + min(max(g, 0), M - 1)) * 5;
    HlBox q;
    q.cls = min(max((int)lab[0], 0), C - 1);
    q.gx = lab[1];
    q.gy = lab[2];
    q.gw = lab[3];
    q.gh = lab[4];
    return q;
}

// losses.py:15-36 for one pair; the intersection's edges and the flags of the winning side are kept for the backward
struct HlIou { double iou, wi, hi, en, den; double dl, dt, dr, db; };      // d*: d edge_of_intersection / d edge_of_prediction (1, 0.5 at a tie, 0)
__device__ __forceinline__ HlIou hl_iou(double px, double py, double pw, double ph, const HlBox& q) {
    typedef double T;
    const T pl = px - pw / 2, pt = py - ph / 2, pr = px + pw / 2, pb = py + ph / 2;
    const T gl = q.gx - q.gw / 2, gt = q.gy - q.gh / 2, gr = q.gx + q.gw / 2, gb = q.gy + q.gh / 2;
    const T tlx = pl > gl ? pl : gl, tly = pt > gt ? pt : gt, brx = pr < gr ? pr : gr, bry = pb < gb ? pb : gb;
    HlIou r;
    r.en = (tlx < brx ? (T)1 : (T)0) * (tly < bry ? (T)1 : (T)0);
    r.wi = brx - tlx;
    r.hi = bry - tly;
    const T area_i = r.wi * r.hi * r.en;
    r.den = pw * ph + q.gw * q.gh - area_i + (T)1e-16;
    r.iou = area_i / r.den;
    r.dl = pl > gl ? (T)1 : (pl == gl ? (T)0.5 : (T)0);
    r.dt = pt > gt ? (T)1 : (pt == gt ? (T)0.5 : (T)0);
    r.dr = pr < gr ? (T)1 : (pr == gr ? (T)0.5 : (T)0);
    r.db = pb < gb ? (T)1 : (pb == gb ? (T)0.5 : (T)0);
    return r;
}

// get_l1_target :747-752
__device__ __forceinline__ void hl_l1_target(const HlBox& q, double s, double xs, double ys, double t[4]) {
    t[0] = q.gx / s - xs;
    t[1] = q.gy / s - ys;
    t[2] = log(q.gw / s + 1e-8);
    t[3] = log(q.gh / s + 1e-8);
}

template <typename T>
__global__ void __launch_bounds__(HL_TB)
hl_fwd_kernel(HlIn<T> p, double* __restrict__ part) {
    __shared__ double sm[HL_TB / 64];
    const int a = blockIdx.x * HL_TB + threadIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
    double s_iou = 0, s_obj = 0, s_cls = 0, s_l1 = 0;
    bool isfg = false;
    int cls = 0;
    T tiou = 0;
    if (a < p.A) {
        const size_t i = (size_t)b * p.A + a;
        const T* o = p.outputs + i * p.ld;
        isfg = p.fg[i] != 0 && p.M > 0;
        s_obj = (double)hl_bce<T>(o[4], isfg ? (T)1 : (T)0);
        if (isfg) {
            const HlBox q = hl_box<T>(p.labels, b, p.M, p.mg[i], p.C);
            cls = q.cls;
            tiou = p.miou[i];
            const HlIou r = hl_iou(o[0], o[1], o[2], o[3], q);
            s_iou = 1.0 - r.iou * r.iou;
            if (p.origin) {
                const T* og = p.origin + i * p.ldo;
                double t[4];
                hl_l1_target(q, p.st[a], p.xs[a], p.ys[a], t);
#pragma unroll
                for (int k = 0; k < 4; ++k) s_l1 += hl_abs<double>((double)og[k] - t[k]);
            }
        }
    }
    // the class term: every foreground anchor of the wave in turn, its classes over the 64 lanes
    unsigned long long m = __ballot(isfg);
    const size_t wave0 = (size_t)b * p.A + (size_t)(blockIdx.x * HL_TB + (threadIdx.x & ~63));
    while (m) {
        const int j = __ffsll(m) - 1;
        m &= m - 1;
        const int cj = __shfl(cls, j, 64);
        const T tj = __shfl(tiou, j, 64);
        const T* oc = p.outputs + (wave0 + j) * p.ld + 5;
        T l = 0;
        for (int c = lane; c < p.C; c += 64) l += hl_bce<T>(oc[c], c == cj ? tj : (T)0);
        s_cls += (double)l;
    }
    double* dst = part + ((size_t)b * gridDim.x + blockIdx.x) * 4;
    const double r0 = block_sum<HL_TB>(s_iou, sm), r1 = block_sum<HL_TB>(s_obj, sm), r2 = block_sum<HL_TB>(s_cls, sm), r3 = block_sum<HL_TB>(s_l1, sm);
    if (threadIdx.x == 0) {
        dst[0] = r0;
        dst[1] = r1;
        dst[2] = r2;
        dst[3] = r3;
    }
}

__device__ __forceinline__ long long hl_count(const int* __restrict__ v, int B, int hi, long long* sm) {      // sum of clamp(v[b], 0, hi)
    long long s = 0;
    for (int b = threadIdx.x; b < B; b += HL_TB) s += min(max(v[b], 0), hi);
    return block_sum<HL_TB>(s, sm);
}

template <typename T>
__global__ void __launch_bounds__(HL_TB)
hl_final_kernel(const double* __restrict__ part, size_t nblocks, const int* __restrict__ num_fg, const int* __restrict__ num_gt, int B, int A,
                int M, double reg_weight, T* __restrict__ out) {
    __shared__ double sm[HL_TB / 64];
    __shared__ long long si[HL_TB / 64];
    double s[4] = {0, 0, 0, 0};
    for (size_t k = threadIdx.x; k < nblocks; k += HL_TB)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += part[k * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = block_sum<HL_TB>(s[q], sm);
    const long long nfg = hl_count(num_fg, B, A, si), ngt = hl_count(num_gt, B, M, si);
    if (threadIdx.x == 0) {
        const double n = (double)(nfg > 1 ? nfg : 1);
        out[0] = (T)((T)reg_weight * (T)(s[0] / n));
        out[1] = (T)(s[1] / n);
        out[2] = (T)(s[2] / n);
        out[3] = (T)(s[3] / n);
        out[4] = (T)(n / (double)(ngt > 1 ? ngt : 1));      // the reference divides its clamped num_fg: 1.0 with no box at all
    }
}

__global__ void __launch_bounds__(HL_TB)
hl_count_kernel(const int* __restrict__ num_fg, int B, int A, long long* __restrict__ n_out) {
    __shared__ long long si[HL_TB / 64];
    const long long nfg = hl_count(num_fg, B, A, si);
    if (threadIdx.x == 0) *n_out = nfg > 1 ? nfg : 1;
}

template <typename T>
__global__ void __launch_bounds__(HL_TB)
hl_bwd_kernel(HlIn<T> p, const T* __restrict__ gout, const long long* __restrict__ n_in, double reg_weight, T* __restrict__ g_out, int ldg,
              T* __restrict__ g_org) {
    __shared__ T s_head[HL_TB][5];
    __shared__ T s_iou[HL_TB];
    __shared__ int s_cls[HL_TB];
    const int t = threadIdx.x, a0 = blockIdx.x * HL_TB, a = a0 + t, b = blockIdx.y;
    const double n = (double)*n_in;
    const double k_iou = reg_weight * (double)gout[0] / n;
    const T k_obj = (T)((double)gout[1] / n), k_cls = (T)((double)gout[2] / n), k_l1 = (T)((double)gout[3] / n);
    if (a < p.A) {
        const size_t i = (size_t)b * p.A + a;
        const T* o = p.outputs + i * p.ld;
        const bool isfg = p.fg[i] != 0 && p.M > 0;
        T h[5] = {0, 0, 0, 0, (hl_sigmoid<T>(o[4]) - (isfg ? (T)1 : (T)0)) * k_obj};
        T go[4] = {0, 0, 0, 0};
        int cls = -1;
        T tiou = 0;
        if (isfg) {
            const HlBox q = hl_box<T>(p.labels, b, p.M, p.mg[i], p.C);
            cls = q.cls;
            tiou = p.miou[i];
            const double pw = o[2], ph = o[3];
            const HlIou r = hl_iou(o[0], o[1], pw, ph, q);
            // loss = 1 - iou^2, iou = I / D, D = P + G - I + eps, I = wi hi en
            const double d_iou = -2.0 * r.iou * k_iou;
            const double d_I = d_iou * (r.den + r.wi * r.hi * r.en) / (r.den * r.den);      // dI directly and through D
            const double d_P = -d_iou * (r.wi * r.hi * r.en) / (r.den * r.den);
            const double d_brx = d_I * r.hi * r.en, d_bry = d_I * r.wi * r.en;              // tl gets the negative
            const double d_pl = -d_brx * r.dl, d_pr = d_brx * r.dr, d_pt = -d_bry * r.dt, d_pb = d_bry * r.db;
            h[0] = (T)(d_pl + d_pr);
            h[1] = (T)(d_pt + d_pb);
            h[2] = (T)((d_pr - d_pl) / 2 + d_P * ph);
            h[3] = (T)((d_pb - d_pt) / 2 + d_P * pw);
            if (p.origin && g_org) {
                const T* og = p.origin + i * p.ldo;
                double tg[4];
                hl_l1_target(q, p.st[a], p.xs[a], p.ys[a], tg);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double d = (double)og[k] - tg[k];
                    go[k] = d > 0 ? k_l1 : (d < 0 ? -k_l1 : (T)0);
                }
            }
        }
        if (g_org) {
#pragma unroll
            for (int k = 0; k < 4; ++k) g_org[i * 4 + k] = go[k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) s_head[t][k] = h[k];
        s_iou[t] = tiou;
        s_cls[t] = cls;
    }
    if (!g_out) return;
    __syncthreads();
    // the block's tile of grad_outputs: rows a0 .. a0 + rows - 1, columns 0 .. 4 + C; the pitch padding is not touched
    const int rows = min(HL_TB, p.A - a0), W = 5 + p.C, total = rows * W;
    const T* in0 = p.outputs + ((size_t)b * p.A + a0) * p.ld;
    T* out0 = g_out + ((size_t)b * p.A + a0) * ldg;
    for (int e = t; e < total; e += HL_TB) {
        const int j = e / W, col = e - j * W;
        T v;
        if (col < 5) {
            v = s_head[j][col];
        } else {
            const int cj = s_cls[j];
            v = 0;
            if (cj >= 0) v = (hl_sigmoid<T>(in0[(size_t)j * p.ld + col]) - (col - 5 == cj ? s_iou[j] : (T)0)) * k_cls;
        }
        out0[(size_t)j * ldg + col] = v;
    }
}

template <typename T>
int hl_check(const HlArgs<T>& a, const char* what) {
    const HlIn<T>& p = a.in;
    UNI_REQUIRE(hl_shape_ok(a.B, p.A, p.M, p.C), "%s: shape B=%d A=%d M=%d C=%d outside 1 <= B <= 65535, 1 <= A < 2^24, 0 <= M <= 1024, 1 <= C <= 256",
                what, a.B, p.A, p.M, p.C);
    UNI_REQUIRE(p.ld >= 5 + p.C, "%s: ld_out %d < 5 + C = %d", what, p.ld, 5 + p.C);
    UNI_REQUIRE(!p.origin || p.ldo >= 4, "%s: ld_org %d < 4", what, p.ldo);
    const size_t need = hl_ws_bytes(a.B, p.A);
    UNI_REQUIRE(a.ws_bytes >= need, "%s: workspace %zu < %zu", what, a.ws_bytes, need);
    UNI_REQUIRE(((uintptr_t)a.ws & 7) == 0, "%s: workspace must be 8-byte aligned", what);
    return 0;
}

}  // namespace

size_t head_loss_workspace_bytes(int B, int A, int C) {
    if (!hl_shape_ok(B, A, 0, C)) return 0;
    return hl_ws_bytes(B, A);
}

template <typename T>
int launch_head_loss_fwd(const HlArgs<T>& a, T* out, hipStream_t s) {
    if (int rc = hl_check<T>(a, "head_loss_fwd")) return rc;
    const int ax = cdiv(a.in.A, HL_TB);
    double* part = reinterpret_cast<double*>(a.ws);
    hl_fwd_kernel<T><<<dim3(ax, a.B), HL_TB, 0, s>>>(a.in, part);
    hl_final_kernel<T><<<1, HL_TB, 0, s>>>(part, (size_t)ax * a.B, a.num_fg, a.num_gt, a.B, a.in.A, a.in.M, a.reg_weight, out);
    return 0;
}

template <typename T>
int launch_head_loss_bwd(const HlArgs<T>& a, const T* gout, T* g_out, int ldg, T* g_org, hipStream_t s) {
    if (int rc = hl_check<T>(a, "head_loss_bwd")) return rc;
    UNI_REQUIRE(!g_out || ldg >= 5 + a.in.C, "head_loss_bwd: ld_grad %d < 5 + C = %d", ldg, 5 + a.in.C);
    UNI_REQUIRE(!g_org || a.in.origin, "head_loss_bwd: grad_origin without origin_preds");
    if (!g_out && !g_org) return 0;
    long long* n = reinterpret_cast<long long*>(a.ws);
    hl_count_kernel<<<1, HL_TB, 0, s>>>(a.num_fg, a.B, a.in.A, n);
    hl_bwd_kernel<T><<<dim3(cdiv(a.in.A, HL_TB), a.B), HL_TB, 0, s>>>(a.in, gout, n, a.reg_weight, g_out, ldg, g_org);
    return 0;
}

template int launch_head_loss_fwd<float>(const HlArgs<float>&, float*, hipStream_t);
template int launch_head_loss_fwd<double>(const HlArgs<double>&, double*, hipStream_t);
template int launch_head_loss_bwd<float>(const HlArgs<float>&, const float*, float*, int, float*, hipStream_t);
template int launch_head_loss_bwd<double>(const HlArgs<double>&, const double*, double*, int, double*, hipStream_t);
