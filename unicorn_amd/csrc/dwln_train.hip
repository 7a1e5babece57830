// Depthwise 7x7 + bias + LayerNorm(C) for TRAINING (convnext.py:32-33,43-45): forward with per-pixel statistics and a recomputing, deterministic
// backward, fp32 and fp64.  x, y, grad_y, grad_x dense [B][H][W][C], weight [49][C] (the layout of uni_dwconv7_ln_ex), stats [B H W][2] = mean, rstd.
//
//   dwln_conv_kernel<MODE 0>  forward: u = conv(x) + b in registers, two-pass mean / variance over C, y and the statistics
//   dwln_conv_kernel<MODE 1>  backward pass A: u recomputed, xhat from the saved statistics, du -> workspace, per-block dgamma / dbeta partials
//   dwln_conv_kernel<MODE 2>  backward pass B (data): dx = conv(du) with the flipped window
//   dwln_dw_kernel            backward pass B (weights): one channel per lane, the 7x7 window of x and the 49 + 1 sums in registers while the
//                             wave walks a strip of one row; the four waves of a block are added through LDS -> per-block partials
//   dwln_reduce_kernel        partials -> dw [49][C], db, dgamma, dbeta: rows in ascending order, double accumulation (train_ops.h, shared
//                             with lncf_train.hip)
//
// The three conv modes share one mapping: a lane owns 4 consecutive channels (16-byte loads, coalesced over C) of a strip of PXT pixels of one
// row; the C / 4 lanes of a strip are whole waves (`slot`), so a sum over C is a wave butterfly plus the slot's waves through LDS in ascending order.
// A row of the window that lies outside the map is skipped and a column outside it is loaded as zero: rows are addressed inside the strip's own
// image only, so nothing of a neighbouring image enters a halo.  Every output element has one writer, no atomics: bitwise reproducible.
// Element offsets are 64-bit; pixel and strip indices are int (B H W < 2^31 is required).
#include "kernels.h"
#include "train_ops.h"

template <typename T>
using dv4 = T __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ dv4<T> dv4_splat(T s) {
    dv4<T> r = {s, s, s, s};
    return r;
}
template <typename T>
__device__ __forceinline__ T dv4_sum(dv4<T> v) {
    return (v[0] + v[1]) + (v[2] + v[3]);
}

template <typename T>
struct DwlnK {                                  // kernel arguments (by value)
    const T* in;                                // x (modes 0, 1) or du (mode 2)
    const T *w, *bias, *gamma, *beta, *gy, *stats_in;
    T *out, *stats_out, *part;
    T eps;
    int H, W, C, CG, CGp, NS, segs, nstrips, need_du, need_gb;
};

// acc[i] += sum over the window of w[ky][kx] * in[pixel (y + ky - 3, x0 + i + kx - 3)], channels c .. c + 3.  FLIP: the window of the data gradient.
template <typename T, int PXT, bool FLIP>
__device__ __forceinline__ void dwln_conv_strip(const T* __restrict__ in, const T* __restrict__ w, int H, int W, int C, int row, int y, int x0,
                                                int c, dv4<T> (&acc)[PXT]) {
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
        const int yy = y + ky - 3;
        if (yy < 0 || yy >= H) continue;        // uniform over the slot's waves
        dv4<T> wr[7];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const int t = ky * 7 + kx;
            wr[kx] = *reinterpret_cast<const dv4<T>*>(w + (size_t)(FLIP ? 48 - t : t) * C + c);
        }
        const T* rp = in + (size_t)(row + ky - 3) * W * C + c;
#pragma unroll
        for (int j = 0; j < PXT + 6; ++j) {
            const int xx = x0 + j - 3;
            dv4<T> v = dv4_splat<T>(0);
            if (xx >= 0 && xx < W) v = *reinterpret_cast<const dv4<T>*>(rp + (size_t)xx * C);
#pragma unroll
            for (int i = 0; i < PXT; ++i)
                if (j - i >= 0 && j - i < 7) acc[i] += wr[j - i] * v;
        }
    }
}

// sums of NV values over the lanes of one slot (wps whole waves, waves slot * wps ...); every lane of the slot gets the totals.  One
// __syncthreads when wps > 1: every thread of the block calls it.
template <typename T, int NV>
__device__ __forceinline__ void dwln_slot_sum(T (&v)[NV], T* sm, int wps, int slot) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (wps == 1) return;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) sm[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        T r = 0;
        for (int k = 0; k < wps; ++k) r += sm[(slot * wps + k) * NV + i];
        v[i] = r;
    }
}

extern __shared__ double dwln_dyn_lds[];

template <typename T, int PXT, int MODE>
__global__ __launch_bounds__(512) void dwln_conv_kernel(DwlnK<T> p) {
    __shared__ T sm1[8 * 2 * PXT];
    __shared__ T sm2[8 * 2 * PXT];
    const int tid = threadIdx.x;
    const int wps = p.CGp >> 6;
    const int slot = tid / p.CGp, cg = tid - slot * p.CGp;
    const bool cok = cg < p.CG;
    const int c = cg * 4, C = p.C, W = p.W;
    dv4<T> gam = dv4_splat<T>(0), bet = gam, bia = gam, dg = gam, db = gam;
    if (cok && MODE != 2) {
        gam = *reinterpret_cast<const dv4<T>*>(p.gamma + c);
        bia = *reinterpret_cast<const dv4<T>*>(p.bias + c);
        if (MODE == 0) bet = *reinterpret_cast<const dv4<T>*>(p.beta + c);
    }
    const T invC = T(1) / T(C);
    const int nsb = (p.nstrips + p.NS - 1) / p.NS;
    int it = 0;
    for (int sb = blockIdx.x; sb < nsb; sb += gridDim.x, ++it) {
        const int strip = sb * p.NS + slot;
        const bool live = strip < p.nstrips && cok;
        const int row = strip / p.segs, x0 = (strip - row * p.segs) * PXT, y = row % p.H;
        const size_t pix0 = (size_t)row * W + x0;
        dv4<T> acc[PXT];
#pragma unroll
        for (int i = 0; i < PXT; ++i) acc[i] = bia;
        if (live) dwln_conv_strip<T, PXT, MODE == 2>(p.in, p.w, p.H, W, C, row, y, x0, c, acc);
        if (MODE == 2) {
            if (live) {
#pragma unroll
                for (int i = 0; i < PXT; ++i)
                    if (x0 + i < W) *reinterpret_cast<dv4<T>*>(p.out + (pix0 + i) * C + c) = acc[i];
            }
            continue;
        }
        if (MODE == 0) {
            T s[PXT];
#pragma unroll
            for (int i = 0; i < PXT; ++i) s[i] = cok ? dv4_sum(acc[i]) : T(0);
            dwln_slot_sum<T, PXT>(s, sm1, wps, slot);
            T q[PXT];
#pragma unroll
            for (int i = 0; i < PXT; ++i) {
                s[i] *= invC;
                acc[i] -= dv4_splat(s[i]);
                q[i] = cok ? dv4_sum(acc[i] * acc[i]) : T(0);
            }
            dwln_slot_sum<T, PXT>(q, sm2, wps, slot);
            if (live) {
#pragma unroll
                for (int i = 0; i < PXT; ++i) {
                    if (x0 + i >= W) continue;
                    const T rstd = T(1) / sqrt(q[i] * invC + p.eps);
                    *reinterpret_cast<dv4<T>*>(p.out + (pix0 + i) * C + c) = acc[i] * dv4_splat(rstd) * gam + bet;
                    if (cg == 0) {
                        p.stats_out[(pix0 + i) * 2] = s[i];
                        p.stats_out[(pix0 + i) * 2 + 1] = rstd;
                    }
                }
            }
        }
        if (MODE == 1) {
            T rstd[PXT];
            dv4<T> gg[PXT];
            T r[2 * PXT];
#pragma unroll
            for (int i = 0; i < PXT; ++i) {
                T mean = 0;
                rstd[i] = 0;
                dv4<T> g = dv4_splat<T>(0);
                if (live && x0 + i < W) {
                    mean = p.stats_in[(pix0 + i) * 2];
                    rstd[i] = p.stats_in[(pix0 + i) * 2 + 1];
                    g = *reinterpret_cast<const dv4<T>*>(p.gy + (pix0 + i) * C + c);
                }
                acc[i] = (acc[i] - dv4_splat(mean)) * dv4_splat(rstd[i]);      // xhat
                dg += g * acc[i];
                db += g;
                gg[i] = g * gam;
                r[i] = dv4_sum(gg[i]);
                r[PXT + i] = dv4_sum(gg[i] * acc[i]);
            }
            if (p.need_du) {
                dwln_slot_sum<T, 2 * PXT>(r, (it & 1) ? sm2 : sm1, wps, slot);
                if (live) {
#pragma unroll
                    for (int i = 0; i < PXT; ++i)
                        if (x0 + i < W)
                            *reinterpret_cast<dv4<T>*>(p.out + (pix0 + i) * C + c) =
                                dv4_splat(rstd[i]) * (gg[i] - dv4_splat(r[i] * invC) - acc[i] * dv4_splat(r[PXT + i] * invC));
                }
            }
        }
    }
    if (MODE == 1 && p.need_gb) {                // the block's slots in ascending order -> one row of partials [2][C]
        T* sg = reinterpret_cast<T*>(dwln_dyn_lds);
        for (int s = 0; s < p.NS; ++s) {
            if (slot == s && cok) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sg[c + j] = (s ? sg[c + j] : T(0)) + dg[j];
                    sg[C + c + j] = (s ? sg[C + c + j] : T(0)) + db[j];
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < 2 * C; i += blockDim.x) p.part[(size_t)blockIdx.x * 2 * C + i] = sg[i];
    }
}

// dw[ky][kx][c] = sum_p du[p][c] x[p + (ky - 3, kx - 3)][c], db[c] = sum_p du[p][c]: lane = channel, wave = one strip of <= slen pixels of one row.
// win[ky][slot] holds the 7 x 7 window of x; a step loads the 7 values of the entering column into the slot of the leaving one (the step loop is
// unrolled by 7, so every slot index is a constant).  part [gridDim.x][50][C].
template <typename T>
__global__ __launch_bounds__(256) void dwln_dw_kernel(const T* __restrict__ x, const T* __restrict__ du, T* __restrict__ part, int H, int W, int C,
                                                      int slen, int segs, int nstrips) {
    __shared__ T sm[50 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool cok = c < C;
    const int strip = blockIdx.x * 4 + wave;
    T acc[49], accb = 0;
#pragma unroll
    for (int k = 0; k < 49; ++k) acc[k] = 0;
    if (strip < nstrips && cok) {
        const int row = strip / segs, x0 = (strip - row * segs) * slen, y = row % H;
        const int len = min(slen, W - x0);
        const T* xr[7];
        bool rok[7];
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            rok[ky] = y + ky - 3 >= 0 && y + ky - 3 < H;
            xr[ky] = x + (size_t)(rok[ky] ? row + ky - 3 : row) * W * C + c;
        }
        const T* dr = du + (size_t)row * W * C + c;
        T win[7][7];
#pragma unroll
        for (int kx = 0; kx < 6; ++kx) {
            const int xx = x0 + kx - 3;
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) win[ky][kx] = (rok[ky] && xx >= 0 && xx < W) ? xr[ky][(size_t)xx * C] : T(0);
        }
        for (int s0 = 0; s0 < len; s0 += 7) {
#pragma unroll
            for (int ss = 0; ss < 7; ++ss) {
                const int s = s0 + ss;
                if (s < len) {
                    const int xn = x0 + s + 3;
#pragma unroll
                    for (int ky = 0; ky < 7; ++ky) win[ky][(ss + 6) % 7] = (rok[ky] && xn < W) ? xr[ky][(size_t)xn * C] : T(0);
                    const T d = dr[(size_t)(x0 + s) * C];
#pragma unroll
                    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 7; ++kx) acc[ky * 7 + kx] += d * win[ky][(ss + kx) % 7];
                    accb += d;
                }
            }
        }
    }
    for (int w = 0; w < 4; ++w) {                // the four waves in ascending order
        if (wave == w) {
#pragma unroll
            for (int k = 0; k < 49; ++k) sm[k * 64 + lane] = (w ? sm[k * 64 + lane] : T(0)) + acc[k];
            sm[49 * 64 + lane] = (w ? sm[49 * 64 + lane] : T(0)) + accb;
        }
        __syncthreads();
    }
    if (cok)
        for (int k = wave; k < 50; k += 4) part[((size_t)blockIdx.x * 50 + k) * C + c] = sm[k * 64 + lane];
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t dwln_train_workspace_bytes(int B, int H, int W, int C) { return dwln_plan_workspace_bytes(B, H, W, C); }

template <typename T>
static int dwln_check(const char* what, const DwlnArgs<T>& a, DwlnPlan& q) {
    if (!dwln_plan(a.B, a.H, a.W, a.C, sizeof(T) == 8, q)) return train_shape_refused(what, a.B, a.H, a.W, a.C);
    UNI_REQUIRE(aligned16(a.x) && aligned16(a.w) && aligned16(a.bias) && aligned16(a.gamma), "%s: a pointer is not 16-byte aligned", what);
    return 0;
}

template <typename T>
int launch_dwln_train_fwd(const DwlnArgs<T>& a, T* y, T* stats, hipStream_t s) {
    constexpr int PXT = DwlnPx<T>::value;
    const char* tn = train_ename(0, sizeof(T) == 8);
    DwlnPlan q;
    if (int rc = dwln_check("dwln_train_fwd", a, q)) return rc;
    UNI_REQUIRE(aligned16(a.beta) && aligned16(y) && aligned16(stats), "dwln_train_fwd: a pointer is not 16-byte aligned");
    UNI_REQUIRE(a.eps > 0, "dwln_train_fwd: eps %g is not positive", a.eps);
    DwlnK<T> k{a.x, a.w, a.bias, a.gamma, a.beta, nullptr, nullptr, y, stats, nullptr, (T)a.eps,
               a.H, a.W, a.C, q.CG, q.CGp, q.NS, q.segs, q.nstrips, 0, 0};
    char cls[48] = "";
    if (train_tracing()) dwln_plan_class(q, tn, cls, sizeof(cls));
    uni_variant_note("dwln_train fwd%s", cls);
    hipLaunchKernelGGL((dwln_conv_kernel<T, PXT, 0>), dim3(q.nsb), dim3(q.threads), 0, s, k);
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_dwln_train_bwd(const DwlnArgs<T>& a, const T* stats, const T* gy, T* gx, T* gw, T* gb, T* ggamma, T* gbeta, void* ws, size_t ws_bytes,
                          hipStream_t s) {
    constexpr int PXT = DwlnPx<T>::value;
    const char* tn = train_ename(0, sizeof(T) == 8);
    DwlnPlan q;
    if (int rc = dwln_check("dwln_train_bwd", a, q)) return rc;
    UNI_REQUIRE((gw != nullptr) == (gb != nullptr) && (ggamma != nullptr) == (gbeta != nullptr),
                "dwln_train_bwd: grad_weight / grad_bias and grad_ln_weight / grad_ln_bias come in pairs");
    const size_t need = dwln_train_workspace_bytes(a.B, a.H, a.W, a.C) * (sizeof(T) / 4);
    UNI_REQUIRE(ws_bytes >= need, "dwln_train_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    UNI_REQUIRE(aligned16(stats) && aligned16(gy) && aligned16(gx) && aligned16(gw) && aligned16(ws),
                "dwln_train_bwd: a pointer is not 16-byte aligned");
    const bool need_du = gx || gw, need_gb = ggamma != nullptr;
    if (!need_du && !need_gb) return 0;
    T* du = reinterpret_cast<T*>(ws);
    T* part_a = du + q.off_pa;
    T* part_b = du + q.off_pb;
    DwlnK<T> k{a.x, a.w, a.bias, a.gamma, nullptr, gy, stats, du, nullptr, part_a, T(0),
               a.H, a.W, a.C, q.CG, q.CGp, q.NS, q.segs, q.nstrips, (int)need_du, (int)need_gb};
    char cls[48] = "";
    if (train_tracing()) dwln_plan_class(q, tn, cls, sizeof(cls));
    uni_variant_note("dwln_train bwd_a%s du=%d gb=%d", cls, (int)need_du, (int)need_gb);
    hipLaunchKernelGGL((dwln_conv_kernel<T, PXT, 1>), dim3(q.RA), dim3(q.threads), need_gb ? q.lds_a : 0, s, k);
    if (gx) {
        DwlnK<T> kx{du, a.w, nullptr, nullptr, nullptr, nullptr, nullptr, gx, nullptr, nullptr, T(0),
                    a.H, a.W, a.C, q.CG, q.CGp, q.NS, q.segs, q.nstrips, 0, 0};
        uni_variant_note("dwln_train bwd_dx%s", cls);
        hipLaunchKernelGGL((dwln_conv_kernel<T, PXT, 2>), dim3(q.nsb), dim3(q.threads), 0, s, kx);
    }
    if (gw) {
        uni_variant_note("dwln_train bwd_dw<%s> slen=%d", tn, q.slen);
        hipLaunchKernelGGL((dwln_dw_kernel<T>), dim3(q.RB, q.NCT), dim3(256), 0, s, a.x, (const T*)du, part_b, a.H, a.W, a.C, q.slen, q.segs_w,
                           q.nstrips_w);
    }
    DwlnRJob jw{part_b, gw, gb, q.RB, 50 * a.C, 49 * a.C, gw ? cdiv(50 * a.C, 64) : 0};
    DwlnRJob jg{part_a, ggamma, gbeta, q.RA, 2 * a.C, a.C, need_gb ? cdiv(2 * a.C, 64) : 0};
    if (jw.blocks + jg.blocks) {
        uni_variant_note("dwln_train reduce<%s> dw=%d gb=%d", tn, gw != nullptr, (int)need_gb);
        hipLaunchKernelGGL((dwln_reduce_kernel<T>), dim3(jw.blocks + jg.blocks), dim3(256), 0, s, jw, jg);
    }
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template int launch_dwln_train_fwd<float>(const DwlnArgs<float>&, float*, float*, hipStream_t);
template int launch_dwln_train_fwd<double>(const DwlnArgs<double>&, double*, double*, hipStream_t);
template int launch_dwln_train_bwd<float>(const DwlnArgs<float>&, const float*, const float*, float*, float*, float*, float*, float*, void*, size_t,
                                          hipStream_t);
template int launch_dwln_train_bwd<double>(const DwlnArgs<double>&, const double*, const double*, double*, double*, double*, double*, double*, void*,
                                           size_t, hipStream_t);
