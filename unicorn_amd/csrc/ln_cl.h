// The LayerNorm over the channels of channels-last memory [B][H][W][C] for TRAINING, one kernel under lncf_train.hip (ops.layernorm_cf) and
// down_train.hip (ops.downsample_ln); fp32 (x / grad_x fp32, fp16 or bf16, converted in registers; all arithmetic fp32) and fp64.
//
//   ln_cl_kernel<T, XT, V, NV, MODE, IO>   a pixel belongs to G lanes of ONE wave (G a power of two, 1 .. 64); a lane owns NV vectors of V
//                                  consecutive channels (vector k of lane g = channels (k G + g) V ...; V = 4, or 8 for half x with
//                                  C % 8 == 0: 16-byte loads of x either way), so the row of a pixel is in registers, x is read once, the variance
//                                  is the second pass over registers and a sum over C is a butterfly over the G lanes: no LDS, no barrier.  A
//                                  block of four waves takes 256 / G pixels at once (C = 96: G = 8, NV = 3, 32 pixels).  lncf_plan
//                                  (train_plan.h, channels-last) picks V, NV and G.
//   MODE 0   forward: u = mean_c x, rstd = 1 / sqrt(mean_c (x - u)^2 + eps), stats_out [pixel][2] = u, rstd, then the output row
//            weight * (x - u) * rstd + bias.  Rebuild (stats_in given, where the policy allows it; uniform in the launch): the statistics are read
//            instead of computed and stats_out is not written; every other instruction is shared, so the row has the forward's bits.
//   MODE 1   backward: xhat = (x - u) * rstd, t = g * weight, grad_x = rstd * (t - mean_c t - xhat * mean_c (t * xhat)),
//            part[block][2][C] = the block's sums of g * xhat and of g -> dwln_reduce_kernel (train_ops.h)
//
// The policy IO, a second kernel argument by value, says where the output row (MODE 0) and the incoming gradient row g (MODE 1) of a pixel live:
//   static constexpr bool REBUILD                  may MODE 0 be given stats_in
//   static void place(io, pix, live, C, kept&, ea&)  kept = the pixel has such a row (live is pix < M; kept implies live), ea = its element offset.
//                                                  A pixel that is live and not kept writes its statistics and nothing else in MODE 0; in MODE 1
//                                                  it is not read, adds nothing to the sums and gets exact zeros in grad_x
//   static void store<V>(io, off, r)               V elements of the output row at element offset off
//   static void load<V>(io, off, r)                V elements of the incoming gradient row
// Two things about the form are load-bearing for the register allocation (profiles/ln_cl_shared.txt has the tables).  The body is the
// __global__ function itself: as an inlined function under one thin kernel per operator it takes more registers in nearly every
// instantiation.  And the policy's functions are static and take the policy BY VALUE: as member functions they reach its fields through
// `this`, a generic pointer to the kernel argument's private copy, and the forward of the downsample policy then holds the pixel's place
// across the statistics (1 .. 4 VGPRs more, one occupancy step at fp32 NV = 3).
//
// C is the kernel's one copy of the channel count (p.C): a policy gets it, it does not carry one of its own.
//
// Every output element has one writer, no atomics, fixed summation orders: bitwise reproducible.  Element offsets are 64-bit; pixel and group
// indices fit 32 bits (B H W < 2^31 is required).
#pragma once
#include "train_ops.h"

// sum over the G lanes of a pixel (G a power of two, the lanes are consecutive): xor butterfly, every lane gets the total
template <typename T>
__device__ __forceinline__ T ln_group_sum(T v, int G) {
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T>
struct LnClK {                                  // kernel arguments (by value)
    const void* x;
    const T *w, *bias, *stats_in;
    T* stats_out;
    void* gx;                                   // the element type of x
    T* part;
    T eps;
    int C;
    long long M;                                // B H W
};

extern __shared__ double ln_cl_dyn_lds[];

template <typename T, typename XT, int V, int NV, int MODE, typename IO>
__global__ __launch_bounds__(256) void ln_cl_kernel(LnClK<T> p, IO io, int G, int lgG, unsigned ngroups) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = tid & (G - 1), slot = tid >> lgG, PPB = 256 >> lgG;
    const int C = p.C, nvec = C / V;
    const T cnt = T(C);
    bool vok[NV];
    int c[NV];
    T wv[NV][V], bv[NV][V], dg[NV][V], db[NV][V];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int vec = k * G + g;
        vok[k] = vec < nvec;
        c[k] = vec * V;
#pragma unroll
        for (int j = 0; j < V; ++j) wv[k][j] = bv[k][j] = dg[k][j] = db[k][j] = T(0);
        if (vok[k]) {
            vec_load<T, V>(p.w + c[k], wv[k]);
            if (MODE == 0) vec_load<T, V>(p.bias + c[k], bv[k]);
        }
    }
    for (unsigned grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long pix = (long long)grp * PPB + slot;
        const bool live = pix < p.M;            // the same in the G lanes of a pixel
        bool kept;
        size_t ea;
        IO::place(io, pix, live, C, kept, ea);
        const size_t e = (size_t)pix * C;
        const bool rd = MODE == 0 ? live : kept;        // the backward does not read a pixel without a gradient row
        T xv[NV][V];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int j = 0; j < V; ++j) xv[k][j] = T(0);
            if (rd && vok[k]) vec_load<XT, V>(reinterpret_cast<const XT*>(p.x) + e + c[k], xv[k]);
        }
        if (MODE == 0) {
            T mean, rstd;
            if (IO::REBUILD && p.stats_in) {    // rebuild; uniform in the launch
                mean = live ? p.stats_in[(size_t)pix * 2] : T(0);
                rstd = live ? p.stats_in[(size_t)pix * 2 + 1] : T(0);
#pragma unroll
                for (int k = 0; k < NV; ++k)
#pragma unroll
                    for (int j = 0; j < V; ++j) xv[k][j] = vok[k] ? xv[k][j] - mean : T(0);
            } else {
                T s = 0;
#pragma unroll
                for (int k = 0; k < NV; ++k)
#pragma unroll
                    for (int j = 0; j < V; ++j) s += xv[k][j];
                mean = ln_group_sum(s, G) / cnt;
                T q = 0;
#pragma unroll
                for (int k = 0; k < NV; ++k)
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        xv[k][j] = vok[k] ? xv[k][j] - mean : T(0);
                        q += xv[k][j] * xv[k][j];
                    }
                rstd = T(1) / sqrt(ln_group_sum(q, G) / cnt + p.eps);
                if (live && g == 0) {
                    p.stats_out[(size_t)pix * 2] = mean;
                    p.stats_out[(size_t)pix * 2 + 1] = rstd;
                }
            }
            if (kept) {
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    if (!vok[k]) continue;
                    T o[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) o[j] = (xv[k][j] * rstd) * wv[k][j] + bv[k][j];
                    IO::template store<V>(io, ea + c[k], o);
                }
            }
        } else {
            T gv[NV][V];
            T mean = 0, rstd = 0;
            if (kept) {
                mean = p.stats_in[(size_t)pix * 2];
                rstd = p.stats_in[(size_t)pix * 2 + 1];
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) {
#pragma unroll
                for (int j = 0; j < V; ++j) gv[k][j] = T(0);
                if (kept && vok[k]) IO::template load<V>(io, ea + c[k], gv[k]);
            }
            T s1 = 0, s2 = 0;
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const T xh = vok[k] ? (xv[k][j] - mean) * rstd : T(0);
                    const T t = gv[k][j] * wv[k][j];
                    if (p.part) {
                        dg[k][j] += gv[k][j] * xh;
                        db[k][j] += gv[k][j];
                    }
                    s1 += t;
                    s2 += t * xh;
                    xv[k][j] = xh;
                    gv[k][j] = t;
                }
            if (p.gx) {
                const T a = ln_group_sum(s1, G) / cnt, b = ln_group_sum(s2, G) / cnt;
                if (live) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        if (!vok[k]) continue;
                        T o[V];
#pragma unroll
                        for (int j = 0; j < V; ++j) o[j] = kept ? rstd * (gv[k][j] - a - xv[k][j] * b) : T(0);
                        vec_store<XT, V>(reinterpret_cast<XT*>(p.gx) + e + c[k], o);
                    }
                }
            }
        }
    }
    if (MODE == 1 && p.part) {                  // the pixel slots of a wave by butterfly, then the four waves in ascending order -> one row [2][C];
        double* sg = ln_cl_dyn_lds;             // in double: a lane's own sum has few terms, the sum over the lanes has many
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int k = 0; k < NV; ++k) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        double a = (double)dg[k][j], b = (double)db[k][j];
                        for (int o = G; o < 64; o <<= 1) {
                            a += __shfl_xor(a, o, 64);
                            b += __shfl_xor(b, o, 64);
                        }
                        if (lane < G && vok[k]) {
                            sg[c[k] + j] = (w ? sg[c[k] + j] : 0.0) + a;
                            sg[C + c[k] + j] = (w ? sg[C + c[k] + j] : 0.0) + b;
                        }
                    }
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < 2 * C; i += 256) p.part[(size_t)blockIdx.x * 2 * C + i] = (T)sg[i];
    }
}

// launches mode MODE of the kernel with the element type XT of x as the channels-last plan q says
template <typename T, typename XT, int MODE, typename IO>
static void ln_cl_launch(const LncfPlan& q, const LnClK<T>& k, const IO& io, hipStream_t s) {
    train_with_vwidth<XT>(q.V, [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        train_with_nv<V>(q.NV, [&](auto ntag) {
            constexpr int NV = decltype(ntag)::value;
            hipLaunchKernelGGL((ln_cl_kernel<T, XT, V, NV, MODE, IO>), dim3(q.grid), dim3(q.block), q.lds, s, k, io, 1 << q.lg, q.lg, q.units);
        });
    });
}
