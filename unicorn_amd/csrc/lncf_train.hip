// The channels-first LayerNorm of the ConvNeXt backbone for TRAINING (convnext.py:160-184, data_format == "channels_first"): forward with per-pixel
// statistics and a deterministic backward, fp32 (x / grad_x fp32, fp16 or bf16, converted in registers; all arithmetic fp32) and fp64.
//
//   forward   u = mean_c x, rstd = 1 / sqrt(mean_c (x - u)^2 + eps), y[n][c][h][w] = weight[c] * (x - u) * rstd + bias[c], stats [B H W][2] = u, rstd
//   backward  xhat = (x - u) * rstd, t = grad_y * weight, grad_x = rstd * (t - mean_c t - xhat * mean_c (t * xhat)),
//             part[block][2][C] = the block's sums of grad_y * xhat and of grad_y
//
//   ln_cl_kernel<V, NV, MODE, LncfIO>  channels-last memory [B][H][W][C]: the kernel of ln_cl.h, which down_train.hip runs too, with the policy below:
//                                  y and grad_y are dense rows [B H W][C] of the math type, and every pixel has one.
//   lncf_nchw_kernel<CH, KEEP, MODE>  NCHW-contiguous memory: a tile = 64 consecutive pixels of one image (lane = pixel: a wave reads 64 consecutive
//                                  elements of a channel plane, whatever H W is: no alignment is assumed and a tile ends with its image), the eight
//                                  waves of a block split the channels (wave w owns c = w, w + 8, ...).  KEEP: the slice of <= CH channels stays in
//                                  registers (C <= 256: x is read once, two-pass variance per slice).  Otherwise (wider C) the slice is walked in chunks
//                                  of CH channels, two-pass inside a chunk, and x is read a second time for the output.  Chunks and slices are
//                                  combined with the pairwise mean / M2 update (Chan et al.), the slices through LDS in ascending wave order.
//   dwln_reduce_kernel             partials [R][2][C] -> grad_weight, grad_bias (train_ops.h)
//
// mode 0 = forward, 1 = backward.  Every output element has one writer, no atomics, fixed summation orders: bitwise reproducible.  Element
// offsets are 64-bit; pixel, group and tile indices fit 32 bits (B H W < 2^31 is required).
#include "kernels.h"
#include "ln_cl.h"

template <typename T>
struct LncfK {                                  // kernel arguments (by value)
    const void* x;
    const T *w, *bias, *gy, *stats_in;
    T *y, *stats_out;
    void* gx;                                   // the element type of x
    T* part;
    T eps;
    int HW, C;
    long long M;                                // B H W
};

// the output row / incoming gradient row of a pixel for ln_cl_kernel (ln_cl.h): dense [B H W][C] in the math type, every pixel has one
template <typename T>
struct LncfIO {
    static constexpr bool REBUILD = false;
    T* y;
    const T* gy;
    static __device__ __forceinline__ void place(LncfIO, long long pix, bool live, int C, bool& kept, size_t& ea) {
        kept = live;
        ea = (size_t)pix * C;
    }
    template <int V>
    static __device__ __forceinline__ void store(LncfIO io, size_t off, const T (&r)[V]) { vec_store<T, V>(io.y + off, r); }
    template <int V>
    static __device__ __forceinline__ void load(LncfIO io, size_t off, T (&r)[V]) { vec_load<T, V>(io.gy + off, r); }
};

extern __shared__ double lncf_dyn_lds[];

// channels of wave w of the NCHW path: c = w, w + LNCF_NW, ... < C
__device__ __forceinline__ int lncf_slice(int C, int w) { return (C - w + LNCF_NW - 1) / LNCF_NW; }

// (na, mean, m2) of a set of na values <- that set and a set of nb > 0 values with mean mb and sum of squared deviations qb
template <typename T>
__device__ __forceinline__ void lncf_merge(T& na, T& mean, T& m2, T nb, T mb, T qb) {
    const T nn = na + nb, d = mb - mean;
    mean += d * (nb / nn);
    m2 += qb + d * d * (na * nb / nn);
    na = nn;
}

// up to CH values of one lane's channel slice from k0 on: v[j] = element (k0 + j) of the slice (0 beyond nb or outside the image)
template <typename T, typename E, int CH>
__device__ __forceinline__ void lncf_chunk_load(const E* base, size_t HW, int wave, int k0, int nb, bool ok, T (&v)[CH]) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        v[j] = T(0);
        if (j < nb && ok) v[j] = (T)base[(size_t)((k0 + j) * LNCF_NW + wave) * HW];
    }
}

template <typename T, typename XT, int CH, bool KEEP, int MODE>
__global__ __launch_bounds__(512) void lncf_nchw_kernel(LncfK<T> p, unsigned tpi, unsigned ntiles) {
    __shared__ T sm[2][2][LNCF_NW][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, HW = p.HW;
    const int ks = lncf_slice(C, wave);         // may be 0 (C < 8)
    const T cnt = T(C);
    // backward with partials.  KEEP: a lane sums its pixels of the block's tiles in registers.  Otherwise the 64 pixels of a tile are summed by
    // butterfly (in double) and the tiles in ascending order in acc [2][C] (LDS, double; channel c is touched by lane 0 of wave c % 8 only).
    T dgr[KEEP ? CH : 1], dbr[KEEP ? CH : 1];
#pragma unroll
    for (int j = 0; j < (KEEP ? CH : 1); ++j) dgr[j] = dbr[j] = T(0);
    double* acc = lncf_dyn_lds;
    if (MODE == 1 && !KEEP && p.part) {
        for (int i = tid; i < 2 * C; i += 512) acc[i] = 0.0;
        __syncthreads();
    }
    int it = 0;
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x, ++it) {
        const unsigned n = t / tpi;
        const long long q = (long long)(t - n * tpi) * 64 + lane;
        const bool ok = q < HW;
        const size_t img = (size_t)n * C * HW + (size_t)q, pix = (size_t)n * HW + (size_t)q;
        const XT* xp = reinterpret_cast<const XT*>(p.x) + img;
        T(&buf)[2][LNCF_NW][64] = sm[it & 1];
        T xv[CH];
        if (MODE == 0) {
            T na = 0, mw = 0, qw = 0;            // the slice of this wave
            for (int k0 = 0; k0 < ks; k0 += CH) {
                const int nb = ks - k0 < CH ? ks - k0 : CH;
                lncf_chunk_load<T, XT, CH>(xp, HW, wave, k0, nb, ok, xv);
                T s = 0;
#pragma unroll
                for (int j = 0; j < CH; ++j) s += xv[j];
                const T mb = s / T(nb);
                T qb = 0;
#pragma unroll
                for (int j = 0; j < CH; ++j)
                    if (j < nb) qb += (xv[j] - mb) * (xv[j] - mb);
                lncf_merge(na, mw, qw, T(nb), mb, qb);
            }
            buf[0][wave][lane] = mw;
            buf[1][wave][lane] = qw;
            __syncthreads();
            T nt = 0, mean = 0, m2 = 0;
#pragma unroll
            for (int w = 0; w < LNCF_NW; ++w) {
                const int nw = lncf_slice(C, w);
                if (nw > 0) lncf_merge(nt, mean, m2, T(nw), buf[0][w][lane], buf[1][w][lane]);
            }
            const T rstd = T(1) / sqrt(m2 / cnt + p.eps);
            T* yp = p.y + img;
            for (int k0 = 0; k0 < ks; k0 += CH) {
                const int nb = ks - k0 < CH ? ks - k0 : CH;
                if (!KEEP) lncf_chunk_load<T, XT, CH>(xp, HW, wave, k0, nb, ok, xv);
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (j < nb) {
                        const int c = (k0 + j) * LNCF_NW + wave;
                        const T r = ((xv[j] - mean) * rstd) * p.w[c] + p.bias[c];
                        if (ok) yp[(size_t)c * HW] = r;
                    }
                }
            }
            if (wave == 0 && ok) {
                p.stats_out[pix * 2] = mean;
                p.stats_out[pix * 2 + 1] = rstd;
            }
        } else {
            const T* gp = p.gy + img;
            T gv[CH];
            T mean = 0, rstd = 0;
            if (ok) {
                mean = p.stats_in[pix * 2];
                rstd = p.stats_in[pix * 2 + 1];
            }
            T s1 = 0, s2 = 0;
            for (int k0 = 0; k0 < ks; k0 += CH) {
                const int nb = ks - k0 < CH ? ks - k0 : CH;
                lncf_chunk_load<T, XT, CH>(xp, HW, wave, k0, nb, ok, xv);
                lncf_chunk_load<T, T, CH>(gp, HW, wave, k0, nb, ok, gv);
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (j < nb) {                // uniform in the wave
                        const int c = (k0 + j) * LNCF_NW + wave;
                        const T xh = (xv[j] - mean) * rstd;
                        const T tt = gv[j] * p.w[c];
                        s1 += tt;
                        s2 += tt * xh;
                        if (p.part) {
                            if constexpr (KEEP) {
                                dgr[j] += gv[j] * xh;
                                dbr[j] += gv[j];
                            } else {
                                const double a = wave_sum((double)(gv[j] * xh)), b = wave_sum((double)gv[j]);
                                if (lane == 0) {
                                    acc[c] += a;
                                    acc[C + c] += b;
                                }
                            }
                        }
                    }
                }
            }
            if (p.gx) {
                buf[0][wave][lane] = s1;
                buf[1][wave][lane] = s2;
                __syncthreads();
                T a = 0, b = 0;
#pragma unroll
                for (int w = 0; w < LNCF_NW; ++w) {
                    a += buf[0][w][lane];
                    b += buf[1][w][lane];
                }
                a /= cnt;
                b /= cnt;
                XT* op = reinterpret_cast<XT*>(p.gx) + img;
                for (int k0 = 0; k0 < ks; k0 += CH) {
                    const int nb = ks - k0 < CH ? ks - k0 : CH;
                    if (!KEEP) {
                        lncf_chunk_load<T, XT, CH>(xp, HW, wave, k0, nb, ok, xv);
                        lncf_chunk_load<T, T, CH>(gp, HW, wave, k0, nb, ok, gv);
                    }
#pragma unroll
                    for (int j = 0; j < CH; ++j) {
                        if (j < nb) {
                            const int c = (k0 + j) * LNCF_NW + wave;
                            const T xh = (xv[j] - mean) * rstd;
                            const T r = rstd * (gv[j] * p.w[c] - a - xh * b);
                            if (ok) op[(size_t)c * HW] = (XT)r;
                        }
                    }
                }
            }
        }
    }
    if (MODE == 1 && p.part) {                  // one row [2][C]
        T* row = p.part + (size_t)blockIdx.x * 2 * C;
        if constexpr (KEEP) {                   // the 64 lanes of the owning wave by butterfly, in double
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (j < ks) {
                    const double a = wave_sum((double)dgr[j]), b = wave_sum((double)dbr[j]);
                    if (lane == 0) {
                        row[j * LNCF_NW + wave] = (T)a;
                        row[C + j * LNCF_NW + wave] = (T)b;
                    }
                }
            }
        } else {
            __syncthreads();
            for (int i = tid; i < 2 * C; i += 512) row[i] = (T)acc[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t lncf_train_workspace_bytes(int B, int H, int W, int C) { return lncf_plan_workspace_bytes(B, H, W, C); }

// launches mode MODE with the element type XT of x as lncf_plan (train_plan.h) says; *rows = the rows of partials it writes
template <typename T, typename XT, int MODE>
static void lncf_launch(const LncfArgs<T>& a, const LncfK<T>& k, int* rows, hipStream_t s) {
    const LncfPlan q = lncf_plan(a.B, a.H, a.W, a.C, sizeof(XT), sizeof(T) == 8, a.nchw != 0, MODE == 1 && k.part);
    *rows = q.rows;
    char cls[48] = "";
    if (train_tracing()) lncf_plan_class(q, train_ename(a.x_dtype, sizeof(T) == 8), cls, sizeof(cls));
    uni_variant_note("lncf_train %s_%s gx=%d gwb=%d", MODE ? "bwd" : "fwd", cls, k.gx != nullptr, k.part != nullptr);
    auto nchw = [&](auto ch, auto keep) {
        hipLaunchKernelGGL((lncf_nchw_kernel<T, XT, decltype(ch)::value, decltype(keep)::value, MODE>), dim3(q.grid), dim3(q.block), q.lds, s, k,
                           q.per_image, q.units);
    };
    switch (q.family) {
        case LNCF_NCHW_REGS16: return nchw(std::integral_constant<int, 16>(), std::true_type());
        case LNCF_NCHW_REGS32:                  // never the plan of the fp64 form
            if constexpr (sizeof(T) == 4) nchw(std::integral_constant<int, 32>(), std::true_type());
            return;
        case LNCF_NCHW_STREAM8: return nchw(std::integral_constant<int, 8>(), std::false_type());
    }
    ln_cl_launch<T, XT, MODE>(q, LnClK<T>{k.x, k.w, k.bias, k.stats_in, k.stats_out, k.gx, k.part, k.eps, k.C, k.M}, LncfIO<T>{k.y, k.gy}, s);
}

template <typename T, int MODE>
static int lncf_dispatch(const char* what, const LncfArgs<T>& a, const LncfK<T>& k, int* rows, hipStream_t s) {
    return train_with_etype<T>(what, "x_dtype", a.x_dtype, [&](auto e) { lncf_launch<T, typename decltype(e)::type, MODE>(a, k, rows, s); });
}

template <typename T>
static int lncf_check(const char* what, const LncfArgs<T>& a) {
    if (!train_shape_ok(a.B, a.H, a.W, a.C)) return train_shape_refused(what, a.B, a.H, a.W, a.C);
    UNI_REQUIRE(aligned16(a.x) && aligned16(a.w) && aligned16(a.bias), "%s: a pointer is not 16-byte aligned", what);
    return 0;
}

template <typename T>
int launch_lncf_train_fwd(const LncfArgs<T>& a, T* y, T* stats, hipStream_t s) {
    if (int rc = lncf_check("lncf_train_fwd", a)) return rc;
    UNI_REQUIRE(aligned16(y) && aligned16(stats), "lncf_train_fwd: a pointer is not 16-byte aligned");
    UNI_REQUIRE(a.eps > 0, "lncf_train_fwd: eps %g is not positive", a.eps);
    const LncfK<T> k{a.x, a.w, a.bias, nullptr, nullptr, y, stats, nullptr, nullptr, (T)a.eps, a.H * a.W, a.C, (long long)a.B * a.H * a.W};
    int rows;
    if (int rc = lncf_dispatch<T, 0>("lncf_train_fwd", a, k, &rows, s)) return rc;
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_lncf_train_bwd(const LncfArgs<T>& a, const T* stats, const T* gy, void* gx, T* gw, T* gb, void* ws, size_t ws_bytes, hipStream_t s) {
    if (int rc = lncf_check("lncf_train_bwd", a)) return rc;
    UNI_REQUIRE((gw != nullptr) == (gb != nullptr), "lncf_train_bwd: grad_weight and grad_bias come as a pair");
    UNI_REQUIRE(aligned16(stats) && aligned16(gy) && aligned16(gx) && aligned16(gw) && aligned16(gb) && aligned16(ws),
                "lncf_train_bwd: a pointer is not 16-byte aligned");
    if (!gx && !gw) return 0;
    T* part;
    if (int rc = train_partials("lncf_train_bwd", gw != nullptr, ws, ws_bytes, lncf_train_workspace_bytes(a.B, a.H, a.W, a.C), &part)) return rc;
    const LncfK<T> k{a.x, a.w, nullptr, gy, stats, nullptr, nullptr, gx, part, T(0), a.H * a.W, a.C, (long long)a.B * a.H * a.W};
    int rows;
    if (int rc = lncf_dispatch<T, 1>("lncf_train_bwd", a, k, &rows, s)) return rc;
    if (gw) train_reduce_2c<T>(part, rows, a.C, gw, gb, "lncf_train", s);
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template int launch_lncf_train_fwd<float>(const LncfArgs<float>&, float*, float*, hipStream_t);
template int launch_lncf_train_fwd<double>(const LncfArgs<double>&, double*, double*, hipStream_t);
template int launch_lncf_train_bwd<float>(const LncfArgs<float>&, const float*, const float*, void*, float*, float*, void*, size_t, hipStream_t);
template int launch_lncf_train_bwd<double>(const LncfArgs<double>&, const double*, const double*, void*, double*, double*, void*, size_t, hipStream_t);
