// The four downsample layers of the ConvNeXt backbone for TRAINING (convnext.py:77-87): a convolution whose kernel equals its stride is a GEMM
// over non-overlapping patches, the GEMM stays with the vendor library and everything around it is here.
//
//   LN to patches   the channels-first LayerNorm (convnext.py:180-183) in front of Conv2d(C, Co, 2, stride=2), written straight into the
//                   patch matrix of that convolution: x dense [B][H][W][C] (fp32, fp16 or bf16, converted in registers; all arithmetic fp32, fp64
//                   in the fp64 form), z = weight * (x - mean) * rstd + bias rounded once to the element type of A, stored at row
//                   m = (n Ho + h / 2) Wo + w / 2, column ((h & 1) 2 + (w & 1)) C + c of A [M][4 C] (Ho = H / 2, Wo = W / 2, M = B Ho Wo): in
//                   channels-last memory a 2x2 patch is four runs of C elements.  A pixel of a dropped last row or column (odd H or W) writes
//                   its statistics and nothing else.
//   backward        reads grad_A at the same addresses: t = grad_A * weight, grad_x = rstd * (t - mean_c t - xhat * mean_c (t * xhat)), exact
//                   zeros at the dropped pixels, which are not read and add nothing to the sums;
//                   part[block][2][C] = the block's sums of grad_A * xhat and of grad_A -> dwln_reduce_kernel (train_ops.h)
//   stem patches    x [B][Cin][H][W] (NCHW-contiguous) <-> A [M][Cin 16], column (c 4 + kh) 4 + kw: the order of weight.reshape(Co, Cin 16)
//
//   down_cl_kernel<V, NV, MODE>   the lane mapping of lncf_cl_kernel (lncf_train.hip; lncf_plan, channels-last): a pixel belongs to G lanes of ONE
//                                 wave, a lane owns NV vectors of V consecutive channels, the row of a pixel is in registers, the variance is
//                                 the second pass over registers, a sum over C is a butterfly over the G lanes.  MODE 0 = forward (stats_in
//                                 NULL) and rebuild (stats_in given: the statistics are read instead of computed, stats_out is not written;
//                                 every other instruction is shared, so A has the forward's bits), 1 = backward.  The element type of A is a
//                                 run-time argument: one branch per vector, uniform in the launch.
//   patch4_kernel<SCATTER>        a lane takes the four elements kw = 0 .. 3 of a patch row: one 16-byte (8-byte) access on the side of A,
//                                 four element accesses on the side of x (W need not be a multiple of 4)
//
// Every output element has one writer, no atomics, fixed summation orders: bitwise reproducible.  Element offsets are 64-bit (A can pass 2^31
// elements); pixel and group indices fit 32 bits (B H W < 2^31 is required).
#include "kernels.h"
#include "train_ops.h"

template <typename T>
struct DownK {                                  // kernel arguments (by value)
    const void* x;
    const T *w, *bias, *stats_in;
    const void* ga;                             // the element type of A
    void* a;
    T* stats_out;
    void* gx;                                   // the element type of x
    T* part;
    T eps;
    int a_dtype;
    int H, W, Ho, Wo, C;
    long long M;                                // B H W
};

template <typename T>
__device__ __forceinline__ T down_group_sum(T v, int G) {      // lncf_group_sum
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// V elements of the patch matrix at element offset `off`, in the element type a_dtype names (the fp64 form has one)
template <typename T, int V>
__device__ __forceinline__ void down_a_store(void* a, size_t off, int a_dtype, const T (&r)[V]) {
    if constexpr (sizeof(T) == 8) {
        vec_store<double, V>(reinterpret_cast<double*>(a) + off, r);
    } else {
        if (a_dtype == 0) vec_store<float, V>(reinterpret_cast<float*>(a) + off, r);
        else if (a_dtype == 1) vec_store<f16, V>(reinterpret_cast<f16*>(a) + off, r);
        else vec_store<bf16, V>(reinterpret_cast<bf16*>(a) + off, r);
    }
}
template <typename T, int V>
__device__ __forceinline__ void down_a_load(const void* a, size_t off, int a_dtype, T (&r)[V]) {
    if constexpr (sizeof(T) == 8) {
        vec_load<double, V>(reinterpret_cast<const double*>(a) + off, r);
    } else {
        if (a_dtype == 0) vec_load<float, V>(reinterpret_cast<const float*>(a) + off, r);
        else if (a_dtype == 1) vec_load<f16, V>(reinterpret_cast<const f16*>(a) + off, r);
        else vec_load<bf16, V>(reinterpret_cast<const bf16*>(a) + off, r);
    }
}

extern __shared__ double down_dyn_lds[];

template <typename T, typename XT, int V, int NV, int MODE>
__global__ __launch_bounds__(256) void down_cl_kernel(DownK<T> p, int G, int lgG, unsigned ngroups) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = tid & (G - 1), slot = tid >> lgG, PPB = 256 >> lgG;
    const int C = p.C, nvec = C / V, HW = p.H * p.W;
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
        // the patch element of the pixel: kept = it lies inside the 2 Ho x 2 Wo region the convolution reads
        const int n = live ? (int)(pix / HW) : 0, r = live ? (int)(pix - (long long)n * HW) : 0, h = r / p.W, w = r - h * p.W;
        const bool kept = live && (h >> 1) < p.Ho && (w >> 1) < p.Wo;
        const size_t ea = (((size_t)n * p.Ho + (h >> 1)) * p.Wo + (w >> 1)) * 4 * C + (size_t)((h & 1) * 2 + (w & 1)) * C;
        const size_t e = (size_t)pix * C;
        const bool rd = MODE == 0 ? live : kept;        // the backward does not read a dropped pixel
        T xv[NV][V];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int j = 0; j < V; ++j) xv[k][j] = T(0);
            if (rd && vok[k]) vec_load<XT, V>(reinterpret_cast<const XT*>(p.x) + e + c[k], xv[k]);
        }
        if (MODE == 0) {
            T mean, rstd;
            if (p.stats_in) {                   // rebuild; uniform in the launch
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
                mean = down_group_sum(s, G) / cnt;
                T q = 0;
#pragma unroll
                for (int k = 0; k < NV; ++k)
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        xv[k][j] = vok[k] ? xv[k][j] - mean : T(0);
                        q += xv[k][j] * xv[k][j];
                    }
                rstd = T(1) / sqrt(down_group_sum(q, G) / cnt + p.eps);
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
                    down_a_store<T, V>(p.a, ea + c[k], p.a_dtype, o);
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
                if (kept && vok[k]) down_a_load<T, V>(p.ga, ea + c[k], p.a_dtype, gv[k]);
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
                const T a = down_group_sum(s1, G) / cnt, b = down_group_sum(s2, G) / cnt;
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
    if (MODE == 1 && p.part) {                  // as lncf_cl_kernel: the pixel slots of a wave by butterfly, then the four waves in ascending
        double* sg = down_dyn_lds;              // order -> one row [2][C]; in double
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

// stem patches.  gather: unit u = (m Cin + c) 4 + kh -> A[u 4 ..] = x[n][c][4 ho + kh][4 wo ..].  scatter: unit u = ((n Cin + c) H + h) wg + j
// -> grad_x[n][c][h][4 j ..] = grad_A[...] inside the 4 Ho x 4 Wo region, zeros in the margin (the group j = Wo is the margin of a row).
template <typename XT, typename AT, bool SCATTER>
__global__ __launch_bounds__(256) void patch4_kernel(const XT* x, XT* gx, AT* a, const AT* ga, int Cin, int H, int W, int Ho, int Wo, int wg,
                                                     long long units) {
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
        if constexpr (!SCATTER) {
            const int kh = (int)(u & 3);
            const long long mc = u >> 2;
            const int c = (int)(mc % Cin);
            const long long m = mc / Cin;
            const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
            const long long n = m / ((long long)Wo * Ho);
            const XT* src = x + (((size_t)n * Cin + c) * H + (size_t)(4 * ho + kh)) * W + 4 * wo;
            if constexpr (sizeof(XT) == 8) {
                double vd[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) vd[i] = src[i];
                vec_store<AT, 4>(a + (size_t)u * 4, vd);
            } else {
                float v[4];                     // a value travels unchanged or is rounded once: float holds fp16 and bf16 exactly
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (float)src[i];
                vec_store<AT, 4>(a + (size_t)u * 4, v);
            }
        } else {
            const int j = (int)(u % wg);
            const long long nch = u / wg;
            const int h = (int)(nch % H);
            const long long nc = nch / H;
            const int c = (int)(nc % Cin);
            const long long n = nc / Cin;
            XT* dst = gx + (size_t)nch * W + 4 * j;
            const int nw = W - 4 * j < 4 ? W - 4 * j : 4;
            if (j < Wo && (h >> 2) < Ho) {      // nw == 4
                const size_t m = ((size_t)n * Ho + (h >> 2)) * Wo + j;
                const AT* src = ga + ((m * Cin + c) * 4 + (h & 3)) * 4;
                if constexpr (sizeof(XT) == 8) {
                    double vd[4];
                    vec_load<AT, 4>(src, vd);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[i] = (XT)vd[i];
                } else {
                    float v[4];
                    vec_load<AT, 4>(src, v);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[i] = (XT)v[i];
                }
            } else {
                for (int i = 0; i < nw; ++i) dst[i] = XT(0);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t down_train_workspace_bytes(int B, int H, int W, int C) { return down_plan_workspace_bytes(B, H, W, C); }

static inline int down_shape_refused(const char* what, int B, int H, int W, int C) {
    uni_set_error("%s: shape B=%d H=%d W=%d C=%d is outside B >= 1, H, W >= 2, C %% 4 == 0, 4 <= C <= %d, B H W < 2^31", what, B, H, W, C, TRAIN_MAX_C);
    return -1;
}

// launches mode MODE with the element type XT of x as lncf_plan (train_plan.h, channels-last) says; *rows = the rows of partials it writes
template <typename T, typename XT, int MODE>
static void down_launch(const DownArgs<T>& a, const DownK<T>& k, int* rows, hipStream_t s) {
    const LncfPlan q = lncf_plan(a.B, a.H, a.W, a.C, sizeof(XT), sizeof(T) == 8, false, MODE == 1 && k.part);
    *rows = q.rows;
    char cls[64] = "";
    const bool f64 = sizeof(T) == 8;
    if (train_tracing()) down_plan_class(q, train_ename(a.x_dtype, f64), train_ename(a.a_dtype, f64), cls, sizeof(cls));
    if (MODE == 1) uni_variant_note("down_train bwd_%s gx=%d gwb=%d", cls, k.gx != nullptr, k.part != nullptr);
    else uni_variant_note("down_train %s_%s", k.stats_in ? "rebuild" : "fwd", cls);
    train_with_vwidth<XT>(q.V, [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        auto run = [&](auto ntag) {
            constexpr int NV = decltype(ntag)::value;
            hipLaunchKernelGGL((down_cl_kernel<T, XT, V, NV, MODE>), dim3(q.grid), dim3(q.block), q.lds, s, k, 1 << q.lg, q.lg, q.units);
        };
        switch (q.NV) {
            case 1: run(std::integral_constant<int, 1>()); break;
            case 2: run(std::integral_constant<int, 2>()); break;
            case 3: run(std::integral_constant<int, 3>()); break;
            case 4: run(std::integral_constant<int, 4>()); break;
            default:                            // 6 or 8: more than 256 vectors, so V = 4
                if constexpr (V == 4) {
                    if (q.NV == 6) run(std::integral_constant<int, 6>());
                    else run(std::integral_constant<int, 8>());
                }
        }
    });
}

template <typename T, int MODE>
static int down_dispatch(const char* what, const DownArgs<T>& a, const DownK<T>& k, int* rows, hipStream_t s) {
    return train_with_etype<T>(what, "x_dtype", a.x_dtype, [&](auto e) { down_launch<T, typename decltype(e)::type, MODE>(a, k, rows, s); });
}

template <typename T>
static int down_check(const char* what, const DownArgs<T>& a) {
    if (!down_shape_ok(a.B, a.H, a.W, a.C)) return down_shape_refused(what, a.B, a.H, a.W, a.C);
    if (int rc = train_with_etype<T>(what, "a_dtype", a.a_dtype, [](auto) {})) return rc;
    UNI_REQUIRE(aligned16(a.x) && aligned16(a.w) && aligned16(a.bias), "%s: a pointer is not 16-byte aligned", what);
    return 0;
}

template <typename T>
static DownK<T> down_args(const DownArgs<T>& a) {
    DownK<T> k{};
    k.x = a.x, k.w = a.w, k.bias = a.bias, k.eps = (T)a.eps, k.a_dtype = a.a_dtype;
    k.H = a.H, k.W = a.W, k.Ho = a.H / 2, k.Wo = a.W / 2, k.C = a.C, k.M = (long long)a.B * a.H * a.W;
    return k;
}

template <typename T>
int launch_down_train_fwd(const DownArgs<T>& a, int rebuild, void* A, T* stats, hipStream_t s) {
    if (int rc = down_check("down_train_fwd", a)) return rc;
    UNI_REQUIRE(aligned16(A) && aligned16(stats), "down_train_fwd: a pointer is not 16-byte aligned");
    UNI_REQUIRE(rebuild || a.eps > 0, "down_train_fwd: eps %g is not positive", a.eps);
    DownK<T> k = down_args(a);
    k.a = A;
    if (rebuild) k.stats_in = stats;
    else k.stats_out = stats;
    int rows;
    if (int rc = down_dispatch<T, 0>("down_train_fwd", a, k, &rows, s)) return rc;
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_down_train_bwd(const DownArgs<T>& a, const T* stats, const void* gA, void* gx, T* gw, T* gb, void* ws, size_t ws_bytes, hipStream_t s) {
    if (int rc = down_check("down_train_bwd", a)) return rc;
    UNI_REQUIRE((gw != nullptr) == (gb != nullptr), "down_train_bwd: grad_ln_weight and grad_ln_bias come as a pair");
    UNI_REQUIRE(aligned16(stats) && aligned16(gA) && aligned16(gx) && aligned16(gw) && aligned16(gb) && aligned16(ws),
                "down_train_bwd: a pointer is not 16-byte aligned");
    if (!gx && !gw) return 0;
    T* part;
    if (int rc = train_partials("down_train_bwd", gw != nullptr, ws, ws_bytes, down_train_workspace_bytes(a.B, a.H, a.W, a.C), &part)) return rc;
    DownK<T> k = down_args(a);
    k.stats_in = stats, k.ga = gA, k.gx = gx, k.part = part;
    int rows;
    if (int rc = down_dispatch<T, 1>("down_train_bwd", a, k, &rows, s)) return rc;
    if (gw) {
        const DwlnRJob none{nullptr, nullptr, nullptr, 0, 0, 0, 0};
        const DwlnRJob job{part, gw, gb, rows, 2 * a.C, a.C, cdiv(2 * a.C, 64)};
        uni_variant_note("down_train reduce<%s>", train_ename(0, sizeof(T) == 8));
        hipLaunchKernelGGL((dwln_reduce_kernel<T>), dim3(job.blocks), dim3(256), 0, s, none, job);
    }
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T, bool SCATTER>
static int patch4_launch(const char* what, const void* x, void* gx, int x_dtype, void* A, const void* gA, int a_dtype, int B, int Cin, int H, int W,
                         hipStream_t s) {
    if (!patch4_shape_ok(B, Cin, H, W)) {
        uni_set_error("%s: shape B=%d Cin=%d H=%d W=%d is outside B >= 1, 1 <= Cin <= %d, H, W >= 4, B H W < 2^31", what, B, Cin, H, W, P4_MAX_CIN);
        return -1;
    }
    UNI_REQUIRE(aligned16(x) && aligned16(gx) && aligned16(A) && aligned16(gA), "%s: a pointer is not 16-byte aligned", what);
    const Patch4Plan q = patch4_plan(B, Cin, H, W, SCATTER);
    const bool f64 = sizeof(T) == 8;
    if (int rc = train_with_etype<T>(what, "a_dtype", a_dtype, [](auto) {})) return rc;
    if (int rc = train_with_etype<T>(what, "x_dtype", x_dtype, [&](auto ex) {
            using XT = typename decltype(ex)::type;
            train_with_etype<T>(what, "a_dtype", a_dtype, [&](auto ea) {
                using AT = typename decltype(ea)::type;
                char cls[32] = "";
                if (train_tracing()) patch4_plan_class(train_ename(x_dtype, f64), train_ename(a_dtype, f64), cls, sizeof(cls));
                uni_variant_note("down_train %s%s", SCATTER ? "scatter4" : "gather4", cls);
                hipLaunchKernelGGL((patch4_kernel<XT, AT, SCATTER>), dim3(q.grid), dim3(q.block), 0, s, reinterpret_cast<const XT*>(x),
                                   reinterpret_cast<XT*>(gx), reinterpret_cast<AT*>(A), reinterpret_cast<const AT*>(gA), Cin, H, W, q.Ho, q.Wo, q.wg,
                                   q.units);
            });
        }))
        return rc;
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_patch4_gather(const void* x, int x_dtype, int B, int Cin, int H, int W, void* A, int a_dtype, hipStream_t s) {
    return patch4_launch<T, false>("patch4_gather", x, nullptr, x_dtype, A, nullptr, a_dtype, B, Cin, H, W, s);
}
template <typename T>
int launch_patch4_scatter(const void* gA, int a_dtype, int B, int Cin, int H, int W, void* gx, int x_dtype, hipStream_t s) {
    return patch4_launch<T, true>("patch4_scatter", nullptr, gx, x_dtype, nullptr, gA, a_dtype, B, Cin, H, W, s);
}

template int launch_down_train_fwd<float>(const DownArgs<float>&, int, void*, float*, hipStream_t);
template int launch_down_train_fwd<double>(const DownArgs<double>&, int, void*, double*, hipStream_t);
template int launch_down_train_bwd<float>(const DownArgs<float>&, const float*, const void*, void*, float*, float*, void*, size_t, hipStream_t);
template int launch_down_train_bwd<double>(const DownArgs<double>&, const double*, const void*, void*, double*, double*, void*, size_t, hipStream_t);
template int launch_patch4_gather<float>(const void*, int, int, int, int, int, void*, int, hipStream_t);
template int launch_patch4_gather<double>(const void*, int, int, int, int, int, void*, int, hipStream_t);
template int launch_patch4_scatter<float>(const void*, int, int, int, int, int, void*, int, hipStream_t);
template int launch_patch4_scatter<double>(const void*, int, int, int, int, int, void*, int, hipStream_t);
