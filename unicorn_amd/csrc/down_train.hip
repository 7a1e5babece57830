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
//   ln_cl_kernel<V, NV, MODE, DownIO>  the kernel of ln_cl.h, which lncf_train.hip runs too (lncf_plan, channels-last), with the policy below: the
//                                 row of a pixel is its run of C elements in A / grad_A, and a dropped pixel has none.  MODE 0 = forward
//                                 (stats_in NULL) and rebuild (stats_in given: A has the forward's bits), 1 = backward.
//   patch4_kernel<SCATTER>        a lane takes the four elements kw = 0 .. 3 of a patch row: one 16-byte (8-byte) access on the side of A,
//                                 four element accesses on the side of x (W need not be a multiple of 4)
//
// Every output element has one writer, no atomics, fixed summation orders: bitwise reproducible.  Element offsets are 64-bit (A can pass 2^31
// elements); pixel and group indices fit 32 bits (B H W < 2^31 is required).
#include "kernels.h"
#include "ln_cl.h"

// the row of a pixel in the patch matrix A (MODE 0) / grad_A (MODE 1) for ln_cl_kernel (ln_cl.h).  The element type of A is a run-time
// argument: one branch per vector, uniform in the launch (the fp64 form has one type)
struct DownIO {
    static constexpr bool REBUILD = true;
    void* a;
    const void* ga;
    int a_dtype;
    int H, W, Ho, Wo;
    // kept = the pixel lies inside the 2 Ho x 2 Wo region the convolution reads
    static __device__ __forceinline__ void place(DownIO io, long long pix, bool live, int C, bool& kept, size_t& ea) {
        const int HW = io.H * io.W;
        const int n = live ? (int)(pix / HW) : 0, r = live ? (int)(pix - (long long)n * HW) : 0, h = r / io.W, w = r - h * io.W;
        kept = live && (h >> 1) < io.Ho && (w >> 1) < io.Wo;
        ea = (((size_t)n * io.Ho + (h >> 1)) * io.Wo + (w >> 1)) * 4 * C + (size_t)((h & 1) * 2 + (w & 1)) * C;
    }
    template <int V, typename T>
    static __device__ __forceinline__ void store(DownIO io, size_t off, const T (&r)[V]) {
        if constexpr (sizeof(T) == 8) {
            vec_store<double, V>(reinterpret_cast<double*>(io.a) + off, r);
        } else {
            if (io.a_dtype == 0) vec_store<float, V>(reinterpret_cast<float*>(io.a) + off, r);
            else if (io.a_dtype == 1) vec_store<f16, V>(reinterpret_cast<f16*>(io.a) + off, r);
            else vec_store<bf16, V>(reinterpret_cast<bf16*>(io.a) + off, r);
        }
    }
    template <int V, typename T>
    static __device__ __forceinline__ void load(DownIO io, size_t off, T (&r)[V]) {
        if constexpr (sizeof(T) == 8) {
            vec_load<double, V>(reinterpret_cast<const double*>(io.ga) + off, r);
        } else {
            if (io.a_dtype == 0) vec_load<float, V>(reinterpret_cast<const float*>(io.ga) + off, r);
            else if (io.a_dtype == 1) vec_load<f16, V>(reinterpret_cast<const f16*>(io.ga) + off, r);
            else vec_load<bf16, V>(reinterpret_cast<const bf16*>(io.ga) + off, r);
        }
    }
};

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
static void down_launch(const DownArgs<T>& a, const LnClK<T>& k, const DownIO& io, int* rows, hipStream_t s) {
    const LncfPlan q = lncf_plan(a.B, a.H, a.W, a.C, sizeof(XT), sizeof(T) == 8, false, MODE == 1 && k.part);
    *rows = q.rows;
    char cls[64] = "";
    const bool f64 = sizeof(T) == 8;
    if (train_tracing()) down_plan_class(q, train_ename(a.x_dtype, f64), train_ename(a.a_dtype, f64), cls, sizeof(cls));
    if (MODE == 1) uni_variant_note("down_train bwd_%s gx=%d gwb=%d", cls, k.gx != nullptr, k.part != nullptr);
    else uni_variant_note("down_train %s_%s", k.stats_in ? "rebuild" : "fwd", cls);
    ln_cl_launch<T, XT, MODE>(q, k, io, s);
}

template <typename T, int MODE>
static int down_dispatch(const char* what, const DownArgs<T>& a, const LnClK<T>& k, const DownIO& io, int* rows, hipStream_t s) {
    return train_with_etype<T>(what, "x_dtype", a.x_dtype, [&](auto e) { down_launch<T, typename decltype(e)::type, MODE>(a, k, io, rows, s); });
}

template <typename T>
static int down_check(const char* what, const DownArgs<T>& a) {
    if (!down_shape_ok(a.B, a.H, a.W, a.C)) return down_shape_refused(what, a.B, a.H, a.W, a.C);
    if (int rc = train_with_etype<T>(what, "a_dtype", a.a_dtype, [](auto) {})) return rc;
    UNI_REQUIRE(aligned16(a.x) && aligned16(a.w) && aligned16(a.bias), "%s: a pointer is not 16-byte aligned", what);
    return 0;
}

template <typename T>
static LnClK<T> down_args(const DownArgs<T>& a) {
    LnClK<T> k{};
    k.x = a.x, k.w = a.w, k.bias = a.bias, k.eps = (T)a.eps, k.C = a.C, k.M = (long long)a.B * a.H * a.W;
    return k;
}
template <typename T>
static DownIO down_io(const DownArgs<T>& a, void* A, const void* gA) { return DownIO{A, gA, a.a_dtype, a.H, a.W, a.H / 2, a.W / 2}; }

template <typename T>
int launch_down_train_fwd(const DownArgs<T>& a, int rebuild, void* A, T* stats, hipStream_t s) {
    if (int rc = down_check("down_train_fwd", a)) return rc;
    UNI_REQUIRE(aligned16(A) && aligned16(stats), "down_train_fwd: a pointer is not 16-byte aligned");
    UNI_REQUIRE(rebuild || a.eps > 0, "down_train_fwd: eps %g is not positive", a.eps);
    LnClK<T> k = down_args(a);
    if (rebuild) k.stats_in = stats;
    else k.stats_out = stats;
    int rows;
    if (int rc = down_dispatch<T, 0>("down_train_fwd", a, k, down_io(a, A, nullptr), &rows, s)) return rc;
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
    LnClK<T> k = down_args(a);
    k.stats_in = stats, k.gx = gx, k.part = part;
    int rows;
    if (int rc = down_dispatch<T, 1>("down_train_bwd", a, k, down_io(a, nullptr, gA), &rows, s)) return rc;
    if (gw) train_reduce_2c<T>(part, rows, a.C, gw, gb, "down_train", s);
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
