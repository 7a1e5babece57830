// What the training operators (dwln_train.hip, block_tail.hip, lncf_train.hip, down_train.hip, pw_mlp.hip, gn_act_train.hip) share and that needs HIP: the refusal
// of a shape, the host helpers of their launchers, the converting 16-byte vector access and the ordered reduce of per-block partial sums.  Plain
// functions.  The shape limits and the launch plans are in train_plan.h, which compiles for the host alone.
#pragma once
#include "common.h"
#include "train_plan.h"
#include <type_traits>

static inline int train_shape_refused(const char* what, int B, int H, int W, int C) {
    uni_set_error("%s: shape B=%d H=%d W=%d C=%d is outside B, H, W >= 1, C %% 4 == 0, 4 <= C <= %d, B H W < 2^31", what, B, H, W, C, TRAIN_MAX_C);
    return -1;
}
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the plan class of a tag (the *_plan_class formatters of train_plan.h) is formatted only while the variant trace is on
static inline bool train_tracing() { return g_uni_variant_trace.load(std::memory_order_relaxed) != 0; }

// The element type E of a tensor that comes as (void*, dtype) next to the math type T: f(tag) with decltype(tag)::type = E.  `arg` names the
// dtype argument ("y_dtype": the tensor is its first letter).
template <typename E>
struct TrainE { using type = E; };
template <typename T, typename F>
static int train_with_etype(const char* what, const char* arg, int dtype, F&& f) {
    if constexpr (sizeof(T) == 8) {
        UNI_REQUIRE(dtype == 0, "%s: %s %d: the fp64 form takes fp64 %.1s (0) only", what, arg, dtype, arg);
        f(TrainE<double>());
    } else {
        UNI_REQUIRE(dtype >= 0 && dtype <= 2, "%s: %s %d is not 0 (fp32), 1 (fp16) or 2 (bf16)", what, arg, dtype);
        if (dtype == 0) f(TrainE<float>());
        else if (dtype == 1) f(TrainE<f16>());
        else f(TrainE<bf16>());
    }
    return 0;
}
// a plan's channels per lane V (train_vwidth: 8 for a half type E only) as a template argument: f(integral_constant<int, V>)
template <typename E, typename F>
static void train_with_vwidth(int V, F&& f) {
    if constexpr (sizeof(E) == 2) {
        if (V == 8) return f(std::integral_constant<int, 8>());
    }
    f(std::integral_constant<int, 4>());
}
// a channels-last plan's vectors per lane NV (lncf_plan: 1, 2, 3, 4, 6 or 8) next to its V as a template argument: f(integral_constant<int, NV>).
// 6 and 8 mean more than 256 vectors, which only V = 4 has
template <int V, typename F>
static void train_with_nv(int NV, F&& f) {
    switch (NV) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        default:
            if constexpr (V == 4) {
                if (NV == 6) f(std::integral_constant<int, 6>());
                else f(std::integral_constant<int, 8>());
            }
    }
}
// the partials of a backward that has them `wanted`: *part = ws, which must hold f32_bytes (twice that for T = double); otherwise null
template <typename T>
static int train_partials(const char* what, bool wanted, void* ws, size_t ws_bytes, size_t f32_bytes, T** part) {
    *part = wanted ? reinterpret_cast<T*>(ws) : nullptr;
    if (wanted) {
        const size_t need = f32_bytes * (sizeof(T) / 4);
        UNI_REQUIRE(ws && ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", what, ws ? ws_bytes : (size_t)0, need);
    }
    return 0;
}

// V consecutive elements in accesses of 16 bytes (8 for four halves), converted to / from the math type
template <typename E, int V, typename T>
__device__ __forceinline__ void vec_load(const E* p, T (&v)[V]) {
    constexpr int N = V * sizeof(E) >= 16 ? 16 / sizeof(E) : V;
    using vec = E __attribute__((ext_vector_type(N)));
#pragma unroll
    for (int k = 0; k < V / N; ++k) {
        const vec t = *reinterpret_cast<const vec*>(p + k * N);
#pragma unroll
        for (int i = 0; i < N; ++i) v[k * N + i] = (T)t[i];
    }
}
template <typename E, int V, typename T>
__device__ __forceinline__ void vec_store(E* p, const T (&v)[V]) {
    constexpr int N = V * sizeof(E) >= 16 ? 16 / sizeof(E) : V;
    using vec = E __attribute__((ext_vector_type(N)));
#pragma unroll
    for (int k = 0; k < V / N; ++k) {
        vec t;
#pragma unroll
        for (int i = 0; i < N; ++i) t[i] = (E)v[k * N + i];
        *reinterpret_cast<vec*>(p + k * N) = t;
    }
}

// The ordered reduce of per-block partial sums that dwln_train.hip, lncf_train.hip and down_train.hip share: part [R][N] -> out, two jobs in one launch.
// out[n] = sum over the R rows of part [R][N], rows in ascending order inside each of the four waves, then the waves in ascending order; double sums
struct DwlnRJob {
    const void* part;
    void *out1, *out2;                          // column n -> out1[n] for n < n1, else out2[n - n1]
    int R, N, n1, blocks;
};
template <typename T>
__global__ __launch_bounds__(256) void dwln_reduce_kernel(DwlnRJob j0, DwlnRJob j1) {
    __shared__ double sm[4][64];
    const bool first = (int)blockIdx.x < j0.blocks;
    const int b = first ? blockIdx.x : blockIdx.x - j0.blocks;
    const T* part = reinterpret_cast<const T*>(first ? j0.part : j1.part);
    T* out1 = reinterpret_cast<T*>(first ? j0.out1 : j1.out1);
    T* out2 = reinterpret_cast<T*>(first ? j0.out2 : j1.out2);
    const int R = first ? j0.R : j1.R, N = first ? j0.N : j1.N, n1 = first ? j0.n1 : j1.n1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = b * 64 + lane;
    double a = 0;
    if (n < N)
        for (int r = wave; r < R; r += 4) a += (double)part[(size_t)r * N + n];
    sm[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && n < N) {
        a = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
        if (n < n1) out1[n] = (T)a;
        else out2[n - n1] = (T)a;
    }
}
// one job alone: the partials [rows][2][C] of a LayerNorm backward -> gw [C], gb [C]; `op` is the operator in the tag `<op> reduce<f32>`
template <typename T>
static void train_reduce_2c(const T* part, int rows, int C, T* gw, T* gb, const char* op, hipStream_t s) {
    const DwlnRJob none{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    const DwlnRJob job{part, gw, gb, rows, 2 * C, C, cdiv(2 * C, 64)};
    uni_variant_note("%s reduce<%s>", op, train_ename(0, sizeof(T) == 8));
    hipLaunchKernelGGL((dwln_reduce_kernel<T>), dim3(job.blocks), dim3(256), 0, s, none, job);
}
