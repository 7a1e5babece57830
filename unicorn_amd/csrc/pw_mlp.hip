// The point-wise middle of the ConvNeXt block's MLP for TRAINING (convnext.py:46-48: pwconv1 -> GELU -> pwconv2; the two GEMMs stay with the
// vendor library): the exact (erf) GELU forward, and a backward that REBUILDS a = gelu(h) from h instead of reading a kept copy, fp32 (h, a,
// grad_a, grad_h, grad_y fp32, fp16 or bf16, converted in registers; all arithmetic fp32) and fp64.
//
//   forward   a = gelu(h) = h Phi(h),  Phi(v) = (1 + erf(v / sqrt 2)) / 2
//   backward  a = gelu(h),  grad_h = grad_a * gelu'(h),  gelu'(v) = Phi(v) + v phi(v),  phi(v) = exp(-v^2 / 2) / sqrt(2 pi),
//             part1[block row][Hd] = the block's column sums of the UNROUNDED grad_h,  part2[block row][Co] = those of grad_y
//
//   pw_map_kernel<V, MODE>   rows = the M pixels, columns = the N hidden units, row pitch N.  A row is cut into nvec = N / V vectors of V
//                            consecutive columns (16 bytes: V = 4, or 8 for a half type with N % 8 == 0).  A block of 256 threads = RPB rows
//                            x L vectors (L a power of two, RPB = 256 / L; blockIdx.x = the column tile of L vectors, blockIdx.y = the row
//                            of partials): thread (slot, g) owns ONE vector of columns for the whole launch and walks the rows
//                            (blockIdx.y + k gridDim.y) RPB + slot, so its column sums stay in registers.  At the end the RPB slots of a
//                            column are added in ascending order in double (through LDS) into one row of partials.
//                            MODE 0: a = gelu(h).  1: a and / or grad_h and / or the partials, whatever is asked for.  2: column sums of x.
//   dwln_reduce_kernel       partials [R][N] -> grad_b1 and, as the second job of the same launch, grad_b2 (train_ops.h)
//
// Every element is read and then written by the same lane, so a may be h and grad_h may be grad_a.  One writer per element, no atomics, fixed
// summation orders: bitwise reproducible.  Element offsets are 64-bit; row indices fit 32 bits (M < 2^31 is required).
#include "kernels.h"
#include "train_ops.h"

template <typename T>
struct PwK {                                    // kernel arguments (by value)
    const void *h, *g;                          // MODE 0: h.  1: h, grad_a.  2: h = the map to sum
    void *a, *gh;
    T* part;
    int M, N;
};

template <typename T>
__device__ __forceinline__ T pw_erf(T v);
template <>
__device__ __forceinline__ float pw_erf<float>(float v) { return erff(v); }
template <>
__device__ __forceinline__ double pw_erf<double>(double v) { return erf(v); }
template <typename T>
__device__ __forceinline__ T pw_exp(T v);
template <>
__device__ __forceinline__ float pw_exp<float>(float v) { return expf(v); }
template <>
__device__ __forceinline__ double pw_exp<double>(double v) { return exp(v); }

template <typename T>
__device__ __forceinline__ T pw_Phi(T v) { return T(0.5) * (T(1) + pw_erf<T>(v * T(0.70710678118654752440))); }

template <typename T, typename E, int V, int MODE>
__global__ __launch_bounds__(256) void pw_map_kernel(PwK<T> p, int L, int lgL, unsigned ngroups) {
    const int tid = threadIdx.x;
    const int g = tid & (L - 1), slot = tid >> lgL, RPB = 256 >> lgL;
    const int vec = blockIdx.x * L + g;
    const bool vok = vec < p.N / V;
    const size_t c = (size_t)vec * V;
    T sum[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sum[j] = T(0);
    for (unsigned grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
        const long long row = (long long)grp * RPB + slot;
        if (!vok || row >= p.M) continue;
        const size_t e = (size_t)row * p.N + c;
        T hv[V];
        vec_load<E, V>(reinterpret_cast<const E*>(p.h) + e, hv);
        if (MODE == 2) {
#pragma unroll
            for (int j = 0; j < V; ++j) sum[j] += hv[j];
            continue;
        }
        T gv[V];
        if (MODE == 1 && (p.gh || p.part)) vec_load<E, V>(reinterpret_cast<const E*>(p.g) + e, gv);
        if (MODE == 0 || p.a) {
            T r[V];
#pragma unroll
            for (int j = 0; j < V; ++j) r[j] = hv[j] * pw_Phi(hv[j]);
            vec_store<E, V>(reinterpret_cast<E*>(p.a) + e, r);
        }
        if (MODE == 1 && (p.gh || p.part)) {
            T r[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const T v = hv[j];
                const T d = pw_Phi(v) + v * (pw_exp<T>(T(-0.5) * v * v) * T(0.39894228040143267794));
                r[j] = gv[j] * d;
                sum[j] += r[j];
            }
            if (p.gh) vec_store<E, V>(reinterpret_cast<E*>(p.gh) + e, r);
        }
    }
    if constexpr (MODE != 0) {
        if (p.part) {                           // uniform in the block.  The slots of a column in ascending order, in double.  A lane's own
            __shared__ double sm[256 * V];      // fp32 sum has M L / 65536 terms (1025 measured within the bound: tests/test_train_scale_gpu.py)
#pragma unroll
            for (int j = 0; j < V; ++j) sm[tid * V + j] = (double)sum[j];
            __syncthreads();
            if (slot == 0 && vok) {
                T r[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    double s = 0;
                    for (int k = 0; k < RPB; ++k) s += sm[((k << lgL) + g) * V + j];
                    r[j] = (T)s;
                }
                vec_store<T, V>(p.part + (size_t)blockIdx.y * p.N + c, r);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int pw_shape_refused(const char* what, int M, int Hd, int Co) {
    uni_set_error("%s: shape M=%d Hd=%d Co=%d is outside 1 <= M < 2^31, Hd %% 4 == 0, 4 <= Hd <= %d, Co %% 4 == 0, 4 <= Co <= %d", what, M, Hd, Co,
                  PW_MAX_H, PW_MAX_H);
    return -1;
}
size_t pw_mlp_workspace_bytes(int M, int Hd, int Co) { return pw_plan_workspace_bytes(M, Hd, Co); }

// launches MODE over the M x N map(s) of k with the element type E as pw_plan (train_plan.h) says; *rows = the rows of partials it writes
template <typename T, typename E, int MODE>
static void pw_launch(const char* note, PwK<T> k, int M, int N, int dtype, int* rows, hipStream_t s) {
    const PwPlan q = pw_plan(M, N, sizeof(E));
    *rows = q.rows;
    k.M = M;
    k.N = N;
    char cls[32] = "";
    if (train_tracing()) pw_plan_class(q, train_ename(dtype, sizeof(T) == 8), cls, sizeof(cls));
    if (MODE == 0) uni_variant_note("pw_mlp act_fwd%s", cls);
    else if (MODE == 1) uni_variant_note("pw_mlp act_bwd%s %s", cls, note);
    else uni_variant_note("pw_mlp colsum%s", cls);
    train_with_vwidth<E>(q.V, [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        hipLaunchKernelGGL((pw_map_kernel<T, E, V, MODE>), dim3(q.grid_x, q.grid_y), dim3(q.block), 0, s, k, 1 << q.lg, q.lg, q.ngroups);
    });
}

template <typename T>
int launch_pw_mlp_act_fwd(const void* h, int h_dtype, int M, int Hd, void* a, hipStream_t s) {
    if (!pw_shape_ok(M, Hd, 4)) return pw_shape_refused("pw_mlp_act_fwd", M, Hd, 4);
    UNI_REQUIRE(aligned16(h) && aligned16(a), "pw_mlp_act_fwd: a pointer is not 16-byte aligned");
    int rows;
    const PwK<T> k{h, nullptr, a, nullptr, nullptr, 0, 0};
    if (int rc = train_with_etype<T>("pw_mlp_act_fwd", "h_dtype", h_dtype,
                                     [&](auto e) { pw_launch<T, typename decltype(e)::type, 0>("", k, M, Hd, h_dtype, &rows, s); }))
        return rc;
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_pw_mlp_act_bwd(const PwBwdArgs<T>& a, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!pw_shape_ok(a.M, a.Hd, a.Co)) return pw_shape_refused("pw_mlp_act_bwd", a.M, a.Hd, a.Co);
    const bool map = a.a || a.gh || a.gb1, col = a.gb2 != nullptr;
    UNI_REQUIRE(!map || (a.h && (a.ga || !(a.gh || a.gb1))), "pw_mlp_act_bwd: NULL h or grad_a next to an output that reads it");
    UNI_REQUIRE(!col || a.gy, "pw_mlp_act_bwd: NULL grad_y next to grad_b2");
    UNI_REQUIRE(aligned16(a.h) && aligned16(a.ga) && aligned16(a.a) && aligned16(a.gh) && aligned16(a.gb1) && aligned16(a.gy) && aligned16(a.gb2) &&
                    aligned16(ws), "pw_mlp_act_bwd: a pointer is not 16-byte aligned");
    // the element type is checked even where nothing is launched
    if (int rc = train_with_etype<T>("pw_mlp_act_bwd", "h_dtype", a.h_dtype, [](auto) {})) return rc;
    if (!map && !col) return 0;
    T* part;
    if (int rc = train_partials("pw_mlp_act_bwd", a.gb1 || col, ws, ws_bytes, pw_mlp_workspace_bytes(a.M, a.Hd, a.Co), &part)) return rc;
    T* part2 = part ? part + (size_t)PW_ROWS * a.Hd : nullptr;
    DwlnRJob j0{nullptr, nullptr, nullptr, 0, 0, 0, 0}, j1 = j0;
    if (map) {
        char note[32];
        snprintf(note, sizeof(note), "a=%d gh=%d gb=%d", a.a != nullptr, a.gh != nullptr, a.gb1 != nullptr);
        const PwK<T> k{a.h, a.ga, a.a, a.gh, a.gb1 ? part : nullptr, 0, 0};
        int rows;
        train_with_etype<T>("pw_mlp_act_bwd", "h_dtype", a.h_dtype,
                            [&](auto e) { pw_launch<T, typename decltype(e)::type, 1>(note, k, a.M, a.Hd, a.h_dtype, &rows, s); });
        if (a.gb1) j0 = DwlnRJob{part, a.gb1, nullptr, rows, a.Hd, a.Hd, cdiv(a.Hd, 64)};
    }
    if (col) {
        const PwK<T> k{a.gy, nullptr, nullptr, nullptr, part2, 0, 0};
        int rows;
        train_with_etype<T>("pw_mlp_act_bwd", "h_dtype", a.h_dtype,
                            [&](auto e) { pw_launch<T, typename decltype(e)::type, 2>("", k, a.M, a.Co, a.h_dtype, &rows, s); });
        j1 = DwlnRJob{part2, a.gb2, nullptr, rows, a.Co, a.Co, cdiv(a.Co, 64)};
    }
    if (j0.blocks + j1.blocks) {
        uni_variant_note("pw_mlp reduce<%s>", train_ename(0, sizeof(T) == 8));
        hipLaunchKernelGGL((dwln_reduce_kernel<T>), dim3(j0.blocks + j1.blocks), dim3(256), 0, s, j0, j1);
    }
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template int launch_pw_mlp_act_fwd<float>(const void*, int, int, int, void*, hipStream_t);
template int launch_pw_mlp_act_fwd<double>(const void*, int, int, int, void*, hipStream_t);
template int launch_pw_mlp_act_bwd<float>(const PwBwdArgs<float>&, void*, size_t, hipStream_t);
template int launch_pw_mlp_act_bwd<double>(const PwBwdArgs<double>&, void*, size_t, hipStream_t);
