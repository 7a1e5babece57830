// GroupNorm + activation for TRAINING: what every BaseConv of the YOLOX-PAFPN and of the head runs after convert_bn_model_to_gn
// (network_blocks.py:29-51: act(bn(conv(x))) with bn = GroupNorm(16, C, eps=1e-3), act = SiLU), the CondInst mask branch (GroupNorm + ReLU)
// and unicorn.py:38 (GroupNorm(32, C), no activation): forward with per-(sample, group) statistics and a deterministic backward that
// recomputes xhat, z and act'(z); fp32 (x / grad_x fp32, fp16 or bf16, converted in registers; all arithmetic fp32) and fp64.
//
//   forward   mean, var over the cpg H W elements of a (n, group), cpg = C / G; rstd = 1 / sqrt(var + eps); z = (x - mean) rstd weight[c] + bias[c];
//             y = act(z), act = none (0), ReLU (1) or SiLU z sigmoid(z) (3); stats [B G][2] = mean, rstd
//   backward  xhat = (x - mean) rstd, dz = grad_y act'(z); per (n, c): S1 = sum_hw dz, S2 = sum_hw dz xhat; grad_bias[c] = sum_n S1, grad_weight[c] =
//             sum_n S2; per (n, g), m = cpg H W: A = sum_c weight[c] S1, Bq = sum_c weight[c] S2; grad_x = rstd (weight[c] dz - (A + xhat Bq) / m)
//
// A block belongs to ONE image n and to one of the rpi rows of that image: row r takes the pixel units r, r + rpi, ... (train_plan.h: gn_plan).
//   gn_cl_kernel<V, MODE>     channels-last memory [B][H][W][C]: L lanes of V channels side by side on a pixel (blockIdx.y walks the column tiles of L
//                             vectors), 256 / L pixels per step.  A vector may hold channels of two groups (cpg = 6, 12): the statistics are looked up
//                             per channel.  Sums over the pixels of a block: a lane's own, then the 256 / L lanes of a column in ascending order through
//                             LDS in double.
//   gn_nchw_kernel<MODE>      NCHW-contiguous memory: lane = pixel, a wave reads 64 consecutive elements of a channel plane element-wise (no alignment
//                             is assumed), a wave takes one channel at a time, a block GN_NCHW_CT channels.  Sums: a lane's own, then the wave's
//                             butterfly in double.
//   MODE 0  forward, partial statistics: part[row][0][c] = the mean of channel c over the pixels of the row, [1][c] = the sum of squared deviations
//           from it (two passes over x: no E[x^2] - E[x]^2)        MODE 1  forward, y
//   MODE 2  backward, part[row][0][c] = sum dz xhat, [1][c] = sum dz                                                   MODE 3  backward, grad_x
//   gn_stats_kernel           partials -> stats: a block per (n, g) combines the (count, mean, M2) parts of its channels and rows (Chan et al., with the
//                             counts known) in double, a thread's items ascending, then the fixed tree of block_sum
//   gn_bwd_combine_kernel     partials -> A / m, Bq / m per (n, g) (a block each) and -> grad_weight, grad_bias (16 columns x 16 slices of rows per
//                             block, rows ascending inside a slice, then the slices ascending), both in double, both in ONE launch
//
// Every output element has one writer, no atomics, fixed summation orders: bitwise reproducible.  Element offsets are 64-bit.
#include "kernels.h"
#include "train_ops.h"

template <typename T>
struct GnK {                                    // kernel arguments (by value)
    const void* x;
    const T *w, *bias, *gy, *stats, *ab;
    T* y;
    void* gx;                                   // the element type of x
    T* part;
    int act, HW, C, cpg, G, unit, rpi, planes;
    unsigned upi;
};

template <typename T>
__device__ __forceinline__ T gn_act(T z, int act) {
    if (act == 1) return z > T(0) ? z : T(0);
    if (act == 3) return z / (T(1) + exp(-z));
    return z;
}
template <typename T>
__device__ __forceinline__ T gn_dact(T z, int act) {
    if (act == 1) return z > T(0) ? T(1) : T(0);
    if (act == 3) {
        const T s = T(1) / (T(1) + exp(-z));
        return s * (T(1) + z * (T(1) - s));
    }
    return T(1);
}

// v[j] <- the sum of v[j] over the 256 / L lanes of a column, slots in ascending order; valid in the lanes of slot 0
template <int V>
__device__ __forceinline__ void gn_slot_sum(double (&v)[V], double* sm, int tid, int col, int slot, int L) {
#pragma unroll
    for (int j = 0; j < V; ++j) sm[tid * V + j] = v[j];
    __syncthreads();
    if (slot == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            double a = 0;
            for (int t = col; t < 256; t += L) a += sm[t * V + j];
            v[j] = a;
        }
    }
    __syncthreads();
}

template <typename T, typename XT, int V, int MODE>
__global__ __launch_bounds__(256) void gn_cl_kernel(GnK<T> p, int lgL) {
    __shared__ double sm[(MODE == 0 || MODE == 2) ? 256 * V : 1];
    __shared__ T bc[MODE == 0 ? 256 * V : 1];
    const int tid = threadIdx.x, L = 1 << lgL, col = tid & (L - 1), slot = tid >> lgL, rpb = 256 >> lgL;
    const int C = p.C, n = blockIdx.x / p.rpi, r = blockIdx.x - n * p.rpi;
    const int vec = blockIdx.y * L + col, c0 = vec * V;
    const bool vok = vec < C / V;               // a block runs every barrier with all of its lanes: idle lanes add zeros
    const long long HW = p.HW;
    const size_t img = (size_t)n * HW * C + c0;
    const XT* xp = reinterpret_cast<const XT*>(p.x) + img;
    T wv[V], bv[V], mean[V], rstd[V], av[V], bq[V];
#pragma unroll
    for (int j = 0; j < V; ++j) wv[j] = bv[j] = mean[j] = rstd[j] = av[j] = bq[j] = T(0);
    if (MODE != 0 && vok) {
        vec_load<T, V>(p.w + c0, wv);
        vec_load<T, V>(p.bias + c0, bv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const size_t sg = (size_t)n * p.G + (c0 + j) / p.cpg;
            mean[j] = p.stats[sg * 2];
            rstd[j] = p.stats[sg * 2 + 1];
            if (MODE == 3) {
                av[j] = p.ab[sg * 2];
                bq[j] = p.ab[sg * 2 + 1];
            }
        }
    }
    double s1[V], s2[V];                        // MODE 0: sum x, sum (x - mean)^2; MODE 2: sum dz xhat, sum dz
    T f1[V], f2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0, f1[j] = f2[j] = T(0);
    for (int pass = 0; pass < (MODE == 0 ? 2 : 1); ++pass) {
        for (unsigned u = r; u < p.upi; u += p.rpi) {
            const long long q0 = (long long)u * p.unit, q1 = q0 + p.unit < HW ? q0 + p.unit : HW;
            for (long long q = q0 + slot; q < q1; q += rpb) {
                if (!vok) continue;
                const size_t e = (size_t)q * C;
                T xv[V];
                vec_load<XT, V>(xp + e, xv);
                if (MODE == 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        if (pass == 0) s1[j] += (double)xv[j];
                        else f2[j] += (xv[j] - mean[j]) * (xv[j] - mean[j]);
                    }
                } else if (MODE == 1) {
                    T o[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) o[j] = gn_act(((xv[j] - mean[j]) * rstd[j]) * wv[j] + bv[j], p.act);
                    vec_store<T, V>(p.y + img + e, o);
                } else {
                    T gv[V], o[V];
                    vec_load<T, V>(p.gy + img + e, gv);
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const T xh = (xv[j] - mean[j]) * rstd[j];
                        const T dz = gv[j] * gn_dact(xh * wv[j] + bv[j], p.act);
                        if (MODE == 2) {
                            f1[j] += dz * xh;
                            f2[j] += dz;
                        } else {
                            o[j] = rstd[j] * (wv[j] * dz - (av[j] + xh * bq[j]));
                        }
                    }
                    if (MODE == 3) vec_store<XT, V>(reinterpret_cast<XT*>(p.gx) + img + e, o);
                }
            }
        }
        if (MODE == 0 && pass == 0) {           // the mean of every channel over the pixels of this row, to all lanes of its column
            const double cnt = (double)gn_row_pixels(HW, p.unit, p.upi, p.rpi, r);
            gn_slot_sum<V>(s1, sm, tid, col, slot, L);
            if (slot == 0) {
#pragma unroll
                for (int j = 0; j < V; ++j) bc[col * V + j] = (T)(s1[j] / cnt);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < V; ++j) mean[j] = bc[col * V + j];
        }
    }
    if (MODE == 0 || MODE == 2) {
        T* row = p.part + (size_t)blockIdx.x * p.planes * C;
        if (MODE == 2) {
#pragma unroll
            for (int j = 0; j < V; ++j) s1[j] = (double)f1[j];
            gn_slot_sum<V>(s1, sm, tid, col, slot, L);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) s2[j] = (double)f2[j];
        if (MODE == 2 || p.planes == 2) gn_slot_sum<V>(s2, sm, tid, col, slot, L);      // uniform in the block
        if (slot == 0 && vok) {
            T o[V];
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = MODE == 0 ? mean[j] : (T)s1[j];
            vec_store<T, V>(row + c0, o);
            if (p.planes == 2) {
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = (T)s2[j];
                vec_store<T, V>(row + C + c0, o);
            }
        }
    }
}

template <typename T, typename XT, int MODE>
__global__ __launch_bounds__(256) void gn_nchw_kernel(GnK<T> p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int C = p.C, n = blockIdx.x / p.rpi, r = blockIdx.x - n * p.rpi;
    const long long HW = p.HW;
    for (int cc = wave; cc < GN_NCHW_CT; cc += 4) {
        const int c = blockIdx.y * GN_NCHW_CT + cc;
        if (c >= C) break;                      // uniform in the wave; no barrier in this kernel
        const size_t plane = ((size_t)n * C + c) * HW;
        const XT* xp = reinterpret_cast<const XT*>(p.x) + plane;
        T wc = T(0), bc = T(0), mean = T(0), rstd = T(0), av = T(0), bq = T(0);
        if (MODE != 0) {
            const size_t sg = (size_t)n * p.G + c / p.cpg;
            wc = p.w[c], bc = p.bias[c], mean = p.stats[sg * 2], rstd = p.stats[sg * 2 + 1];
            if (MODE == 3) av = p.ab[sg * 2], bq = p.ab[sg * 2 + 1];
        }
        double s1 = 0.0;
        T f1 = T(0), f2 = T(0);
        for (int pass = 0; pass < (MODE == 0 ? 2 : 1); ++pass) {
            for (unsigned u = r; u < p.upi; u += p.rpi) {
                const long long q0 = (long long)u * p.unit, q1 = q0 + p.unit < HW ? q0 + p.unit : HW;
                for (long long q = q0 + lane; q < q1; q += 64) {
                    const T xv = (T)xp[q];
                    if (MODE == 0) {
                        if (pass == 0) s1 += (double)xv;
                        else f2 += (xv - mean) * (xv - mean);
                    } else if (MODE == 1) {
                        p.y[plane + q] = gn_act(((xv - mean) * rstd) * wc + bc, p.act);
                    } else {
                        const T xh = (xv - mean) * rstd;
                        const T dz = p.gy[plane + q] * gn_dact(xh * wc + bc, p.act);
                        if (MODE == 2) {
                            f1 += dz * xh;
                            f2 += dz;
                        } else {
                            reinterpret_cast<XT*>(p.gx)[plane + q] = (XT)(rstd * (wc * dz - (av + xh * bq)));
                        }
                    }
                }
            }
            if (MODE == 0 && pass == 0) mean = (T)(wave_sum(s1) / (double)gn_row_pixels(HW, p.unit, p.upi, p.rpi, r));
        }
        if (MODE == 0 || MODE == 2) {
            T* row = p.part + (size_t)blockIdx.x * p.planes * C;
            const double a = MODE == 2 ? wave_sum((double)f1) : 0.0, b = wave_sum((double)f2);
            if (lane == 0) {
                row[c] = MODE == 0 ? mean : (T)a;
                if (p.planes == 2) row[C + c] = (T)b;
            }
        }
    }
}

// partials -> stats.  A block per (n, g); its items are the (row, channel of the group) pairs, item i = r cpg + cc, a thread takes the items tid,
// tid + 256, ... in ascending order (r and cc advance without a division), then block_sum (common.h: the lanes of a wave by the butterfly, the waves
// ascending), all in double.  Pass A: mean = sum n_r mean_i / (cpg H W) with n_r the pixels of row r.  Pass B: M2 = sum (M2_i + n_r (mean_i - mean)^2),
// the pairwise update of Chan et al. applied to parts whose counts are known: no division per item and no E[x^2] - E[x]^2.
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* part, T* stats, double eps, int planes, int HW, int C, int cpg, int G, int unit, int rpi,
                                                       unsigned upi, long long BG) {
    __shared__ double sm[4], mean_all;
    const int tid = threadIdx.x, items = cpg * rpi;             // <= C max(B, TRAIN_ROWS) / B: fits 32 bits
    const int dq = 256 / cpg, dr = 256 - dq * cpg, r0 = tid / cpg, c0 = tid - r0 * cpg;
    const GnRowCount rc = gn_row_count(HW, unit, upi, rpi);
    const double cnt = (double)cpg * HW;
    for (long long idx = blockIdx.x; idx < BG; idx += gridDim.x) {      // uniform in the block
        const long long n = idx / G;
        const int g = (int)(idx - n * G);
        const T* base = part + (size_t)n * rpi * planes * C + g * cpg;
        double s = 0;
        int r = r0, cc = c0;
#pragma unroll 4
        for (int i = tid; i < items; i += 256) {
            s += (double)gn_row_pixels(rc, r) * (double)base[(size_t)r * planes * C + cc];
            r += dq, cc += dr;
            if (cc >= cpg) cc -= cpg, ++r;
        }
        s = block_sum<256>(s, sm);
        if (tid == 0) mean_all = s / cnt;
        __syncthreads();
        const double mean = mean_all;           // the next write of mean_all lies behind the barriers of two block sums
        double q = 0;
        r = r0, cc = c0;
#pragma unroll 4
        for (int i = tid; i < items; i += 256) {
            const T* row = base + (size_t)r * planes * C + cc;
            const double d = (double)row[0] - mean;
            q += (planes == 2 ? (double)row[C] : 0.0) + (double)gn_row_pixels(rc, r) * d * d;
            r += dq, cc += dr;
            if (cc >= cpg) cc -= cpg, ++r;
        }
        q = block_sum<256>(q, sm);
        if (tid == 0) {
            stats[(size_t)idx * 2] = (T)mean;
            stats[(size_t)idx * 2 + 1] = (T)(1.0 / sqrt(q / cnt + eps));
        }
    }
}

// partials -> A / m, Bq / m per (n, g): a block each, the items and their order as in gn_stats_kernel; and -> grad_weight, grad_bias: a block takes
// GN_RED_COLS columns of [2 C] and sixteen slices of rows, a slice its rows r = slice, slice + 16, ... in ascending order, then the slices ascending.
// Both in double, both in ONE launch (the first ab_blocks blocks do the first job).
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_combine_kernel(const T* part, const T* w, T* ab, T* gw, T* gb, int HW, int C, int cpg, int G, int rpi, int rows,
                                                             long long BG, unsigned ab_blocks) {
    __shared__ double sm[256 / GN_RED_COLS][GN_RED_COLS];
    __shared__ double sm4[4];
    if (blockIdx.x < ab_blocks) {               // uniform in the block
        const int tid = threadIdx.x, items = cpg * rpi;
        const int dq = 256 / cpg, dr = 256 - dq * cpg, r0 = tid / cpg, c0 = tid - r0 * cpg;
        for (long long idx = blockIdx.x; idx < BG; idx += ab_blocks) {
            const long long n = idx / G;
            const int g = (int)(idx - n * G);
            const T* base = part + (size_t)n * rpi * 2 * C + g * cpg;
            double a = 0, b = 0;
            int r = r0, cc = c0;
#pragma unroll 4
            for (int i = tid; i < items; i += 256) {
                const T* row = base + (size_t)r * 2 * C + cc;
                const double wc = (double)w[g * cpg + cc];
                b += wc * (double)row[0];
                a += wc * (double)row[C];
                r += dq, cc += dr;
                if (cc >= cpg) cc -= cpg, ++r;
            }
            a = block_sum<256>(a, sm4);
            b = block_sum<256>(b, sm4);
            if (tid == 0) {
                const double m = (double)cpg * HW;
                ab[(size_t)idx * 2] = (T)(a / m);
                ab[(size_t)idx * 2 + 1] = (T)(b / m);
            }
        }
        return;
    }
    const int cb = threadIdx.x % GN_RED_COLS, slice = threadIdx.x / GN_RED_COLS;
    const int col = (blockIdx.x - ab_blocks) * GN_RED_COLS + cb;      // of [2 C]: grad_weight, then grad_bias; 2 C is a multiple of 8
    double a = 0;
    if (col < 2 * C) {
#pragma unroll 8
        for (int r = slice; r < rows; r += 256 / GN_RED_COLS) a += (double)part[(size_t)r * 2 * C + col];
    }
    sm[slice][cb] = a;
    __syncthreads();
    if (slice == 0 && col < 2 * C) {
        a = 0;
        for (int t = 0; t < 256 / GN_RED_COLS; ++t) a += sm[t][cb];
        if (col < C) gw[col] = (T)a;
        else gb[col - C] = (T)a;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t gn_act_train_workspace_bytes(int B, int H, int W, int C, int G) { return gn_plan_workspace_bytes(B, H, W, C, G); }

static const char* const GN_MODE[] = {"fwd_part", "fwd_apply", "bwd_part", "bwd_dx"};

// launches mode MODE with the element type XT of x as gn_plan (train_plan.h) says
template <typename T, typename XT, int MODE>
static void gn_launch(const GnArgs<T>& a, const GnPlan& q, const GnK<T>& k, const char* flags, hipStream_t s) {
    char cls[48] = "";
    if (train_tracing()) gn_plan_class(q, train_ename(a.x_dtype, sizeof(T) == 8), cls, sizeof(cls));
    uni_variant_note("gn_act %s_%s %s", GN_MODE[MODE], cls, flags);
    const dim3 grid(q.grid_x, q.grid_y);
    if (q.nchw) {
        hipLaunchKernelGGL((gn_nchw_kernel<T, XT, MODE>), grid, dim3(q.block), 0, s, k);
        return;
    }
    train_with_vwidth<XT>(q.V, [&](auto vtag) {
        hipLaunchKernelGGL((gn_cl_kernel<T, XT, decltype(vtag)::value, MODE>), grid, dim3(q.block), 0, s, k, q.lg);
    });
}

template <typename T, int MODE>
static int gn_dispatch(const char* what, const GnArgs<T>& a, const GnPlan& q, const GnK<T>& k, const char* flags, hipStream_t s) {
    return train_with_etype<T>(what, "x_dtype", a.x_dtype, [&](auto e) { gn_launch<T, typename decltype(e)::type, MODE>(a, q, k, flags, s); });
}

template <typename T>
static int gn_check(const char* what, const GnArgs<T>& a) {
    if (!gn_shape_ok(a.B, a.H, a.W, a.C, a.G)) {
        uni_set_error("%s: shape B=%d H=%d W=%d C=%d G=%d is outside B, H, W >= 1, C %% 4 == 0, 4 <= C <= %d, B H W < 2^31, 1 <= G <= C, C %% G == 0", what,
                      a.B, a.H, a.W, a.C, a.G, TRAIN_MAX_C);
        return -1;
    }
    UNI_REQUIRE(a.act == 0 || a.act == 1 || a.act == 3, "%s: act %d is not 0 (none), 1 (ReLU) or 3 (SiLU)", what, a.act);
    UNI_REQUIRE(aligned16(a.x) && aligned16(a.w) && aligned16(a.bias), "%s: a pointer is not 16-byte aligned", what);
    return 0;
}

template <typename T>
static GnK<T> gn_args(const GnArgs<T>& a, const GnPlan& q) {
    GnK<T> k{};
    k.x = a.x, k.w = a.w, k.bias = a.bias;
    k.act = a.act, k.HW = a.H * a.W, k.C = a.C, k.cpg = a.C / a.G, k.G = a.G, k.unit = q.unit, k.rpi = q.rpi, k.planes = 2, k.upi = q.upi;
    return k;
}

// The forward has no workspace: the partial statistics [rows][planes][C] lie in y, which the third launch overwrites completely.  They fit:
// rpi <= ceil(H W / 16), so planes rpi <= H W (planes = 1 where H W == 1); tools/train_plan_check.cpp holds every plan to it.
template <typename T>
int launch_gn_act_train_fwd(const GnArgs<T>& a, T* y, T* stats, hipStream_t s) {
    if (int rc = gn_check("gn_act_train_fwd", a)) return rc;
    UNI_REQUIRE(aligned16(y) && aligned16(stats), "gn_act_train_fwd: a pointer is not 16-byte aligned");
    UNI_REQUIRE(a.eps > 0, "gn_act_train_fwd: eps %g is not positive", a.eps);
    const GnPlan q = gn_plan(a.B, a.H, a.W, a.C, a.G, a.x_dtype ? 2 : (int)sizeof(T), a.nchw != 0);
    GnK<T> k = gn_args(a, q);
    k.planes = q.planes, k.part = y;
    char flags[16];
    std::snprintf(flags, sizeof(flags), "act=%d", a.act);
    if (int rc = gn_dispatch<T, 0>("gn_act_train_fwd", a, q, k, flags, s)) return rc;
    const long long BG = (long long)a.B * a.G;
    uni_variant_note("gn_act fwd_stats<%s>", train_ename(0, sizeof(T) == 8));
    hipLaunchKernelGGL((gn_stats_kernel<T>), dim3(q.comb_blocks), dim3(256), 0, s, y, stats, a.eps, q.planes, k.HW, a.C, k.cpg, a.G, q.unit, q.rpi, q.upi,
                       BG);
    k.part = nullptr, k.stats = stats, k.y = y;
    if (int rc = gn_dispatch<T, 1>("gn_act_train_fwd", a, q, k, flags, s)) return rc;
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_gn_act_train_bwd(const GnArgs<T>& a, const T* stats, const T* gy, void* gx, T* gw, T* gb, void* ws, size_t ws_bytes, hipStream_t s) {
    if (int rc = gn_check("gn_act_train_bwd", a)) return rc;
    UNI_REQUIRE((gw != nullptr) == (gb != nullptr), "gn_act_train_bwd: grad_weight and grad_bias come as a pair");
    UNI_REQUIRE(aligned16(stats) && aligned16(gy) && aligned16(gx) && aligned16(gw) && aligned16(gb) && aligned16(ws),
                "gn_act_train_bwd: a pointer is not 16-byte aligned");
    if (!gx && !gw) return 0;
    T* part;
    if (int rc = train_partials("gn_act_train_bwd", true, ws, ws_bytes, gn_act_train_workspace_bytes(a.B, a.H, a.W, a.C, a.G), &part)) return rc;
    const GnPlan q = gn_plan(a.B, a.H, a.W, a.C, a.G, a.x_dtype ? 2 : (int)sizeof(T), a.nchw != 0);
    GnK<T> k = gn_args(a, q);
    k.stats = stats, k.gy = gy, k.part = part;
    char flags[24];
    std::snprintf(flags, sizeof(flags), "act=%d gx=%d gwb=%d", a.act, gx != nullptr, gw != nullptr);
    if (int rc = gn_dispatch<T, 2>("gn_act_train_bwd", a, q, k, flags, s)) return rc;
    const long long BG = (long long)a.B * a.G;
    const unsigned ab_blocks = gx ? q.comb_blocks : 0, w_blocks = gw ? (unsigned)cdiv(2 * a.C, GN_RED_COLS) : 0;
    T* ab = part + q.off_ab;
    uni_variant_note("gn_act bwd_comb<%s> gx=%d gwb=%d", train_ename(0, sizeof(T) == 8), gx != nullptr, gw != nullptr);
    hipLaunchKernelGGL((gn_bwd_combine_kernel<T>), dim3(ab_blocks + w_blocks), dim3(256), 0, s, part, a.w, ab, gw, gb, k.HW, a.C, k.cpg, a.G, q.rpi, q.rows, BG,
                       ab_blocks);
    if (gx) {
        k.part = nullptr, k.ab = ab, k.gx = gx;
        if (int rc = gn_dispatch<T, 3>("gn_act_train_bwd", a, q, k, flags, s)) return rc;
    }
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template int launch_gn_act_train_fwd<float>(const GnArgs<float>&, float*, float*, hipStream_t);
template int launch_gn_act_train_fwd<double>(const GnArgs<double>&, double*, double*, hipStream_t);
template int launch_gn_act_train_bwd<float>(const GnArgs<float>&, const float*, const float*, void*, float*, float*, void*, size_t, hipStream_t);
template int launch_gn_act_train_bwd<double>(const GnArgs<double>&, const double*, const double*, void*, double*, double*, void*, size_t, hipStream_t);
