// The close of a ConvNeXt block for TRAINING (convnext.py:49-53): layer scale, per-sample drop-path factor, residual add, forward and backward,
// fp32 (y / grad_y fp32, fp16 or bf16, converted in registers; all arithmetic fp32) and fp64.
//
//   forward   out[n][c][h][w] = x[n][c][h][w] + (gamma[c] * y[n][h][w][c]) * s[n]                    x = residual, out in channels-last memory
//   backward  gs = x * s[n], grad_y[n][h][w][c] = gamma[c] * gs, part[block][c] = sum over the block's pixels of gs * y        x = grad_out
//
//   bt_cl_kernel<MODE>     x in channels-last memory: elementwise.  A lane owns V consecutive channels (4; 8 for half y when C % 8 == 0) of one
//                          pixel, the PP = 512 / (C / V) pixels a block takes at once are contiguous memory, a block walks chunks of 4 PP (2 PP for V = 8)
//                          pixels of one image and keeps its grad_gamma sums in registers; the PP lanes of a channel are added through LDS in
//                          ascending order.
//   bt_nchw_kernel<MODE>   x NCHW-contiguous: a tile of 64 pixels x 64 channels of one image goes through LDS.  It is read from global memory
//                          along the pixels of a channel plane (lane = pixel, wave = 16 of the channels) into tile[channel][pixel], pitch 65:
//                          the 32 lanes of a store group hit 32 banks.  It is read back with lane = (4 channels, pixel): the sixteen channel
//                          groups of a pixel are 256 contiguous bytes of y / out, and the pixel of a lane is rotated by two for the upper eight
//                          channel groups, so that the 32 lanes of a read group hit the banks 4 cg + j + {0, 1} and 4 (cg - 8) + j + {2, 3}: no
//                          conflict on either side in fp32 (the fp64 form, kept for checks, has two-way conflicts on the read side).
//   bt_reduce_kernel       part [R][C] -> grad_gamma: rows in ascending order inside each of the sixteen waves, then the waves in ascending
//                          order, double accumulation (the scheme of dwln_train.hip with more waves: a wave's row loads are a dependent chain)
//
// mode 0 = forward, 1 = backward.  A sample with s[n] == 0 is not read in y (forward) or in x and y (backward): out = residual, grad_y = 0 and
// nothing is added to grad_gamma, whatever y holds.  One writer per element, no atomics.  Element offsets are 64-bit; pixel indices are int.
#include "kernels.h"
#include "train_ops.h"

template <typename T>
struct BtK {                                    // kernel arguments (by value)
    const void* y;
    const T *x, *gamma, *scale;
    T* out;                                     // forward
    void* gy;                                   // backward, the element type of y
    T* part;
    int HW, C;
};

// one lane's V channels of one pixel: element offset e of out / grad_y; xv, yv = the V values of x and y (loaded by the caller where they are needed)
template <typename T, typename YT, int V, int MODE>
__device__ __forceinline__ void bt_pixel(const BtK<T>& p, size_t e, const T (&xv)[V], const T (&yv)[V], const T (&gam)[V], T s, bool live,
                                         T (&dg)[V]) {
    T r[V];
    if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = live ? xv[j] + (gam[j] * yv[j]) * s : xv[j];
        vec_store<T, V>(p.out + e, r);
        return;
    }
    if (p.gy) {
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = live ? gam[j] * (xv[j] * s) : T(0);
        vec_store<YT, V>(reinterpret_cast<YT*>(p.gy) + e, r);
    }
    if (live && p.part) {
#pragma unroll
        for (int j = 0; j < V; ++j) dg[j] += (xv[j] * s) * yv[j];
    }
}

// A chunk = BtU steps of PP pixels of ONE image (so the factor s is the same in the whole block); a block takes the chunks blockIdx.x,
// blockIdx.x + gridDim.x, ...  All loads of a chunk are issued before the first use, and the factor of the next chunk is fetched a chunk ahead.
template <typename T, typename YT, int V, int MODE>
__global__ __launch_bounds__(512) void bt_cl_kernel(BtK<T> p, int CG, int PP, unsigned cpi, unsigned nchunks) {
    constexpr int BT_U = BtU<V>::value;
    __shared__ T sm[MODE == 1 ? 512 * V : 1];
    const int tid = threadIdx.x;
    const int slot = tid / CG, cg = tid - slot * CG;
    const bool on = slot < PP;
    const int c = cg * V, C = p.C;
    const bool want_y = MODE == 0 || p.part != nullptr;
    T gam[V], dg[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        gam[j] = (on && p.gamma) ? p.gamma[c + j] : T(1);
        dg[j] = 0;
    }
    if (on) {
        unsigned t = blockIdx.x;                // < nchunks: the grid is no larger
        T s = p.scale ? p.scale[t / cpi] : T(1);
        while (t < nchunks) {
            const unsigned n = t / cpi, tn = t + gridDim.x;
            const long long q0 = (long long)(t - n * cpi) * (BT_U * PP) + slot;
            T sn = s;
            if (p.scale && tn < nchunks) sn = p.scale[tn / cpi];
            const bool live = s != T(0);
            T xv[BT_U][V] = {}, yv[BT_U][V] = {};
            size_t e[BT_U];
            bool ok[BT_U];
#pragma unroll
            for (int u = 0; u < BT_U; ++u) {
                const long long q = q0 + u * PP;
                ok[u] = q < p.HW;
                e[u] = ((size_t)n * p.HW + (size_t)q) * C + c;
                if (ok[u] && (MODE == 0 || live)) vec_load<T, V>(p.x + e[u], xv[u]);
                if (ok[u] && live && want_y) vec_load<YT, V>(reinterpret_cast<const YT*>(p.y) + e[u], yv[u]);
            }
#pragma unroll
            for (int u = 0; u < BT_U; ++u)
                if (ok[u]) bt_pixel<T, YT, V, MODE>(p, e[u], xv[u], yv[u], gam, s, live, dg);
            t = tn;
            s = sn;
        }
    }
    if (MODE == 1 && p.part) {                  // the block's PP pixel slots in ascending order -> one row of partials [C]
        if (on) {
#pragma unroll
            for (int j = 0; j < V; ++j) sm[slot * C + c + j] = dg[j];
        }
        __syncthreads();
        for (int ch = tid; ch < C; ch += blockDim.x) {
            T a = 0;
            for (int k = 0; k < PP; ++k) a += sm[k * C + ch];
            p.part[(size_t)blockIdx.x * C + ch] = a;
        }
    }
}

template <typename T, typename YT, int MODE>
__global__ __launch_bounds__(256) void bt_nchw_kernel(BtK<T> p, unsigned tpi, unsigned ntiles) {
    __shared__ T tile[BT_TILE][BT_TILE + 1];
    __shared__ T red[MODE == 1 ? 16 : 1][BT_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = p.C, HW = p.HW, c0 = blockIdx.y * BT_TILE;
    const int cg = lane & 15, pl = ((lane >> 4) + 2 * (cg >> 3)) & 3;
    const int c = c0 + cg * 4;
    const bool cok = c < C;
    const bool want_y = MODE == 0 || p.part != nullptr;
    T gam[4], dg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gam[j] = (cok && p.gamma) ? p.gamma[c + j] : T(1);
        dg[j] = 0;
    }
    unsigned t = blockIdx.x;                    // < ntiles: the grid is no larger
    T s = p.scale ? p.scale[t / tpi] : T(1);
    while (t < ntiles) {
        const unsigned n = t / tpi, tn = t + gridDim.x;
        const int q0 = (int)(t - n * tpi) * BT_TILE, left = HW - q0;       // pixels of the image from q0 on: > 0
        T sn = s;
        if (p.scale && tn < ntiles) sn = p.scale[tn / tpi];
        const bool live = s != T(0);            // the same in every thread of the block
        T yv[4][4] = {};
        size_t e[4];
        bool ok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {           // y of the four steps, in flight while the tile is staged
            const int kq = i * 16 + wave * 4 + pl;
            ok[i] = cok && kq < left;
            e[i] = ((size_t)n * HW + q0 + kq) * C + c;
            if (ok[i] && live && want_y) vec_load<YT, 4>(reinterpret_cast<const YT*>(p.y) + e[i], yv[i]);
        }
        if (MODE == 0 || live) {
            const T* plane = p.x + (size_t)n * C * HW + q0 + lane;
#pragma unroll
            for (int k = 0; k < BT_TILE / 4; ++k) {
                const int ch = k * 4 + wave;
                if (c0 + ch < C && lane < left) tile[ch][lane] = plane[(size_t)(c0 + ch) * HW];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (ok[i]) {
                const int kq = i * 16 + wave * 4 + pl;
                T xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = tile[cg * 4 + j][kq];
                bt_pixel<T, YT, 4, MODE>(p, e[i], xv, yv[i], gam, s, live, dg);
            }
        }
        __syncthreads();
        t = tn;
        s = sn;
    }
    if (MODE == 1 && p.part) {                  // the sixteen pixel slots of a channel in ascending order -> 64 columns of one row of partials
        const int slot = wave * 4 + (lane >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) red[slot][cg * 4 + j] = dg[j];
        __syncthreads();
        if (tid < BT_TILE && c0 + tid < C) {
            T a = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) a += red[k][tid];
            p.part[(size_t)blockIdx.x * C + c0 + tid] = a;
        }
    }
}

// out[c] = sum over the R rows of part [R][C]: rows in ascending order inside each of the sixteen waves (eight loads in flight), then the waves
// in ascending order; double sums
template <typename T>
__global__ __launch_bounds__(1024) void bt_reduce_kernel(const T* __restrict__ part, T* __restrict__ out, int R, int C) {
    __shared__ double sm[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double a = 0;
    if (c < C) {
        int r = wave;
        for (; r + 7 * 16 < R; r += 8 * 16) {
            T v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = part[(size_t)(r + k * 16) * C + c];
#pragma unroll
            for (int k = 0; k < 8; ++k) a += (double)v[k];
        }
        for (; r < R; r += 16) a += (double)part[(size_t)r * C + c];
    }
    sm[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && c < C) {
        double tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += sm[w][lane];
        out[c] = (T)tot;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t block_tail_workspace_bytes(int B, int H, int W, int C) { return bt_plan_workspace_bytes(B, H, W, C); }

// launches mode MODE with the element type YT of y as bt_plan (train_plan.h) says; *rows = the rows of partials it writes
template <typename T, typename YT, int MODE>
static void bt_launch(const BtArgs<T>& a, const BtK<T>& k, int* rows, hipStream_t s) {
    const BtPlan q = bt_plan(a.B, a.H, a.W, a.C, sizeof(YT), a.nchw != 0);
    *rows = q.rows;
    char cls[32] = "";
    if (train_tracing()) bt_plan_class(q, train_ename(a.y_dtype, sizeof(T) == 8), cls, sizeof(cls));
    uni_variant_note("block_tail %s_%s gy=%d gg=%d", MODE ? "bwd" : "fwd", cls, k.gy != nullptr, k.part != nullptr);
    if (q.nchw) {
        hipLaunchKernelGGL((bt_nchw_kernel<T, YT, MODE>), dim3(q.grid_x, q.grid_y), dim3(q.block), 0, s, k, q.per_image, q.units);
        return;
    }
    train_with_vwidth<YT>(q.V, [&](auto vtag) {
        constexpr int V = decltype(vtag)::value;
        hipLaunchKernelGGL((bt_cl_kernel<T, YT, V, MODE>), dim3(q.grid_x), dim3(q.block), 0, s, k, q.CG, q.PP, q.per_image, q.units);
    });
}

template <typename T, int MODE>
static int bt_dispatch(const BtArgs<T>& a, const BtK<T>& k, int* rows, hipStream_t s) {
    return train_with_etype<T>("block_tail", "y_dtype", a.y_dtype,
                               [&](auto e) { bt_launch<T, typename decltype(e)::type, MODE>(a, k, rows, s); });
}

template <typename T>
static int bt_check(const char* what, const BtArgs<T>& a) {
    if (!train_shape_ok(a.B, a.H, a.W, a.C)) return train_shape_refused(what, a.B, a.H, a.W, a.C);
    UNI_REQUIRE(aligned16(a.y) && aligned16(a.x), "%s: a pointer is not 16-byte aligned", what);      // gamma, scale: scalar reads
    return 0;
}

template <typename T>
int launch_block_tail_fwd(const BtArgs<T>& a, T* out, hipStream_t s) {
    if (int rc = bt_check("block_tail_fwd", a)) return rc;
    UNI_REQUIRE(aligned16(out), "block_tail_fwd: a pointer is not 16-byte aligned");
    const BtK<T> k{a.y, a.x, a.gamma, a.scale, out, nullptr, nullptr, a.H * a.W, a.C};
    int rows;
    if (int rc = bt_dispatch<T, 0>(a, k, &rows, s)) return rc;
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int launch_block_tail_bwd(const BtArgs<T>& a, void* gy, T* ggamma, void* ws, size_t ws_bytes, hipStream_t s) {
    if (int rc = bt_check("block_tail_bwd", a)) return rc;
    UNI_REQUIRE(aligned16(gy) && aligned16(ws), "block_tail_bwd: a pointer is not 16-byte aligned");
    if (!gy && !ggamma) return 0;
    T* part;
    if (int rc = train_partials("block_tail_bwd", ggamma != nullptr, ws, ws_bytes, block_tail_workspace_bytes(a.B, a.H, a.W, a.C), &part)) return rc;
    const BtK<T> k{a.y, a.x, a.gamma, a.scale, nullptr, gy, part, a.H * a.W, a.C};
    int rows;
    if (int rc = bt_dispatch<T, 1>(a, k, &rows, s)) return rc;
    if (ggamma) {
        uni_variant_note("block_tail reduce<%s>", train_ename(0, sizeof(T) == 8));
        hipLaunchKernelGGL((bt_reduce_kernel<T>), dim3(cdiv(a.C, 64)), dim3(1024), 0, s, (const T*)part, ggamma, rows, a.C);
    }
    UNI_CHECK_HIP(hipGetLastError());
    return 0;
}

template int launch_block_tail_fwd<float>(const BtArgs<float>&, float*, hipStream_t);
template int launch_block_tail_fwd<double>(const BtArgs<double>&, double*, hipStream_t);
template int launch_block_tail_bwd<float>(const BtArgs<float>&, void*, float*, void*, size_t, hipStream_t);
template int launch_block_tail_bwd<double>(const BtArgs<double>&, void*, double*, void*, size_t, hipStream_t);
