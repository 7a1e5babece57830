// The MOT instance-contrastive loss of training (unicorn/models/unicorn.py:407-466, compute_loss_mot_corr) for a whole batch, forward and
// backward, fp32 and fp64, in a constant number of launches and without a host read: the instance counts and the labels are found on the
// device from `targets`.
//
//   targets [B][2][M][6] fp32 rows (cls, cx, cy, w, h, trackid).  Per sample b and frame f:
//   n_f      = number of rows with trackid != 0; the instances are the FIRST n_f rows (the reference's range(n_f))
//   row[i]   = smallest j < n1 with id1[j] == id0[i], else -1;  col[j] = LARGEST i < n0 with row[i] == j, else -1 (bidirect only)
//   E_f[i]   = the embedding of frame f at the centre of instance i:
//              grid_sample  g = (clamp(c / s - 0.5, 0, size-1) / (size-1) - 0.5) * 2 in fp32, then grid_sample(align_corners=False, border):
//                           x = clip(((g + 1) size - 1) / 2, 0, size-1) in the embedding's type, bilinear over the in-range corners
//              otherwise    the one pixel rint(clamp(c / s, 0, size-1)) (half to even)
//   S        = E_0 E_1^T;  loss_b = 0.5 (CE(S, row) + CE(S^T, col)), or CE(S, row); CE = mean over the labelled rows, so a sample
//              without a matched pair (or without instances) gives NaN, and a gradient of exactly zero.
//
//   mc_prep_kernel     block = sample: counts, labels, |R| and |Q|, the corner pixel and the two fractions of every instance
//   mc_gather_kernel   block = (instance, frame, sample), thread = channel: E_f through the element strides of the map
//   mc_sim_kernel      32 x 32 tile of S per block from LDS tiles, plain FMAs with double accumulators (the product is ~2.6 MFLOP at
//                      100 x 100 x 128; a product of two fp32 values is exact in double, so the fp32 S is rounded once)
//   mc_lse_kernel      wave = one row (or column) of S: max-subtracted log-sum-exp, kept in double in both precisions
//   mc_loss_kernel     block = sample: sum of lse - S[label] over the labelled rows / columns in a fixed tree, the two means
//   backward: the four kernels above again (nothing is kept between the calls), then
//   mc_ds_kernel       dS in place of S
//   mc_de_kernel       block = (instance, frame, sample), thread = channel: dE_0 = dS E_1, dE_1 = dS^T E_0, summed in index order
//   mc_zero_kernel     the dense gradient maps, through their strides
//   mc_scatter_kernel  thread = (sample, frame, channel) walks the instances in index order and adds weight * dE into the one to four
//                      source pixels: one writer per element and a fixed order, so instances that share a pixel need no atomic.
//
// No float atomic anywhere (integer LDS atomics count); two runs give the same bits.  The file is compiled without FMA contraction so
// that the coordinate lines round like the reference's separate tensor operations; the dot products call fma explicitly.
// The sums over instances (S, the log-sum-exps, the loss, dE) are accumulated in double in the fp32 form as well.
#include <algorithm>
#include <utility>

#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int MC_TB = 256;
constexpr int MC_TILE = 32;
constexpr int MC_MAXM = 1024;

struct McLayout { size_t meta, lab, pix, frac, E, S, lse, dE, total; };      // byte offsets, each 256-aligned
McLayout mc_layout(int B, int M, int C, size_t es) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t bm = (size_t)B * M;
    McLayout l;
    l.meta = 0;                                   // [B][4] int: n0, n1, |R|, |Q|
    l.lab = al(l.meta + (size_t)B * 4 * 4);       // [B][2][M] int: row, col
    l.pix = al(l.lab + bm * 2 * 4);               // [B][2][M][2] int: x0, y0
    l.frac = al(l.pix + bm * 4 * 4);              // [B][2][M][2] T: x - x0, y - y0
    l.E = al(l.frac + bm * 4 * es);               // [B][2][M][C] T
    l.S = al(l.E + bm * 2 * C * es);              // [B][M][M] T, dS in the backward
    l.lse = al(l.S + bm * M * es);                // [B][2][M] double
    l.dE = al(l.lse + bm * 2 * 8);                // [B][2][M][C] T
    l.total = al(l.dE + bm * 2 * C * es);
    return l;
}
bool mc_shape_ok(int B, int M, int C) { return B >= 1 && B <= 65535 && M >= 1 && M <= MC_MAXM && C >= 1 && C <= 1024; }

__device__ __forceinline__ float mc_exp(float x) { return expf(x); }
__device__ __forceinline__ double mc_exp(double x) { return exp(x); }
template <typename T>
__device__ __forceinline__ T mc_wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// one axis of the sampling position: c = box centre in input pixels, n = size of the map along the axis
template <typename T>
__device__ __forceinline__ void mc_coord(float c, float s, int n, bool grid, int& p0, T& fr) {
    if (grid) {
        const float q = c / s - 0.5f;
        const float g = (fminf(fmaxf(q, 0.f), (float)(n - 1)) / (float)(n - 1) - 0.5f) * 2.0f;      // unicorn.py:435-437, fp32
        T x = (((T)g + 1) * n - 1) / 2;                                                             // grid_sample's un-normalise ...
        x = x > 0 ? x : (T)0;                                                                       // ... and border clip (a NaN becomes 0)
        x = x < (T)(n - 1) ? x : (T)(n - 1);
        const T fl = floor(x);
        p0 = (int)fl;
        fr = x - fl;
    } else {
        const float q = fminf(fmaxf(c / s, 0.f), (float)(n - 1));                                    // :442-444
        p0 = (int)rintf(q);
        fr = 0;
    }
    p0 = min(max(p0, 0), n - 1);
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_prep_kernel(const float* __restrict__ targets, int M, int H, int W, float stride, int flags, int* __restrict__ meta, int* __restrict__ lab,
               int* __restrict__ pix, T* __restrict__ frac) {
    __shared__ int s_n[2], s_cnt[2];
    __shared__ int s_row[MC_MAXM];
    __shared__ float s_id1[MC_MAXM];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* tg = targets + (size_t)b * 2 * M * 6;
    if (t < 2) { s_n[t] = 0; s_cnt[t] = 0; }
    __syncthreads();
    for (int e = t; e < 2 * M; e += MC_TB) {
        const float id = tg[(size_t)e * 6 + 5];
        if (e >= M) s_id1[e - M] = id;
        if (id != 0.f) atomicAdd(&s_n[e / M], 1);
    }
    __syncthreads();
    const int n0 = s_n[0], n1 = s_n[1];
    for (int i = t; i < M; i += MC_TB) {
        int r = -1;
        if (i < n0) {
            const float a = tg[(size_t)i * 6 + 5];
            for (int j = 0; j < n1; ++j)
                if (a == s_id1[j]) { r = j; break; }
        }
        s_row[i] = r;
        lab[((size_t)b * 2 + 0) * M + i] = r;
        if (r >= 0) atomicAdd(&s_cnt[0], 1);
    }
    __syncthreads();
    for (int j = t; j < M; j += MC_TB) {
        int c = -1;
        if ((flags & 1) && j < n1)
            for (int i = n0 - 1; i >= 0; --i)
                if (s_row[i] == j) { c = i; break; }
        lab[((size_t)b * 2 + 1) * M + j] = c;
        if (c >= 0) atomicAdd(&s_cnt[1], 1);
    }
    for (int e = t; e < 2 * M; e += MC_TB) {
        int x0 = 0, y0 = 0;
        T fx = 0, fy = 0;
        if (e % M < s_n[e / M]) {
            mc_coord<T>(tg[(size_t)e * 6 + 1], stride, W, flags & 2, x0, fx);
            mc_coord<T>(tg[(size_t)e * 6 + 2], stride, H, flags & 2, y0, fy);
        }
        const size_t o = ((size_t)b * 2 * M + e) * 2;
        pix[o] = x0;
        pix[o + 1] = y0;
        frac[o] = fx;
        frac[o + 1] = fy;
    }
    __syncthreads();
    if (t == 0) {
        meta[b * 4 + 0] = n0;
        meta[b * 4 + 1] = n1;
        meta[b * 4 + 2] = s_cnt[0];
        meta[b * 4 + 3] = s_cnt[1];
    }
}

// the corners of one instance in the order nw, ne, sw, se: offsets relative to (b, c = 0), grid_sample's weights (nw = (x0 + 1 - x)(y0 + 1 - y),
// ...) and a bit per corner that is used: a corner outside the map is left out, as is every corner but the first without grid_sample
template <typename T>
struct McCorners { long long off[4]; T w[4]; int use; };
template <typename T>
__device__ __forceinline__ McCorners<T> mc_corners(const int* __restrict__ pix, const T* __restrict__ frac, size_t inst, McStride st, int H, int W,
                                                   bool grid) {
    const int x0 = pix[inst * 2], y0 = pix[inst * 2 + 1];
    const T fx = frac[inst * 2], fy = frac[inst * 2 + 1];
    const T gx = 1 - fx, gy = 1 - fy;
    const bool xok = grid && x0 + 1 < W, yok = grid && y0 + 1 < H;
    McCorners<T> q;
    q.off[0] = y0 * st.y + x0 * st.x;
    q.off[1] = q.off[0] + st.x;
    q.off[2] = q.off[0] + st.y;
    q.off[3] = q.off[2] + st.x;
    q.w[0] = grid ? gx * gy : (T)1;
    q.w[1] = fx * gy;
    q.w[2] = gx * fy;
    q.w[3] = fx * fy;
    q.use = 1 | (xok ? 2 : 0) | (yok ? 4 : 0) | (xok && yok ? 8 : 0);
    return q;
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_gather_kernel(const T* __restrict__ e0, const T* __restrict__ e1, McStride s0, McStride s1, const int* __restrict__ meta,
                 const int* __restrict__ pix, const T* __restrict__ frac, int M, int C, int H, int W, int flags, T* __restrict__ E) {
    const int i = blockIdx.x, f = blockIdx.y, b = blockIdx.z;
    if (i >= meta[b * 4 + f]) return;
    const McStride st = f ? s1 : s0;
    const size_t inst = ((size_t)b * 2 + f) * M + i;
    const McCorners<T> q = mc_corners<T>(pix, frac, inst, st, H, W, flags & 2);
    const T* src = (f ? e1 : e0) + b * st.b;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const T* p = src + c * st.c;
        T v = q.w[0] * p[q.off[0]];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (q.use >> k & 1) v += q.w[k] * p[q.off[k]];
        E[inst * C + c] = v;
    }
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_sim_kernel(const T* __restrict__ E, const int* __restrict__ meta, int M, int C, T* __restrict__ S) {
    __shared__ T As[MC_TILE][MC_TILE + 1], Bs[MC_TILE][MC_TILE + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * MC_TILE, j0 = blockIdx.x * MC_TILE, t = threadIdx.x;
    const int n0 = meta[b * 4], n1 = meta[b * 4 + 1];
    if (i0 >= n0 || j0 >= n1) return;
    const T* E0 = E + (size_t)b * 2 * M * C;
    const T* E1 = E0 + (size_t)M * C;
    const int tx = t & 15, ty = t >> 4;
    double a00 = 0, a01 = 0, a10 = 0, a11 = 0;      // fp32 products are exact in double: S is rounded once
    for (int k0 = 0; k0 < C; k0 += MC_TILE) {
        for (int e = t; e < MC_TILE * MC_TILE; e += MC_TB) {
            const int r = e >> 5, k = e & 31;
            const bool kok = k0 + k < C;
            As[r][k] = (kok && i0 + r < n0) ? E0[(size_t)(i0 + r) * C + k0 + k] : (T)0;
            Bs[r][k] = (kok && j0 + r < n1) ? E1[(size_t)(j0 + r) * C + k0 + k] : (T)0;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < MC_TILE; ++k) {
            const double x0 = As[ty][k], x1 = As[ty + 16][k], y0 = Bs[tx][k], y1 = Bs[tx + 16][k];
            a00 = fma(x0, y0, a00);
            a01 = fma(x0, y1, a01);
            a10 = fma(x1, y0, a10);
            a11 = fma(x1, y1, a11);
        }
        __syncthreads();
    }
    T* Sb = S + (size_t)b * M * M;
    const int i = i0 + ty, j = j0 + tx;
    if (i < n0 && j < n1) Sb[(size_t)i * M + j] = (T)a00;
    if (i < n0 && j + 16 < n1) Sb[(size_t)i * M + j + 16] = (T)a01;
    if (i + 16 < n0 && j < n1) Sb[(size_t)(i + 16) * M + j] = (T)a10;
    if (i + 16 < n0 && j + 16 < n1) Sb[(size_t)(i + 16) * M + j + 16] = (T)a11;
}

// block (one wave) = row i of S (dir 0) or column i (dir 1)
template <typename T>
__global__ void __launch_bounds__(64)
mc_lse_kernel(const T* __restrict__ S, const int* __restrict__ meta, int M, double* __restrict__ lse) {
    const int i = blockIdx.x, dir = blockIdx.y, b = blockIdx.z;
    const int ns = meta[b * 4 + dir], no = meta[b * 4 + 1 - dir];
    if (i >= ns || no == 0) return;
    const T* p = S + (size_t)b * M * M + (dir ? (size_t)i : (size_t)i * M);
    const size_t step = dir ? M : 1;
    T m = -INFINITY;
    for (int k = threadIdx.x; k < no; k += 64) {
        const T v = p[k * step];
        m = v > m ? v : m;
    }
    m = mc_wave_max(m);
    double sum = 0;
    for (int k = threadIdx.x; k < no; k += 64) sum += (double)mc_exp(p[k * step] - m);
    sum = wave_sum(sum);
    if (threadIdx.x == 0) lse[((size_t)b * 2 + dir) * M + i] = (double)m + log(sum);
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_loss_kernel(const T* __restrict__ S, const double* __restrict__ lse, const int* __restrict__ meta, const int* __restrict__ lab, int M, int flags,
               T* __restrict__ loss) {
    __shared__ double sm[MC_TB / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n0 = meta[b * 4], n1 = meta[b * 4 + 1];
    const T* Sb = S + (size_t)b * M * M;
    const int* row = lab + (size_t)b * 2 * M;
    const int* col = row + M;
    const double* l0 = lse + (size_t)b * 2 * M;
    const double* l1 = l0 + M;
    double ar = 0, ac = 0;
    for (int i = t; i < n0; i += MC_TB) {
        const int r = row[i];
        if (r >= 0) ar += l0[i] - Sb[(size_t)i * M + r];
    }
    ar = block_sum<MC_TB>(ar, sm);
    if (flags & 1) {
        for (int j = t; j < n1; j += MC_TB) {
            const int c = col[j];
            if (c >= 0) ac += l1[j] - Sb[(size_t)c * M + j];
        }
        ac = block_sum<MC_TB>(ac, sm);
    }
    if (t == 0) {
        const double cr = ar / (double)meta[b * 4 + 2];                    // 0 / 0 = NaN: no labelled row
        loss[b] = (T)((flags & 1) ? 0.5 * (cr + ac / (double)meta[b * 4 + 3]) : cr);
    }
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_ds_kernel(T* __restrict__ S, const double* __restrict__ lse, const int* __restrict__ meta, const int* __restrict__ lab, const T* __restrict__ gout,
             int M, int flags) {
    const int j = blockIdx.x * MC_TB + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    if (i >= meta[b * 4] || j >= meta[b * 4 + 1]) return;
    const int r = lab[(size_t)b * 2 * M + i], c = lab[((size_t)b * 2 + 1) * M + j];
    const T g = gout[b];
    const size_t idx = ((size_t)b * M + i) * M + j;
    const T s = S[idx];
    T d = 0;
    if (flags & 1) {
        if (r >= 0) d += g * ((T)0.5 / (T)meta[b * 4 + 2]) * (mc_exp((T)(s - lse[(size_t)b * 2 * M + i])) - (T)(j == r));
        if (c >= 0) d += g * ((T)0.5 / (T)meta[b * 4 + 3]) * (mc_exp((T)(s - lse[((size_t)b * 2 + 1) * M + j])) - (T)(i == c));
    } else if (r >= 0) {
        d = g * ((T)1 / (T)meta[b * 4 + 2]) * (mc_exp((T)(s - lse[(size_t)b * 2 * M + i])) - (T)(j == r));
    }
    S[idx] = d;
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_de_kernel(const T* __restrict__ dS, const T* __restrict__ E, const int* __restrict__ meta, int M, int C, int want0, int want1,
             T* __restrict__ dE) {
    const int i = blockIdx.x, f = blockIdx.y, b = blockIdx.z;
    if (!(f ? want1 : want0) || i >= meta[b * 4 + f]) return;
    const int no = meta[b * 4 + 1 - f];
    const T* Eo = E + ((size_t)b * 2 + 1 - f) * M * C;
    const T* d = dS + (size_t)b * M * M + (f ? (size_t)i : (size_t)i * M);
    const size_t step = f ? M : 1;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double acc = 0;
        for (int k = 0; k < no; ++k) acc = fma((double)d[k * step], (double)Eo[(size_t)k * C + c], acc);
        dE[(((size_t)b * 2 + f) * M + i) * C + c] = (T)acc;
    }
}

template <typename T>
__global__ void __launch_bounds__(MC_TB)
mc_zero_kernel(T* __restrict__ g0, T* __restrict__ g1, McStride s0, McStride s1, int C, int H, int W, int c_inner0, int c_inner1) {
    const int b = blockIdx.y, f = blockIdx.z;
    T* dst = f ? g1 : g0;
    if (!dst) return;
    const McStride st = f ? s1 : s0;
    const bool c_inner = f ? c_inner1 : c_inner0;
    dst += b * st.b;
    const unsigned total = (unsigned)C * H * W;
    for (unsigned e = blockIdx.x * MC_TB + threadIdx.x; e < total; e += gridDim.x * MC_TB) {
        unsigned c, y, x;
        if (c_inner) { c = e % C; x = (e / C) % W; y = e / C / W; }      // the order of the writes only: every element is written either way
        else { x = e % W; y = (e / W) % H; c = e / W / H; }
        dst[c * st.c + y * st.y + x * st.x] = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(64)
mc_scatter_kernel(const T* __restrict__ dE, const int* __restrict__ meta, const int* __restrict__ pix, const T* __restrict__ frac, T* __restrict__ g0,
                  T* __restrict__ g1, McStride s0, McStride s1, int M, int C, int H, int W, int flags) {
    const int c = blockIdx.x * 64 + threadIdx.x, f = blockIdx.y, b = blockIdx.z;
    T* dst = f ? g1 : g0;
    if (!dst || c >= C) return;
    const McStride st = f ? s1 : s0;
    T* p = dst + b * st.b + c * st.c;
    const int n = meta[b * 4 + f];
    for (int i = 0; i < n; ++i) {                                        // index order: the one fixed order of the sums
        const size_t inst = ((size_t)b * 2 + f) * M + i;
        const McCorners<T> q = mc_corners<T>(pix, frac, inst, st, H, W, flags & 2);
        const T g = dE[inst * C + c];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q.use >> k & 1) p[q.off[k]] += q.w[k] * g;
    }
}

// the elements of a gradient map are distinct addresses: in the order of the strides, each stride covers the extent of the one before
bool mc_disjoint(McStride s, int B, int C, int H, int W) {
    std::pair<long long, long long> d[4] = {{s.b, B}, {s.c, C}, {s.y, H}, {s.x, W}};
    std::sort(d, d + 4);
    long long reach = 1;      // one more than the largest offset of the dimensions so far
    for (const auto& q : d) {
        if (q.second <= 1) continue;
        if (q.first < reach) return false;
        reach = q.first * (q.second - 1) + reach;
    }
    return true;
}

template <typename T>
int mc_check(const McArgs& a, const char* what) {
    UNI_REQUIRE(mc_shape_ok(a.B, a.M, a.C), "%s: shape B=%d M=%d C=%d outside 1 <= B <= 65535, 1 <= M <= 1024, 1 <= C <= 1024", what, a.B, a.M, a.C);
    UNI_REQUIRE(a.H >= 1 && a.W >= 1 && (size_t)a.C * a.H * a.W < ((size_t)1 << 31), "%s: map C=%d H=%d W=%d empty or C H W >= 2^31", what, a.C,
                a.H, a.W);
    UNI_REQUIRE(a.stride > 0.f, "%s: stride %g is not positive", what, (double)a.stride);
    UNI_REQUIRE((a.flags & ~3) == 0, "%s: flags %d unknown (1 = bidirect, 2 = grid_sample)", what, a.flags);
    const size_t need = mc_layout(a.B, a.M, a.C, 4).total * (sizeof(T) / 4);
    UNI_REQUIRE(a.ws_bytes >= need, "%s: workspace %zu < %zu", what, a.ws_bytes, need);
    UNI_REQUIRE(((uintptr_t)a.ws & 7) == 0, "%s: workspace must be 8-byte aligned", what);
    UNI_REQUIRE(a.s0.b >= 0 && a.s0.c >= 0 && a.s0.y >= 0 && a.s0.x >= 0 && a.s1.b >= 0 && a.s1.c >= 0 && a.s1.y >= 0 && a.s1.x >= 0,
                "%s: negative embedding stride", what);
    return 0;
}

// counts, labels, sampled embeddings, S and the log-sum-exps into the workspace: the part the two calls share
template <typename T>
void mc_common(const McArgs& a, const McLayout& l, hipStream_t s) {
    char* w = reinterpret_cast<char*>(a.ws);
    int *meta = (int*)(w + l.meta), *lab = (int*)(w + l.lab), *pix = (int*)(w + l.pix);
    T *frac = (T*)(w + l.frac), *E = (T*)(w + l.E), *S = (T*)(w + l.S);
    double* lse = (double*)(w + l.lse);
    const int tiles = cdiv(a.M, MC_TILE), ct = std::min(MC_TB, cdiv(a.C, 64) * 64);
    mc_prep_kernel<T><<<a.B, MC_TB, 0, s>>>(a.targets, a.M, a.H, a.W, a.stride, a.flags, meta, lab, pix, frac);
    mc_gather_kernel<T><<<dim3(a.M, 2, a.B), ct, 0, s>>>((const T*)a.e0, (const T*)a.e1, a.s0, a.s1, meta, pix, frac, a.M, a.C, a.H, a.W, a.flags, E);
    mc_sim_kernel<T><<<dim3(tiles, tiles, a.B), MC_TB, 0, s>>>(E, meta, a.M, a.C, S);
    mc_lse_kernel<T><<<dim3(a.M, (a.flags & 1) ? 2 : 1, a.B), 64, 0, s>>>(S, meta, a.M, lse);
}

}  // namespace

size_t mot_corr_workspace_bytes(int B, int M, int C) {
    if (!mc_shape_ok(B, M, C)) return 0;
    return mc_layout(B, M, C, 4).total;
}

template <typename T>
int launch_mot_corr_fwd(const McArgs& a, T* loss, hipStream_t s) {
    if (int rc = mc_check<T>(a, "mot_corr_loss_fwd")) return rc;
    const McLayout l = mc_layout(a.B, a.M, a.C, sizeof(T));
    mc_common<T>(a, l, s);
    char* w = reinterpret_cast<char*>(a.ws);
    mc_loss_kernel<T><<<a.B, MC_TB, 0, s>>>((const T*)(w + l.S), (const double*)(w + l.lse), (const int*)(w + l.meta), (const int*)(w + l.lab), a.M,
                                            a.flags, loss);
    return 0;
}

template <typename T>
int launch_mot_corr_bwd(const McArgs& a, const T* gout, T* g0, McStride gs0, T* g1, McStride gs1, hipStream_t s) {
    if (int rc = mc_check<T>(a, "mot_corr_loss_bwd")) return rc;
    if (!g0 && !g1) return 0;
    UNI_REQUIRE(!g0 || mc_disjoint(gs0, a.B, a.C, a.H, a.W), "mot_corr_loss_bwd: strides of grad_embed_0 must be >= 1 and must not overlap");
    UNI_REQUIRE(!g1 || mc_disjoint(gs1, a.B, a.C, a.H, a.W), "mot_corr_loss_bwd: strides of grad_embed_1 must be >= 1 and must not overlap");
    const McLayout l = mc_layout(a.B, a.M, a.C, sizeof(T));
    mc_common<T>(a, l, s);
    char* w = reinterpret_cast<char*>(a.ws);
    const int *meta = (const int*)(w + l.meta), *lab = (const int*)(w + l.lab), *pix = (const int*)(w + l.pix);
    const T *frac = (const T*)(w + l.frac), *E = (const T*)(w + l.E);
    const double* lse = (const double*)(w + l.lse);
    T *S = (T*)(w + l.S), *dE = (T*)(w + l.dE);
    const int ct = std::min(MC_TB, cdiv(a.C, 64) * 64);
    mc_ds_kernel<T><<<dim3(cdiv(a.M, MC_TB), a.M, a.B), MC_TB, 0, s>>>(S, lse, meta, lab, gout, a.M, a.flags);
    mc_de_kernel<T><<<dim3(a.M, 2, a.B), ct, 0, s>>>(S, E, meta, a.M, a.C, g0 != nullptr, g1 != nullptr, dE);
    const size_t chw = (size_t)a.C * a.H * a.W;
    mc_zero_kernel<T><<<dim3((unsigned)std::min((size_t)1024, (chw + MC_TB - 1) / MC_TB), a.B, 2), MC_TB, 0, s>>>(g0, g1, gs0, gs1, a.C, a.H, a.W,
                                                                                                          gs0.c < gs0.x, gs1.c < gs1.x);
    mc_scatter_kernel<T><<<dim3(cdiv(a.C, 64), 2, a.B), 64, 0, s>>>(dE, meta, pix, frac, g0, g1, gs0, gs1, a.M, a.C, a.H, a.W, a.flags);
    return 0;
}

template int launch_mot_corr_fwd<float>(const McArgs&, float*, hipStream_t);
template int launch_mot_corr_fwd<double>(const McArgs&, double*, hipStream_t);
template int launch_mot_corr_bwd<float>(const McArgs&, const float*, float*, McStride, float*, McStride, hipStream_t);
template int launch_mot_corr_bwd<double>(const McArgs&, const double*, double*, McStride, double*, McStride, hipStream_t);
