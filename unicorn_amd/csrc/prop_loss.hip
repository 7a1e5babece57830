// What stands around the label propagation in the SOT / VOS training losses (unicorn/models/unicorn.py:315-390, compute_loss_sot /
// compute_loss_vos), for a whole batch, fp32 and fp64, in a constant number of launches and without a host read.  The propagation
// itself (values @ softmax(E0^T E1)) stays with corr.hip / corr_bwd.hip; autograd joins the pieces (ops.sot_prop_loss / vos_prop_loss).
//
//   targets [B][2][M][6] fp32 rows (cls, cx, cy, w, h, trackid); maps of H8 x W8 pixels, images of H = 8 H8, W = 8 W8.
//
//   pl_match_kernel   block = sample.  VOS: for i = 0 .. M-1 with id0[i] != 0 the first j with id1[j] != 0 && id1[j] == id0[i] (fp32
//                     compare, :352-361); the matched i take the slots 0, 1, .. in the order of i, at most Kc of them.  matched[b][s] =
//                     (i, j), -1 behind num_matched[b].  SOT: one slot (0, 0) per sample (:324, :332 read row 0 whatever its id).
//   pl_label_kernel   thread = up to 4 neighbouring pixels of one slot and frame: the label row gt_f[b][s][H8 W8].
//                     boxes: F.interpolate(get_label_map(box), 1/8, bilinear) = the mean of the central 2 x 2 of every 8 x 8 block of the
//                            full-resolution box mask, which is never formed: corners cx -+ 0.5 w in fp32, rounded half to even, the start
//                            clamped to >= 0, the end with Python's slice rules (negative: size + end; above the size: clipped; end <= start:
//                            empty) -- the reference's labels[b, 0, y1:y2, x1:x2] = 1 (:521-533).
//                     masks: the bilinear 1/r of masks[b][0][i] and masks[b][1][j] (:365-366), r = 1, 2, 4: the pixel, the 2 x 2 block, the
//                            central 2 x 2 of the 4 x 4 block; fp32 or uint8 masks, read in place through the match table.
//   pl_fwd_kernel     thread = one 4 x 4 block of pred (B, Kc, H8, W8): its four p16 values (rows / cols 2y, 2y+1), its p32 value (rows / cols
//                     4y+1, 4y+2; :329-331, :372-374), and its share of sum x t, sum x^2, sum t^2; wave sums by shuffle, one partial triple
//                     per thread block into the workspace.  Sizes that are no multiple of 2 / 4 keep F.interpolate's floor: trailing rows and
//                     columns have no parent.
//   pl_final_kernel   wave = one Dice: the partials in a fixed order -> I, X2, T2 (kept in `sums` for the backward) and
//                     loss = 1 - 2 I / (X2 + T2 + 1e-5) (:509-519).  VOS: per slot, 0 behind num_matched (read on the device); SOT: ONE Dice
//                     over the batch, as the reference flattens it.
//   pl_bwd_kernel     thread = up to 4 neighbouring pixels of pred: d pred = g_p8 + 0.25 g_p16[parent] + 0.25 g_p32[parent]
//                     + g_loss (-2 t / U + 4 I x / U^2), U = X2 + T2 + eps.  Every pixel has at most one parent per level, so every element
//                     has one writer: no atomic, two runs give the same bits.  A NULL upstream gradient is left out; slots behind
//                     num_matched get exactly zero.
//
// The partial sums, I, X2, T2 and the Dice coefficients are double in both precisions.  The file is compiled without FMA contraction so
// that the corners round like the reference's separate tensor operations.
#include <algorithm>
#include <type_traits>

#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int PL_TB = 256;
constexpr int PL_MAXM = 1024;
constexpr double PL_EPS = 1e-5;

template <typename T, int V>
struct alignas(sizeof(T) * V) PlVec { T v[V]; };

template <typename T, int V>
__device__ __forceinline__ PlVec<T, V> pl_load(const T* p) { return *reinterpret_cast<const PlVec<T, V>*>(p); }
template <typename T, int V>
__device__ __forceinline__ void pl_store(T* p, const PlVec<T, V>& x) { *reinterpret_cast<PlVec<T, V>*>(p) = x; }

__global__ void __launch_bounds__(PL_TB)
pl_match_kernel(const float* __restrict__ targets, int M, int Kc, int sot, int* __restrict__ matched, int* __restrict__ num_matched) {
    __shared__ float s_id1[PL_MAXM];
    __shared__ int s_w[PL_TB / 64];
    __shared__ int s_base;
    const int b = blockIdx.x, t = threadIdx.x;
    int* mt = matched + (size_t)b * Kc * 2;
    if (sot) {
        if (t == 0) { mt[0] = 0; mt[1] = 0; num_matched[b] = 1; }
        for (int e = 2 + t; e < 2 * Kc; e += PL_TB) mt[e] = -1;
        return;
    }
    const float* tg = targets + (size_t)b * 2 * M * 6;
    for (int j = t; j < M; j += PL_TB) s_id1[j] = tg[(size_t)(M + j) * 6 + 5];
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < M; i0 += PL_TB) {
        const int i = i0 + t;
        int j = -1;
        if (i < M) {
            const float a = tg[(size_t)i * 6 + 5];
            if (a != 0.f)
                for (int c = 0; c < M; ++c) {
                    const float d = s_id1[c];
                    if (d != 0.f && d == a) { j = c; break; }
                }
        }
        const unsigned long long bal = __ballot(j >= 0);
        const int lane = t & 63, wave = t >> 6;
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int slot = s_base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) slot += s_w[w];
        if (j >= 0 && slot < Kc) { mt[slot * 2] = i; mt[slot * 2 + 1] = j; }
        __syncthreads();
        if (t == 0) {
            int n = s_base;
            for (int w = 0; w < PL_TB / 64; ++w) n += s_w[w];
            s_base = n;
        }
        __syncthreads();
    }
    const int n = min(s_base, Kc);
    for (int e = 2 * n + t; e < 2 * Kc; e += PL_TB) mt[e] = -1;
    if (t == 0) num_matched[b] = n;
}

// one rounded corner pair of an axis -> [lo, hi) in full-resolution pixels, as labels[.., v1:v2] selects them after v1 = max(0, v1)
__device__ __forceinline__ void pl_span(float c, float ext, int size, int& lo, int& hi) {
    const float lim = 1073741824.f;
    const float a = fminf(fmaxf(rintf(c - 0.5f * ext), -lim), lim), e = fminf(fmaxf(rintf(c + 0.5f * ext), -lim), lim);
    const int v1 = (int)a, v2 = (int)e;
    lo = min(max(v1, 0), size);
    hi = v2 < 0 ? max(v2 + size, 0) : min(v2, size);
}
// how many of the two central pixels 8 p + 3, 8 p + 4 of block p lie in [lo, hi)
__device__ __forceinline__ int pl_hits(int p, int lo, int hi) {
    const int a = 8 * p + 3;
    return (a >= lo && a < hi) + (a + 1 >= lo && a + 1 < hi);
}

__device__ __forceinline__ float pl_mask_at(const float* m, size_t i) { return m[i]; }
__device__ __forceinline__ float pl_mask_at(const unsigned char* m, size_t i) { return (float)m[i]; }

// MT = float / unsigned char masks, or void: boxes
template <typename T, typename MT, int V>
__global__ void __launch_bounds__(PL_TB)
pl_label_kernel(const float* __restrict__ targets, const MT* __restrict__ masks, const int* __restrict__ matched, const int* __restrict__ num_matched,
                int M, int Kc, int H, int W, int H8, int W8, int r, T* __restrict__ gt0, T* __restrict__ gt1) {
    const int slot = blockIdx.y >> 1, f = blockIdx.y & 1, b = slot / Kc, s = slot % Kc;
    const int Q = H8 * W8;
    const int e0 = (blockIdx.x * PL_TB + threadIdx.x) * V;
    if (e0 >= Q) return;
    T* dst = (f ? gt1 : gt0) + (size_t)slot * Q;
    T out[V];
#pragma unroll
    for (int k = 0; k < V; ++k) out[k] = 0;
    if (s < num_matched[b]) {
        const int idx = matched[(size_t)slot * 2 + f];
        if constexpr (std::is_void<MT>::value) {
            const float* row = targets + (((size_t)b * 2 + f) * M + idx) * 6;
            int x1, x2, y1, y2;
            pl_span(row[1], row[3], W, x1, x2);
            pl_span(row[2], row[4], H, y1, y2);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int e = e0 + k;
                if (e < Q) out[k] = (T)0.25 * (T)(pl_hits(e / W8, y1, y2) * pl_hits(e % W8, x1, x2));
            }
        } else {
            const int Wm = r * W8;
            const MT* m = masks + (((size_t)b * 2 + f) * M + idx) * (size_t)(r * H8) * Wm;
            const int o = r == 4 ? 1 : 0;                       // first of the two source rows / columns inside the r x r block
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int e = e0 + k;
                if (e >= Q) continue;
                const size_t p = (size_t)(r * (e / W8) + o) * Wm + r * (e % W8) + o;
                if (r == 1) {
                    out[k] = (T)pl_mask_at(m, p);
                } else {                                        // upsample_bilinear2d's order with all four weights 0.5
                    const T a = (T)pl_mask_at(m, p), c = (T)pl_mask_at(m, p + 1), d = (T)pl_mask_at(m, p + Wm), g = (T)pl_mask_at(m, p + Wm + 1);
                    out[k] = (T)0.5 * ((T)0.5 * a + (T)0.5 * c) + (T)0.5 * ((T)0.5 * d + (T)0.5 * g);
                }
            }
        }
    }
    if constexpr (V > 1) {
        if (e0 + V <= Q) {
            PlVec<T, V> x;
#pragma unroll
            for (int k = 0; k < V; ++k) x.v[k] = out[k];
            pl_store<T, V>(dst + e0, x);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (e0 + k < Q) dst[e0 + k] = out[k];
}

// VEC: W8 % 4 == 0 and every pointer aligned for 4 (pred, gt) / 2 (p16) elements
template <typename T, bool VEC>
__global__ void __launch_bounds__(PL_TB)
pl_fwd_kernel(const T* __restrict__ pred, const T* __restrict__ gt, int H8, int W8, T* __restrict__ p16, T* __restrict__ p32,
              double* __restrict__ partial, int pitch) {
    __shared__ double sm[PL_TB / 64][3];
    const int slot = blockIdx.y, t = threadIdx.x;
    const int H16 = H8 / 2, W16 = W8 / 2, H32 = H8 / 4, W32 = W8 / 4;
    const int nbx = (W8 + 3) / 4, nby = (H8 + 3) / 4;
    const int blk = blockIdx.x * PL_TB + t;
    double si = 0, sx = 0, st = 0;
    if (blk < nbx * nby) {
        const int by = blk / nbx, bx = blk % nbx;
        const int y0 = 4 * by, x0 = 4 * bx;
        const T* ps = pred + (size_t)slot * H8 * W8;
        const T* gs = gt + (size_t)slot * H8 * W8;
        T x[4][4];
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            T g[4];
            const int y = y0 + dy;
            if (VEC) {
                if (y < H8) {
                    const PlVec<T, 4> a = pl_load<T, 4>(ps + (size_t)y * W8 + x0), c = pl_load<T, 4>(gs + (size_t)y * W8 + x0);
#pragma unroll
                    for (int dx = 0; dx < 4; ++dx) { x[dy][dx] = a.v[dx]; g[dx] = c.v[dx]; }
                } else {
#pragma unroll
                    for (int dx = 0; dx < 4; ++dx) { x[dy][dx] = 0; g[dx] = 0; }
                }
            } else {
#pragma unroll
                for (int dx = 0; dx < 4; ++dx) {
                    const bool ok = y < H8 && x0 + dx < W8;
                    x[dy][dx] = ok ? ps[(size_t)y * W8 + x0 + dx] : (T)0;
                    g[dx] = ok ? gs[(size_t)y * W8 + x0 + dx] : (T)0;
                }
            }
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {                    // elements outside the map are zeros: they add nothing
                const double a = (double)x[dy][dx], c = (double)g[dx];
                si = fma(a, c, si);
                sx = fma(a, a, sx);
                st = fma(c, c, st);
            }
        }
#pragma unroll
        for (int hy = 0; hy < 2; ++hy) {
            const int y16 = 2 * by + hy;
            if (y16 >= H16) continue;
            T* d = p16 + ((size_t)slot * H16 + y16) * W16 + 2 * bx;
            const T v0 = (T)0.25 * ((x[2 * hy][0] + x[2 * hy][1]) + (x[2 * hy + 1][0] + x[2 * hy + 1][1]));
            const T v1 = (T)0.25 * ((x[2 * hy][2] + x[2 * hy][3]) + (x[2 * hy + 1][2] + x[2 * hy + 1][3]));
            if (VEC) {
                PlVec<T, 2> o;
                o.v[0] = v0;
                o.v[1] = v1;
                pl_store<T, 2>(d, o);
            } else {
                if (2 * bx < W16) d[0] = v0;
                if (2 * bx + 1 < W16) d[1] = v1;
            }
        }
        if (by < H32 && bx < W32) p32[((size_t)slot * H32 + by) * W32 + bx] = (T)0.25 * ((x[1][1] + x[1][2]) + (x[2][1] + x[2][2]));
    }
    si = wave_sum(si);
    sx = wave_sum(sx);
    st = wave_sum(st);
    if ((t & 63) == 0) { sm[t >> 6][0] = si; sm[t >> 6][1] = sx; sm[t >> 6][2] = st; }
    __syncthreads();
    if (t < 3) {
        double a = 0;
        for (int w = 0; w < PL_TB / 64; ++w) a += sm[w][t];
        partial[((size_t)slot * pitch + blockIdx.x) * 3 + t] = a;
    }
}

// block (one wave) = one Dice: group g covers `span` slots starting at g * span, nblk partial triples each
template <typename T>
__global__ void __launch_bounds__(64)
pl_final_kernel(const double* __restrict__ partial, int pitch, int nblk, int span, const int* __restrict__ num_matched, int Kc, T* __restrict__ loss,
                double* __restrict__ sums) {
    const int g = blockIdx.x, lane = threadIdx.x;
    double a[3] = {0, 0, 0};
    for (int e = lane; e < span * nblk; e += 64) {
        const double* p = partial + ((size_t)(g * span + e / nblk) * pitch + e % nblk) * 3;
        a[0] += p[0];
        a[1] += p[1];
        a[2] += p[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = wave_sum(a[k]);
    if (lane == 0) {
        const bool live = !num_matched || g % Kc < num_matched[g / Kc];
        sums[(size_t)g * 3 + 0] = a[0];
        sums[(size_t)g * 3 + 1] = a[1];
        sums[(size_t)g * 3 + 2] = a[2];
        const double u = a[1] + a[2] + PL_EPS;
        loss[g] = live ? (T)(1.0 - 2.0 * a[0] / u) : (T)0;
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(PL_TB)
pl_bwd_kernel(const T* __restrict__ pred, const T* __restrict__ gt, const int* __restrict__ num_matched, const double* __restrict__ sums,
              const T* __restrict__ g8, const T* __restrict__ g16, const T* __restrict__ g32, const T* __restrict__ gl, int Kc, int H8, int W8,
              T* __restrict__ gpred) {
    const int slot = blockIdx.y;
    const int nx = (W8 + V - 1) / V;
    const int e = blockIdx.x * PL_TB + threadIdx.x;
    if (e >= nx * H8) return;
    const int y = e / nx, x0 = (e % nx) * V;
    const int H16 = H8 / 2, W16 = W8 / 2, H32 = H8 / 4, W32 = W8 / 4;
    const size_t o = ((size_t)slot * H8 + y) * W8 + x0;
    T out[V];
#pragma unroll
    for (int k = 0; k < V; ++k) out[k] = 0;
    const bool live = !num_matched || slot % Kc < num_matched[slot / Kc];
    if (live) {
        if (g8) {
            if constexpr (V > 1) {
                const PlVec<T, V> a = pl_load<T, V>(g8 + o);
#pragma unroll
                for (int k = 0; k < V; ++k) out[k] = a.v[k];
            } else {
                out[0] = g8[o];
            }
        }
        if (g16 && y / 2 < H16) {
            const T* p = g16 + ((size_t)slot * H16 + y / 2) * W16;
#pragma unroll
            for (int k = 0; k < V; ++k)
                if ((x0 + k) / 2 < W16) out[k] += (T)0.25 * p[(x0 + k) / 2];
        }
        if (g32 && (y & 3) >= 1 && (y & 3) <= 2 && y / 4 < H32) {
            const T* p = g32 + ((size_t)slot * H32 + y / 4) * W32;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int x = x0 + k;
                if ((x & 3) >= 1 && (x & 3) <= 2 && x / 4 < W32) out[k] += (T)0.25 * p[x / 4];
            }
        }
        if (gl) {
            const int g = num_matched ? slot : 0;
            const double I = sums[(size_t)g * 3], U = sums[(size_t)g * 3 + 1] + sums[(size_t)g * 3 + 2] + PL_EPS;
            const double gg = (double)gl[g];
            const T ct = (T)(-2.0 * gg / U), cx = (T)(4.0 * gg * I / (U * U));
            if constexpr (V > 1) {
                const PlVec<T, V> a = pl_load<T, V>(pred + o), c = pl_load<T, V>(gt + o);
#pragma unroll
                for (int k = 0; k < V; ++k) out[k] += ct * c.v[k] + cx * a.v[k];
            } else {
                out[0] += ct * gt[o] + cx * pred[o];
            }
        }
    }
    if constexpr (V > 1) {
        PlVec<T, V> r;
#pragma unroll
        for (int k = 0; k < V; ++k) r.v[k] = out[k];
        pl_store<T, V>(gpred + o, r);
    } else {
        gpred[o] = out[0];
    }
}

bool pl_shape_ok(int B, int Kc, long long Q) {
    return B >= 1 && Kc >= 1 && Kc <= PL_MAXM && (long long)B * Kc <= 32767 && Q >= 16 && (long long)B * Kc * Q < (1ll << 31);
}
int pl_pitch(long long Q) { return (int)((Q + 1023) / 1024); }      // >= the thread blocks of pl_fwd_kernel per slot: ceil(H8/4) ceil(W8/4) <= Q / 4 for H8, W8 >= 4

bool pl_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

size_t prop_workspace_bytes(int B, int Kc, int Q) {
    if (!pl_shape_ok(B, Kc, Q)) return 0;
    return ((size_t)B * Kc * pl_pitch(Q) * 3 * sizeof(double) + 255) & ~(size_t)255;
}

template <typename T>
int launch_prop_labels(const PlLabelArgs& a, T* gt0, T* gt1, hipStream_t s) {
    const int B = a.B, M = a.M, Kc = a.Kc, H8 = a.H8, W8 = a.W8, r = a.r;
    const long long Q = (long long)H8 * W8;
    UNI_REQUIRE(H8 >= 4 && W8 >= 4 && pl_shape_ok(B, Kc, Q), "prop_labels: shape B=%d Kc=%d H8=%d W8=%d outside H8, W8 >= 4, 1 <= Kc <= 1024, B Kc <= 32767, B Kc H8 W8 < 2^31",
                B, Kc, H8, W8);
    UNI_REQUIRE(M >= 1 && M <= PL_MAXM && Kc <= M, "prop_labels: M=%d outside 1 .. 1024 or Kc=%d > M", M, Kc);
    UNI_REQUIRE(!a.sot || (Kc == 1 && !a.masks), "prop_labels: the SOT form has one slot per sample and no masks");
    UNI_REQUIRE(!a.masks || r == 1 || r == 2 || r == 4, "prop_labels: mask rate r=%d is not 1, 2 or 4", r);
    UNI_REQUIRE(H8 <= (1 << 27) && W8 <= (1 << 27), "prop_labels: map too large");
    const int V = (Q % 4 == 0 && pl_aligned(gt0, 4 * sizeof(T)) && pl_aligned(gt1, 4 * sizeof(T))) ? 4 : 1;
    const int kind = !a.masks ? 0 : a.mask_u8 ? 2 : 1;
    uni_variant_note("prop_labels %s kind=%s vec=%d sot=%d", sizeof(T) == 8 ? "f64" : "f32", kind == 0 ? "box" : kind == 1 ? "mask_f32" : "mask_u8", V, a.sot);
    pl_match_kernel<<<B, PL_TB, 0, s>>>(a.targets, M, Kc, a.sot, a.matched, a.num_matched);
    const dim3 grid(cdiv(cdiv((int)Q, V), PL_TB), 2 * B * Kc);
    const int H = 8 * H8, W = 8 * W8;
#define PL_LABEL(MT, VV) \
    pl_label_kernel<T, MT, VV><<<grid, PL_TB, 0, s>>>(a.targets, (const MT*)a.masks, a.matched, a.num_matched, M, Kc, H, W, H8, W8, r, gt0, gt1)
    if (kind == 0) { if (V == 4) PL_LABEL(void, 4); else PL_LABEL(void, 1); }
    else if (kind == 1) { if (V == 4) PL_LABEL(float, 4); else PL_LABEL(float, 1); }
    else { if (V == 4) PL_LABEL(unsigned char, 4); else PL_LABEL(unsigned char, 1); }
#undef PL_LABEL
    return 0;
}

template <typename T>
int launch_prop_dice_pyramid_fwd(const PlDiceArgs<T>& a, T* p16, T* p32, T* loss, double* sums, void* ws, size_t ws_bytes, hipStream_t s) {
    const int B = a.B, Kc = a.Kc, H8 = a.H8, W8 = a.W8;
    const long long Q = (long long)H8 * W8;
    UNI_REQUIRE(H8 >= 4 && W8 >= 4 && pl_shape_ok(B, Kc, Q), "prop_dice_pyramid_fwd: shape B=%d Kc=%d H8=%d W8=%d outside H8, W8 >= 4, 1 <= Kc <= 1024, B Kc <= 32767, B Kc H8 W8 < 2^31",
                B, Kc, H8, W8);
    UNI_REQUIRE(ws_bytes >= prop_workspace_bytes(B, Kc, (int)Q), "prop_dice_pyramid_fwd: workspace %zu < %zu", ws_bytes, prop_workspace_bytes(B, Kc, (int)Q));
    UNI_REQUIRE(pl_aligned(ws, 8) && pl_aligned(sums, 8), "prop_dice_pyramid_fwd: workspace and sums must be 8-byte aligned");
    const int slots = B * Kc, pitch = pl_pitch(Q);
    const int nblk = cdiv(cdiv(H8, 4) * cdiv(W8, 4), PL_TB);
    UNI_REQUIRE(nblk <= pitch, "prop_dice_pyramid_fwd: internal: %d partial blocks > pitch %d", nblk, pitch);
    const bool vec = W8 % 4 == 0 && pl_aligned(a.pred, 4 * sizeof(T)) && pl_aligned(a.gt1, 4 * sizeof(T)) && pl_aligned(p16, 2 * sizeof(T));
    uni_variant_note("prop_dice_pyramid_fwd %s vec=%d sot=%d", sizeof(T) == 8 ? "f64" : "f32", vec, a.num_matched == nullptr);
    double* partial = reinterpret_cast<double*>(ws);
    if (vec) pl_fwd_kernel<T, true><<<dim3(nblk, slots), PL_TB, 0, s>>>(a.pred, a.gt1, H8, W8, p16, p32, partial, pitch);
    else pl_fwd_kernel<T, false><<<dim3(nblk, slots), PL_TB, 0, s>>>(a.pred, a.gt1, H8, W8, p16, p32, partial, pitch);
    if (a.num_matched) pl_final_kernel<T><<<slots, 64, 0, s>>>(partial, pitch, nblk, 1, a.num_matched, Kc, loss, sums);
    else pl_final_kernel<T><<<1, 64, 0, s>>>(partial, pitch, nblk, slots, nullptr, Kc, loss, sums);
    return 0;
}

template <typename T>
int launch_prop_dice_pyramid_bwd(const PlDiceArgs<T>& a, const double* sums, const T* g8, const T* g16, const T* g32, const T* gl, T* gpred,
                                 hipStream_t s) {
    const int B = a.B, Kc = a.Kc, H8 = a.H8, W8 = a.W8;
    const long long Q = (long long)H8 * W8;
    UNI_REQUIRE(H8 >= 4 && W8 >= 4 && pl_shape_ok(B, Kc, Q), "prop_dice_pyramid_bwd: shape B=%d Kc=%d H8=%d W8=%d outside H8, W8 >= 4, 1 <= Kc <= 1024, B Kc <= 32767, B Kc H8 W8 < 2^31",
                B, Kc, H8, W8);
    UNI_REQUIRE(pl_aligned(sums, 8), "prop_dice_pyramid_bwd: sums must be 8-byte aligned");
    const size_t al = 4 * sizeof(T);
    const bool vec = W8 % 4 == 0 && pl_aligned(a.pred, al) && pl_aligned(a.gt1, al) && pl_aligned(gpred, al) && (!g8 || pl_aligned(g8, al));
    uni_variant_note("prop_dice_pyramid_bwd %s vec=%d sot=%d", sizeof(T) == 8 ? "f64" : "f32", vec, a.num_matched == nullptr);
    const int V = vec ? 4 : 1;
    const dim3 grid(cdiv(cdiv(W8, V) * H8, PL_TB), B * Kc);
    if (vec) pl_bwd_kernel<T, 4><<<grid, PL_TB, 0, s>>>(a.pred, a.gt1, a.num_matched, sums, g8, g16, g32, gl, Kc, H8, W8, gpred);
    else pl_bwd_kernel<T, 1><<<grid, PL_TB, 0, s>>>(a.pred, a.gt1, a.num_matched, sums, g8, g16, g32, gl, Kc, H8, W8, gpred);
    return 0;
}

template int launch_prop_labels<float>(const PlLabelArgs&, float*, float*, hipStream_t);
template int launch_prop_labels<double>(const PlLabelArgs&, double*, double*, hipStream_t);
template int launch_prop_dice_pyramid_fwd<float>(const PlDiceArgs<float>&, float*, float*, float*, double*, void*, size_t, hipStream_t);
template int launch_prop_dice_pyramid_fwd<double>(const PlDiceArgs<double>&, double*, double*, double*, double*, void*, size_t, hipStream_t);
template int launch_prop_dice_pyramid_bwd<float>(const PlDiceArgs<float>&, const double*, const float*, const float*, const float*, const float*,
                                                 float*, hipStream_t);
template int launch_prop_dice_pyramid_bwd<double>(const PlDiceArgs<double>&, const double*, const double*, const double*, const double*,
                                                  const double*, double*, hipStream_t);
