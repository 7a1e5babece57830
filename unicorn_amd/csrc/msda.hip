// K3: multi-scale deformable attention (replaces the reference's only hand-written CUDA op,
// unicorn/models/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299, bilinear :33-84; backward :87-234, 301-920).
// Three kernels: `msda_kernel`, the reference-compatible general op behind uni_msda_fwd (any N / heads / levels / points:
// one lane per (query, head, channel), a corner fetch = one contiguous D*4-byte segment), `msda_bwd_kernel`, its gradient behind
// uni_msda_bwd (one wave per (n, query, head), float atomics into grad_value), both for float and double, and `msda_wave_kernel`, the
// engine's fused version for Unicorn's fixed geometry (one wave per (token, head), cross-group shuffle reductions).
// value is 8 MB per frame pair at 800x1280 -> L2/MALL resident; the op is bound by L2 gather bandwidth, no LDS needed.
#include "kernels.h"
#include <cstdlib>

struct MsdaShapes { int H[8], W[8], start[8]; };

template <typename T>
__device__ __forceinline__ T msda_bilinear(const T* v, int H, int W, int stride, T h, T w) {
    // ms_deform_im2col_cuda.cuh:33-84: corners outside the map contribute 0
    const int h0 = (int)floor(h), w0 = (int)floor(w);
    const T lh = h - h0, lw = w - w0, hh = T(1) - lh, hw = T(1) - lw;
    const int h1 = h0 + 1, w1 = w0 + 1;
    T v1 = 0, v2 = 0, v3 = 0, v4 = 0;
    if (h0 >= 0 && w0 >= 0) v1 = v[(size_t)(h0 * W + w0) * stride];
    if (h0 >= 0 && w1 <= W - 1) v2 = v[(size_t)(h0 * W + w1) * stride];
    if (h1 <= H - 1 && w0 >= 0) v3 = v[(size_t)(h1 * W + w0) * stride];
    if (h1 <= H - 1 && w1 <= W - 1) v4 = v[(size_t)(h1 * W + w1) * stride];
    return hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4;
}

template <typename T>
__global__ __launch_bounds__(256) void msda_kernel(const T* __restrict__ value, const T* __restrict__ loc,
                                                   const T* __restrict__ attn, T* __restrict__ out,
                                                   MsdaShapes shp, int N, int S, int M, int D, int Lq, int L, int P) {
    const long total = (long)N * Lq * M * D;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int d = idx % D;
    const int m = (idx / D) % M;
    const int q = (idx / ((long)D * M)) % Lq;
    const int n = idx / ((long)D * M * Lq);
    const T* lp = loc + (((size_t)n * Lq + q) * M + m) * L * P * 2;
    const T* ap = attn + (((size_t)n * Lq + q) * M + m) * L * P;
    const int stride = M * D;
    T acc = 0;
    for (int l = 0; l < L; ++l) {
        const int H = shp.H[l], W = shp.W[l];
        const T* vb = value + ((size_t)n * S + shp.start[l]) * stride + m * D + d;
        for (int pt = 0; pt < P; ++pt) {
            const T x = lp[(l * P + pt) * 2] * W - T(0.5);
            const T y = lp[(l * P + pt) * 2 + 1] * H - T(0.5);
            const T wgt = ap[l * P + pt];
            if (y > -1 && x > -1 && y < H && x < W) acc += wgt * msda_bilinear<T>(vb, H, W, stride, y, x);
        }
    }
    out[idx] = acc;
}

// shapes / level starts of the host arrays -> kernel argument; `scatter` additionally holds every level inside [0, S) (the backward WRITES
// through these offsets, so a level_start_index that points outside value is refused instead of trusted)
static int msda_shapes(const int64_t* shapes, const int64_t* lsi, int S, int L, bool scatter, MsdaShapes* shp) {
    UNI_REQUIRE(L >= 1 && L <= 8, "msda: n_levels=%d unsupported (1..8)", L);
    long tot = 0;
    for (int l = 0; l < L; ++l) {
        shp->H[l] = (int)shapes[2 * l];
        shp->W[l] = (int)shapes[2 * l + 1];
        shp->start[l] = (int)lsi[l];
        tot += shapes[2 * l] * shapes[2 * l + 1];
        if (scatter)
            UNI_REQUIRE(shapes[2 * l] > 0 && shapes[2 * l + 1] > 0 && lsi[l] >= 0 && lsi[l] + shapes[2 * l] * shapes[2 * l + 1] <= S,
                        "msda_bwd: level %d (%ld x %ld at %ld) lies outside value (S=%d)", l, (long)shapes[2 * l],
                        (long)shapes[2 * l + 1], (long)lsi[l], S);
    }
    UNI_REQUIRE(tot == S, "msda: sum(H*W)=%ld != S=%d", tot, S);   // ms_deform_attn.py:94
    return 0;
}

template <typename T>
int launch_msda(const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc, const T* attn,
                T* out, int N, int S, int M, int D, int Lq, int L, int P, hipStream_t s) {
    MsdaShapes shp;
    if (int rc = msda_shapes(shapes, lsi, S, L, false, &shp)) return rc;
    const long total = (long)N * Lq * M * D;
    if (total == 0) return 0;
    hipLaunchKernelGGL(msda_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, value, loc, attn, out, shp,
                       N, S, M, D, Lq, L, P);
    return 0;
}
template int launch_msda<float>(const float*, const int64_t*, const int64_t*, const float*, const float*, float*, int, int, int, int,
                                int, int, int, hipStream_t);
template int launch_msda<double>(const double*, const int64_t*, const int64_t*, const double*, const double*, double*, int, int, int,
                                 int, int, int, int, hipStream_t);

// Backward of the general op (replaces ms_deform_im2col_cuda.cuh:87-234 col2im bilinear + the six col2im kernel variants
// :301-920, dispatched by channel count :956-1326).  One CDNA4 kernel instead: ONE WAVE owns one (n, q, m) and walks its L*P samples,
// lanes walk channels.  grad_sampling_loc and grad_attn_weight are sums over D of one (n, q, m, l, p): exactly one wave holds all their
// addends, so they are register partial sums + an xor-shuffle butterfly and ONE plain store each (no LDS, no atomics; samples skipped by
// the -1 < x < W, -1 < y < H rule store 0).  grad_value is the only sum across waves: atomicAdd into a buffer the launcher zeroed
// (global_atomic_add_f32 / _f64 under -munsafe-fp-atomics, no compare-and-swap loop), so its last bits depend on arrival order.
// Atomic shape: a wave instruction adds one dword per lane; it runs at the full rate as 256 contiguous bytes or two 128-byte row segments.
//   D32 = false: lanes stride over the channels in chunks of 64 (contiguous D*sizeof(T) bytes of a head row per corner).
//   D32 = true (Unicorn: 8 heads x 32 channels, a 128-byte fp32 head row): the two half-waves take two DIFFERENT samples, lane & 31 is
//   the channel, so every atomic instruction is two 128-byte segments and the butterfly stops at 16.
template <typename T>
struct MsdaTap {            // one sample's bilinear geometry: corner row offsets (elements, < 0 = outside the map) and weights
    long o[4];
    T w[4], cx[4], cy[4];   // value weight, d/dx and d/dy coefficient of each corner
};
template <typename T>
__device__ __forceinline__ void msda_tap(MsdaTap<T>& t, int H, int W, long stride, T y, T x) {
    const int h0 = (int)floor(y), w0 = (int)floor(x);
    const T lh = y - h0, lw = x - w0, hh = T(1) - lh, hw = T(1) - lw;
    const bool yok0 = h0 >= 0, yok1 = h0 + 1 <= H - 1, xok0 = w0 >= 0, xok1 = w0 + 1 <= W - 1;
    t.o[0] = yok0 && xok0 ? ((long)h0 * W + w0) * stride : -1;
    t.o[1] = yok0 && xok1 ? ((long)h0 * W + w0 + 1) * stride : -1;
    t.o[2] = yok1 && xok0 ? ((long)(h0 + 1) * W + w0) * stride : -1;
    t.o[3] = yok1 && xok1 ? ((long)(h0 + 1) * W + w0 + 1) * stride : -1;
    t.w[0] = hh * hw; t.w[1] = hh * lw; t.w[2] = lh * hw; t.w[3] = lh * lw;
    t.cx[0] = -hh; t.cx[1] = hh; t.cx[2] = -lh; t.cx[3] = lh;
    t.cy[0] = -hw; t.cy[1] = -lw; t.cy[2] = hw; t.cy[3] = lw;
}
// one channel of one sample: scatter w * attn * grad_out into the corner rows, accumulate the three D-sums' addends
template <typename T>
__device__ __forceinline__ void msda_bwd_channel(const MsdaTap<T>& t, const T* __restrict__ vb, T* __restrict__ gvb, T g, T aw,
                                                 T& ga, T& gx, T& gy) {
    const T tg = g * aw;
    T val = 0, dx = 0, dy = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (t.o[c] >= 0) {
            const T v = vb[t.o[c]];
            atomicAdd(gvb + t.o[c], t.w[c] * tg);
            val += t.w[c] * v; dx += t.cx[c] * v; dy += t.cy[c] * v;
        }
    ga += g * val; gx += tg * dx; gy += tg * dy;
}
template <typename T, int FIRST>
__device__ __forceinline__ T msda_lane_sum(T v) {      // butterfly over xor FIRST, FIRST/2, .., 1
#pragma unroll
    for (int o = FIRST; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T, bool D32>
__global__ __launch_bounds__(256) void msda_bwd_kernel(const T* __restrict__ value, const T* __restrict__ loc,
                                                       const T* __restrict__ attn, const T* __restrict__ gout,
                                                       T* __restrict__ gvalue, T* __restrict__ gloc, T* __restrict__ gattn,
                                                       MsdaShapes shp, long tasks, int S, int M, int D, int Lq, int L, int P) {
    const int lane = threadIdx.x & 63;
    const long task = (long)blockIdx.x * 4 + (threadIdx.x >> 6);            // (n, q, m)
    if (task >= tasks) return;                                               // wave-uniform
    const int m = (int)(task % M);
    const long n = task / ((long)M * Lq);
    const int LP = L * P;
    const T* lp = loc + task * LP * 2;
    const T* ap = attn + task * LP;
    const T* go = gout + task * D;                                           // grad_output [N][Lq][M*D]
    T* gl = gloc + task * LP * 2;
    T* gw = gattn + task * LP;
    const long stride = (long)M * D;
    if (D32) {
        const int half = lane >> 5, d = lane & 31;
        const T g = go[d];
        for (int s0 = 0; s0 < LP; s0 += 2) {
            const int l0 = s0 / P, l1 = min(s0 + 1, LP - 1) / P;            // wave-uniform level of each half's sample
            const int H = half ? shp.H[l1] : shp.H[l0], W = half ? shp.W[l1] : shp.W[l0];
            const int start = half ? shp.start[l1] : shp.start[l0];
            const int sm = s0 + half;
            const bool live = sm < LP;                                       // odd L*P: the upper half idles in the last step
            const int sc = live ? sm : s0;
            const T x = lp[sc * 2] * W - T(0.5), y = lp[sc * 2 + 1] * H - T(0.5);
            const T aw = ap[sc];
            T ga = 0, gx = 0, gy = 0;
            if (live && y > -1 && x > -1 && y < H && x < W) {
                MsdaTap<T> t;
                msda_tap<T>(t, H, W, stride, y, x);
                const long base = (n * S + start) * stride + (long)m * D + d;
                msda_bwd_channel<T>(t, value + base, gvalue + base, g, aw, ga, gx, gy);
            }
            ga = msda_lane_sum<T, 16>(ga); gx = msda_lane_sum<T, 16>(gx); gy = msda_lane_sum<T, 16>(gy);
            if (d == 0 && live) { gl[sm * 2] = gx * W; gl[sm * 2 + 1] = gy * H; gw[sm] = ga; }
        }
    } else {
        for (int l = 0; l < L; ++l) {
            const int H = shp.H[l], W = shp.W[l];
            const long base = (n * S + shp.start[l]) * stride + (long)m * D;
            for (int pt = 0; pt < P; ++pt) {
                const int sm = l * P + pt;
                const T x = lp[sm * 2] * W - T(0.5), y = lp[sm * 2 + 1] * H - T(0.5);
                const T aw = ap[sm];
                T ga = 0, gx = 0, gy = 0;
                if (y > -1 && x > -1 && y < H && x < W) {                    // wave-uniform
                    MsdaTap<T> t;
                    msda_tap<T>(t, H, W, stride, y, x);
                    for (int d = lane; d < D; d += 64)
                        msda_bwd_channel<T>(t, value + base + d, gvalue + base + d, go[d], aw, ga, gx, gy);
                }
                ga = msda_lane_sum<T, 32>(ga); gx = msda_lane_sum<T, 32>(gx); gy = msda_lane_sum<T, 32>(gy);
                if (lane == 0) { gl[sm * 2] = gx * W; gl[sm * 2 + 1] = gy * H; gw[sm] = ga; }
            }
        }
    }
}

template <typename T>
int launch_msda_bwd(const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc, const T* attn, const T* gout,
                    T* gvalue, T* gloc, T* gattn, int N, int S, int M, int D, int Lq, int L, int P, hipStream_t s) {
    MsdaShapes shp;
    if (int rc = msda_shapes(shapes, lsi, S, L, true, &shp)) return rc;
    UNI_REQUIRE(N >= 0 && M >= 0 && D >= 0 && Lq >= 0 && P >= 0, "msda_bwd: negative size");
    const size_t nv = (size_t)N * S * M * D;
    if (nv) UNI_CHECK_HIP(hipMemsetAsync(gvalue, 0, nv * sizeof(T), s));
    const long tasks = (long)N * Lq * M;
    if (tasks == 0 || D == 0 || P == 0) return 0;
    UNI_REQUIRE((tasks + 3) / 4 <= 0x7fffffffL, "msda_bwd: N*Lq*M=%ld too large", tasks);
    const dim3 grid((unsigned)((tasks + 3) / 4));
    if (D == 32)
        hipLaunchKernelGGL((msda_bwd_kernel<T, true>), grid, dim3(256), 0, s, value, loc, attn, gout, gvalue, gloc, gattn, shp, tasks,
                           S, M, D, Lq, L, P);
    else
        hipLaunchKernelGGL((msda_bwd_kernel<T, false>), grid, dim3(256), 0, s, value, loc, attn, gout, gvalue, gloc, gattn, shp, tasks,
                           S, M, D, Lq, L, P);
    return 0;
}
template int launch_msda_bwd<float>(const float*, const int64_t*, const int64_t*, const float*, const float*, const float*, float*,
                                    float*, float*, int, int, int, int, int, int, int, hipStream_t);
template int launch_msda_bwd<double>(const double*, const int64_t*, const int64_t*, const double*, const double*, const double*,
                                     double*, double*, double*, int, int, int, int, int, int, int, hipStream_t);

// Engine variant for Unicorn's fixed geometry (8 heads x 32 ch, 2 levels = ref / cur frame of identical (h,w), 4 points): fuses
// ms_deform_attn.py:98-105 (softmax over the 8 logits, loc = ref + off/(W,H)) and deformable_transformer.py:141-153 (reference
// points) into the sampler; emits the operand format of output_proj.
// CDNA4 shape of the same op: ONE WAVE per (token, head).  The 64 lanes are 8 groups x 8 lanes: group g owns sampling point g
// (level g >> 2, point g & 3), lane j of a group owns channels 4j..4j+3 of the 32-channel head row, so a corner fetch of a
// group is one 128-byte row as 8 x float4.  The softmax over the 8 logits and the final sum over the 8 points are butterfly
// reductions ACROSS the groups (xor 8 / 16 / 32 shuffles); location / bilinear math runs once per point (8-fold instead of
// 32-fold redundancy), 4 float4 loads per lane instead of 32 scalar ones.  Semantics = ms_deform_im2col_cuda.cuh:237-299
// (zero padding per corner, sample skipped unless -1 < x < W and -1 < y < H), ms_deform_attn.py:98-105.
__device__ __forceinline__ float xgroup_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 8, 64)); v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xgroup_sum(float v) {
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64);
}
__global__ __launch_bounds__(256) void msda_wave_kernel(MsdaFusedArgs p) {
    const int hw = p.h * p.w, Lq = 2 * hw;
    const int lane = threadIdx.x & 63;
    const long task = (long)blockIdx.x * 4 + (threadIdx.x >> 6);          // (token, head)
    if (task >= (long)Lq * 8 * p.B) return;                                 // wave-uniform
    const int m = (int)(task & 7);
    const int qg = (int)(task >> 3);                                        // token over [B][2 frames][hw]
    const int sb = qg / Lq, q = qg - sb * Lq;
    const int g = lane >> 3, j = lane & 7;
    const float* row = p.offaw + (size_t)qg * p.ldo;
    const float ox = row[m * 16 + g * 2], oy = row[m * 16 + g * 2 + 1];
    const float lg = row[128 + m * 8 + g];
    const float mx = xgroup_max(lg);
    const float e = __expf(lg - mx);
    const float wgt = e / xgroup_sum(e);
    const int pos = q % hw, i0 = pos / p.w, j0 = pos - i0 * p.w;
    const float lx = (j0 + 0.5f) / p.w + ox / p.w, ly = (i0 + 0.5f) / p.h + oy / p.h;
    const float x = lx * p.w - 0.5f, y = ly * p.h - 0.5f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (y > -1 && x > -1 && y < p.h && x < p.w) {
        const int y0 = (int)floorf(y), x0 = (int)floorf(x);
        const float ly1 = y - y0, lx1 = x - x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const float* vb = p.value + ((size_t)sb * Lq + (size_t)(g >> 2) * hw) * 256 + m * 32 + j * 4;
        const bool yok0 = y0 >= 0, yok1 = y0 + 1 <= p.h - 1, xok0 = x0 >= 0, xok1 = x0 + 1 <= p.w - 1;
        f32x4 v1 = {0.f, 0.f, 0.f, 0.f}, v2 = v1, v3 = v1, v4 = v1;
        if (yok0 && xok0) v1 = *reinterpret_cast<const f32x4*>(vb + (size_t)(y0 * p.w + x0) * 256);
        if (yok0 && xok1) v2 = *reinterpret_cast<const f32x4*>(vb + (size_t)(y0 * p.w + x0 + 1) * 256);
        if (yok1 && xok0) v3 = *reinterpret_cast<const f32x4*>(vb + (size_t)((y0 + 1) * p.w + x0) * 256);
        if (yok1 && xok1) v4 = *reinterpret_cast<const f32x4*>(vb + (size_t)((y0 + 1) * p.w + x0 + 1) * 256);
        // same association as the reference kernel: w1 v1 + w2 v2 + w3 v3 + w4 v4, then times the attention weight
        acc = (ly0 * lx0) * v1 + (ly0 * lx1) * v2 + (ly1 * lx0) * v3 + (ly1 * lx1) * v4;
        acc *= wgt;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = xgroup_sum(acc[c]);
    if (g == 0) act_store4(p.out, (size_t)qg * 256 + m * 32 + j * 4, acc[0], acc[1], acc[2], acc[3], p.b32);
}

int launch_msda_fused(const MsdaFusedArgs& a, hipStream_t s) {
    const long tasks = (long)2 * a.h * a.w * 8 * a.B;
    uni_variant_note("msda_fused fmt=%s batched=%d", uni_fmt_name(a.b32), a.B > 1);
    hipLaunchKernelGGL(msda_wave_kernel, dim3((unsigned)((tasks + 3) / 4)), dim3(256), 0, s, a);
    return 0;
}
