// The tail of a training iteration in one pass: GradScaler.step (unscale + non-finite check + skip), torch.optim.AdamW (single-tensor form,
// amsgrad = maximize = False), GradScaler.update and ModelEMA.update (unicorn/core/trainer.py:260-275, unicorn/utils/ema.py:50-63) over a
// LIST of fp32 tensors, without a host read-back.  Multi-tensor apply through two tables in device memory (include/unicorn_hip.h states the
// layouts): the tensor table holds the pointers and per-tensor scalars, the block map sends block -> (tensor, chunk of OS_CH elements).  At
// most three launches whatever the list: check (scaler only), update, finish.  Every element has one writer, no atomics, no LDS: two calls
// from the same state give the same bits.  The found_inf word is cleared by a memset node and then written only with the constant 1.0f.
//
// Forms: a `vec` chunk moves 16 bytes per lane and array with a scalar head / tail of at most 3 elements each (all pointers of the entry
// share their address modulo 16); a `scalar` chunk moves 4 bytes per lane (pointers misaligned relative to each other).  The block map lists
// the vec chunks first; a vec chunk whose pointers turn out not to share their alignment is processed by the scalar form.
#include <cfloat>

#include "kernels.h"

namespace {

constexpr int OS_TB = 256;                    // lanes per block
constexpr int OS_U = 4;                       // 16-byte groups per lane and chunk, loaded two at a time (10 independent loads in flight)
constexpr int OS_CH = OS_TB * 4 * OS_U;       // elements per chunk
constexpr int OS_HAS_GRAD = 1;

struct OsTensor {                             // uni_opt_tensor of the header, 64 bytes
    float* p; const float* g; float* m; float* v; float* e;
    long long n;
    double lr_factor;
    float wd;
    int flags;
};
static_assert(sizeof(OsTensor) == 64, "table entry layout");
struct OsBlock { int tensor; unsigned chunk; };
static_assert(sizeof(OsBlock) == 8, "block map layout");

struct OsArgs {
    const OsTensor* tab; const OsBlock* map;
    int n_tensors, vec_chunks;
    const float* step; const float* scale; float* found_inf;
    double lr, beta1, beta2, eps;
    float d, omd;                             // float(decay), float(1 - decay)
};

// the table's pointers are generic when they come out of memory; every array is global memory: say so (global_load / global_store, not flat)
typedef __attribute__((address_space(1))) float gfloat;
typedef float os_f4 __attribute__((ext_vector_type(4)));        // a native 16-byte vector (float4 is a struct: no address-space copy)
typedef __attribute__((address_space(1))) os_f4 gfloat4;
struct OsPtr {
    gfloat* p; const gfloat* g; gfloat* m; gfloat* v; gfloat* e;
    __device__ explicit OsPtr(const OsTensor& t) : p((gfloat*)t.p), g((const gfloat*)t.g), m((gfloat*)t.m), v((gfloat*)t.v), e((gfloat*)t.e) {}
};

struct OsCoef { float inv, wdmul, w1, b2, omb2, step_size, bc2s, eps, d, omd; };

// fl(fl(e d) + fl((1 - d) p)): the two lines of ModelEMA.update round three times; a fused multiply-add here changes the bits
__device__ __forceinline__ float os_ema(float e, float p, const OsCoef& c) {
#pragma clang fp contract(off)
    const float a = e * c.d;
    const float b = c.omd * p;
    return a + b;
}
// torch's _single_tensor_adamw on one element
__device__ __forceinline__ void os_adam(float& p, float g, float& m, float& v, const OsCoef& c) {
    const float gh = g * c.inv;
    p = p * c.wdmul;
    m = m + (gh - m) * c.w1;
    v = v * c.b2 + c.omb2 * gh * gh;
    const float denom = sqrtf(v) / c.bc2s + c.eps;
    p = p - c.step_size * (m / denom);
}
__device__ __forceinline__ bool os_bad(float g, float inv) { return !(fabsf(g * inv) <= FLT_MAX); }
__device__ __forceinline__ float os_inv_scale(const float* scale) { return scale ? (float)(1.0 / (double)*scale) : 1.f; }

// b^n for an integral n >= 0 by squaring, both bases at once (double; log2(n) roundings)
__device__ __forceinline__ void os_pow2(double b1, double b2, long long n, double& r1, double& r2) {
    r1 = 1.0; r2 = 1.0;
    while (n > 0) {
        if (n & 1) { r1 *= b1; r2 *= b2; }
        b1 *= b1; b2 *= b2;
        n >>= 1;
    }
}

__device__ __forceinline__ OsCoef os_coef(const OsArgs& a, const OsTensor& t, bool full) {
    OsCoef c;
    c.d = a.d; c.omd = a.omd;
    c.inv = 1.f; c.wdmul = 1.f; c.w1 = 0.f; c.b2 = 1.f; c.omb2 = 0.f; c.step_size = 0.f; c.bc2s = 1.f; c.eps = 1.f;
    if (full) {
        const double lr = a.lr * t.lr_factor;
        const double tt = (double)*a.step + 1.0;
        double p1, p2;
        os_pow2(a.beta1, a.beta2, (long long)tt, p1, p2);
        c.inv = os_inv_scale(a.scale);
        c.wdmul = (float)(1.0 - lr * (double)t.wd);
        c.w1 = (float)(1.0 - a.beta1);
        c.b2 = (float)a.beta2;
        c.omb2 = (float)(1.0 - a.beta2);
        c.step_size = (float)(lr / (1.0 - p1));
        c.bc2s = (float)sqrt(1.0 - p2);
        c.eps = (float)a.eps;
    }
    return c;
}

template <bool FULL>
__device__ __forceinline__ void os_one(const OsPtr& t, long long i, const OsCoef& c) {
    float p = t.p[i];
    if (FULL) {
        float m = t.m[i], v = t.v[i];
        os_adam(p, t.g[i], m, v, c);
        t.p[i] = p; t.m[i] = m; t.v[i] = v;
    }
    t.e[i] = os_ema(t.e[i], p, c);
}

template <bool FULL>
__device__ __forceinline__ void os_chunk_scalar(const OsPtr& t, long long lo, long long hi, const OsCoef& c) {
    constexpr int UN = 4;
    for (long long base = lo + threadIdx.x; base < hi; base += (long long)OS_TB * UN) {
        float p[UN], g[UN], m[UN], v[UN], e[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const long long i = base + (long long)u * OS_TB;
            if (i < hi) {
                p[u] = t.p[i]; e[u] = t.e[i];
                if (FULL) { g[u] = t.g[i]; m[u] = t.m[i]; v[u] = t.v[i]; }
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const long long i = base + (long long)u * OS_TB;
            if (i < hi) {
                if (FULL) {
                    os_adam(p[u], g[u], m[u], v[u], c);
                    t.p[i] = p[u]; t.m[i] = m[u]; t.v[i] = v[u];
                }
                t.e[i] = os_ema(e[u], p[u], c);
            }
        }
    }
}

// elements [lo, hi) of the entry; head = elements of the chunk in front of the first 16-byte boundary (the same for every array)
template <bool FULL>
__device__ __forceinline__ void os_chunk_vec(const OsPtr& t, long long lo, long long hi, int head, const OsCoef& c) {
    const long long a0 = lo + head < hi ? lo + head : hi;
    const int nvec = (int)((hi - a0) >> 2);
    const long long t0 = a0 + 4ll * nvec;                          // tail: [t0, hi), at most 3 elements
    const int tid = threadIdx.x;
    if (tid < (int)(a0 - lo)) os_one<FULL>(t, lo + tid, c);
    if (tid >= 64 && tid - 64 < (int)(hi - t0)) os_one<FULL>(t, t0 + (tid - 64), c);
    const gfloat4* p4 = (const gfloat4*)(t.p + a0);
    const gfloat4* e4 = (const gfloat4*)(t.e + a0);
    const gfloat4* g4 = (const gfloat4*)(t.g + a0);
    const gfloat4* m4 = (const gfloat4*)(t.m + a0);
    const gfloat4* v4 = (const gfloat4*)(t.v + a0);
#pragma unroll
    for (int k0 = 0; k0 < OS_U; k0 += 2) {
        os_f4 p[2], g[2], m[2], v[2], e[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + (k0 + u) * OS_TB;
            if (i < nvec) {
                p[u] = p4[i]; e[u] = e4[i];
                if (FULL) { g[u] = g4[i]; m[u] = m4[i]; v[u] = v4[i]; }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + (k0 + u) * OS_TB;
            if (i < nvec) {
                if (FULL) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float pj = p[u][j], mj = m[u][j], vj = v[u][j];
                        os_adam(pj, g[u][j], mj, vj, c);
                        p[u][j] = pj; m[u][j] = mj; v[u][j] = vj;
                    }
                    ((gfloat4*)(t.p + a0))[i] = p[u];
                    ((gfloat4*)(t.m + a0))[i] = m[u];
                    ((gfloat4*)(t.v + a0))[i] = v[u];
                }
                os_f4 r;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = os_ema(e[u][j], p[u][j], c);
                ((gfloat4*)(t.e + a0))[i] = r;
            }
        }
    }
}

__device__ __forceinline__ unsigned os_lo4(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u); }

__global__ __launch_bounds__(OS_TB) void os_update_kernel(const OsArgs a) {
    const OsBlock bm = a.map[blockIdx.x];
    if ((unsigned)bm.tensor >= (unsigned)a.n_tensors) return;
    const OsTensor t = a.tab[bm.tensor];
    const long long lo = (long long)bm.chunk * OS_CH;
    if (lo >= t.n) return;
    const long long hi = t.n - lo < OS_CH ? t.n : lo + OS_CH;
    bool full = (t.flags & OS_HAS_GRAD) && t.g && t.m && t.v;
    if (a.scale && *a.found_inf != 0.f) full = false;              // the skipped step: the moving average alone
    const OsCoef c = os_coef(a, t, full);
    const unsigned al = os_lo4(t.p);
    bool vec = (int)blockIdx.x < a.vec_chunks && os_lo4(t.e) == al && (al & 3u) == 0;
    if (full) vec = vec && os_lo4(t.g) == al && os_lo4(t.m) == al && os_lo4(t.v) == al;
    const OsPtr q(t);
    if (vec) {
        const int head = (int)(((16u - al) & 15u) >> 2);           // OS_CH is a multiple of 4: every chunk of the entry has the same head
        if (full) os_chunk_vec<true>(q, lo, hi, head, c); else os_chunk_vec<false>(q, lo, hi, head, c);
    } else {
        if (full) os_chunk_scalar<true>(q, lo, hi, c); else os_chunk_scalar<false>(q, lo, hi, c);
    }
}

// any(!isfinite(g * inv)) over the gradients -> *found_inf = 1.0f.  The gradient's own alignment decides head and tail here.
__global__ __launch_bounds__(OS_TB) void os_check_kernel(const OsArgs a) {
    const OsBlock bm = a.map[blockIdx.x];
    if ((unsigned)bm.tensor >= (unsigned)a.n_tensors) return;
    const OsTensor t = a.tab[bm.tensor];
    const long long lo = (long long)bm.chunk * OS_CH;
    if (!(t.flags & OS_HAS_GRAD) || !t.g || lo >= t.n) return;
    const long long hi = t.n - lo < OS_CH ? t.n : lo + OS_CH;
    const float inv = os_inv_scale(a.scale);
    const int tid = threadIdx.x;
    const gfloat* tg = (const gfloat*)t.g;
    bool bad = false;
    const unsigned al = os_lo4(t.g);
    if (al & 3u) {                                                 // not even 4-byte aligned: refused by the Python surface; stay correct
        for (long long i = lo + tid; i < hi; i += OS_TB) bad |= os_bad(tg[i], inv);
    } else {
        const int head = (int)(((16u - al) & 15u) >> 2);
        const long long a0 = lo + head < hi ? lo + head : hi;
        const int nvec = (int)((hi - a0) >> 2);
        const long long t0 = a0 + 4ll * nvec;
        if (tid < (int)(a0 - lo)) bad |= os_bad(tg[lo + tid], inv);
        if (tid >= 64 && tid - 64 < (int)(hi - t0)) bad |= os_bad(tg[t0 + (tid - 64)], inv);
        const gfloat4* g4 = (const gfloat4*)(tg + a0);
        os_f4 g[OS_U];
#pragma unroll
        for (int k = 0; k < OS_U; ++k) {
            const int i = tid + k * OS_TB;
            g[k] = 0.f;
            if (i < nvec) g[k] = g4[i];
        }
#pragma unroll
        for (int k = 0; k < OS_U; ++k) bad |= os_bad(g[k].x, inv) | os_bad(g[k].y, inv) | os_bad(g[k].z, inv) | os_bad(g[k].w, inv);
    }
    if (bad) *a.found_inf = 1.0f;
}

// step += 1 unless skipped; torch's _amp_update_scale_ (ATen/native/cuda/AmpKernels.cu) word for word
__global__ void os_finish_kernel(float* step, float* scale, int* tracker, const float* found_inf, double growth, double backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool skipped = scale && *found_inf != 0.f;
    if (!skipped) *step = *step + 1.f;
    if (!scale) return;
    if (skipped) {
        *scale = (float)((double)*scale * backoff);
        *tracker = 0;
    } else {
        const int successful = *tracker + 1;
        if (successful == interval) {
            const float grown = (float)((double)*scale * growth);
            if (fabsf(grown) <= FLT_MAX) *scale = grown;
            *tracker = 0;
        } else {
            *tracker = successful;
        }
    }
}

inline bool os_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

int opt_chunk_elems() { return OS_CH; }

size_t opt_table_bytes(int n_tensors, long long total_chunks) {
    if (n_tensors < 0 || total_chunks < 0 || total_chunks > 0x7fffffffll) return 0;
    const size_t tab = ((size_t)n_tensors * sizeof(OsTensor) + 255) & ~(size_t)255;
    return tab + (((size_t)total_chunks * sizeof(OsBlock) + 255) & ~(size_t)255);
}

int launch_opt_step(const void* table, size_t table_bytes, const void* block_map, size_t map_bytes, int n_tensors, int vec_chunks, int total_chunks,
                    float* step, float* scale, int* growth_tracker, float* found_inf, double lr, double beta1, double beta2, double eps,
                    double ema_decay, double growth_factor, double backoff_factor, int growth_interval, hipStream_t s) {
    UNI_REQUIRE(n_tensors >= 0 && total_chunks >= 0 && vec_chunks >= 0, "opt_step: negative size (n_tensors=%d, vec_chunks=%d, total_chunks=%d)", n_tensors,
                vec_chunks, total_chunks);
    UNI_REQUIRE(vec_chunks <= total_chunks, "opt_step: vec_chunks=%d > total_chunks=%d", vec_chunks, total_chunks);
    UNI_REQUIRE(total_chunks == 0 || n_tensors > 0, "opt_step: %d chunks of no tensor", total_chunks);
    UNI_REQUIRE(table_bytes >= (size_t)n_tensors * sizeof(OsTensor), "opt_step: table too small (%zu < %zu bytes for %d tensors)", table_bytes,
                (size_t)n_tensors * sizeof(OsTensor), n_tensors);
    UNI_REQUIRE(map_bytes >= (size_t)total_chunks * sizeof(OsBlock), "opt_step: block map too small (%zu < %zu bytes for %d chunks)", map_bytes,
                (size_t)total_chunks * sizeof(OsBlock), total_chunks);
    UNI_REQUIRE(os_aligned(table, 8) && os_aligned(block_map, 8), "opt_step: the tables must be 8-byte aligned");
    UNI_REQUIRE(os_aligned(step, 4) && os_aligned(scale, 4) && os_aligned(growth_tracker, 4) && os_aligned(found_inf, 4), "opt_step: misaligned state word");
    UNI_REQUIRE(!scale || (growth_tracker && found_inf), "opt_step: a scaler needs growth_tracker and found_inf (NULL argument)");
    UNI_REQUIRE(!scale || growth_interval >= 1, "opt_step: growth_interval=%d < 1", growth_interval);
    OsArgs a;
    a.tab = static_cast<const OsTensor*>(table); a.map = static_cast<const OsBlock*>(block_map);
    a.n_tensors = n_tensors; a.vec_chunks = vec_chunks;
    a.step = step; a.scale = scale; a.found_inf = scale ? found_inf : nullptr;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.d = (float)ema_decay; a.omd = (float)(1.0 - ema_decay);
    const int sc = scale != nullptr;
    if (sc) UNI_CHECK_HIP(hipMemsetAsync(found_inf, 0, sizeof(float), s));
    if (total_chunks > 0) {
        if (sc) {
            uni_variant_note("opt_step check scaler=1");
            os_check_kernel<<<total_chunks, OS_TB, 0, s>>>(a);
        }
        uni_variant_note("opt_step update scaler=%d forms=%s", sc, vec_chunks == 0 ? "scalar" : vec_chunks == total_chunks ? "vec" : "vec+scalar");
        os_update_kernel<<<total_chunks, OS_TB, 0, s>>>(a);
    }
    uni_variant_note("opt_step finish scaler=%d", sc);
    os_finish_kernel<<<1, 64, 0, s>>>(step, scale, growth_tracker, a.found_inf, growth_factor, backoff_factor, growth_interval);
    return 0;
}
