// Gradient of K4 (corr.hip): the label propagation of the reference's TRAINING losses, unicorn/models/unicorn.py:321-326 (compute_loss_sot)
// and :342-371 (compute_loss_vos), under autograd.  Per frame, R reference pixels, Q current pixels, D = 128, K value rows:
//     S[r,q] = <Eref[r,:], Ecur[q,:]>     P[r,q] = exp(S[r,q] - lse[q])     out[k,q] = sum_r V[k,r] P[r,q]
//     delta[q] = sum_k G[k,q] out[k,q]    T[r,q] = sum_k V[k,r] G[k,q]      dS[r,q] = P[r,q] (T[r,q] - delta[q])
//     dV[k,r] = sum_q G[k,q] P[r,q]       dEref[r,:] = sum_q dS[r,q] Ecur[q,:]      dEcur[q,:] = sum_r dS[r,q] Eref[r,:]
// Flash-style: P and dS are recomputed tile by tile from the embeddings and the forward's lse; the R x Q matrices never reach HBM.
//
// Structure (DESIGN.md "Correlation backward"): TWO recompute passes of ONE kernel template, each with one writer per output row --
//   pass "own = q": a wave keeps 32 current-frame pixels stationary, streams the reference map, accumulates dEcur^T in 64 accumulators;
//   pass "own = r": the roles swapped, accumulates dEref^T and dV.
// Four MFMA products instead of three, but no float atomics, no zeroing, bitwise reproducible results, and a gradient that is not
// wanted costs nothing (its pass is not launched).  The second product of a pass needs NO LDS crossing: the score accumulator of
// v_mfma_f32_32x32x2_f32 holds, in register r of the two half-waves, rows rowof(r,0) / rowof(r,1) of one own column -- exactly the k pair
// of one MFMA step -- so dS (computed in place in the accumulator registers) is the B operand of
//     dOwn^T[d, o] += sum_s Estream[s, d] dS[s, o]
// and the A operand is the stream tile already in LDS, read along d instead of along s.
// A block is 2 own groups x 4 stream quarters (8 waves): a 128-row stream super-tile is staged per step, wave (wo, wsp) contracts rows
// 32 wsp .. 32 wsp + 31 for own columns 32 wo .. 32 wo + 31, and the four quarter sums are added in a fixed order through LDS at the end
// (16000 own rows give 250 blocks x 8 waves: one block per CU, two waves per SIMD).
#include "kernels.h"

namespace {
constexpr int CD = 128;          // embedding dim
constexpr int LDA = 132;         // padded LDS row stride (floats), as corr_f32_kernel
constexpr int TR = 32;           // stream rows per wave and step
constexpr int NWO = 2, NWS = 4;  // own groups x stream quarters per block
constexpr int ST = TR * NWS;     // stream rows per step (super-tile)
constexpr int OB = 32 * NWO;     // own rows per block
constexpr int NT = 64 * NWO * NWS;
constexpr int KMAX = 8;          // value rows per pass (the 16-row instantiation spills, as in the exact-fp32 forward: more rows run in chunks)

__device__ __forceinline__ int rowof(int r, int fh) { return (r & 3) + 8 * (r >> 2) + 4 * fh; }

// delta[b][q] = sum_{k < K} G[b][k][q] out[b][k][q]   (G, out: chunk pointers, frame stride fs)
__global__ void corr_delta_kernel(const float* __restrict__ g, const float* __restrict__ out, float* __restrict__ delta, int Q, int K, long fs) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const size_t z = blockIdx.y;
    g += z * fs;
    out += z * fs;
    float d = 0.f;
    for (int k = 0; k < K; ++k) d = fmaf(g[(size_t)k * Q + q], out[(size_t)k * Q + q], d);
    delta[z * Q + q] = d;
}

// OWN_Q: own = current-frame pixels (writes dEcur), stream = reference pixels; else own = reference pixels (writes dEref, dV), stream = current.
// g: G chunk [K][Q], v: V chunk [K][R], K <= KMAX; lse / delta [Q]; down [n_own][128] (may be NULL: dV only); dv [K][R] (own = r only, may be NULL).
// The value rows are a RUN-TIME loop over LDS rows (K is 1 in the SOT loss): the register set does not depend on K.  dV of row 0 is summed in a
// register, rows 1.. in a private LDS cell per thread.
// LDS: As [2][ST][LDA] | Sv [2][KMAX + 2][ST] (stream-side rows: K vector rows, lse, delta) | Ov [KMAX][OB] (own-side rows) | Dv [K - 1][NT]
constexpr int NVRM = KMAX + 2;
constexpr int LDS_FIXED = 2 * ST * LDA + 2 * NVRM * ST + KMAX * OB;      // floats
constexpr int DV0_OFF = 2 * (NWS - 1) * 64 * 64;                         // dV row 0 parks behind the quarter sums (inside As, free after the loop)

template <bool OWN_Q>
__global__ __launch_bounds__(NT) void corr_bwd_kernel(const float* __restrict__ eown, const float* __restrict__ estr, int n_own, int n_str,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      const float* __restrict__ g, long g_fs, const float* __restrict__ v, long v_fs,
                                                      float* __restrict__ down, float* __restrict__ dv, long dv_fs, int K, int Q, int R,
                                                      int accumulate, int dv_accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Sv = smem + 2 * ST * LDA;
    float* Ov = Sv + 2 * NVRM * ST;
    float* Dv = Ov + KMAX * OB;
    {
        const size_t z = blockIdx.y;
        eown += z * (size_t)n_own * CD;
        estr += z * (size_t)n_str * CD;
        lse += z * (size_t)Q;
        delta += z * (size_t)Q;
        g += z * (size_t)g_fs;
        v += z * (size_t)v_fs;
        if (down) down += z * (size_t)n_own * CD;
        if (dv) dv += z * (size_t)dv_fs;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const int wo = wave % NWO, wsp = wave / NWO;
    const int o = blockIdx.x * OB + wo * 32 + fr;
    const int oc = o < n_own ? o : n_own - 1;
    const float* ovec = OWN_Q ? g : v;              // own-side K-vector (G[k][q] or V[k][r]), row stride n_own
    const float* svec = OWN_Q ? v : g;              // stream-side K-vector, row stride n_str
    const bool want_dv = !OWN_Q && dv != nullptr;

    // stationary operand, K-permutation of corr_f32_kernel: MFMA step t contracts dims {t, 64 + t}
    float b[64];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(eown + (size_t)oc * CD + fh * 64);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            f32x4 t = src[i];
            b[4 * i] = t[0]; b[4 * i + 1] = t[1]; b[4 * i + 2] = t[2]; b[4 * i + 3] = t[3];
        }
    }
    if (wsp == 0 && fh == 0)
        for (int k = 0; k < K; ++k) Ov[k * OB + wo * 32 + fr] = ovec[(size_t)k * n_own + oc];
    if (want_dv)
        for (int k = 1; k < K; ++k) Dv[(k - 1) * NT + tid] = 0.f;
    const float* ovl = Ov + wo * 32 + fr;
    float* dvl = Dv + tid;
    const float lse_o = OWN_Q ? lse[oc] : 0.f, del_o = OWN_Q ? delta[oc] : 0.f;
    const int ntiles = (n_str + ST - 1) / ST;
    const int nvr = OWN_Q ? K : K + 2;              // rows of Sv in use: K vector rows (+ lse, delta of the stream pixels)

    // the next super-tile travels through registers in eight pieces (the other LDS buffer is free for the whole step): 4 + 1 registers live.
    // Stream-side rows: thread tid stages element tid of [row][ST] (rows 0..3: all of K = 1, 2); further rows are copied without the register stage.
    f32x4 ga;
    float gvv;
    auto gload_e = [&](int t, int h) __attribute__((always_inline)) {
        const int r0 = t * ST;
        const int idx = tid + NT * h;
        const int row = min(r0 + (idx >> 5), n_str - 1);
        ga = *reinterpret_cast<const f32x4*>(estr + (size_t)row * CD + (idx & 31) * 4);
    };
    auto sstore_e = [&](int buf, int h) __attribute__((always_inline)) {
        const int idx = tid + NT * h;
        *reinterpret_cast<f32x4*>(As + buf * ST * LDA + (idx >> 5) * LDA + (idx & 31) * 4) = ga;
    };
    auto vload = [&](int idx, int r0) __attribute__((always_inline)) -> float {
        const int vr = idx / ST, s = r0 + (idx % ST);
        float x = 0.f;
        if (vr < K) {
            if (s < n_str) x = svec[(size_t)vr * n_str + s];
        } else if (!OWN_Q && vr < nvr) {
            if (vr == K) x = s < n_str ? lse[s] : INFINITY;            // a row past the end: P = exp(-inf) = 0
            else x = s < n_str ? delta[s] : 0.f;
        }
        return x;
    };
    auto gload_v = [&](int t) __attribute__((always_inline)) { gvv = vload(tid, t * ST); };
    auto sstore_v = [&](int t, int buf) __attribute__((always_inline)) {
        if (tid < nvr * ST) Sv[buf * NVRM * ST + tid] = gvv;
#pragma unroll 1
        for (int idx = tid + NT; idx < nvr * ST; idx += NT) Sv[buf * NVRM * ST + idx] = vload(idx, t * ST);
    };

    f32x16 dacc[4];
    float dv0 = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[dt][r] = 0.f;

    gload_v(0);
    sstore_v(0, 0);
#pragma unroll
    for (int h = 0; h < 8; ++h) { gload_e(0, h); sstore_e(0, h); }
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        const bool more = t + 1 < ntiles;
        if (more) { gload_e(t + 1, 0); gload_v(t + 1); }
        const float* at = As + buf * ST * LDA + wsp * TR * LDA;
        const float* arow = at + fr * LDA + fh * 64;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {                 // S tile, the forward's contraction order (the same bits as the scores lse came from)
            f32x4 a4 = *reinterpret_cast<const f32x4*>(arow + 4 * i);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[0], b[4 * i], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[1], b[4 * i + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[2], b[4 * i + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[3], b[4 * i + 3], acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) { sstore_e(buf ^ 1, 0); sstore_v(t + 1, buf ^ 1); gload_e(t + 1, 1); }
        __builtin_amdgcn_sched_barrier(0);
        // acc[r] = S[stream row rowof(r, fh)][own column fr]  ->  dS in place; P by the accurate expf (arguments reach -100 and below)
        const float* sv = Sv + buf * NVRM * ST + wsp * TR;
        const int s0 = t * ST + wsp * TR;
        const bool full = s0 + TR <= n_str;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int off = 8 * gq + 4 * fh;          // rowof(4 gq + j, fh) = off + j
            f32x4 l4 = {lse_o, lse_o, lse_o, lse_o}, p4;
            if (!OWN_Q) l4 = *reinterpret_cast<const f32x4*>(sv + K * ST + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p = expf(acc[4 * gq + j] - l4[j]);
                if (OWN_Q && !full && s0 + off + j >= n_str) p = 0.f;      // own = r: the staged lse of a row past the end is +inf
                p4[j] = p;
            }
            f32x4 x = *reinterpret_cast<const f32x4*>(sv + off);
            f32x4 tv = ovl[0] * x;
            if (want_dv) dv0 += p4[0] * x[0] + p4[1] * x[1] + p4[2] * x[2] + p4[3] * x[3];
#pragma unroll 1
            for (int k = 1; k < K; ++k) {
                x = *reinterpret_cast<const f32x4*>(sv + k * ST + off);
                tv += ovl[k * OB] * x;
                if (want_dv) dvl[(k - 1) * NT] += p4[0] * x[0] + p4[1] * x[1] + p4[2] * x[2] + p4[3] * x[3];
            }
            f32x4 d4 = {del_o, del_o, del_o, del_o};
            if (!OWN_Q) d4 = *reinterpret_cast<const f32x4*>(sv + (K + 1) * ST + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * gq + j] = p4[j] * (tv[j] - d4[j]);
            __builtin_amdgcn_sched_barrier(0);       // keep the LDS reads of one row quad from being hoisted over the others (register budget)
        }
        if (more) { sstore_e(buf ^ 1, 1); gload_e(t + 1, 2); }
        // dOwn^T[d][o] += sum_s Estream[s][d] dS[s][o]: step r contracts the stream rows rowof(r, 0), rowof(r, 1) -- the accumulator IS the operand
        if (down) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* ap = at + rowof(r, fh) * LDA + fr;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) dacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[32 * dt], acc[r], dacc[dt], 0, 0, 0);
                if (more && r % 3 == 1) { sstore_e(buf ^ 1, 2 + r / 3); gload_e(t + 1, 3 + r / 3); }      // r = 1, 4, 7, 10, 13: pieces 2..6 out, 3..7 in
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) {
            if (!down) {                              // dV-only pass: no second product to hide the copies behind
#pragma unroll
                for (int h = 2; h < 7; ++h) { sstore_e(buf ^ 1, h); gload_e(t + 1, h + 1); }
            }
            sstore_e(buf ^ 1, 7);
        }
        __syncthreads();
    }
    // the four stream quarters of an own group: quarters 1..3 park their sums in LDS, quarter 0 adds them in a fixed order and writes
    if (wsp > 0) {
        float* red = smem + (size_t)(wo * (NWS - 1) + (wsp - 1)) * 64 * 64 + lane;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) red[(dt * 16 + i) * 64] = dacc[dt][i];
    }
    smem[DV0_OFF + tid] = dv0;
    __syncthreads();
    if (wsp > 0) return;
    if (want_dv && fh == 0 && o < n_own) {
        for (int k = 0; k < K; ++k) {
            const float* src = k ? Dv + (k - 1) * NT : smem + DV0_OFF;
            float sum = 0.f;
            for (int w = 0; w < NWS; ++w) sum += src[(w * NWO + wo) * 64 + fr] + src[(w * NWO + wo) * 64 + 32 + fr];
            float* p = dv + (size_t)k * R + o;
            *p = dv_accumulate ? *p + sum : sum;
        }
    }
    if (!down || o >= n_own) return;
    for (int sp = 0; sp < NWS - 1; ++sp) {
        const float* rp = smem + (size_t)(wo * (NWS - 1) + sp) * 64 * 64 + lane;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) dacc[dt][i] += rp[(dt * 16 + i) * 64];
    }
    // lane (fr, fh) holds dOwn[o][32 dt + rowof(i, fh)]: four consecutive dims per register quad
    float* dst = down + (size_t)o * CD + 4 * fh;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            f32x4 x = {dacc[dt][4 * gq], dacc[dt][4 * gq + 1], dacc[dt][4 * gq + 2], dacc[dt][4 * gq + 3]};
            f32x4* p = reinterpret_cast<f32x4*>(dst + 32 * dt + 8 * gq);
            if (accumulate) x += *p;
            *p = x;
        }
}

template <bool OWN_Q>
int run_pass(const float* eown, const float* estr, int n_own, int n_str, const float* lse, const float* delta, const float* g, long g_fs,
             const float* v, long v_fs, float* down, float* dv, long dv_fs, int K, int Q, int R, int accumulate, int dv_accumulate, int B,
             hipStream_t s) {
    const size_t lds = (size_t)(LDS_FIXED + (dv && K > 1 ? (K - 1) * NT : 0)) * sizeof(float);
    static DevOnce attr_once;      // > 64 KiB dynamic LDS needs the opt-in attribute (for the largest request: KMAX rows with dV)
    UNI_LDS_OPTIN(attr_once, "corr_bwd", (size_t)(LDS_FIXED + (KMAX - 1) * NT) * sizeof(float), reinterpret_cast<const void*>(&corr_bwd_kernel<OWN_Q>));
    hipLaunchKernelGGL((corr_bwd_kernel<OWN_Q>), dim3(cdiv(n_own, OB), B), dim3(NT), lds, s, eown, estr, n_own, n_str, lse, delta, g, g_fs,
                       v, v_fs, down, dv, dv_fs, K, Q, R, accumulate, dv_accumulate);
    return 0;
}

// ---------------------------------------------------------------- fp64: one wave per output row, FMA loops, fixed summation order
__device__ __forceinline__ double dot128(const double* __restrict__ a, double b0, double b1, int lane) {
    return wave_sum(fma(a[lane], b0, a[lane + 64] * b1));
}

// wave per (frame, q): lse[q], out[k][q]
__global__ __launch_bounds__(64) void corr_f64_kernel(const double* __restrict__ eref, const double* __restrict__ ecur, const double* __restrict__ v,
                                                       double* __restrict__ out, double* __restrict__ lse, int R, int Q, int K, long v_fs) {
    const size_t z = blockIdx.y;
    const int q = blockIdx.x, lane = threadIdx.x;
    eref += z * (size_t)R * CD;
    v += z * (size_t)v_fs;
    const double* eq = ecur + (z * Q + q) * CD;
    const double b0 = eq[lane], b1 = eq[lane + 64];
    double m = -INFINITY;
    for (int r = 0; r < R; ++r) m = fmax(m, dot128(eref + (size_t)r * CD, b0, b1, lane));
    double l = 0.0;
    for (int r = 0; r < R; ++r) l += exp(dot128(eref + (size_t)r * CD, b0, b1, lane) - m);
    const double ls = m + log(l);
    if (lane == 0) lse[z * Q + q] = ls;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        double o = 0.0;
        for (int r = 0; r < R; ++r) {
            const double p = exp(dot128(eref + (size_t)r * CD, b0, b1, lane) - ls);
            if (k < K) o = fma(v[(size_t)k * R + r], p, o);
        }
        if (k < K) out[(z * K + k) * Q + q] = o;
    }
}

// wave per (frame, own row); OWN_Q: dEcur[q][:]; else dEref[r][:]
template <bool OWN_Q>
__global__ __launch_bounds__(64) void corr_bwd_f64_kernel(const double* __restrict__ eown, const double* __restrict__ estr, int n_own, int n_str,
                                                           const double* __restrict__ v, long v_fs, const double* __restrict__ out,
                                                           const double* __restrict__ lse, const double* __restrict__ g, double* __restrict__ down,
                                                           int R, int Q, int K) {
    const size_t z = blockIdx.y;
    const int o = blockIdx.x, lane = threadIdx.x;
    eown += z * (size_t)n_own * CD;
    estr += z * (size_t)n_str * CD;
    v += z * (size_t)v_fs;
    out += z * (size_t)K * Q;
    g += z * (size_t)K * Q;
    lse += z * (size_t)Q;
    const double b0 = eown[(size_t)o * CD + lane], b1 = eown[(size_t)o * CD + lane + 64];
    double a0 = 0.0, a1 = 0.0;
    if (down) {
        for (int s = 0; s < n_str; ++s) {
            const int r = OWN_Q ? s : o, q = OWN_Q ? o : s;
            const double* es = estr + (size_t)s * CD;
            const double p = exp(dot128(es, b0, b1, lane) - lse[q]);
            double tmd = 0.0;                         // T[r,q] - delta[q] = sum_k G[k,q] (V[k,r] - out[k,q]), evaluated as the two sums of the formula
            double tt = 0.0, dd = 0.0;
            for (int k = 0; k < K; ++k) {
                const double gk = g[(size_t)k * Q + q];
                tt = fma(v[(size_t)k * R + r], gk, tt);
                dd = fma(gk, out[(size_t)k * Q + q], dd);
            }
            tmd = tt - dd;
            const double ds = p * tmd;
            a0 = fma(ds, es[lane], a0);
            a1 = fma(ds, es[lane + 64], a1);
        }
        double* dst = down + (z * n_own + o) * CD;
        dst[lane] = a0;
        dst[lane + 64] = a1;
    }
}

// wave per (frame or 0, r): dV[k][r] = sum_q G[k][q] P[r][q]; shared value rows (nb = B frames walked in order by the one writer) or per frame
__global__ __launch_bounds__(64) void corr_dv_f64_kernel(const double* __restrict__ eref, const double* __restrict__ ecur, const double* __restrict__ lse,
                                                          const double* __restrict__ g, double* __restrict__ dv, int R, int Q, int K, int nb) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const size_t z0 = (size_t)blockIdx.y * (nb == 1 ? 1 : 0);
    dv += (nb == 1 ? (size_t)blockIdx.y : 0) * (size_t)K * R;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        double acc = 0.0;
        for (int b = 0; b < nb; ++b) {
            const size_t z = z0 + b;
            const double* er = eref + (z * R + r) * CD;
            const double b0 = er[lane], b1 = er[lane + 64];
            for (int q = 0; q < Q; ++q) {
                const double p = exp(dot128(ecur + (z * Q + q) * CD, b0, b1, lane) - lse[z * Q + q]);
                if (k < K) acc = fma(g[(z * K + k) * Q + q], p, acc);
            }
        }
        if (k < K) dv[(size_t)k * R + r] = acc;
    }
}
}  // namespace

size_t corr_bwd_workspace_bytes(int B, int R, int Q, int K) {
    if (B < 1 || R < 1 || Q < 1 || K < 1) return 0;
    const size_t f = corr_workspace_bytes_batched(B, R, Q, K), d = (size_t)B * Q * sizeof(float);
    return f > d ? f : d;
}

int launch_corr_bwd(const float* eref, const float* ecur, const float* v, const float* out, const float* lse, const float* gout, float* gref,
                    float* gcur, float* gv, int B, int R, int Q, int D, int K, int values_per_frame, int precision, void* workspace,
                    size_t ws_bytes, hipStream_t s) {
    UNI_REQUIRE(D == CD, "corr_bwd: embedding dim %d unsupported (128)", D);
    UNI_REQUIRE(B > 0 && R > 0 && Q > 0 && K > 0, "corr_bwd: empty problem B=%d R=%d Q=%d K=%d", B, R, Q, K);
    UNI_REQUIRE(precision == 0, "corr_bwd: precision %d not implemented (the backward runs in 0 = exact fp32 MFMA only)", precision);
    UNI_REQUIRE(((uintptr_t)eref & 15) == 0 && ((uintptr_t)ecur & 15) == 0 && ((uintptr_t)gref & 15) == 0 && ((uintptr_t)gcur & 15) == 0,
                "corr_bwd: embeddings and their gradients must be 16-B aligned");
    UNI_REQUIRE(((uintptr_t)workspace & 15) == 0 && ws_bytes >= corr_bwd_workspace_bytes(B, R, Q, K), "corr_bwd: workspace too small or misaligned");
    if (!gref && !gcur && !gv) return 0;
    float* delta = reinterpret_cast<float*>(workspace);          // [B][Q], per chunk of value rows
    const long vfs = values_per_frame ? (long)K * R : 0, gfs = (long)K * Q;
    const bool dv_shared = gv && !values_per_frame && B > 1;     // [K][R] summed over the frames: the frames run one after the other
    // dS is linear in the value rows: chunks of up to 16 rows add into the embedding gradients (one writer per row: a plain read-add-write)
    for (int k0 = 0; k0 < K; k0 += KMAX) {
        const int kc = K - k0 < KMAX ? K - k0 : KMAX;
        const float *gk = gout + (size_t)k0 * Q, *vk = v + (size_t)k0 * R, *ok = out + (size_t)k0 * Q;
        float* gvk = gv ? gv + (size_t)k0 * R : nullptr;
        if (gref || gcur) hipLaunchKernelGGL(corr_delta_kernel, dim3(cdiv(Q, 256), B), dim3(256), 0, s, gk, ok, delta, Q, kc, gfs);
        int rc = 0;
        if (gcur) rc = run_pass<true>(ecur, eref, Q, R, lse, delta, gk, gfs, vk, vfs, gcur, (float*)nullptr, 0L, kc, Q, R, k0 > 0, 0, B, s);
        if (rc) return rc;
        if (!gref && !gv) continue;
        if (!dv_shared) {
            rc = run_pass<false>(eref, ecur, R, Q, lse, delta, gk, gfs, vk, vfs, gref, gvk, vfs, kc, Q, R, k0 > 0, 0, B, s);
        } else {
            for (int b = 0; b < B && !rc; ++b)
                rc = run_pass<false>(eref + (size_t)b * R * CD, ecur + (size_t)b * Q * CD, R, Q, lse + (size_t)b * Q, delta + (size_t)b * Q,
                                       gk + (size_t)b * gfs, gfs, vk, 0L, gref ? gref + (size_t)b * R * CD : nullptr, gvk, 0L, kc, Q, R, k0 > 0,
                                       b > 0, 1, s);
        }
        if (rc) return rc;
    }
    return 0;
}

int launch_corr_f64(const double* eref, const double* ecur, const double* v, double* out, double* lse, int B, int R, int Q, int D, int K,
                    int values_per_frame, hipStream_t s) {
    UNI_REQUIRE(D == CD, "corr_f64: embedding dim %d unsupported (128)", D);
    UNI_REQUIRE(B > 0 && R > 0 && Q > 0 && K > 0, "corr_f64: empty problem B=%d R=%d Q=%d K=%d", B, R, Q, K);
    UNI_REQUIRE(B <= 65535, "corr_f64: more than 65535 frames");
    hipLaunchKernelGGL(corr_f64_kernel, dim3(Q, B), dim3(64), 0, s, eref, ecur, v, out, lse, R, Q, K, values_per_frame ? (long)K * R : 0L);
    return 0;
}

int launch_corr_bwd_f64(const double* eref, const double* ecur, const double* v, const double* out, const double* lse, const double* gout,
                        double* gref, double* gcur, double* gv, int B, int R, int Q, int D, int K, int values_per_frame, hipStream_t s) {
    UNI_REQUIRE(D == CD, "corr_bwd_f64: embedding dim %d unsupported (128)", D);
    UNI_REQUIRE(B > 0 && R > 0 && Q > 0 && K > 0, "corr_bwd_f64: empty problem B=%d R=%d Q=%d K=%d", B, R, Q, K);
    UNI_REQUIRE(B <= 65535, "corr_bwd_f64: more than 65535 frames");
    const long vfs = values_per_frame ? (long)K * R : 0L;
    if (gcur)
        hipLaunchKernelGGL(corr_bwd_f64_kernel<true>, dim3(Q, B), dim3(64), 0, s, ecur, eref, Q, R, v, vfs, out, lse, gout, gcur, R, Q, K);
    if (gref)
        hipLaunchKernelGGL(corr_bwd_f64_kernel<false>, dim3(R, B), dim3(64), 0, s, eref, ecur, R, Q, v, vfs, out, lse, gout, gref, R, Q, K);
    if (gv) {
        const int nb = values_per_frame ? 1 : B;
        hipLaunchKernelGGL(corr_dv_f64_kernel, dim3(R, values_per_frame ? B : 1), dim3(64), 0, s, eref, ecur, lse, gout, gv, R, Q, K, nb);
    }
    return 0;
}
