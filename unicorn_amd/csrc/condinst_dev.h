// The CondInst mask loss arithmetic, defined ONCE for condinst_loss.hip (one image, compacted instances) and head_mask_loss.hip (the whole
// batch from the device-side assignment).  The kernels of both files are shells: a shell works out which instance (compacted index or table
// slot) it handles and which logits / ground-truth / parameter rows that instance reads, and calls a body below.
//
//   cl_inputs / cl_mlp / cl_mlp_bwd   the 10-8-8-1 MLP of an instance at a coarse pixel and its backward
//   cl_map / cl_taps                  fine-pixel thread mapping, tap softmax of the convex upsample
//   cl_dice_accum / cl_dice_combine   (sum s g, sum s^2, sum g^2) of an instance over a wave; block partials of a group of up to CL_IC instances
//   cl_dice_partial / cl_dice_finish  block partials -> sums[3], 1 - 2 I / U
//   cl_du_instance / cl_stage_taps    du and d up_masks of one instance at a fine pixel; A[p][t] = sum_sub w_t du through LDS
//   cl_gather_pixel                   dL[q] = sum_t A[q - delta_t][t]
//   cl_dparams_half                   one half of the 169 parameter gradients of an instance: block partials
//   cl_dfeat_instance                 one instance's step of the d mask_feats loop
//
// Every sum has a fixed order (both operators promise bitwise-reproducible results and the batched one is tested against a loop of the
// per-image one): a change of an order, of the 1e-5 or of the zero padding of a tap is made here, for both.
#pragma once
#include "kernels.h"

namespace {

constexpr int CL_NP = 169;     // 80 | 64 | 8 | 8 | 8 | 1 (parse_dynamic_params)
constexpr int CL_IC = 8;       // dice forward: instances per block pass (the tap softmax does not depend on the instance, misc.hip CU_IC)
constexpr int CL_PPT = 4;      // parameter-gradient kernels: coarse pixels per thread
constexpr int CL_FB = 128;     // d mask_feats kernels: block

template <typename T> __device__ __forceinline__ T cl_exp(T x);
template <> __device__ __forceinline__ float cl_exp<float>(float x) { return expf(x); }        // accurate: this path is differentiated
template <> __device__ __forceinline__ double cl_exp<double>(double x) { return exp(x); }

// Thread mapping of the fine-pixel kernels: a block owns PX consecutive coarse pixels; tid = i (PX r) + xl r + j, so a wave reads contiguous
// ground-truth rows (r = 4: 64 consecutive floats).
__device__ __forceinline__ void cl_map(int r, int PX, int HWc, int& pix, int& i, int& j, int& xl, bool& valid) {
    const int span = PX * r, tid = threadIdx.x;
    i = tid / span;
    const int rem = tid - i * span;
    xl = rem / r;
    j = rem - xl * r;
    pix = blockIdx.x * PX + xl;
    valid = tid < span * r && pix < HWc;
}

template <typename T>
__device__ __forceinline__ void cl_inputs(const T* __restrict__ mask_feats, const T* __restrict__ inst_loc, const int* __restrict__ inst_lvl,
                                          int inst, int pix, int W, T in[10]) {
    const T soi_tab[5] = {(T)64, (T)128, (T)256, (T)512, (T)1024};
    const T soi = soi_tab[min(max(inst_lvl[inst], 0), 4)];
    const int y = pix / W, x = pix - y * W;
    in[0] = (inst_loc[inst * 2] - (T)(x * 8 + 4)) / soi;       // comm.py:30-43 locations = arange * 8 + 4
    in[1] = (inst_loc[inst * 2 + 1] - (T)(y * 8 + 4)) / soi;
#pragma unroll
    for (int c = 0; c < 8; ++c) in[2 + c] = mask_feats[(size_t)pix * 8 + c];
}

// condinst_mlp_kernel's arithmetic (misc.hip), keeping the hidden activations
template <typename T>
__device__ __forceinline__ T cl_mlp(const T* prm, const T in[10], T h0[8], T h1[8]) {
    const T *w0 = prm, *w1 = prm + 80, *w2 = prm + 144, *b0 = prm + 152, *b1 = prm + 160, *b2 = prm + 168;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        T s = b0[o];
#pragma unroll
        for (int i = 0; i < 10; ++i) s += w0[o * 10 + i] * in[i];
        h0[o] = s > (T)0 ? s : (T)0;
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        T s = b1[o];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += w1[o * 8 + i] * h0[i];
        h1[o] = s > (T)0 ? s : (T)0;
    }
    T s = b2[0];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += w2[i] * h1[i];
    return s;
}

// normalised tap weights of one fine pixel and the (zero-padded) neighbour offsets of its coarse pixel
template <typename T>
__device__ __forceinline__ void cl_taps(const T* __restrict__ up_masks, int pix, int sub, int rr, int H, int W, bool valid, T wt[9], int off[9]) {
    if (!valid) {
#pragma unroll
        for (int t = 0; t < 9; ++t) { wt[t] = (T)0; off[t] = -1; }
        return;
    }
    const T* um = up_masks + (size_t)pix * 9 * rr + sub;
    const int y = pix / W, x = pix - y * W;
    T mx = um[0];
#pragma unroll
    for (int t = 0; t < 9; ++t) { wt[t] = um[t * rr]; mx = wt[t] > mx ? wt[t] : mx; }
    T sum = (T)0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        wt[t] = cl_exp<T>(wt[t] - mx);
        sum += wt[t];
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        off[t] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? yy * W + xx : -1;
    }
    const T inv = (T)1 / sum;
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] *= inv;
}

template <typename T>
__device__ __forceinline__ T cl_wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// parameter columns of the two halves the parameter-gradient kernel is split into (169 accumulators per thread do not fit the register
// file next to the recomputation): half 0 = W0 | b0 (88 columns), half 1 = W1 | W2 | b1 | b2 (81 columns)
__device__ __forceinline__ constexpr bool cl_in_half(int half, int i) { return ((i < 80 || (i >= 152 && i < 160)) ? 0 : 1) == half; }

// backward of the three layers at one pixel: accumulates the parameter gradients of one half (HALF 0 / 1; gp[169], the other half's entries
// are never touched) or returns d in[2..9] (HALF < 0, dmf)
template <typename T, int HALF>
__device__ __forceinline__ void cl_mlp_bwd(const T* prm, const T in[10], T dLv, T* gp, T* dmf) {
    const T *w0 = prm, *w1 = prm + 80, *w2 = prm + 144;
    T h0[8], h1[8], dh1[8], dh0[8];
    cl_mlp(prm, in, h0, h1);
#pragma unroll
    for (int o = 0; o < 8; ++o) dh1[o] = h1[o] > (T)0 ? dLv * w2[o] : (T)0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        T s = (T)0;
#pragma unroll
        for (int o = 0; o < 8; ++o) s += w1[o * 8 + i] * dh1[o];
        dh0[i] = h0[i] > (T)0 ? s : (T)0;
    }
    if (HALF == 0) {
#pragma unroll
        for (int o = 0; o < 8; ++o) {
#pragma unroll
            for (int i = 0; i < 10; ++i) gp[o * 10 + i] += dh0[o] * in[i];
            gp[152 + o] += dh0[o];
        }
    }
    if (HALF == 1) {
#pragma unroll
        for (int o = 0; o < 8; ++o) {
#pragma unroll
            for (int i = 0; i < 8; ++i) gp[80 + o * 8 + i] += dh1[o] * h0[i];
            gp[144 + o] += dLv * h1[o];
            gp[160 + o] += dh1[o];
        }
        gp[168] += dLv;
    }
    if (HALF < 0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            T s = (T)0;
#pragma unroll
            for (int o = 0; o < 8; ++o) s += w0[o * 10 + 2 + c] * dh0[o];
            dmf[c] += s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the kernel bodies

// U of the dice loss from sum s^2 and sum g^2
template <typename T>
__device__ __forceinline__ T cl_dice_den(T ss, T gg) { return ss + gg + (T)1e-5; }

// (s g, s^2, g^2) of instance inst (logits[inst]; g_at(inst) = its ground truth at the thread's fine pixel, read only by a mapped thread)
// summed over each wave -> red[wave][3 k ..]: k < CL_IC counts the instances of the group a block handles between two cl_dice_combine
template <typename T, typename G>
__device__ __forceinline__ void cl_dice_accum(const T (&wt)[9], const int (&off)[9], bool valid, const T* logits, int HWc, G g_at, int inst,
                                              T (*red)[3 * CL_IC], int k) {
    T sg = (T)0, ss = (T)0, gg = (T)0;
    if (valid) {
        const T* L = logits + (size_t)inst * HWc;
        T u = (T)0;
#pragma unroll
        for (int t = 0; t < 9; ++t) u += wt[t] * (off[t] >= 0 ? L[off[t]] : (T)0);
        const T s = (T)1 / ((T)1 + cl_exp<T>(-u));
        const T g = g_at(inst);
        sg = s * g; ss = s * s; gg = g * g;
    }
    sg = cl_wave_sum(sg); ss = cl_wave_sum(ss); gg = cl_wave_sum(gg);
    if ((threadIdx.x & 63) == 0) {
        const int wave = threadIdx.x >> 6;
        red[wave][3 * k] = sg; red[wave][3 * k + 1] = ss; red[wave][3 * k + 2] = gg;
    }
}

// the block partials of the group i0 .. i0 + cnt - 1 that cl_dice_accum left in red: the four waves in order -> part[inst][blockIdx.x][3].
// 256 threads; a caller that goes on to another group puts a barrier behind it.
template <typename T>
__device__ __forceinline__ void cl_dice_combine(int i0, int cnt, T (*red)[3 * CL_IC], T* part, int nblk) {
    __syncthreads();
    if ((int)threadIdx.x < 3 * cnt) {
        const int e = threadIdx.x;
        part[((size_t)(i0 + e / 3) * nblk + blockIdx.x) * 3 + e % 3] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

// the thread's strided share a[3] of the nblk block partials of instance inst
template <typename T>
__device__ __forceinline__ void cl_dice_partial(const T* part, int inst, int nblk, T (&a)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = (T)0;
    for (int b = threadIdx.x; b < nblk; b += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] += part[((size_t)inst * nblk + b) * 3 + c];
    }
}

// the 256 shares of cl_dice_partial -> sums[inst][3] and the dice loss of the instance: a 256-wide halving tree.  A caller that goes round
// again puts a barrier in front of it (red).
template <typename T>
__device__ __forceinline__ void cl_dice_finish(const T (&a)[3], T (*red)[256], int inst, T* sums, T* loss) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][tid] = a[c];
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const T I = red[0][0], U = cl_dice_den(red[1][0], red[2][0]);
        sums[inst * 3] = I; sums[inst * 3 + 1] = red[1][0]; sums[inst * 3 + 2] = red[2][0];
        loss[inst] = (T)1 - (T)2 * I / U;
    }
}

// instance inst (sums[inst], logits[inst], go = d loss / d its dice, g_at(inst) as in cl_dice_accum) at the thread's fine pixel:
// c[t] = w_t du with du = go (-2 g / U + 4 I s / U^2) s (1 - s) (zeros for an unmapped thread), acc[t] += c[t] (L_t - u)
template <typename T, typename G>
__device__ __forceinline__ void cl_du_instance(const T* sums, T go, const T (&wt)[9], const int (&off)[9], bool valid,
                                               const T* logits, int HWc, G g_at, int inst, T (&c)[9], T (&acc)[9]) {
    const T I = sums[inst * 3], U = cl_dice_den(sums[inst * 3 + 1], sums[inst * 3 + 2]);
    const T ca = (T)-2 * go / U, cb = (T)4 * go * I / (U * U);
#pragma unroll
    for (int t = 0; t < 9; ++t) c[t] = (T)0;
    if (valid) {
        const T* L = logits + (size_t)inst * HWc;
        T Lt[9], u = (T)0;
#pragma unroll
        for (int t = 0; t < 9; ++t) { Lt[t] = off[t] >= 0 ? L[off[t]] : (T)0; u += wt[t] * Lt[t]; }
        const T s = (T)1 / ((T)1 + cl_exp<T>(-u));
        const T g = g_at(inst);
        const T du = (ca * g + cb * s) * (s * ((T)1 - s));
#pragma unroll
        for (int t = 0; t < 9; ++t) { c[t] = wt[t] * du; acc[t] += c[t] * (Lt[t] - u); }
    }
}

// A[k][p][t] = sum over the r x r fine pixels of coarse pixel p of c[t], in a fixed order through LDS (k = the instance's row of the staged
// A buffer; the block owns the coarse pixels pix0 .. pix0 + PX - 1).  256 threads, a barrier on both sides of the sum.
template <typename T>
__device__ __forceinline__ void cl_stage_taps(const T (&c)[9], T (*cs)[256], T* A, int k, int r, int PX, int HWc) {
    const int span = PX * r, pix0 = blockIdx.x * PX;
#pragma unroll
    for (int t = 0; t < 9; ++t) cs[t][threadIdx.x] = c[t];
    __syncthreads();
    for (int o = threadIdx.x; o < PX * 9; o += 256) {
        const int pl = o / 9, t = o - pl * 9;
        if (pix0 + pl < HWc) {
            T s = (T)0;
            for (int ii = 0; ii < r; ++ii)
                for (int jj = 0; jj < r; ++jj) s += cs[t][ii * span + pl * r + jj];
            A[((size_t)k * HWc + pix0 + pl) * 9 + t] = s;
        }
    }
    __syncthreads();
}

// dL of the instance staged in row k of A at the coarse pixel q = (y, x): the 9 taps that read q, one writer
template <typename T>
__device__ __forceinline__ T cl_gather_pixel(const T* A, int k, int y, int x, int H, int W) {
    const int HWc = H * W;
    T s = (T)0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {      // the coarse pixel p whose tap t reads q: p + delta_t = q
        const int yy = y - (t / 3 - 1), xx = x - (t % 3 - 1);
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) s += A[((size_t)k * HWc + yy * W + xx) * 9 + t];
    }
    return s;
}

// one half of the parameter gradients of instance inst (prm = its parameters in LDS; it indexes inst_loc / inst_lvl / dL / part) over the
// CL_PPT x 256 coarse pixels of block blockIdx.x: per-thread accumulators, wave sums, the four waves in order -> part[inst][block][169]
template <typename T, int HALF>
__device__ __forceinline__ void cl_dparams_half(const T* prm, T (*red)[CL_NP], const T* __restrict__ mask_feats, const T* __restrict__ inst_loc,
                                                const int* __restrict__ inst_lvl, const T* __restrict__ dL, int inst, int HWc, int W,
                                                T* __restrict__ part, int nblk) {
    const int tid = threadIdx.x;
    T gp[CL_NP];
#pragma unroll
    for (int i = 0; i < CL_NP; ++i) gp[i] = (T)0;
    for (int k = 0; k < CL_PPT; ++k) {
        const int pix = (blockIdx.x * CL_PPT + k) * 256 + tid;
        if (pix < HWc) {
            T in[10];
            cl_inputs(mask_feats, inst_loc, inst_lvl, inst, pix, W, in);
            cl_mlp_bwd<T, HALF>(prm, in, dL[(size_t)inst * HWc + pix], gp, nullptr);
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int i = 0; i < CL_NP; ++i) {
        if (cl_in_half(HALF, i)) {
            const T v = cl_wave_sum(gp[i]);
            if (lane == 0) red[wave][i] = v;
        }
    }
    __syncthreads();
    if (tid < CL_NP && cl_in_half(HALF, tid))
        part[((size_t)inst * nblk + blockIdx.x) * CL_NP + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one instance's step of the d mask_feats loop of a block of CL_FB coarse pixels: its parameters (prow) into LDS, then dmf += d in[2..9]
template <typename T>
__device__ __forceinline__ void cl_dfeat_instance(T* prm, const T* __restrict__ prow, const T* __restrict__ mask_feats,
                                                  const T* __restrict__ inst_loc, const int* __restrict__ inst_lvl, const T* __restrict__ dL,
                                                  int inst, int pix, bool valid, int HWc, int W, T (&dmf)[8]) {
    __syncthreads();
    for (int i = threadIdx.x; i < CL_NP; i += CL_FB) prm[i] = prow[i];
    __syncthreads();
    if (valid) {
        T in[10];
        cl_inputs(mask_feats, inst_loc, inst_lvl, inst, pix, W, in);
        cl_mlp_bwd<T, -1>(prm, in, dL[(size_t)inst * HWc + pix], nullptr, dmf);
    }
}

}  // namespace
