// Device helpers of the CondInst mask loss shared by condinst_loss.hip (one image, compacted instances) and head_mask_loss.hip (the whole
// batch from the device-side assignment): the 10-8-8-1 MLP of an instance at a coarse pixel and its backward, the tap softmax of the convex
// upsample, the fine-pixel thread mapping.  Moved here unchanged from condinst_loss.hip: both operators evaluate the same arithmetic.
#pragma once
#include "kernels.h"

namespace {

constexpr int CL_NP = 169;     // 80 | 64 | 8 | 8 | 8 | 1 (parse_dynamic_params)

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

}  // namespace
