// The CondInst mask loss of get_losses (unicorn_head_mask.py:568-569, :675-694, :731-732 with dynamic_mask_head.py:247-278) for a whole BATCH,
// fed by the device-side SimOTA assignment, forward and a recomputing backward, without a host read-back:
//
//   F_b = {a : fg_mask[b][a]}   dice_a = condinst_loss.hip's per-instance loss with params[b][a], location stride_a (shift_a + 0.5),
//   level fpn_levels[b][a], ground truth masks[b][matched_gt[b][a]] (read IN PLACE), the maps mask_feats[b] / up_masks[b]
//   loss_mask[b] = mean_{a in F_b} dice_a (0 if F_b is empty)   loss = sum_b loss_mask[b] / max(#{b : F_b not empty}, 1)
//
// The host never learns how many instances there are.  hm_table_kernel builds the instance table (slot -> image, parameter row, mask row,
// location, level; per-image counts and offsets; the number of valid images) by a scan in ascending (image, anchor) order; every other grid is
// sized from the geometry or from `capacity` (the number of slots the workspace holds) and its blocks take their instance range from the
// table: slot-strided loops, or S sub-ranges of an image's instances whose partials are added in a fixed order.  5 launches forward and at
// most 22 backward whatever the data, B, A, M and capacity.  One writer per output element, fixed summation orders, no float atomics.
//
// The per-instance arithmetic is NOT written here: the kernels that have a per-image twin in condinst_loss.hip call the same bodies of
// condinst_dev.h (named on the right) and only choose the slots a block handles and the rows a slot reads (t.row / t.gt / t.img / t.lvl).
//
//   forward   hm_table_kernel   the table; more instances than capacity: the overflow flag, counts forced to 0 (nothing is indexed by a slot)
//             hm_mlp_kernel     block (pixel tile, slot stride)                             cl_inputs, cl_mlp
//             hm_dice_kernel    block (fine-pixel tile, sub-range, image)                   cl_dice_accum, cl_dice_combine per group of CL_IC slots
//             hm_dice_final     block per slot (strided)                                    cl_dice_partial, cl_dice_finish
//             hm_reduce_kernel  out[0] = loss, out[1 + b] = loss_mask[b]; NaN everywhere on overflow
//   backward  hm_table_kernel, hm_mlp_kernel again (the workspace is scratch between calls)
//             HM_NC = 8 passes over the instance range (pass c = slots [c per, (c + 1) per), per = ceil(n / 8) from the table), in stream order:
//               hm_du_kernel      block (fine-pixel tile, image) loops the instances of its image in the pass: d up_masks accumulates in the
//                                 owning thread's registers (pass c adds to what pass c - 1 left)    cl_du_instance, cl_stage_taps -> A[slot - c0]
//               hm_gather_kernel  dL[slot][q]                                                cl_gather_pixel
//             hm_dparams_kernel / hm_dparams_final   per slot (cl_dparams_half) -> partials -> the DENSE grad_params [B][A][169]
//                               (background rows and everything on overflow: exact zeros) through slot_of[b][a]
//             hm_dfeat_kernel / hm_dfeat_final       thread = coarse pixel, S sub-ranges of the image's instances (cl_dfeat_instance) -> partials
//                               -> grad_mask_feats
//
// Workspace, in elements of T after the integer table: capacity x H8 W8 x (1 logits + 1 dL) + ceil(capacity / 8) x H8 W8 x 9 (A) + capacity x (3 nblk_d + 169 nblk_p + 3)
// + B x S x H8 W8 x 8  (hm_layout).
#include "condinst_dev.h"

namespace {

constexpr int HM_S = 8;         // sub-ranges an image's instances are split into (dice forward, d mask_feats)
constexpr int HM_GS = 256;      // most blocks of a slot-strided grid dimension
constexpr int HM_TB = 1024;     // hm_table_kernel block
constexpr int HM_CI = 64;       // hm_table_kernel: images counted per round
constexpr int HM_NC = 8;        // backward: passes the instance range is cut into (the tap sums A are staged per pass)
constexpr int HM_HDR = 4;       // table header: instances in use (0 on overflow), valid images, overflow flag, instances counted

struct HMTable {                // device pointers into the integer part of the workspace
    int *hdr, *cnt, *off, *row, *img, *gt, *lvl, *slot_of;
};

// number of non-zero bytes of a word
__device__ __forceinline__ int hm_nz4(unsigned w) {
    return ((w & 0xffu) != 0) + ((w & 0xff00u) != 0) + ((w & 0xff0000u) != 0) + ((w & 0xff000000u) != 0);
}

// block = image.  Its offset = the number of foreground anchors of the images before it (counted again by every block: B^2 A / 2 bytes, no
// second launch; all threads count an image together, HM_CI images per round through integer LDS counters); its own anchors by a block
// scan over contiguous per-thread segments, so slots ascend with (image, anchor).  fg_mask is read in 4-byte words when A and the pointer
// allow it.
template <typename T>
__global__ __launch_bounds__(HM_TB) void hm_table_kernel(const unsigned char* __restrict__ fg, const int* __restrict__ mg,
                                                         const int* __restrict__ lvl, const T* __restrict__ xs, const T* __restrict__ ys,
                                                         const T* __restrict__ st, int B, int A, int M, int capacity, HMTable t,
                                                         T* __restrict__ loc) {
    __shared__ int s_cnt[HM_CI];
    __shared__ int s_acc[3];
    __shared__ int wtot[HM_TB / 64];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool words = (A & 3) == 0 && ((uintptr_t)fg & 3) == 0;
    int before = 0, total = 0, valid = 0;                    // thread 0's
    for (int b0 = 0; b0 < B; b0 += HM_CI) {
        const int nb = min(HM_CI, B - b0);
        if (tid < HM_CI) s_cnt[tid] = 0;
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            const unsigned char* row = fg + (size_t)(b0 + k) * A;
            int c = 0;
            if (words) {
                const unsigned* rw = reinterpret_cast<const unsigned*>(row);
                for (int i = tid; i < A / 4; i += HM_TB) c += hm_nz4(rw[i]);
            } else {
                for (int a = tid; a < A; a += HM_TB) c += row[a] != 0;
            }
            c = cl_wave_sum(c);
            if (lane == 0 && c) atomicAdd(&s_cnt[k], c);     // integer: the sum does not depend on the order
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < nb; ++k) {
                const int c = s_cnt[k];
                total += c;
                valid += c > 0;
                if (b0 + k < b) before += c;
            }
        }
        __syncthreads();
    }
    if (tid == 0) { s_acc[0] = before; s_acc[1] = total; s_acc[2] = valid; }
    __syncthreads();
    before = s_acc[0]; total = s_acc[1]; valid = s_acc[2];
    const bool over = total > capacity;
    // own image: thread = segment of `seg` (a multiple of 4) consecutive anchors
    const int seg = ((A + HM_TB - 1) / HM_TB + 3) / 4 * 4, a0 = min(tid * seg, A), a1 = min(a0 + seg, A);
    const unsigned char* row = fg + (size_t)b * A;
    auto load4 = [&](int a) -> unsigned {                    // byte k: anchor a + k is foreground (0 beyond a1)
        if (words) return *reinterpret_cast<const unsigned*>(row + a);
        unsigned w = 0;
        for (int k = 0; k < 4; ++k)
            if (a + k < a1 && row[a + k] != 0) w |= 1u << (8 * k);
        return w;
    };
    int c = 0;
    for (int a = a0; a < a1; a += 4) c += hm_nz4(load4(a));
    int incl = c;                                            // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int base = 0, own = 0;
    for (int w = 0; w < HM_TB / 64; ++w) {
        if (w < wave) base += wtot[w];
        own += wtot[w];
    }
    int slot = before + base + incl - c;
    for (int a4 = a0; a4 < a1; a4 += 4) {
        const unsigned w = load4(a4);
        for (int k = 0; k < 4 && a4 + k < a1; ++k) {
            const int a = a4 + k;
            const size_t e = (size_t)b * A + a;
            const bool f = ((w >> (8 * k)) & 0xffu) != 0;
            t.slot_of[e] = (f && !over) ? slot : -1;
            if (f && !over) {                                // !over: total <= capacity, so slot < capacity
                t.row[slot] = (int)e;
                t.img[slot] = b;
                t.gt[slot] = b * M + min(max(mg[e], 0), M - 1);
                t.lvl[slot] = lvl[e];
                loc[slot * 2] = st[a] * (xs[a] + (T)0.5);
                loc[slot * 2 + 1] = st[a] * (ys[a] + (T)0.5);
            }
            slot += f;
        }
    }
    if (tid == 0) {
        t.cnt[b] = over ? 0 : own;
        t.off[b] = before;
        if (b == 0) { t.hdr[0] = over ? 0 : total; t.hdr[1] = valid; t.hdr[2] = over ? 1 : 0; t.hdr[3] = total; }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void hm_mlp_kernel(const T* __restrict__ mask_feats, const T* __restrict__ params, int ldp, HMTable t,
                                                     const T* __restrict__ loc, int HWc, int W, T* __restrict__ logits) {
    __shared__ T prm[CL_NP];
    const int n = t.hdr[0], pix = blockIdx.x * blockDim.x + threadIdx.x;
    for (int slot = blockIdx.y; slot < n; slot += gridDim.y) {
        __syncthreads();
        for (int i = threadIdx.x; i < CL_NP; i += blockDim.x) prm[i] = params[(size_t)t.row[slot] * ldp + i];
        __syncthreads();
        if (pix < HWc) {
            T in[10], h0[8], h1[8];
            cl_inputs(mask_feats + (size_t)t.img[slot] * HWc * 8, loc, t.lvl, slot, pix, W, in);
            logits[(size_t)slot * HWc + pix] = cl_mlp(prm, in, h0, h1);
        }
    }
}

// the slots [k0, k1) of sub-range z (of HM_S) of image b
__device__ __forceinline__ void hm_range(const HMTable& t, int b, int z, int& k0, int& k1) {
    const int n = t.cnt[b], per = (n + HM_S - 1) / HM_S;
    k0 = t.off[b] + min(z * per, n);
    k1 = t.off[b] + min(z * per + per, n);
}

template <typename T>
__global__ __launch_bounds__(256) void hm_dice_kernel(const T* __restrict__ up_masks, const T* __restrict__ logits, const T* __restrict__ masks,
                                                      HMTable t, T* __restrict__ part, int H, int W, int r, int PX, int nblk) {
    __shared__ T red[4][3 * CL_IC];
    int k0, k1;
    hm_range(t, blockIdx.z, blockIdx.y, k0, k1);
    if (k0 >= k1) return;
    const int rr = r * r, HWc = H * W;
    int pix, i, j, xl;
    bool valid;
    cl_map(r, PX, HWc, pix, i, j, xl, valid);
    T wt[9];
    int off[9];
    cl_taps(up_masks + (size_t)blockIdx.z * HWc * 9 * rr, pix, i * r + j, rr, H, W, valid, wt, off);
    const int y = pix / W, x = pix - y * W;
    const size_t fine = (size_t)(r * y + i) * (r * W) + r * x + j, fsz = (size_t)HWc * rr;
    const auto g_at = [=](int slot) { return masks[(size_t)t.gt[slot] * fsz + fine]; };
    for (int i0 = k0; i0 < k1; i0 += CL_IC) {
        const int cnt = min(k1 - i0, CL_IC);
        for (int k = 0; k < cnt; ++k) cl_dice_accum(wt, off, valid, logits, HWc, g_at, i0 + k, red, k);
        cl_dice_combine(i0, cnt, red, part, nblk);
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void hm_dice_final(const T* __restrict__ part, int nblk, HMTable t, T* __restrict__ sums, T* __restrict__ dice) {
    __shared__ T red[3][256];
    const int n = t.hdr[0];
    for (int slot = blockIdx.x; slot < n; slot += gridDim.x) {
        T a[3];
        cl_dice_partial(part, slot, nblk, a);
        __syncthreads();
        cl_dice_finish(a, red, slot, sums, dice);
    }
}

// out[1 + b] = mean of the image's dice losses in slot order (0 without instances), out[0] = their sum in image order / max(valid, 1)
template <typename T>
__global__ __launch_bounds__(256) void hm_reduce_kernel(const T* __restrict__ dice, HMTable t, int B, T* __restrict__ out) {
    const T nan = (T)__builtin_nan("");
    const bool over = t.hdr[2] != 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int n = t.cnt[b], o = t.off[b];
        T s = (T)0;
        for (int k = 0; k < n; ++k) s += dice[o + k];
        out[1 + b] = over ? nan : (n > 0 ? s / (T)n : (T)0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        T s = (T)0;
        for (int b = 0; b < B; ++b) s += out[1 + b];
        out[0] = over ? nan : s / (T)max(t.hdr[1], 1);
    }
}

// the slots [c0, c1) of pass `pass` (of HM_NC) over all instances in use
__device__ __forceinline__ void hm_pass(const HMTable& t, int pass, int& c0, int& c1) {
    const int n = t.hdr[0], per = (n + HM_NC - 1) / HM_NC;
    c0 = min(pass * per, n);
    c1 = min(c0 + per, n);
}

// cl_du_kernel over the instances of image blockIdx.y that fall into this pass: the thread owns its d up_masks elements (pass c adds to
// what pass c - 1 left; pass 0 writes them whatever the counts)
template <typename T>
__global__ __launch_bounds__(256) void hm_du_kernel(const T* __restrict__ up_masks, const T* __restrict__ logits, const T* __restrict__ masks,
                                                    const T* __restrict__ sums, const T* __restrict__ gout, HMTable t, T* __restrict__ A,
                                                    T* __restrict__ grad_um, int H, int W, int r, int PX, int want_dl, int pass) {
    __shared__ T cs[9][256];
    const int rr = r * r, HWc = H * W, b = blockIdx.y;
    int c0, c1;
    hm_pass(t, pass, c0, c1);
    const int n = t.cnt[b], k0 = max(t.off[b], c0), k1 = min(t.off[b] + n, c1);
    if (pass > 0 && k0 >= k1) return;
    int pix, i, j, xl;
    bool valid;
    cl_map(r, PX, HWc, pix, i, j, xl, valid);
    T wt[9], acc[9];
    int off[9];
    cl_taps(up_masks + (size_t)b * HWc * 9 * rr, pix, i * r + j, rr, H, W, valid, wt, off);
    const int y = pix / W, x = pix - y * W;
    const size_t fine = (size_t)(r * y + i) * (r * W) + r * x + j, fsz = (size_t)HWc * rr;
    T* gum = (grad_um && valid) ? grad_um + ((size_t)b * HWc + pix) * 9 * rr + i * r + j : nullptr;
#pragma unroll
    for (int tt = 0; tt < 9; ++tt) acc[tt] = (gum && pass > 0) ? gum[tt * rr] : (T)0;
    const T go = n > 0 ? gout[0] / ((T)n * (T)max(t.hdr[1], 1)) : (T)0;      // d loss / d dice of every instance of this image
    const auto g_at = [=](int slot) { return masks[(size_t)t.gt[slot] * fsz + fine]; };
    for (int slot = k0; slot < k1; ++slot) {
        T c[9];
        cl_du_instance(sums, go, wt, off, valid, logits, HWc, g_at, slot, c, acc);
        if (want_dl) cl_stage_taps(c, cs, A, slot - c0, r, PX, HWc);
    }
    if (gum) {
#pragma unroll
        for (int tt = 0; tt < 9; ++tt) gum[tt * rr] = acc[tt];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void hm_gather_kernel(const T* __restrict__ A, HMTable t, T* __restrict__ dL, int H, int W, int pass) {
    const int HWc = H * W, q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= HWc) return;
    int c0, c1;
    hm_pass(t, pass, c0, c1);
    const int y = q / W, x = q - y * W;
    for (int slot = c0 + blockIdx.y; slot < c1; slot += gridDim.y)
        dL[(size_t)slot * HWc + q] = cl_gather_pixel(A, slot - c0, y, x, H, W);
}

template <typename T>
__global__ __launch_bounds__(256) void hm_dparams_kernel(const T* __restrict__ mask_feats, const T* __restrict__ params, int ldp, HMTable t,
                                                         const T* __restrict__ loc, const T* __restrict__ dL, int HWc, int W,
                                                         T* __restrict__ part, int nblk) {
    __shared__ T prm[CL_NP];
    __shared__ T red[4][CL_NP];
    const int n = t.hdr[0];
    for (int slot = blockIdx.y; slot < n; slot += gridDim.y) {
        __syncthreads();
        for (int i = threadIdx.x; i < CL_NP; i += 256) prm[i] = params[(size_t)t.row[slot] * ldp + i];
        __syncthreads();
        const T* mf = mask_feats + (size_t)t.img[slot] * HWc * 8;
        if (blockIdx.z == 0) cl_dparams_half<T, 0>(prm, red, mf, loc, t.lvl, dL, slot, HWc, W, part, nblk);
        else cl_dparams_half<T, 1>(prm, red, mf, loc, t.lvl, dL, slot, HWc, W, part, nblk);
    }
}

// thread = one element of the dense [B][A][169] gradient: the partials of its slot in order, or an exact zero for a background row
template <typename T>
__global__ __launch_bounds__(256) void hm_dparams_final(const T* __restrict__ part, int nblk, HMTable t, size_t total, T* __restrict__ grad_params,
                                                        int ldg) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t row = e / CL_NP;
    const int col = (int)(e - row * CL_NP), slot = t.slot_of[row];
    T s = (T)0;
    if (slot >= 0)
        for (int b = 0; b < nblk; ++b) s += part[((size_t)slot * nblk + b) * CL_NP + col];
    grad_params[row * ldg + col] = s;
}

template <typename T>
__global__ __launch_bounds__(CL_FB) void hm_dfeat_kernel(const T* __restrict__ mask_feats, const T* __restrict__ params, int ldp, HMTable t,
                                                          const T* __restrict__ loc, const T* __restrict__ dL, int HWc, int W,
                                                          T* __restrict__ part) {
    __shared__ T prm[CL_NP];
    const int pix = blockIdx.x * CL_FB + threadIdx.x, b = blockIdx.z;
    const bool valid = pix < HWc;
    int k0, k1;
    hm_range(t, b, blockIdx.y, k0, k1);
    const T* mf = mask_feats + (size_t)b * HWc * 8;
    T dmf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dmf[c] = (T)0;
    for (int slot = k0; slot < k1; ++slot)
        cl_dfeat_instance(prm, params + (size_t)t.row[slot] * ldp, mf, loc, t.lvl, dL, slot, pix, valid, HWc, W, dmf);
    if (valid) {
#pragma unroll
        for (int c = 0; c < 8; ++c) part[(((size_t)b * HM_S + blockIdx.y) * HWc + pix) * 8 + c] = dmf[c];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void hm_dfeat_final(const T* __restrict__ part, size_t per_img, size_t total, T* __restrict__ grad_mf) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t b = e / per_img, q = e - b * per_img;
    T s = (T)0;
    for (int z = 0; z < HM_S; ++z) s += part[(b * HM_S + z) * per_img + q];
    grad_mf[e] = s;
}

// workspace layout: the integer table first (bytes), then the floating part in elements of T from `fbase` bytes on
struct HMLayout {
    size_t hdr, cnt, off, row, img, gt, lvl, slot_of, fbase;         // int offsets (in ints); fbase in bytes, a multiple of 8
    size_t loc, logits, dL, dice, dpart, A, pp, pf, ftotal;          // T offsets
    int PX, nblk_d, nblk_p;
};
HMLayout hm_layout(int B, int A, int H, int W, int r, int cap) {
    HMLayout l;
    const size_t hw = (size_t)H * W, c = (size_t)cap;
    l.PX = 256 / (r * r);
    l.nblk_d = cdiv(H * W, l.PX);
    l.nblk_p = cdiv(H * W, 256 * CL_PPT);
    size_t o = 0;
    l.hdr = o;     o += HM_HDR;
    l.cnt = o;     o += B;
    l.off = o;     o += B;
    l.row = o;     o += c;
    l.img = o;     o += c;
    l.gt = o;      o += c;
    l.lvl = o;     o += c;
    l.slot_of = o; o += (size_t)B * A;
    l.fbase = (o * sizeof(int) + 7) / 8 * 8;
    o = 0;
    l.loc = o;     o += c * 2;
    l.logits = o;  o += c * hw;
    l.dL = o;      o += c * hw;
    l.dice = o;    o += c;
    l.dpart = o;   o += c * l.nblk_d * 3;
    l.A = o;       o += (size_t)cdiv(cap, HM_NC) * hw * 9;
    l.pp = o;      o += c * l.nblk_p * CL_NP;
    l.pf = o;      o += (size_t)B * HM_S * hw * 8;
    l.ftotal = o;
    return l;
}

bool hm_shape_ok(int B, int A, int H, int W, int r, int cap) {
    return B >= 1 && B <= 65535 && A >= 1 && (size_t)B * A <= (size_t)1 << 28 && H >= 1 && W >= 1 && r >= 1 && r <= 16 &&
           (size_t)H * W * r * r < (size_t)1 << 30 && cap >= 1 && cap <= 1 << 24 && (size_t)B * H * W * 9 * r * r < (size_t)1 << 40;
}

int hm_check(const char* what, int B, int A, int M, int H, int W, int r, int cap, int ldp, const void* ws, size_t ws_bytes, size_t esize) {
    UNI_REQUIRE(hm_shape_ok(B, A, H, W, r, cap),
                "%s: B=%d A=%d H8=%d W8=%d up_rate=%d capacity=%d outside 1 <= B <= 65535, A >= 1, B A <= 2^28, up_rate 1..16, H8 W8 r r < 2^30, "
                "1 <= capacity <= 2^24", what, B, A, H, W, r, cap);
    UNI_REQUIRE(M >= 1 && (size_t)B * M < (size_t)1 << 31, "%s: M=%d ground-truth rows per image (need >= 1, B M < 2^31)", what, M);
    UNI_REQUIRE(ldp >= CL_NP, "%s: ldp %d < 169", what, ldp);
    const HMLayout l = hm_layout(B, A, H, W, r, cap);
    const size_t need = l.fbase + l.ftotal * esize;
    UNI_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= need, "%s: workspace %zu < %zu bytes or misaligned", what, ws_bytes, need);
    return 0;
}

HMTable hm_table(const HMLayout& l, void* ws) {
    int* p = reinterpret_cast<int*>(ws);
    return HMTable{p + l.hdr, p + l.cnt, p + l.off, p + l.row, p + l.img, p + l.gt, p + l.lvl, p + l.slot_of};
}

// the two launches both directions start with: the table and the coarse logits
template <typename T>
void hm_prepare(const HMIn<T>& a, const HMLayout& l, const HMTable& t, T* f, hipStream_t s) {
    hipLaunchKernelGGL(hm_table_kernel<T>, dim3(a.B), dim3(HM_TB), 0, s, a.fg, a.mg, a.lvl, a.xs, a.ys, a.st, a.B, a.A, a.M, a.cap, t, f + l.loc);
    const int hw = a.H * a.W, gs = a.cap < HM_GS ? a.cap : HM_GS;
    hipLaunchKernelGGL(hm_mlp_kernel<T>, dim3(cdiv(hw, 256), gs), dim3(256), 0, s, a.mf, a.params, a.ldp, t, f + l.loc, hw, a.W, f + l.logits);
}

}  // namespace

size_t head_mask_loss_workspace_bytes(int B, int A, int H, int W, int r, int cap) {
    if (!hm_shape_ok(B, A, H, W, r, cap)) return 0;
    const HMLayout l = hm_layout(B, A, H, W, r, cap);
    return l.fbase + l.ftotal * sizeof(float);
}

template <typename T>
int launch_head_mask_loss_fwd(const HMIn<T>& a, T* out, T* sums, void* workspace, size_t ws_bytes, hipStream_t s) {
    if (int rc = hm_check("head_mask_loss_fwd", a.B, a.A, a.M, a.H, a.W, a.r, a.cap, a.ldp, workspace, ws_bytes, sizeof(T))) return rc;
    const HMLayout l = hm_layout(a.B, a.A, a.H, a.W, a.r, a.cap);
    const HMTable t = hm_table(l, workspace);
    T* f = reinterpret_cast<T*>(reinterpret_cast<char*>(workspace) + l.fbase);
    hm_prepare(a, l, t, f, s);
    hipLaunchKernelGGL(hm_dice_kernel<T>, dim3(l.nblk_d, HM_S, a.B), dim3(256), 0, s, a.um, f + l.logits, a.masks, t, f + l.dpart, a.H, a.W, a.r,
                       l.PX, l.nblk_d);
    hipLaunchKernelGGL(hm_dice_final<T>, dim3(a.cap < 1024 ? a.cap : 1024), dim3(256), 0, s, f + l.dpart, l.nblk_d, t, sums, f + l.dice);
    hipLaunchKernelGGL(hm_reduce_kernel<T>, dim3(1), dim3(256), 0, s, f + l.dice, t, a.B, out);
    return 0;
}

template <typename T>
int launch_head_mask_loss_bwd(const HMIn<T>& a, const T* sums, const T* gout, T* gmf, T* gum, T* gpar, int ldg, void* workspace,
                              size_t ws_bytes, hipStream_t s) {
    if (int rc = hm_check("head_mask_loss_bwd", a.B, a.A, a.M, a.H, a.W, a.r, a.cap, a.ldp, workspace, ws_bytes, sizeof(T))) return rc;
    UNI_REQUIRE(!gpar || ldg >= CL_NP, "head_mask_loss_bwd: ld_grad %d < 169", ldg);
    if (!gmf && !gum && !gpar) return 0;
    const HMLayout l = hm_layout(a.B, a.A, a.H, a.W, a.r, a.cap);
    const HMTable t = hm_table(l, workspace);
    T* f = reinterpret_cast<T*>(reinterpret_cast<char*>(workspace) + l.fbase);
    const int hw = a.H * a.W, want_dl = (gmf || gpar) ? 1 : 0, gs = a.cap < HM_GS ? a.cap : HM_GS;
    hm_prepare(a, l, t, f, s);
    const int gp = cdiv(a.cap, HM_NC) < HM_GS ? cdiv(a.cap, HM_NC) : HM_GS;
    for (int pass = 0; pass < HM_NC; ++pass) {               // a fixed number of passes: A holds the tap sums of one pass
        hipLaunchKernelGGL(hm_du_kernel<T>, dim3(l.nblk_d, a.B), dim3(256), 0, s, a.um, f + l.logits, a.masks, sums, gout, t, f + l.A, gum, a.H,
                           a.W, a.r, l.PX, want_dl, pass);
        if (want_dl) hipLaunchKernelGGL(hm_gather_kernel<T>, dim3(cdiv(hw, 256), gp), dim3(256), 0, s, f + l.A, t, f + l.dL, a.H, a.W, pass);
    }
    if (gpar) {
        hipLaunchKernelGGL(hm_dparams_kernel<T>, dim3(l.nblk_p, gs, 2), dim3(256), 0, s, a.mf, a.params, a.ldp, t, f + l.loc, f + l.dL, hw, a.W,
                           f + l.pp, l.nblk_p);
        const size_t total = (size_t)a.B * a.A * CL_NP;
        hipLaunchKernelGGL(hm_dparams_final<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f + l.pp, l.nblk_p, t, total, gpar, ldg);
    }
    if (gmf) {
        hipLaunchKernelGGL(hm_dfeat_kernel<T>, dim3(cdiv(hw, CL_FB), HM_S, a.B), dim3(CL_FB), 0, s, a.mf, a.params, a.ldp, t, f + l.loc, f + l.dL,
                           hw, a.W, f + l.pf);
        const size_t per = (size_t)hw * 8, total = per * a.B;
        hipLaunchKernelGGL(hm_dfeat_final<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f + l.pf, per, total, gmf);
    }
    return 0;
}

template int launch_head_mask_loss_fwd<float>(const HMIn<float>&, float*, float*, void*, size_t, hipStream_t);
template int launch_head_mask_loss_fwd<double>(const HMIn<double>&, double*, double*, void*, size_t, hipStream_t);
template int launch_head_mask_loss_bwd<float>(const HMIn<float>&, const float*, const float*, float*, float*, float*, int, void*, size_t, hipStream_t);
template int launch_head_mask_loss_bwd<double>(const HMIn<double>&, const double*, const double*, double*, double*, double*, int, void*, size_t,
                                               hipStream_t);
