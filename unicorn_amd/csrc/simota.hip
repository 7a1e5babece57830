// SimOTA label assignment of the head loss (unicorn/models/unicorn_head_mask.py:754-983: get_assignments, get_in_boxes_info,
// dynamic_k_matching), for a whole batch in four launches whose count does not depend on the number of boxes or images, fp32.
//
//   centre   xc = x_shift * stride + 0.5 * stride (same for y)
//   in_box   centre strictly inside box g;  in_ctr  centre strictly inside the square of half-side 2.5 stride around the box centre
//            clipped to the image;  fg[a] = any_g (in_box | in_ctr);  both[g][a] = in_box & in_ctr
//   p[a][c]  = sqrt(sigmoid(cls[a][c]) sigmoid(obj[a]));  cls_cost[g][a] = sum_c BCE(p[a][c], onehot(class_g)[c]), logs clamped at -100
//            = base[a] + corr[a][class_g],  base = sum_c -log(1 - p),  corr[c] = -log p + log(1 - p)         (no (G, A, C) tensor)
//   cost     = cls_cost + 3 (-log(iou + 1e-8)) + 1e5 (!both), in that order
//   k_g      = max(1, int(sum of the min(10, n_fg) largest iou[g][:]));  box g selects its k_g cheapest fg anchors;
//   an anchor selected by several boxes goes to argmin_g cost[g][a] over ALL boxes of the image.
//
//   so_anchor_kernel   thread = (image, anchor): loops the image's boxes for fg; base and the C corrections of an fg anchor; zeroes the
//                      selection count of the anchor and the image's num_fg
//   so_pair_kernel     thread = (image, box, anchor): cost and iou into the (B, M, A) workspace pair, +inf / -1 off fg
//   so_select_kernel   block = (image, box): up to 10 rounds of block arg-max over the iou row (summed in descending order), then k_g
//                      rounds of block arg-min over the cost row.  A round does not mark anything: it looks for the best element that comes
//                      strictly after the previous pick in the order (value, anchor index), so the rows stay read-only (they sit in L2).
//                      Every pick increments the anchor's int32 count and stores the box as tentative owner.
//   so_resolve_kernel  thread = (image, anchor): count > 1 -> arg-min over the cost column; writes fg_mask, matched_gt, matched_iou, and
//                      adds the wave's matches to num_fg.
//
// Ties (PyTorch leaves them open): the lower anchor index wins in both top-k passes, the lower box index wins in the arg-min.
// Only integer atomics (counts); no float atomic feeds a decision: two runs give the same bits.
// The whole file is compiled without FMA contraction: the strict `> 0` predicates, the IoU and `3 * iou_loss` round like the
// reference's separate tensor operations, so a centre on a box edge falls the same way.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int SO_TB = 256;       // per-anchor kernels
constexpr int SO_SB = 1024;      // so_select_kernel block (16 waves)
constexpr int SO_TOPK = 10;      // candidates of the dynamic k

struct SoLayout { size_t cost, iou, base, corr, count, owner, gfg, total; };      // byte offsets, each 256-aligned
SoLayout so_layout(int B, int A, int M, int C) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t pa = (size_t)B * A * 4, pr = (size_t)B * M * A * 4;
    SoLayout l;
    l.cost = 0;
    l.iou = al(l.cost + pr);
    l.base = al(l.iou + pr);
    l.corr = al(l.base + pa);
    l.count = al(l.corr + pa * C);
    l.owner = al(l.count + pa);
    l.gfg = al(l.owner + pa);
    l.total = al(l.gfg + pa);
    return l;
}
bool so_shape_ok(int B, int A, int M, int C) {
    return B >= 1 && B <= 65535 && A >= 1 && A < (1 << 24) && M >= 0 && M <= 1024 && C >= 1 && C <= 256;
}

__device__ __forceinline__ float so_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// get_in_boxes_info :883-938 for one (box, anchor): lab = (class, cx, cy, w, h)
__device__ __forceinline__ void so_geom(const float* __restrict__ lab, float xc, float yc, float s, float img_w, float img_h, bool& in_box,
                                        bool& in_ctr) {
    const float gx = lab[1], gy = lab[2], gw = lab[3], gh = lab[4];
    const float bl = xc - (gx - 0.5f * gw), br = (gx + 0.5f * gw) - xc, bt = yc - (gy - 0.5f * gh), bb = (gy + 0.5f * gh) - yc;
    in_box = fminf(fminf(bl, bt), fminf(br, bb)) > 0.f;
    const float qx = fminf(fmaxf(gx, 0.f), img_w), qy = fminf(fmaxf(gy, 0.f), img_h), rad = 2.5f * s;
    const float cl = xc - (qx - rad), cr = (qx + rad) - xc, ct = yc - (qy - rad), cb = (qy + rad) - yc;
    in_ctr = fminf(fminf(cl, ct), fminf(cr, cb)) > 0.f;
}

__device__ __forceinline__ int so_num_gt(const int* __restrict__ num_gt, int b, int M) { return min(max(num_gt[b], 0), M); }

__global__ void __launch_bounds__(SO_TB)
so_anchor_kernel(const float* __restrict__ outputs, int ld, const float* __restrict__ labels, const int* __restrict__ num_gt, int M,
                 const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ st, int A, int C, float img_h, float img_w,
                 float* __restrict__ base, float* __restrict__ corr, int* __restrict__ count, int* __restrict__ gfg, int* __restrict__ num_fg) {
    const int a = blockIdx.x * SO_TB + threadIdx.x, b = blockIdx.y;
    if (a == 0) num_fg[b] = 0;
    if (a >= A) return;
    const int G = so_num_gt(num_gt, b, M);
    const float s = st[a], xc = xs[a] * s + 0.5f * s, yc = ys[a] * s + 0.5f * s;
    int fg = 0;
    for (int g = 0; g < G && !fg; ++g) {
        bool ib, ic;
        so_geom(labels + ((size_t)b * M + g) * 5, xc, yc, s, img_w, img_h, ib, ic);
        fg = ib || ic;
    }
    const size_t i = (size_t)b * A + a;
    gfg[i] = fg;
    count[i] = 0;
    if (!fg) return;
    const float* o = outputs + i * ld;
    const float so = so_sigmoid(o[4]);
    float bs = 0.f;
    for (int c = 0; c < C; ++c) {
        const float p = sqrtf(so_sigmoid(o[5 + c]) * so);
        const float l1 = -fmaxf(logf(p), -100.f), l0 = -fmaxf(logf(1.f - p), -100.f);      // torch.binary_cross_entropy clamps each log at -100
        bs += l0;
        corr[i * C + c] = l1 - l0;
    }
    base[i] = bs;
}

__global__ void __launch_bounds__(SO_TB)
so_pair_kernel(const float* __restrict__ outputs, int ld, const float* __restrict__ labels, const int* __restrict__ num_gt, int M,
               const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ st, int A, int C, float img_h, float img_w,
               const float* __restrict__ base, const float* __restrict__ corr, const int* __restrict__ gfg, float* __restrict__ cost,
               float* __restrict__ iou) {
    const int a = blockIdx.x * SO_TB + threadIdx.x, g = blockIdx.y, b = blockIdx.z;
    if (a >= A || g >= so_num_gt(num_gt, b, M)) return;
    const size_t i = (size_t)b * A + a, j = ((size_t)b * M + g) * A + a;
    if (!gfg[i]) {
        cost[j] = INFINITY;
        iou[j] = -1.f;
        return;
    }
    const float* lab = labels + ((size_t)b * M + g) * 5;
    const float s = st[a], xc = xs[a] * s + 0.5f * s, yc = ys[a] * s + 0.5f * s;
    bool ib, ic;
    so_geom(lab, xc, yc, s, img_w, img_h, ib, ic);
    // bboxes_iou(gt, pred, xyxy=False), utils/boxes.py:164-177
    const float* o = outputs + i * ld;
    const float gx = lab[1], gy = lab[2], gw = lab[3], gh = lab[4], px = o[0], py = o[1], pw = o[2], ph = o[3];
    const float tlx = fmaxf(gx - gw / 2.f, px - pw / 2.f), tly = fmaxf(gy - gh / 2.f, py - ph / 2.f);
    const float brx = fminf(gx + gw / 2.f, px + pw / 2.f), bry = fminf(gy + gh / 2.f, py + ph / 2.f);
    const float en = (tlx < brx ? 1.f : 0.f) * (tly < bry ? 1.f : 0.f);
    const float area_i = (brx - tlx) * (bry - tly) * en;
    const float v = area_i / (gw * gh + pw * ph - area_i);
    const int cg = min(max((int)lab[0], 0), C - 1);
    const float cls = base[i] + corr[i * C + cg];
    cost[j] = cls + 3.0f * (-logf(v + 1e-8f)) + 100000.0f * ((ib && ic) ? 0.f : 1.f);
    iou[j] = v;
}

// (value, index) of the block's best candidate into every thread; MAX: larger value wins, else smaller; equal values: lower index.  idx < 0 = none.
template <bool MAX>
__device__ __forceinline__ void so_block_best(float& v, int& idx, float* sv, int* si) {
    auto better = [](float v2, int i2, float v1, int i1) {
        if (i2 < 0) return false;
        if (i1 < 0) return true;
        return (MAX ? v2 > v1 : v2 < v1) || (v2 == v1 && i2 < i1);
    };
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float v2 = __shfl_down(v, off, 64);
        const int i2 = __shfl_down(idx, off, 64);
        if (better(v2, i2, v, idx)) { v = v2; idx = i2; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sv[w] = v; si[w] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float bv = sv[0];
        int bi = si[0];
        for (int k = 1; k < SO_SB / 64; ++k)
            if (better(sv[k], si[k], bv, bi)) { bv = sv[k]; bi = si[k]; }
        sv[SO_SB / 64] = bv;
        si[SO_SB / 64] = bi;
    }
    __syncthreads();
    v = sv[SO_SB / 64];
    idx = si[SO_SB / 64];
    __syncthreads();      // the next round writes sv / si again
}

__global__ void __launch_bounds__(SO_SB)
so_select_kernel(const float* __restrict__ cost, const float* __restrict__ iou, const int* __restrict__ num_gt, int M, int A,
                 int* __restrict__ count, int* __restrict__ owner) {
    __shared__ float sv[SO_SB / 64 + 1];
    __shared__ int si[SO_SB / 64 + 1];
    const int g = blockIdx.x, b = blockIdx.y;
    if (g >= so_num_gt(num_gt, b, M)) return;
    const float* irow = iou + ((size_t)b * M + g) * A;
    const float* crow = cost + ((size_t)b * M + g) * A;
    // dynamic k: the min(10, n_fg) largest IoUs, summed largest first
    float pv = INFINITY, sum = 0.f;
    int pi = -1;
    for (int r = 0; r < SO_TOPK; ++r) {
        float bv = 0.f;
        int bi = -1;
        for (int a = threadIdx.x; a < A; a += SO_SB) {
            const float v = irow[a];
            if (v >= 0.f && (v < pv || (v == pv && a > pi)) && (bi < 0 || v > bv)) { bv = v; bi = a; }
        }
        so_block_best<true>(bv, bi, sv, si);
        if (bi < 0) break;
        sum += bv;
        pv = bv;
        pi = bi;
    }
    const int k = max(1, (int)sum);
    // the k cheapest fg anchors
    pv = -INFINITY;
    pi = -1;
    for (int r = 0; r < k; ++r) {
        float bv = 0.f;
        int bi = -1;
        for (int a = threadIdx.x; a < A; a += SO_SB) {
            const float v = crow[a];
            if (v < INFINITY && (v > pv || (v == pv && a > pi)) && (bi < 0 || v < bv)) { bv = v; bi = a; }
        }
        so_block_best<false>(bv, bi, sv, si);
        if (bi < 0) break;
        if (threadIdx.x == 0) {
            atomicAdd(&count[(size_t)b * A + bi], 1);
            owner[(size_t)b * A + bi] = g;      // used only where the count stays 1: one writer
        }
        pv = bv;
        pi = bi;
    }
}

__global__ void __launch_bounds__(SO_TB)
so_resolve_kernel(const float* __restrict__ cost, const float* __restrict__ iou, const int* __restrict__ num_gt, int M, int A,
                  const int* __restrict__ count, const int* __restrict__ owner, unsigned char* __restrict__ fg_mask,
                  int* __restrict__ matched_gt, float* __restrict__ matched_iou, int* __restrict__ num_fg) {
    const int a = blockIdx.x * SO_TB + threadIdx.x, b = blockIdx.y;
    int m = -1;
    if (a < A) {
        const size_t i = (size_t)b * A + a;
        const int cnt = count[i];
        if (cnt >= 1) m = owner[i];
        // contested: the cheapest box of ALL boxes, also one that did not select the anchor (:969-971).  The owner read above, which
        // several blocks wrote in no fixed order, never survives here: so_select_kernel picks only costs `< INFINITY` (false for NaN
        // and +inf), so a selected anchor's column holds a cost below `best` and the loop always replaces m, NaN inputs included.
        if (cnt > 1) {
            const int G = so_num_gt(num_gt, b, M);
            float best = INFINITY;
            for (int g = 0; g < G; ++g) {
                const float c = cost[((size_t)b * M + g) * A + a];
                if (c < best) { best = c; m = g; }
            }
        }
        fg_mask[i] = m >= 0;
        matched_gt[i] = m;
        matched_iou[i] = m >= 0 ? iou[((size_t)b * M + m) * A + a] : 0.f;
    }
    const unsigned long long hit = __ballot(m >= 0);
    if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&num_fg[b], __popcll(hit));
}

}  // namespace

size_t simota_workspace_bytes(int B, int A, int M, int C) {
    if (!so_shape_ok(B, A, M, C)) return 0;
    return so_layout(B, A, M, C).total;
}

int launch_simota_assign(const float* outputs, int ld, const float* labels, const int* num_gt, int M, const float* xs, const float* ys,
                         const float* st, int B, int A, int C, int img_h, int img_w, unsigned char* fg_mask, int* matched_gt,
                         float* matched_iou, int* num_fg, void* ws, size_t ws_bytes, hipStream_t s) {
    UNI_REQUIRE(so_shape_ok(B, A, M, C), "simota: shape B=%d A=%d M=%d C=%d outside 1 <= B <= 65535, 1 <= A < 2^24, 0 <= M <= 1024, 1 <= C <= 256",
                B, A, M, C);
    UNI_REQUIRE(ld >= 5 + C, "simota: ld_out %d < 5 + C = %d", ld, 5 + C);
    const SoLayout l = so_layout(B, A, M, C);
    UNI_REQUIRE(ws_bytes >= l.total, "simota: workspace %zu < %zu", ws_bytes, l.total);
    UNI_REQUIRE(((uintptr_t)ws & 3) == 0, "simota: workspace must be 4-byte aligned");
    char* w = reinterpret_cast<char*>(ws);
    float *cost = (float*)(w + l.cost), *iou = (float*)(w + l.iou), *base = (float*)(w + l.base), *corr = (float*)(w + l.corr);
    int *count = (int*)(w + l.count), *owner = (int*)(w + l.owner), *gfg = (int*)(w + l.gfg);
    const int ax = (A + SO_TB - 1) / SO_TB;
    so_anchor_kernel<<<dim3(ax, B), SO_TB, 0, s>>>(outputs, ld, labels, num_gt, M, xs, ys, st, A, C, (float)img_h, (float)img_w, base, corr,
                                                  count, gfg, num_fg);
    if (M > 0) {
        so_pair_kernel<<<dim3(ax, M, B), SO_TB, 0, s>>>(outputs, ld, labels, num_gt, M, xs, ys, st, A, C, (float)img_h, (float)img_w, base, corr,
                                                       gfg, cost, iou);
        so_select_kernel<<<dim3(M, B), SO_SB, 0, s>>>(cost, iou, num_gt, M, A, count, owner);
    }
    so_resolve_kernel<<<dim3(ax, B), SO_TB, 0, s>>>(cost, iou, num_gt, M, A, count, owner, fg_mask, matched_gt, matched_iou, num_fg);
    return 0;
}
