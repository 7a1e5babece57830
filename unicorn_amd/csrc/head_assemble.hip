// Head-output assembly (unicorn/models/unicorn_head_mask.py:339-366 of forward, get_output_and_grid :476-500, the level cats :396-401 and
// :554-558; identically unicorn_head.py, yolo_head_det.py, yolo_head_det_mask.py; n_anchors == 1): the prediction maps of up to four levels ->
// the tensors the loss operators read, forward and backward, fp32 (maps fp32 / fp16 / bf16) and fp64, ONE launch each way.
//
//   outputs [b][a][0 .. 4 + C] = (reg0 + x) * s, (reg1 + y) * s, exp(reg2) * s, exp(reg3) * s, obj, cls;   origin [b][a][0 .. 3] = reg
//   xs / ys / st [a] = x, y, s;   params [b][a][p] = ctrl[b][p][y][x];   levels [b][a] = l;        a = off_l + y w_l + x
//
// Every part is a transpose of (channels, h w) planes into rows of channels (a row copy for a channels-last map).  A block of 256 threads
// takes HA_TILE = 64 anchors of one level of one image and moves them through an LDS tile [64 channels][64 + 1 anchors] in passes of 64 result
// columns: the plane reads run along the anchors (lane = anchor, 256 B per wave-instruction and channel), the row writes along the columns
// (consecutive lanes on consecutive addresses, whole rows where the pitch is the row).  The pad of one element makes both sides
// conflict-free: the loads store [c][lane], the row writes read [c0 + lane % n][j], addresses 65 c + j, so the 32 lanes of a bank group
// differ in c and land in 32 different banks.  A channels-last map is read with the channel running fastest and stored [lane % n][j], the
// same address pattern.  The backward is the mirror image: rows in, planes out, exp(reg) recomputed at the address the gradient goes to.
// The level table -- pointers, sizes, strides, layouts -- travels by value in the kernel arguments (400 bytes).  No workspace, no atomics.
//
// The file is compiled without FMA contraction: the two leading columns are an add and then a multiply, as the eager lines are.
#include "kernels.h"
#include "train_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int HA_TB = 256;
constexpr int HA_PADDED = HA_TILE + 1;
enum { HA_REG = 0, HA_OBJ = 1, HA_CLS = 2, HA_CTRL = 3 };

struct HaLevel {
    const void* map[4];                         // reg, obj, cls, ctrl
    void* grad[4];                              // backward: their gradients (NULL: not computed)
    double stride;
    int h, w;
    int off, tile0;                             // first anchor / first tile of the level
    int nchw;                                   // bit r: map r is NCHW-contiguous
};
struct HaGeom {
    HaLevel lv[HA_MAX_L];
    int L, A, C, P;
};

__device__ __forceinline__ float ha_exp(float x) { return expf(x); }
__device__ __forceinline__ double ha_exp(double x) { return exp(x); }

// element offset of (b, c, anchor a) in a (B, nc, h, w) map with hw = h w
__device__ __forceinline__ size_t ha_at(bool nchw, int b, int nc, int hw, int c, int a) {
    return nchw ? ((size_t)b * nc + c) * hw + a : ((size_t)b * hw + a) * nc + c;
}
// element e of a segment of cnt channels x HA_TILE anchors in the order the map is laid out: -> channel cc, anchor j of the tile
__device__ __forceinline__ void ha_order(bool nchw, int e, int cnt, int& cc, int& j) {
    if (nchw) {
        cc = e >> 6;
        j = e & (HA_TILE - 1);
    } else {
        j = e / cnt;
        cc = e - j * cnt;
    }
}
// element e of `n` result columns x rows in row order
__device__ __forceinline__ void ha_row_order(int e, int n, int& cc, int& j) {
    j = n == HA_TILE ? e >> 6 : e / n;
    cc = e - j * n;
}

struct HaTile {
    int l, hw, w, t0, rows;
    size_t row0;                                // first result row of the tile
};
__device__ __forceinline__ HaTile ha_tile(const HaGeom& g) {
    HaTile q;
    q.l = 0;
#pragma unroll
    for (int k = 1; k < HA_MAX_L; ++k)
        if (k < g.L && (int)blockIdx.x >= g.lv[k].tile0) q.l = k;
    const HaLevel& lv = g.lv[q.l];
    q.w = lv.w;
    q.hw = lv.h * lv.w;
    q.t0 = ((int)blockIdx.x - lv.tile0) * HA_TILE;
    q.rows = min(HA_TILE, q.hw - q.t0);
    q.row0 = (size_t)blockIdx.y * g.A + lv.off + q.t0;
    return q;
}

template <typename T, typename E>
__global__ void __launch_bounds__(HA_TB)
ha_fwd_kernel(HaGeom g, HaOut<T> o) {
    __shared__ T sm[HA_TILE][HA_PADDED];
    __shared__ T raw[4][HA_PADDED];
    const int t = threadIdx.x, b = blockIdx.y;
    const HaTile q = ha_tile(g);
    const HaLevel& lv = g.lv[q.l];
    const T s = (T)lv.stride;

    // one map segment (channels [0, nc) -> result columns [d0, d0 + nc)) of the pass over columns [c0, c0 + n) into the tile
    auto load = [&](int r, int nc, int d0, int c0, int n, auto&& f) {
        const int lo = max(c0, d0), cnt = min(c0 + n, d0 + nc) - lo;
        if (cnt <= 0) return;
        const bool nchw = (lv.nchw >> r) & 1;
        const E* m = reinterpret_cast<const E*>(lv.map[r]);
        for (int e = t; e < cnt * HA_TILE; e += HA_TB) {
            int cc, j;
            ha_order(nchw, e, cnt, cc, j);
            if (j < q.rows) {
                const int ch = lo - d0 + cc;
                sm[lo - c0 + cc][j] = f((T)m[ha_at(nchw, b, nc, q.hw, ch, q.t0 + j)], ch, j);
            }
        }
    };
    auto rows_out = [&](T* dst, int ld, int c0, int n) {
        for (int e = t; e < q.rows * n; e += HA_TB) {
            int cc, j;
            ha_row_order(e, n, cc, j);
            dst[(q.row0 + j) * ld + c0 + cc] = sm[cc][j];
        }
    };
    auto same = [](T v, int, int) { return v; };

    if (o.outputs || o.origin) {
        const int W = 5 + g.C;
        for (int c0 = 0; c0 < (o.outputs ? W : 1); c0 += HA_TILE) {
            const int n = min(HA_TILE, W - c0);
            load(HA_REG, 4, 0, c0, n, [&](T v, int ch, int j) {
                raw[ch][j] = v;
                const int a = q.t0 + j, y = a / q.w, x = a - y * q.w;
                if (ch == 0) return (v + (T)x) * s;
                if (ch == 1) return (v + (T)y) * s;
                return ha_exp(v) * s;
            });
            if (o.outputs) {
                load(HA_OBJ, 1, 4, c0, n, same);
                load(HA_CLS, g.C, 5, c0, n, same);
            }
            __syncthreads();
            if (o.outputs) rows_out(o.outputs, o.ld, c0, n);
            if (c0 == 0 && o.origin && t < q.rows * 4) o.origin[q.row0 * 4 + t] = raw[t & 3][t >> 2];
            __syncthreads();
        }
    }
    if (o.params) {
        for (int c0 = 0; c0 < g.P; c0 += HA_TILE) {
            const int n = min(HA_TILE, g.P - c0);
            load(HA_CTRL, g.P, 0, c0, n, same);
            __syncthreads();
            rows_out(o.params, o.ldp, c0, n);
            __syncthreads();
        }
    }
    if (t < q.rows) {
        const int a = q.t0 + t, y = a / q.w, x = a - y * q.w;
        if (b == 0 && o.xs) {
            o.xs[lv.off + a] = (T)x;
            o.ys[lv.off + a] = (T)y;
            o.st[lv.off + a] = s;
        }
        if (o.levels) o.levels[q.row0 + t] = q.l;
    }
}

template <typename T, typename E>
__global__ void __launch_bounds__(HA_TB)
ha_bwd_kernel(HaGeom g, HaGrad<T> gi) {
    __shared__ T sm[HA_TILE][HA_PADDED];
    __shared__ T raw[4][HA_PADDED];
    const int t = threadIdx.x, b = blockIdx.y;
    const HaTile q = ha_tile(g);
    const HaLevel& lv = g.lv[q.l];
    const T s = (T)lv.stride;

    auto rows_in = [&](const T* src, int ld, int c0, int n) {
        for (int e = t; e < q.rows * n; e += HA_TB) {
            int cc, j;
            ha_row_order(e, n, cc, j);
            sm[cc][j] = src ? src[(q.row0 + j) * ld + c0 + cc] : (T)0;
        }
    };
    auto store = [&](int r, int nc, int d0, int c0, int n, auto&& f) {
        const int lo = max(c0, d0), cnt = min(c0 + n, d0 + nc) - lo;
        E* m = reinterpret_cast<E*>(lv.grad[r]);
        if (cnt <= 0 || !m) return;
        const bool nchw = (lv.nchw >> r) & 1;
        for (int e = t; e < cnt * HA_TILE; e += HA_TB) {
            int cc, j;
            ha_order(nchw, e, cnt, cc, j);
            if (j < q.rows) {
                const int ch = lo - d0 + cc;
                const size_t i = ha_at(nchw, b, nc, q.hw, ch, q.t0 + j);
                m[i] = (E)f(sm[lo - c0 + cc][j], ch, j, i);
            }
        }
    };
    auto same = [](T v, int, int, size_t) { return v; };

    const bool head = lv.grad[HA_REG] || lv.grad[HA_OBJ];
    if (head || lv.grad[HA_CLS]) {
        const int W = 5 + g.C;
        for (int c0 = 0; c0 < W; c0 += HA_TILE) {
            const int n = min(HA_TILE, W - c0);
            if (!(c0 == 0 && head) && !(lv.grad[HA_CLS] && c0 + n > 5)) continue;      // nobody asks for these columns
            rows_in(gi.g_out, gi.ldg, c0, n);
            if (c0 == 0 && t < q.rows * 4) raw[t & 3][t >> 2] = gi.g_org ? gi.g_org[q.row0 * 4 + t] : (T)0;
            __syncthreads();
            store(HA_REG, 4, 0, c0, n, [&](T v, int ch, int j, size_t i) {
                T d = v * s;
                if (ch >= 2) d = d * ha_exp((T) reinterpret_cast<const E*>(lv.map[HA_REG])[i]);
                return d + raw[ch][j];
            });
            store(HA_OBJ, 1, 4, c0, n, same);
            store(HA_CLS, g.C, 5, c0, n, same);
            __syncthreads();
        }
    }
    if (lv.grad[HA_CTRL]) {
        for (int c0 = 0; c0 < g.P; c0 += HA_TILE) {
            const int n = min(HA_TILE, g.P - c0);
            rows_in(gi.g_par, gi.ldgp, c0, n);
            __syncthreads();
            store(HA_CTRL, g.P, 0, c0, n, same);
            __syncthreads();
        }
    }
}

// the level table of a call; tiles = the grid's x
int ha_geom(const char* what, const HaShape& sh, HaGeom* g, int* tiles) {
    UNI_REQUIRE(sh.L >= 1 && sh.L <= HA_MAX_L && sh.B >= 1 && sh.B <= 65535 && sh.C >= 1 && sh.C <= 256 && sh.P >= 0 && sh.P <= 1024,
                "%s: shape L=%d B=%d C=%d P=%d outside 1 <= L <= %d, 1 <= B <= 65535, 1 <= C <= 256, P <= 1024", what, sh.L, sh.B, sh.C, sh.P,
                HA_MAX_L);
    *g = HaGeom{};
    g->L = sh.L, g->C = sh.C, g->P = sh.P;
    long long A = 0;
    int nt = 0;
    for (int l = 0; l < sh.L; ++l) {
        const int h = sh.hs[l], w = sh.ws[l];
        const double s = sh.strides[l];
        UNI_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < (1 << 24), "%s: level %d of h=%d w=%d outside h, w >= 1, h w < 2^24", what, l, h, w);
        UNI_REQUIRE(s > 0 && s <= 1.7e38, "%s: stride %g of level %d is not positive and finite", what, s, l);
        HaLevel& lv = g->lv[l];
        lv.stride = s, lv.h = h, lv.w = w, lv.off = (int)A, lv.tile0 = nt, lv.nchw = sh.layouts[l] & 15;
        A += (long long)h * w;
        nt += cdiv(h * w, HA_TILE);
        UNI_REQUIRE(A < (1 << 24), "%s: more than 2^24 - 1 anchors over the levels", what);
    }
    g->A = (int)A;
    *tiles = nt;
    return 0;
}

}  // namespace

template <typename T>
int launch_head_assemble_fwd(const HaShape& sh, const void* const* reg, const void* const* obj, const void* const* cls, const void* const* ctrl,
                             const HaOut<T>& o, hipStream_t s) {
    const char* what = sizeof(T) == 8 ? "head_assemble_fwd_f64" : "head_assemble_fwd";
    HaGeom g;
    int tiles;
    if (int rc = ha_geom(what, sh, &g, &tiles)) return rc;
    UNI_REQUIRE((ctrl != nullptr) == (sh.P > 0), "%s: P=%d %s controller maps", what, sh.P, ctrl ? "with" : "without");
    UNI_REQUIRE(!o.params || ctrl, "%s: dynamic_params without controller maps", what);
    UNI_REQUIRE(!o.outputs || o.ld >= 5 + sh.C, "%s: ld_out %d < 5 + C = %d", what, o.ld, 5 + sh.C);
    UNI_REQUIRE(!o.params || o.ldp >= sh.P, "%s: ld_par %d < P = %d", what, o.ldp, sh.P);
    UNI_REQUIRE((o.xs != nullptr) == (o.ys != nullptr) && (o.xs != nullptr) == (o.st != nullptr),
                "%s: x_shifts, y_shifts and expanded_strides come together", what);
    for (int l = 0; l < sh.L; ++l) {
        UNI_REQUIRE(reg[l] && obj[l] && cls[l] && (!ctrl || ctrl[l]), "%s: NULL map at level %d", what, l);
        g.lv[l].map[HA_REG] = reg[l], g.lv[l].map[HA_OBJ] = obj[l], g.lv[l].map[HA_CLS] = cls[l], g.lv[l].map[HA_CTRL] = ctrl ? ctrl[l] : nullptr;
    }
    return train_with_etype<T>(what, "map_dtype", sh.map_dtype, [&](auto e) {
        using E = typename decltype(e)::type;
        ha_fwd_kernel<T, E><<<dim3(tiles, sh.B), HA_TB, 0, s>>>(g, o);
    });
}

template <typename T>
int launch_head_assemble_bwd(const HaShape& sh, const void* const* reg, const HaGrad<T>& gi, void* const* g_reg, void* const* g_obj,
                             void* const* g_cls, void* const* g_ctrl, hipStream_t s) {
    const char* what = sizeof(T) == 8 ? "head_assemble_bwd_f64" : "head_assemble_bwd";
    HaGeom g;
    int tiles;
    if (int rc = ha_geom(what, sh, &g, &tiles)) return rc;
    UNI_REQUIRE(!g_ctrl || sh.P > 0, "%s: grad_ctrl with P = 0", what);
    UNI_REQUIRE(!gi.g_out || gi.ldg >= 5 + sh.C, "%s: ld_gout %d < 5 + C = %d", what, gi.ldg, 5 + sh.C);
    UNI_REQUIRE(!gi.g_par || gi.ldgp >= sh.P, "%s: ld_gpar %d < P = %d", what, gi.ldgp, sh.P);
    bool any = false;
    for (int l = 0; l < sh.L; ++l) {
        HaLevel& lv = g.lv[l];
        lv.grad[HA_REG] = g_reg ? g_reg[l] : nullptr, lv.grad[HA_OBJ] = g_obj ? g_obj[l] : nullptr;
        lv.grad[HA_CLS] = g_cls ? g_cls[l] : nullptr, lv.grad[HA_CTRL] = g_ctrl ? g_ctrl[l] : nullptr;
        UNI_REQUIRE(!lv.grad[HA_REG] || (reg && reg[l]), "%s: grad_reg at level %d without the reg map", what, l);
        lv.map[HA_REG] = lv.grad[HA_REG] ? reg[l] : nullptr;
        any = any || lv.grad[HA_REG] || lv.grad[HA_OBJ] || lv.grad[HA_CLS] || lv.grad[HA_CTRL];
    }
    if (!any) return 0;
    return train_with_etype<T>(what, "map_dtype", sh.map_dtype, [&](auto e) {
        using E = typename decltype(e)::type;
        ha_bwd_kernel<T, E><<<dim3(tiles, sh.B), HA_TB, 0, s>>>(g, gi);
    });
}

template int launch_head_assemble_fwd<float>(const HaShape&, const void* const*, const void* const*, const void* const*, const void* const*,
                                             const HaOut<float>&, hipStream_t);
template int launch_head_assemble_fwd<double>(const HaShape&, const void* const*, const void* const*, const void* const*, const void* const*,
                                              const HaOut<double>&, hipStream_t);
template int launch_head_assemble_bwd<float>(const HaShape&, const void* const*, const HaGrad<float>&, void* const*, void* const*, void* const*,
                                             void* const*, hipStream_t);
template int launch_head_assemble_bwd<double>(const HaShape&, const void* const*, const HaGrad<double>&, void* const*, void* const*, void* const*,
                                              void* const*, hipStream_t);
