// How a shape maps to a launch in the four ConvNeXt training operators (dwln_train.hip, block_tail.hip, lncf_train.hip, pw_mlp.hip): the shape
// limits, the vector width, the lane mapping, grid, block, dynamic LDS, the rows of partial sums and the workspace that holds them -- stated
// here and nowhere else.  Plain C++17, no HIP: the launchers read these plans, tools/train_plan_check.cpp checks them over the admitted
// domain and prints them, tests/train_plans.py answers from that listing.  Retune a plan here; the check program says what it breaks.
#pragma once
#include <cstddef>
#include <cstdio>

constexpr int TRAIN_MAX_C = 2048;
constexpr int TRAIN_ROWS = 1024;                // at most this many blocks write partial sums (= rows of partials)
constexpr int PW_MAX_H = 4 * TRAIN_MAX_C;
constexpr int PW_ROWS = 256;                    // pw_mlp: at most this many rows of partials per sum
constexpr int BT_TILE = 64;                     // block_tail, NCHW path: pixels and channels of a tile
constexpr int LNCF_TILE = 64;                   // lncf, NCHW path: pixels of a tile (lane = pixel)
constexpr int LNCF_NW = 8;                      // lncf, NCHW path: waves of a block
constexpr int DWLN_DW_STRIP = 128;              // dwln pass B (weights): longest strip a wave walks
template <typename T>
struct DwlnPx { static constexpr int value = sizeof(T) == 4 ? 8 : 2; };      // dwln: pixels of a strip per lane
template <int V>
struct BtU { static constexpr int value = V == 8 ? 2 : 4; };      // block_tail, channels-last: steps of PP pixels whose loads are in flight together

static inline bool train_shape_ok(int B, int H, int W, int C) {
    return B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && C <= TRAIN_MAX_C && (long long)B * H * W < (1ll << 31);
}
static inline bool pw_width_ok(int N) { return N >= 4 && N % 4 == 0 && N <= PW_MAX_H; }
static inline bool pw_shape_ok(int M, int Hd, int Co) { return M >= 1 && pw_width_ok(Hd) && pw_width_ok(Co); }
static inline const char* train_ename(int dtype, bool f64) { return f64 ? "f64" : dtype == 1 ? "f16" : dtype == 2 ? "bf16" : "f32"; }
static inline int train_rows(unsigned n, int cap) { return n < (unsigned)cap ? (int)n : cap; }      // blocks that take n units of work
// channels per lane of a channels-last kernel: 16 bytes of the element type, so 8 for a half type where C allows it, else 4
static inline int train_vwidth(int esize, int C) { return esize == 2 && C % 8 == 0 ? 8 : 4; }
static inline long long plan_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------------------------------------------- lncf_train
enum LncfFamily { LNCF_CL, LNCF_NCHW_REGS16, LNCF_NCHW_REGS32, LNCF_NCHW_STREAM8 };
struct LncfPlan {
    int family;
    int V, NV, lg;                              // channels-last: channels per vector, vectors per lane, G = 2^lg lanes per pixel
    unsigned per_image, units;                  // NCHW: tiles per image, tiles in all; channels-last: groups of 256 / G pixels in all
    int grid, block;
    size_t lds;                                 // dynamic LDS (bytes)
    int rows;                                   // rows of partials [2][C] (= grid)
};
// channels-last: NV vectors per lane and G = 2^lg lanes per pixel with G NV >= nvec and the fewest idle vector slots (the smaller NV on a tie).
// NCHW: 16 channels per lane in registers (C <= 128), 32 (C <= 256; not fp64, kept for checks: 32 x, grad_y and two sums per lane do not fit
// in registers), else the slice is streamed in chunks of 8.  Partial sums across lanes are formed in double in dynamic LDS.
static inline LncfPlan lncf_plan(int B, int H, int W, int C, int esize, bool f64, bool nchw, bool partials) {
    LncfPlan q{};
    const size_t lds = partials ? (size_t)2 * C * sizeof(double) : 0;
    if (nchw) {
        q.family = C <= 16 * LNCF_NW ? LNCF_NCHW_REGS16 : (!f64 && C <= 32 * LNCF_NW) ? LNCF_NCHW_REGS32 : LNCF_NCHW_STREAM8;
        q.per_image = (unsigned)plan_cdiv((long long)H * W, LNCF_TILE);
        q.units = (unsigned)B * q.per_image;    // <= B H W
        q.block = 64 * LNCF_NW;
        q.lds = q.family == LNCF_NCHW_STREAM8 ? lds : 0;
    } else {
        q.family = LNCF_CL;
        q.V = train_vwidth(esize, C);
        static const int nvs[] = {1, 2, 3, 4, 6, 8};
        int best = 1 << 30;
        for (int k : nvs) {
            int l = 0;
            while ((k << l) < C / q.V) ++l;
            if (l <= 6 && (k << l) < best) {
                best = k << l;
                q.NV = k;
                q.lg = l;
            }
        }
        q.units = (unsigned)plan_cdiv((long long)B * H * W, 256 >> q.lg);
        q.block = 256;
        q.lds = lds;
    }
    q.grid = q.rows = train_rows(q.units, TRAIN_ROWS);
    return q;
}
// the plan-class part of the variant tag: `cl<f16,V=8,NV=3> G=4`, `nchw<f32,regs=16>`
static inline void lncf_plan_class(const LncfPlan& q, const char* en, char* buf, size_t n) {
    static const char* const nchw[] = {"", "regs=16", "regs=32", "stream=8"};
    if (q.family == LNCF_CL) std::snprintf(buf, n, "cl<%s,V=%d,NV=%d> G=%d", en, q.V, q.NV, 1 << q.lg);
    else std::snprintf(buf, n, "nchw<%s,%s>", en, nchw[q.family]);
}
static inline size_t lncf_plan_workspace_bytes(int B, int H, int W, int C) { return train_shape_ok(B, H, W, C) ? (size_t)4 * TRAIN_ROWS * 2 * C : 0; }

// ---------------------------------------------------------------------------------------------------------------- block_tail
struct BtPlan {
    bool nchw;
    int V, CG, PP, steps;                       // a block takes `steps` steps of PP pixels x CG lanes of V channels at once
    unsigned per_image, units;                  // chunks (channels-last) or tiles (NCHW) of steps PP pixels per image, in all
    int grid_x, grid_y, block;
    int rows;                                   // rows of partials [C] (= grid_x)
};
// channels-last: CG = C / V lanes per pixel, PP = 512 / CG pixels per step (CG <= 512).  NCHW: a tile of 64 pixels x 64 channels (grid_y
// walks the channel tiles): sixteen lanes of 4 channels, four steps of sixteen pixels.
static inline BtPlan bt_plan(int B, int H, int W, int C, int esize, bool nchw) {
    BtPlan q{};
    q.nchw = nchw;
    if (nchw) {
        q.V = 4, q.CG = BT_TILE / 4, q.PP = 16, q.steps = BT_TILE / 16;
        q.grid_y = (int)plan_cdiv(C, BT_TILE);
        q.block = 256;
    } else {
        q.V = train_vwidth(esize, C);
        q.CG = C / q.V, q.PP = 512 / q.CG;
        q.steps = q.V == 8 ? BtU<8>::value : BtU<4>::value;
        q.grid_y = 1;
        q.block = (q.PP * q.CG + 63) / 64 * 64;
    }
    q.per_image = (unsigned)plan_cdiv((long long)H * W, q.steps * q.PP);
    q.units = (unsigned)B * q.per_image;        // <= B H W
    q.grid_x = q.rows = train_rows(q.units, TRAIN_ROWS);
    return q;
}
// `cl<f32,V=4>`, `nchw<f16>`
static inline void bt_plan_class(const BtPlan& q, const char* en, char* buf, size_t n) {
    if (q.nchw) std::snprintf(buf, n, "nchw<%s>", en);
    else std::snprintf(buf, n, "cl<%s,V=%d>", en, q.V);
}
static inline size_t bt_plan_workspace_bytes(int B, int H, int W, int C) { return train_shape_ok(B, H, W, C) ? (size_t)4 * TRAIN_ROWS * C : 0; }

// ---------------------------------------------------------------------------------------------------------------- dwln_train
struct DwlnPlan {
    int pxt;                                    // pixels of a strip per lane: DwlnPx of the math type
    int CG, CGp, NS, threads;                   // conv kernels: lanes of a strip, padded to whole waves; strips per block
    int segs, nstrips, nsb, RA;                 // strips of pxt pixels per row, in all, blocks of NS strips, blocks of pass A
    int slen, segs_w, nstrips_w, RB, NCT;       // pass B (weights): strip length, strips per row, in all, blocks per channel tile, channel tiles
    size_t lds_a;                               // pass A with partials: dynamic LDS (bytes)
    size_t off_pa, off_pb, elems;               // workspace (elements): du at 0, partials of pass A [RA][2][C], of pass B [RB][50][C]
};
static inline bool dwln_plan(int B, int H, int W, int C, bool f64, DwlnPlan& q) {
    if (!train_shape_ok(B, H, W, C)) return false;
    const long long M = (long long)B * H * W;
    q.pxt = f64 ? DwlnPx<double>::value : DwlnPx<float>::value;
    q.CG = C / 4;
    q.CGp = (q.CG + 63) / 64 * 64;
    q.NS = 512 / q.CGp;
    q.threads = q.NS * q.CGp;
    q.segs = (int)plan_cdiv(W, q.pxt);
    q.nstrips = B * H * q.segs;
    q.nsb = (int)plan_cdiv(q.nstrips, q.NS);
    q.RA = train_rows(q.nsb, TRAIN_ROWS);       // pass A: blocks = rows of dgamma / dbeta partials
    q.segs_w = (int)plan_cdiv(W, DWLN_DW_STRIP);
    q.slen = (int)plan_cdiv(W, q.segs_w);
    q.segs_w = (int)plan_cdiv(W, q.slen);
    q.nstrips_w = B * H * q.segs_w;
    q.RB = (int)plan_cdiv(q.nstrips_w, 4);
    q.NCT = (int)plan_cdiv(C, 64);
    q.lds_a = (size_t)2 * C * (f64 ? sizeof(double) : sizeof(float));
    auto up = [](size_t n) { return (n + 63) / 64 * 64; };
    q.off_pa = up((size_t)M * C);
    q.off_pb = q.off_pa + up((size_t)q.RA * 2 * C);
    q.elems = q.off_pb + up((size_t)q.RB * 50 * C);
    return true;
}
// `<f32,PXT=8> wps=1 NS=8`
static inline void dwln_plan_class(const DwlnPlan& q, const char* en, char* buf, size_t n) {
    std::snprintf(buf, n, "<%s,PXT=%d> wps=%d NS=%d", en, q.pxt, q.CGp / 64, q.NS);
}
// counted in fp32 elements (the fp64 launchers need twice the bytes) from the plan of the fp64 form: it has the fewer pixels per strip, so
// the more blocks in pass A, and one formula serves both
static inline size_t dwln_plan_workspace_bytes(int B, int H, int W, int C) {
    DwlnPlan q;
    static_assert(DwlnPx<double>::value <= DwlnPx<float>::value, "the workspace is sized by the fp64 plan");
    return dwln_plan(B, H, W, C, true, q) ? 4 * q.elems : 0;
}

// ---------------------------------------------------------------------------------------------------------------- pw_mlp
struct PwPlan {
    int V, lg, rpb;                             // a block = rpb rows x L = 2^lg vectors of V columns, rpb = 256 / L
    unsigned ngroups;                           // groups of rpb rows
    int grid_x, grid_y, block;                  // column tiles of L vectors; rows of partials
    int rows;                                   // rows of partials [N] (= grid_y)
};
// lanes per row of a block: the power of two L in [min(8, nvec rounded up), 256] with the fewest idle vector slots ceil(nvec / L) L - nvec,
// the larger L on a tie
static inline PwPlan pw_plan(int M, int N, int esize) {
    PwPlan q{};
    q.V = train_vwidth(esize, N);
    const int nvec = N / q.V;
    int lo = 0;
    while ((1 << lo) < nvec && lo < 3) ++lo;
    long long best = 1ll << 30;
    q.lg = lo;
    for (int l = lo; l <= 8; ++l) {
        const long long padded = plan_cdiv(nvec, 1 << l) << l;
        if (padded <= best) {
            best = padded;
            q.lg = l;
        }
    }
    q.rpb = 256 >> q.lg;
    q.ngroups = (unsigned)plan_cdiv(M, q.rpb);
    q.grid_x = (int)plan_cdiv(nvec, 1 << q.lg);
    q.grid_y = q.rows = train_rows(q.ngroups, PW_ROWS);
    q.block = 256;
    return q;
}
// `<f16,V=8> L=16`: the instantiation and the lane mapping, as lncf's `cl<...> G=4`
static inline void pw_plan_class(const PwPlan& q, const char* en, char* buf, size_t n) {
    std::snprintf(buf, n, "<%s,V=%d> L=%d", en, q.V, 1 << q.lg);
}
// two sums: [PW_ROWS][Hd] at 0, [PW_ROWS][Co] behind it
static inline size_t pw_plan_workspace_bytes(int M, int Hd, int Co) { return pw_shape_ok(M, Hd, Co) ? (size_t)4 * PW_ROWS * ((size_t)Hd + Co) : 0; }
