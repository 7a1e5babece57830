// How a shape maps to a launch in the training operators (dwln_train.hip, block_tail.hip, lncf_train.hip, down_train.hip, pw_mlp.hip, gn_act_train.hip): the shape
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

// ---------------------------------------------------------------------------------------------------------------- down_train
constexpr int P4_MAX_CIN = 4;                   // stem patches: most input channels
constexpr int P4_BLOCKS = 1 << 16;              // stem patches: at most this many blocks walk the units
// the LayerNorm in front of a 2x2 / stride-2 convolution walks its input map as lncf's channels-last plan says; H, W >= 2 on top of its limits
static inline bool down_shape_ok(int B, int H, int W, int C) { return train_shape_ok(B, H, W, C) && H >= 2 && W >= 2; }
// `cl<f16,V=8,NV=3> G=4 a=f16`: lncf's class (the element type of x) and the element type of the patch matrix
static inline void down_plan_class(const LncfPlan& q, const char* en_x, const char* en_a, char* buf, size_t n) {
    char cls[48];
    lncf_plan_class(q, en_x, cls, sizeof(cls));
    std::snprintf(buf, n, "%s a=%s", cls, en_a);
}
static inline size_t down_plan_workspace_bytes(int B, int H, int W, int C) { return down_shape_ok(B, H, W, C) ? lncf_plan_workspace_bytes(B, H, W, C) : 0; }
// stem patches (kernel 4, stride 4) of an NCHW-contiguous map: a unit = the four elements (kw = 0 .. 3) of one (patch, channel, kh) in the
// gather, of one (n, c, h, group of four columns) in the scatter, whose last group per row is the margin that W % 4 leaves
struct Patch4Plan {
    int Ho, Wo, wg;                             // output map; groups of four columns per row of x (scatter)
    long long M, units;
    int grid, block;
};
static inline bool patch4_shape_ok(int B, int Cin, int H, int W) {
    return B >= 1 && Cin >= 1 && Cin <= P4_MAX_CIN && H >= 4 && W >= 4 && (long long)B * H * W < (1ll << 31);
}
static inline Patch4Plan patch4_plan(int B, int Cin, int H, int W, bool scatter) {
    Patch4Plan q{};
    q.Ho = H / 4, q.Wo = W / 4, q.wg = (int)plan_cdiv(W, 4);
    q.M = (long long)B * q.Ho * q.Wo;
    q.units = scatter ? (long long)B * Cin * H * q.wg : q.M * Cin * 4;      // < 2^33
    q.block = 256;
    const long long nb = plan_cdiv(q.units, q.block);
    q.grid = (int)(nb < P4_BLOCKS ? nb : P4_BLOCKS);
    return q;
}
// `<x=f32,a=f16>`
static inline void patch4_plan_class(const char* en_x, const char* en_a, char* buf, size_t n) { std::snprintf(buf, n, "<x=%s,a=%s>", en_x, en_a); }

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

// ---------------------------------------------------------------------------------------------------------------- gn_act_train
constexpr int GN_UNIT_CL = 256;                 // gn_act: most pixels of a unit (consecutive pixels of ONE image), channels-last memory
constexpr int GN_UNIT_CL_MIN = 16;              // ... fewest: small maps take short units, so that about GN_ROWS_CL rows of blocks share the pixels
constexpr int GN_ROWS_CL = 512;                 // gn_act, channels-last: the rows in all that the choice of the unit aims for
constexpr int GN_RED_COLS = 16;                 // gn_act, combine launch: columns of [2 C] per block (and 256 / 16 slices of rows)
constexpr int GN_UNIT_NCHW = 512;               // ... NCHW memory
constexpr int GN_COMB_BLOCKS = 65536;           // gn_act, combine launches: at most this many blocks walk the (sample, group) pairs
constexpr int GN_NCHW_CT = 16;                  // gn_act, NCHW path: channels of a block (four waves, a wave takes one channel at a time)
static inline bool gn_shape_ok(int B, int H, int W, int C, int G) { return train_shape_ok(B, H, W, C) && G >= 1 && G <= C && C % G == 0; }
// pixels of the units r, r + rpi, r + 2 rpi, ... < upi of an image of HW pixels (the last unit may be short); callable from a kernel.  The row
// count holds what does not depend on r, so that a loop over rows divides nothing.
struct GnRowCount {
    long long full, cut;                        // pixels of upi / rpi whole units; what the last unit lacks
    unsigned rem;                               // rows r < rem take one unit more
    int last, unit;                             // the row of the last unit
};
constexpr GnRowCount gn_row_count(long long HW, int unit, unsigned upi, int rpi) {
    return GnRowCount{(long long)(upi / (unsigned)rpi) * unit, (long long)upi * unit - HW, upi % (unsigned)rpi, (int)((upi - 1) % (unsigned)rpi), unit};
}
constexpr long long gn_row_pixels(const GnRowCount& c, int r) { return c.full + ((unsigned)r < c.rem ? c.unit : 0) - (r == c.last ? c.cut : 0); }
constexpr long long gn_row_pixels(long long HW, int unit, unsigned upi, int rpi, int r) { return gn_row_pixels(gn_row_count(HW, unit, upi, rpi), r); }
struct GnPlan {
    bool nchw;
    int V, lg;                                  // channels-last: channels per vector, L = 2^lg lanes (vectors) per pixel of a block, 256 / L pixels per step
    int unit;                                   // pixels of a unit
    unsigned upi;                               // units per image
    int rpi, rows;                              // rows of partials per image (block r of an image takes the units r, r + rpi, ...), in all (= B rpi)
    int planes;                                 // forward: planes [C] of a row of partials: mean and M2, or the mean alone where H W == 1 (M2 = 0)
    int grid_x, grid_y, block;                  // rows; column tiles of L vectors (channels-last) or of GN_NCHW_CT channels (NCHW)
    unsigned comb_blocks;                       // the two combine launches: blocks that walk the B G (sample, group) pairs, a block each
    size_t off_ab, elems;                       // workspace (elements): partials [rows][2][C] at 0, the group sums [B G][2] at off_ab
};
// A block belongs to one image: rows = B rpi with rpi = min(units per image, max(1, TRAIN_ROWS / B)), so at most max(B, TRAIN_ROWS) rows.
// Channels-last units are as short as that cap allows (a (2, C, 25, 40) map in units of 256 pixels is 8 rows of blocks on 256 compute units).
// Channels-last: the lane mapping of pw_plan over the C / V vectors of a pixel.  NCHW: a wave reads 64 consecutive pixels of a channel plane.
static inline GnPlan gn_plan(int B, int H, int W, int C, int G, int esize, bool nchw) {
    GnPlan q{};
    const long long HW = (long long)H * W;
    q.nchw = nchw;
    q.unit = nchw ? GN_UNIT_NCHW : GN_UNIT_CL_MIN;
    while (!nchw && q.unit < GN_UNIT_CL && (long long)q.unit * GN_ROWS_CL < B * HW) q.unit <<= 1;      // the power of two >= B H W / GN_ROWS_CL in [16, 256]
    q.upi = (unsigned)plan_cdiv(HW, q.unit);
    const int cap = TRAIN_ROWS / B > 1 ? TRAIN_ROWS / B : 1;
    q.rpi = train_rows(q.upi, cap);
    q.rows = B * q.rpi;                         // <= max(B, TRAIN_ROWS) < 2^31
    q.planes = HW == 1 ? 1 : 2;
    q.grid_x = q.rows;
    q.block = 256;
    if (nchw) {
        q.V = 1;
        q.grid_y = (int)plan_cdiv(C, GN_NCHW_CT);
    } else {
        const PwPlan w = pw_plan(1, C, esize);
        q.V = w.V, q.lg = w.lg, q.grid_y = w.grid_x;
    }
    const long long pairs = (long long)B * G;
    q.comb_blocks = (unsigned)(pairs < GN_COMB_BLOCKS ? pairs : GN_COMB_BLOCKS);
    q.off_ab = ((size_t)q.rows * 2 * C + 63) / 64 * 64;
    q.elems = q.off_ab + (size_t)B * G * 2;
    return q;
}
// `cl<f16,V=8> L=16`, `nchw<f32> CT=16`
static inline void gn_plan_class(const GnPlan& q, const char* en, char* buf, size_t n) {
    if (q.nchw) std::snprintf(buf, n, "nchw<%s> CT=%d", en, GN_NCHW_CT);
    else std::snprintf(buf, n, "cl<%s,V=%d> L=%d", en, q.V, 1 << q.lg);
}
// counted in fp32 elements (the fp64 launchers need twice the bytes) from the channels-last plan: it has the shorter units, so the more rows
static inline size_t gn_plan_workspace_bytes(int B, int H, int W, int C, int G) {
    static_assert(GN_UNIT_CL <= GN_UNIT_NCHW, "the workspace is sized by the channels-last plan");
    return gn_shape_ok(B, H, W, C, G) ? 4 * gn_plan(B, H, W, C, G, 4, false).elems : 0;
}
