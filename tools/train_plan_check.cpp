// Host check of unicorn_amd/csrc/train_plan.h: the launch plans of the four ConvNeXt training operators and of gn_act over their admitted domain.  Plain C++
// (built by unicorn_amd/csrc/build.sh into tools/build/train_plan_check, run by tests/test_train_plans_cpu.py; tests/train_plans.py reads
// --list).  Default: every condition below at every point of the domain, then each condition once on a deliberately wrong plan, which it must
// refuse; prints `train_plan_check: OK` or the first violated condition with its arguments and exits non-zero.  --list: one line per
// (operator, layout, element type, C) with the plan class the formatter of the header writes.
#include "../unicorn_amd/csrc/train_plan.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

static std::string g_where;                     // the arguments of the plan under check
static int g_failures = 0;
static bool g_quiet = false;                    // the wrong plans at the end: count, do not stop
#define REQUIRE(cond, ...)                                   \
    do {                                                     \
        if (!(cond)) {                                       \
            ++g_failures;                                    \
            if (!g_quiet) {                                  \
                std::printf("FAIL: %s: ", g_where.c_str());  \
                std::printf(__VA_ARGS__);                    \
                std::printf("  [%s]\n", #cond);              \
                std::exit(1);                                \
            }                                                \
            return;                                          \
        }                                                    \
    } while (0)

constexpr size_t LDS_MAX = 64 * 1024;           // without the opt-in of common.h
struct Map { int B, H, W; };
static const Map MAPS[] = {{1, 1, 1}, {2, 3, 7}, {2, 5, 11}, {1, 10, 13}, {3, 4, 8}, {2, 200, 320}, {7, 300, 300}, {2047, 1024, 1024},
                           {1, 1, 2147483647}};
struct Etype { const char* name; int dtype, esize; bool f64; };
static const Etype ETYPES[] = {{"f32", 0, 4, false}, {"f16", 1, 2, false}, {"bf16", 2, 2, false}, {"f64", 0, 8, true}};
static const int PW_M[] = {1, 42, 255, 256, 257, 65537, 2147483647};

static void where(const char* op, const Map& m, int C, const char* en, const char* layout) {
    char b[160];
    std::snprintf(b, sizeof(b), "%s B=%d H=%d W=%d C=%d %s %s", op, m.B, m.H, m.W, C, en, layout);
    g_where = b;
}

// what every launch must satisfy: the block whole waves within the kernel's __launch_bounds__, the grid within the limits of a launch
static void check_launch(long long gx, long long gy, int block, int bound, size_t lds_static, size_t lds_dyn) {
    REQUIRE(block >= 64 && block % 64 == 0 && block <= bound, "block %d, __launch_bounds__(%d)", block, bound);
    REQUIRE(gx >= 1 && gx < (1ll << 31) && gy >= 1 && gy <= 65535, "grid (%lld, %lld)", gx, gy);
    REQUIRE(lds_static + lds_dyn <= LDS_MAX, "LDS %zu static + %zu dynamic", lds_static, lds_dyn);
}
// partials [rows][row_elems] from element `off` on end inside ws_f32_bytes (fp32 elements; the fp64 form has twice the bytes and twice the element)
static void check_region(int rows, int cap, size_t off, size_t row_elems, size_t ws_f32_bytes) {
    REQUIRE(rows >= 1 && rows <= cap, "%d rows of partials, at most %d", rows, cap);
    REQUIRE((off + (size_t)rows * row_elems) * 4 <= ws_f32_bytes, "partials end at element %zu, the workspace holds %zu", off + (size_t)rows * row_elems,
            ws_f32_bytes / 4);
}

// ---------------------------------------------------------------------------------------------------------------- lncf
static void check_lncf(const LncfPlan& q, const Map& m, int C, const Etype& e, bool partials) {
    const long long M = (long long)m.B * m.H * m.W;
    const size_t tsize = e.f64 ? 8 : 4;
    const bool cl = q.family == LNCF_CL;
    // lncf_nchw_kernel: sm[2][2][LNCF_NW][64] of the math type, __launch_bounds__(512); ln_cl_kernel (ln_cl.h): no static LDS, __launch_bounds__(256)
    check_launch(q.grid, 1, q.block, cl ? 256 : 512, cl ? 0 : 2 * 2 * LNCF_NW * 64 * tsize, q.lds);
    REQUIRE(q.units >= 1 && q.units <= M, "%u work units, %lld pixels", q.units, M);
    REQUIRE(q.grid <= (long long)q.units, "grid %d, %u work units", q.grid, q.units);
    if (cl) {
        REQUIRE(q.lg >= 0 && q.lg <= 6 && ((long long)q.NV << q.lg) >= C / q.V, "G NV = %d x %d, %d vectors", 1 << q.lg, q.NV, C / q.V);
        REQUIRE(q.V == 4 || (q.V == 8 && e.esize == 2 && C % 8 == 0), "V = %d", q.V);
        REQUIRE(q.NV <= 4 || (q.V == 4 && (q.NV == 6 || q.NV == 8)), "NV = %d with V = %d has no instantiation", q.NV, q.V);
        REQUIRE((long long)q.units * (256 >> q.lg) >= M, "%u groups of %d pixels, %lld pixels", q.units, 256 >> q.lg, M);
        REQUIRE(q.block == 256, "block %d", q.block);
    } else {
        REQUIRE((long long)q.per_image * LNCF_TILE >= (long long)m.H * m.W && q.units == (unsigned long long)m.B * q.per_image, "%u tiles per image",
                q.per_image);
        REQUIRE(q.block == 64 * LNCF_NW, "block %d", q.block);
        const int per_lane = (C + LNCF_NW - 1) / LNCF_NW;      // channels of wave 0
        REQUIRE(q.family == LNCF_NCHW_STREAM8 || per_lane <= (q.family == LNCF_NCHW_REGS16 ? 16 : 32), "%d channels per lane kept in registers", per_lane);
        REQUIRE(q.family != LNCF_NCHW_REGS32 || !e.f64, "regs=32 has no fp64 instantiation");
    }
    // the row of partials [2][C] is formed in double in dynamic LDS, except where a lane keeps its sums in registers
    const bool in_regs = q.family == LNCF_NCHW_REGS16 || q.family == LNCF_NCHW_REGS32;
    REQUIRE(q.lds == (partials && !in_regs ? (size_t)2 * C * 8 : 0), "dynamic LDS %zu", q.lds);
    REQUIRE(q.rows == q.grid, "rows %d, grid %d", q.rows, q.grid);
    check_region(q.rows, TRAIN_ROWS, 0, (size_t)2 * C, lncf_plan_workspace_bytes(m.B, m.H, m.W, C));
}

// ---------------------------------------------------------------------------------------------------------------- block_tail
static void check_bt(const BtPlan& q, const Map& m, int C, const Etype& e) {
    const long long M = (long long)m.B * m.H * m.W;
    const size_t tsize = e.f64 ? 8 : 4;
    // bt_cl_kernel: sm[512 V] in the backward, __launch_bounds__(512); bt_nchw_kernel: tile[64][65] + red[16][64], __launch_bounds__(256)
    const size_t lds = q.nchw ? (BT_TILE * (BT_TILE + 1) + 16 * BT_TILE) * tsize : (size_t)512 * q.V * tsize;
    check_launch(q.grid_x, q.grid_y, q.block, q.nchw ? 256 : 512, lds, 0);
    REQUIRE(q.units >= 1 && q.units <= M, "%u work units, %lld pixels", q.units, M);
    REQUIRE(q.grid_x <= (long long)q.units, "grid %d, %u work units", q.grid_x, q.units);
    REQUIRE(q.PP >= 1 && q.PP * q.CG <= 512 && q.PP * q.CG <= q.block, "PP = %d, CG = %d, block %d", q.PP, q.CG, q.block);
    REQUIRE((long long)q.per_image * q.steps * q.PP >= (long long)m.H * m.W && q.units == (unsigned long long)m.B * q.per_image, "%u units per image",
            q.per_image);
    if (q.nchw) {
        REQUIRE(q.V == 4 && q.steps * q.PP == BT_TILE && q.CG * q.V == BT_TILE && (long long)q.grid_y * BT_TILE >= C, "tile %d x %d, %d channel tiles",
                q.steps * q.PP, q.CG * q.V, q.grid_y);
    } else {
        REQUIRE(q.V == 4 || (q.V == 8 && e.esize == 2 && C % 8 == 0), "V = %d", q.V);
        REQUIRE(q.CG * q.V == C && q.grid_y == 1 && q.steps == (q.V == 8 ? BtU<8>::value : BtU<4>::value), "CG = %d, V = %d, %d steps", q.CG, q.V, q.steps);
        REQUIRE((size_t)q.PP * C <= (size_t)512 * q.V, "the PP = %d rows of C sums do not fit sm[512 V]", q.PP);
    }
    REQUIRE(q.rows == q.grid_x, "rows %d, grid %d", q.rows, q.grid_x);
    check_region(q.rows, TRAIN_ROWS, 0, (size_t)C, bt_plan_workspace_bytes(m.B, m.H, m.W, C));
}

// ---------------------------------------------------------------------------------------------------------------- dwln
// q: the plan under check; q64: the fp64 plan of the same shape, which sizes the workspace
static void check_dwln(const DwlnPlan& q, const DwlnPlan& q64, const Map& m, int C, const Etype& e) {
    const long long M = (long long)m.B * m.H * m.W;
    const size_t tsize = e.f64 ? 8 : 4;
    // dwln_conv_kernel: sm1, sm2 [8 * 2 * PXT], __launch_bounds__(512); dwln_dw_kernel: sm[50 * 64], __launch_bounds__(256)
    const size_t lds_conv = (size_t)2 * 8 * 2 * q.pxt * tsize;
    check_launch(q.nsb, 1, q.threads, 512, lds_conv, 0);                           // forward, pass B (data)
    check_launch(q.RA, 1, q.threads, 512, lds_conv, q.lds_a);                      // pass A
    check_launch(q.RB, q.NCT, 256, 256, (size_t)50 * 64 * tsize, 0);               // pass B (weights)
    REQUIRE(q.lds_a == (size_t)2 * C * tsize, "dynamic LDS %zu", q.lds_a);
    REQUIRE(q.NS >= 1 && q.NS * q.CGp <= 512 && q.threads == q.NS * q.CGp && q.CGp % 64 == 0 && q.CGp >= q.CG && q.CG * 4 == C, "NS = %d, CGp = %d, CG = %d",
            q.NS, q.CGp, q.CG);
    REQUIRE(q.NS * (q.CGp / 64) <= 8, "%d waves write sm[8 * 2 * PXT]", q.NS * (q.CGp / 64));
    REQUIRE(q.nstrips >= 1 && q.nstrips <= M && (long long)q.segs * q.pxt >= m.W && q.nstrips == (long long)m.B * m.H * q.segs, "%d strips of %d pixels",
            q.nstrips, q.pxt);
    REQUIRE((long long)q.nsb * q.NS >= q.nstrips && q.nsb <= q.nstrips && q.RA <= q.nsb, "%d blocks of %d strips, %d strips", q.nsb, q.NS, q.nstrips);
    REQUIRE(q.nstrips_w >= 1 && q.nstrips_w <= M && q.slen >= 1 && q.slen <= DWLN_DW_STRIP && (long long)q.segs_w * q.slen >= m.W &&
                q.nstrips_w == (long long)m.B * m.H * q.segs_w && (long long)q.RB * 4 >= q.nstrips_w && q.RB <= q.nstrips_w,
            "weight pass: %d strips of %d pixels, %d blocks", q.nstrips_w, q.slen, q.RB);
    REQUIRE((long long)q.NCT * 64 >= C, "%d channel tiles", q.NCT);
    // du [M][C], then the partials of pass A, then those of pass B: disjoint, in this order, inside the bytes the fp64 plan promises
    const size_t ws = dwln_plan_workspace_bytes(m.B, m.H, m.W, C);
    REQUIRE(ws == 4 * q64.elems, "workspace %zu bytes, the fp64 plan has %zu elements", ws, q64.elems);
    REQUIRE((size_t)M * C <= q.off_pa && q.off_pa + (size_t)q.RA * 2 * C <= q.off_pb && q.off_pa % 4 == 0 && q.off_pb % 4 == 0,
            "du ends at %zu, pass A at %zu .. %zu, pass B from %zu", (size_t)M * C, q.off_pa, q.off_pa + (size_t)q.RA * 2 * C, q.off_pb);
    check_region(q.RA, TRAIN_ROWS, q.off_pa, (size_t)2 * C, ws);
    REQUIRE(q.RB >= 1 && (q.off_pb + (size_t)q.RB * 50 * C) * 4 <= ws && q.elems <= q64.elems, "pass B ends at element %zu, the workspace holds %zu",
            q.off_pb + (size_t)q.RB * 50 * C, ws / 4);
}

// ---------------------------------------------------------------------------------------------------------------- pw_mlp
static void check_pw(const PwPlan& q, int M, int N, int esize, size_t off, size_t ws_f32_bytes) {
    const int nvec = N / q.V, L = 1 << q.lg;
    // pw_map_kernel: sm[256 V] doubles where it sums, __launch_bounds__(256)
    check_launch(q.grid_x, q.grid_y, q.block, 256, (size_t)256 * q.V * 8, 0);
    REQUIRE(q.V == 4 || (q.V == 8 && esize == 2 && N % 8 == 0), "V = %d", q.V);
    REQUIRE(q.ngroups >= 1 && q.ngroups <= (unsigned)M && (long long)q.ngroups * q.rpb >= M, "%u groups of %d rows, %d rows", q.ngroups, q.rpb, M);
    REQUIRE(q.lg >= 0 && q.lg <= 8 && L * q.rpb == 256 && q.block == 256, "L = %d, RPB = %d", L, q.rpb);
    REQUIRE((long long)q.grid_x * L >= nvec && (long long)(q.grid_x - 1) * L < nvec, "%d column tiles of %d vectors, %d vectors", q.grid_x, L, nvec);
    REQUIRE(q.rows == q.grid_y && q.grid_y <= (long long)q.ngroups, "rows %d, grid.y %d, %u groups", q.rows, q.grid_y, q.ngroups);
    check_region(q.rows, PW_ROWS, off, (size_t)N, ws_f32_bytes);
}

// ---------------------------------------------------------------------------------------------------------------- gn_act
static const int GN_GS[] = {1, 2, 4, 16, 32};    // next to G = C and G = C / 4 (cpg = 1 and 4) and G = C / 6, C / 12 where they divide (cpg = 6, 12)
static void check_gn(const GnPlan& q, const Map& m, int C, int G, const Etype& e) {
    const long long HW = (long long)m.H * m.W;
    // gn_cl_kernel: sm[256 V] doubles and bc[256 V] of the math type where it sums, __launch_bounds__(256); gn_nchw_kernel: no LDS, __launch_bounds__(256)
    check_launch(q.grid_x, q.grid_y, q.block, 256, q.nchw ? 0 : (size_t)256 * q.V * (8 + (e.f64 ? 8 : 4)), 0);
    REQUIRE(q.block == 256, "block %d", q.block);
    REQUIRE(q.unit >= (q.nchw ? 64 : GN_UNIT_CL_MIN) && q.unit <= GN_UNIT_NCHW && (q.unit & (q.unit - 1)) == 0 && (long long)q.upi * q.unit >= HW && (long long)(q.upi - 1) * q.unit < HW, "%u units of %d pixels, %lld pixels", q.upi, q.unit, HW);
    REQUIRE(q.rpi >= 1 && (unsigned)q.rpi <= q.upi && q.rows == (long long)m.B * q.rpi && q.grid_x == q.rows, "%d rows per image, %d rows, grid %d", q.rpi,
            q.rows, q.grid_x);
    REQUIRE(q.rows <= (m.B > TRAIN_ROWS ? m.B : TRAIN_ROWS), "%d rows of partials", q.rows);
    long long px = 0;                           // the rows of an image take every pixel once
    for (int r = 0; r < q.rpi; ++r) {
        const long long n = gn_row_pixels(HW, q.unit, q.upi, q.rpi, r);
        REQUIRE(n >= 1, "row %d of %d takes %lld pixels", r, q.rpi, n);
        px += n;
    }
    REQUIRE(px == HW, "the rows take %lld pixels of %lld", px, HW);
    // the forward keeps [rows][planes][C] in y [B][H W][C]
    REQUIRE((q.planes == 2 || (q.planes == 1 && HW == 1)) && (long long)q.rpi * q.planes <= HW, "%d planes x %d rows in a map of %lld pixels", q.planes, q.rpi, HW);
    if (q.nchw) {
        REQUIRE((long long)q.grid_y * GN_NCHW_CT >= C && (long long)(q.grid_y - 1) * GN_NCHW_CT < C, "%d channel tiles", q.grid_y);
    } else {
        const int nvec = C / q.V, L = 1 << q.lg;
        REQUIRE(q.V == 4 || (q.V == 8 && e.esize == 2 && C % 8 == 0), "V = %d", q.V);
        REQUIRE(q.lg >= 0 && q.lg <= 8 && (long long)q.grid_y * L >= nvec && (long long)(q.grid_y - 1) * L < nvec, "%d column tiles of %d vectors, %d vectors", q.grid_y,
                L, nvec);
    }
    REQUIRE(q.comb_blocks >= 1 && q.comb_blocks <= (unsigned)GN_COMB_BLOCKS && (long long)q.comb_blocks <= (long long)m.B * G, "%u combine blocks",
            q.comb_blocks);
    // partials [rows][2][C], then the group sums [B G][2]: disjoint, inside the bytes the size function promises
    const size_t ws = gn_plan_workspace_bytes(m.B, m.H, m.W, C, G);
    REQUIRE((size_t)q.rows * 2 * C <= q.off_ab && q.off_ab % 4 == 0 && q.elems == q.off_ab + (size_t)m.B * G * 2 && q.elems * 4 <= ws,
            "partials end at %zu, group sums at %zu .. %zu, the workspace holds %zu", (size_t)q.rows * 2 * C, q.off_ab, q.elems, ws / 4);
}
static void check_gn_at(const Map& m, int C, int G, const Etype& e, bool nchw) {
    char b[160];
    std::snprintf(b, sizeof(b), "gn_act B=%d H=%d W=%d C=%d G=%d %s %s", m.B, m.H, m.W, C, G, e.name, nchw ? "nchw" : "cl");
    g_where = b;
    REQUIRE(gn_shape_ok(m.B, m.H, m.W, C, G), "gn_shape_ok refuses an admitted shape");
    check_gn(gn_plan(m.B, m.H, m.W, C, G, e.esize, nchw), m, C, G, e);
}
static long long sweep_gn() {
    long long n = 0;
    for (const Map& m : MAPS)
        for (int C = 4; C <= TRAIN_MAX_C; C += 4)
            for (const Etype& e : ETYPES)
                for (int nchw = 0; nchw < 2; ++nchw) {
                    int gs[16], ng = 0;
                    for (int G : GN_GS)
                        if (C % G == 0) gs[ng++] = G;
                    gs[ng++] = C, gs[ng++] = C / 4;
                    if (C % 6 == 0) gs[ng++] = C / 6;
                    if (C % 12 == 0) gs[ng++] = C / 12;
                    for (int i = 0; i < ng; ++i, ++n) check_gn_at(m, C, gs[i], e, nchw);
                }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- the sweeps
static void check_dwln(const Map& m, int C, const Etype& e) {
    DwlnPlan q, q64;
    REQUIRE(dwln_plan(m.B, m.H, m.W, C, e.f64, q) && dwln_plan(m.B, m.H, m.W, C, true, q64), "dwln_plan refuses an admitted shape");
    check_dwln(q, q64, m, C, e);
}
static long long sweep_maps() {
    long long n = 0;
    for (const Map& m : MAPS) {
        for (int C = 4; C <= TRAIN_MAX_C; C += 4)
            for (const Etype& e : ETYPES) {
                for (int nchw = 0; nchw < 2; ++nchw) {
                    for (int partials = 0; partials < 2; ++partials) {
                        where("lncf", m, C, e.name, nchw ? "nchw" : "cl");
                        check_lncf(lncf_plan(m.B, m.H, m.W, C, e.esize, e.f64, nchw, partials), m, C, e, partials);
                        ++n;
                    }
                    where("block_tail", m, C, e.name, nchw ? "nchw" : "cl");
                    check_bt(bt_plan(m.B, m.H, m.W, C, e.esize, nchw), m, C, e);
                    ++n;
                }
                if (e.esize == 2) continue;     // dwln has no half form
                where("dwln", m, C, e.name, "cl");
                check_dwln(m, C, e);
                ++n;
            }
    }
    return n;
}
static long long sweep_pw() {
    long long n = 0;
    for (int M : PW_M)
        for (int N = 4; N <= PW_MAX_H; N += 4)
            for (int esize : {4, 2}) {
                char b[96];
                std::snprintf(b, sizeof(b), "pw_mlp M=%d N=%d esize=%d", M, N, esize);
                g_where = b;
                // as the first sum [PW_ROWS][Hd = N] next to the narrowest second one, and as the second sum [PW_ROWS][Co = N] behind the widest first
                check_pw(pw_plan(M, N, esize), M, N, esize, 0, pw_plan_workspace_bytes(M, N, 4));
                check_pw(pw_plan(M, N, esize), M, N, esize, (size_t)PW_ROWS * PW_MAX_H, pw_plan_workspace_bytes(M, PW_MAX_H, N));
                n += 2;
            }
    return n;
}
// the size functions return 0 exactly where the shape is refused
static void check_sizes() {
    g_where = "workspace size functions";
    static const int CS[] = {-4, 0, 2, 4, 6, 8, 96, 2044, 2046, 2048, 2052, 4096};
    static const Map EDGE[] = {{0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {-1, 4, 4}, {1, 1, 1}, {2, 3, 7}, {1, 1, 2147483647}, {2, 1, 1073741824}, {2048, 1024, 1024},
                               {2047, 1024, 1024}};
    for (const Map& m : EDGE)
        for (int C : CS) {
            const bool ok = train_shape_ok(m.B, m.H, m.W, C);
            REQUIRE((lncf_plan_workspace_bytes(m.B, m.H, m.W, C) != 0) == ok && (bt_plan_workspace_bytes(m.B, m.H, m.W, C) != 0) == ok &&
                        (dwln_plan_workspace_bytes(m.B, m.H, m.W, C) != 0) == ok,
                    "B=%d H=%d W=%d C=%d: admitted %d", m.B, m.H, m.W, C, (int)ok);
        }
    static const int NS[] = {-4, 0, 2, 4, 6, 8, 8188, 8190, 8192, 8196};
    for (int M : {-1, 0, 1, 42, 2147483647})
        for (int Hd : NS)
            for (int Co : NS)
                REQUIRE((pw_plan_workspace_bytes(M, Hd, Co) != 0) == pw_shape_ok(M, Hd, Co), "M=%d Hd=%d Co=%d", M, Hd, Co);
    for (const Map& m : EDGE)
        for (int C : CS)
            for (int G : {-1, 0, 1, 3, 4, 5, 16, 96, 2048, 4096}) {
                const bool ok = train_shape_ok(m.B, m.H, m.W, C) && G >= 1 && G <= C && C % G == 0;
                REQUIRE(gn_shape_ok(m.B, m.H, m.W, C, G) == ok && (gn_plan_workspace_bytes(m.B, m.H, m.W, C, G) != 0) == ok, "B=%d H=%d W=%d C=%d G=%d: admitted %d",
                        m.B, m.H, m.W, C, G, (int)ok);
            }
}

// each condition once on a deliberately wrong plan: `what` must fail
template <typename F>
static void must_fail(const char* what, F&& f) {
    const int before = g_failures;
    g_quiet = true;
    f();
    g_quiet = false;
    if (g_failures == before) {
        std::printf("FAIL: the wrong plan \"%s\" passes\n", what);
        std::exit(1);
    }
}
static int check_that_conditions_bite() {
    const Map m{7, 300, 300};
    const Etype &f32 = ETYPES[0], &f16 = ETYPES[1], &f64 = ETYPES[3];
    const size_t pw_ws = pw_plan_workspace_bytes(65537, 192, 768);          // the plan under check is that of the second sum, Co = 768
    int n = 0;
    auto lncf = [&](const char* what, bool nchw, int C, auto&& spoil) {
        LncfPlan q = lncf_plan(m.B, m.H, m.W, C, 4, false, nchw, true);
        spoil(q);
        must_fail(what, [&] { check_lncf(q, m, C, f32, true); });
        ++n;
    };
    lncf("lncf: rows + 1", false, 96, [](LncfPlan& q) { q.rows = ++q.grid; });
    lncf("lncf: G halved", false, 96, [](LncfPlan& q) { --q.lg; });
    lncf("lncf: block of 320", false, 96, [](LncfPlan& q) { q.block = 320; });
    lncf("lncf: a tile less per image", true, 96, [](LncfPlan& q) { --q.per_image; });
    lncf("lncf: 33 channels per lane in registers", true, 264, [](LncfPlan& q) { q.family = LNCF_NCHW_REGS32; q.lds = 0; });
    lncf("lncf: dynamic LDS beyond 64 KiB", true, 2048, [](LncfPlan& q) { q.lds = LDS_MAX; });
    lncf("lncf: no room for the row of partials in LDS", false, 96, [](LncfPlan& q) { q.lds = 0; });
    lncf("lncf: a counter that wrapped", false, 96, [](LncfPlan& q) { q.units = 4000000000u; });
    auto bt = [&](const char* what, bool nchw, int C, const Etype& e, auto&& spoil) {
        BtPlan q = bt_plan(m.B, m.H, m.W, C, e.esize, nchw);
        spoil(q);
        must_fail(what, [&] { check_bt(q, m, C, e); });
        ++n;
    };
    bt("block_tail: rows + 1", false, 384, f32, [](BtPlan& q) { q.rows = ++q.grid_x; });
    bt("block_tail: PP + 1", false, 384, f32, [](BtPlan& q) { ++q.PP; });
    bt("block_tail: PP = 0", false, 2048, f32, [](BtPlan& q) { q.PP = 0; });
    bt("block_tail: V = 8 for fp32", false, 384, f32, [](BtPlan& q) { q.V = 8; q.CG = 48; });
    bt("block_tail: a chunk less per image", false, 384, f16, [](BtPlan& q) { --q.per_image; });
    bt("block_tail: a channel tile less", true, 1000, f32, [](BtPlan& q) { --q.grid_y; });
    bt("block_tail: grid.y beyond 65535", true, 1000, f32, [](BtPlan& q) { q.grid_y = 65536; });
    auto dwln = [&](const char* what, int C, const Etype& e, auto&& spoil) {
        DwlnPlan q, q64;
        dwln_plan(m.B, m.H, m.W, C, e.f64, q);
        dwln_plan(m.B, m.H, m.W, C, true, q64);
        spoil(q);
        must_fail(what, [&] { check_dwln(q, q64, m, C, e); });
        ++n;
    };
    dwln("dwln: rows + 1", 96, f64, [](DwlnPlan& q) { ++q.RA; });
    dwln("dwln: NS + 1", 96, f32, [](DwlnPlan& q) { ++q.NS; q.threads += q.CGp; });
    dwln("dwln: NS = 0", 2048, f32, [](DwlnPlan& q) { q.NS = q.threads = 0; });
    dwln("dwln: pass A partials inside du", 96, f32, [](DwlnPlan& q) { q.off_pa -= 64; });
    dwln("dwln: pass B partials inside those of pass A", 96, f32, [](DwlnPlan& q) { q.off_pb -= 64; });
    dwln("dwln: a block more in the weight pass of the fp64 form", 96, f64, [](DwlnPlan& q) { ++q.RB; });
    dwln("dwln: strips longer than DWLN_DW_STRIP", 96, f32, [](DwlnPlan& q) { q.slen = 150; q.segs_w = 2; });
    auto pw = [&](const char* what, size_t off, auto&& spoil) {
        PwPlan q = pw_plan(65537, 768, 4);
        spoil(q);
        must_fail(what, [&] { check_pw(q, 65537, 768, 4, off, pw_ws); });
        ++n;
    };
    const size_t second = (size_t)PW_ROWS * 192;
    pw("pw_mlp: rows + 1", second, [](PwPlan& q) { q.rows = ++q.grid_y; });
    pw("pw_mlp: L halved", second, [](PwPlan& q) { --q.lg; });
    pw("pw_mlp: a column tile less", second, [](PwPlan& q) { --q.grid_x; });
    pw("pw_mlp: the second sum a row late", second + 768, [](PwPlan&) {});
    auto gn = [&](const char* what, const Map& gm, bool nchw, int C, int G, auto&& spoil) {
        GnPlan q = gn_plan(gm.B, gm.H, gm.W, C, G, 4, nchw);
        spoil(q);
        must_fail(what, [&] { check_gn(q, gm, C, G, f32); });
        ++n;
    };
    const Map one{3, 1, 1};
    gn("gn_act: a row more per image", m, false, 96, 16, [](GnPlan& q) { ++q.rpi; });
    gn("gn_act: rows + 1", m, false, 96, 16, [](GnPlan& q) { q.grid_x = ++q.rows; });
    gn("gn_act: a unit less per image", m, true, 96, 16, [](GnPlan& q) { --q.upi; });
    gn("gn_act: units of 8 pixels", m, false, 96, 16, [](GnPlan& q) { q.unit = 8; q.upi = 11250; });
    gn("gn_act: two planes in a map of one pixel", one, false, 96, 16, [](GnPlan& q) { q.planes = 2; });
    gn("gn_act: a column tile less", m, false, 1000, 5, [](GnPlan& q) { --q.grid_y; });
    gn("gn_act: a channel tile less", m, true, 1000, 5, [](GnPlan& q) { --q.grid_y; });
    gn("gn_act: V = 8 for fp32", m, false, 96, 16, [](GnPlan& q) { q.V = 8; });
    gn("gn_act: the group sums inside the partials", m, false, 96, 16, [](GnPlan& q) { q.off_ab -= 64; });
    gn("gn_act: more combine blocks than pairs", one, false, 96, 1, [](GnPlan& q) { q.comb_blocks = 4; });
    gn("gn_act: block of 512", m, true, 96, 16, [](GnPlan& q) { q.block = 512; });
    g_where = "";
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- --list
static int list() {
    const Map m{1, 1, 1};                       // the class depends on C, the layout and the element type alone
    char cls[64];
    for (const Etype& e : ETYPES)
        for (int nchw = 0; nchw < 2; ++nchw)
            for (int C = 4; C <= TRAIN_MAX_C; C += 4) {
                lncf_plan_class(lncf_plan(m.B, m.H, m.W, C, e.esize, e.f64, nchw, false), e.name, cls, sizeof(cls));
                std::printf("lncf %s %s %d | %s\n", nchw ? "nchw" : "cl", e.name, C, cls);
                const BtPlan b = bt_plan(m.B, m.H, m.W, C, e.esize, nchw);
                bt_plan_class(b, e.name, cls, sizeof(cls));
                std::printf("block_tail %s %s %d | %s | PP=%d block=%d\n", nchw ? "nchw" : "cl", e.name, C, cls, b.PP, b.block);
            }
    for (const Etype& e : ETYPES) {
        if (e.esize == 2) continue;
        for (int C = 4; C <= TRAIN_MAX_C; C += 4) {
            DwlnPlan q;
            dwln_plan(m.B, m.H, m.W, C, e.f64, q);
            dwln_plan_class(q, e.name, cls, sizeof(cls));
            std::printf("dwln - %s %d | %s\n", e.name, C, cls);
        }
    }
    for (const Etype& e : ETYPES)
        for (int N = 4; N <= PW_MAX_H; N += 4) {
            const PwPlan q = pw_plan(1, N, e.esize);
            pw_plan_class(q, e.name, cls, sizeof(cls));
            // at M = 1: gx column tiles of L vectors; idle = the vector slots of those tiles that no vector fills
            std::printf("pw_mlp - %s %d | %s | L=%d gx=%d idle=%d\n", e.name, N, cls, 1 << q.lg, q.grid_x, (q.grid_x << q.lg) - N / q.V);
        }
    std::printf("limits | TRAIN_MAX_C=%d TRAIN_ROWS=%d PW_MAX_H=%d PW_ROWS=%d\n", TRAIN_MAX_C, TRAIN_ROWS, PW_MAX_H, PW_ROWS);
    // gn_act: the class depends on C, the layout and the element type alone; G = 4 divides every C.  ws = the workspace bytes of the parity map
    // (2, 9, 7) at G = 4, gy = column (channel) tiles, unit = the most pixels of a unit (what a map of TRAIN_ROWS such units or more takes)
    for (const Etype& e : ETYPES)
        for (int nchw = 0; nchw < 2; ++nchw)
            for (int C = 4; C <= TRAIN_MAX_C; C += 4) {
                const GnPlan q = gn_plan(2, 9, 7, C, 4, e.esize, nchw);
                gn_plan_class(q, e.name, cls, sizeof(cls));
                std::printf("gn_act %s %s %d | %s | gy=%d unit=%d ws=%zu\n", nchw ? "nchw" : "cl", e.name, C, cls, q.grid_y, nchw ? GN_UNIT_NCHW : GN_UNIT_CL,
                            gn_plan_workspace_bytes(2, 9, 7, C, 4));
            }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) return list();
    if (argc != 1) {
        std::printf("usage: %s [--list]\n", argv[0]);
        return 2;
    }
    const long long maps = sweep_maps();
    std::printf("lncf, block_tail, dwln: %lld plans over %zu maps x C = 4, 8, ..., %d x every element type and layout\n", maps, sizeof(MAPS) / sizeof(MAPS[0]),
                TRAIN_MAX_C);
    const long long pw = sweep_pw();
    std::printf("pw_mlp: %lld plans over %zu row counts x N = 4, 8, ..., %d x both vector widths, as the first and as the second sum\n", pw,
                sizeof(PW_M) / sizeof(PW_M[0]), PW_MAX_H);
    const long long gn = sweep_gn();
    std::printf("gn_act: %lld plans over the same maps, widths, element types and layouts x G = 1, 2, 4, 16, 32, C, C / 4, C / 6, C / 12 where they divide C\n", gn);
    check_sizes();
    std::printf("workspace sizes: 0 exactly where train_shape_ok / pw_shape_ok / gn_shape_ok refuses\n");
    std::printf("each condition bites: %d deliberately wrong plans refused\n", check_that_conditions_bite());
    std::printf("train_plan_check: OK\n");
    return 0;
}
