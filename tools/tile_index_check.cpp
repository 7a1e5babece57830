// Exhaustive host check of unicorn_amd/csrc/tile_index.h: every index function over its stated domain.  Plain C++ (built by
// unicorn_amd/csrc/build.sh into tools/build/tile_index_check, run by tests/test_tile_order_cpu.py).  Exits non-zero with the first
// counter-example.
#include "../unicorn_amd/csrc/tile_index.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define FAIL(...)                         \
    do {                                  \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");                \
        std::exit(1);                     \
    } while (0)

// xcd_remap: a bijection of [0, n) for every grid size; the blocks with equal b % 8 get one contiguous range, range sizes differ by <= 1
static void check_remap() {
    for (int n = 1; n <= 700; ++n) {
        std::vector<int> hit(n, 0);
        int lo[8], hi[8], cnt[8] = {0};
        for (int b = 0; b < n; ++b) {
            const int L = xcd_remap(b, n), x = b & 7;
            if (L < 0 || L >= n || hit[L]++) FAIL("xcd_remap(%d, %d) = %d: outside [0, n) or taken twice", b, n, L);
            lo[x] = cnt[x] ? (L < lo[x] ? L : lo[x]) : L;
            hi[x] = cnt[x] ? (L > hi[x] ? L : hi[x]) : L;
            ++cnt[x];
        }
        int cmin = n, cmax = 0;
        for (int x = 0; x < 8; ++x) {
            if (cnt[x] && hi[x] - lo[x] + 1 != cnt[x]) FAIL("xcd_remap: n = %d, XCD %d: %d blocks in [%d, %d], not contiguous", n, x, cnt[x], lo[x], hi[x]);
            cmin = cnt[x] < cmin ? cnt[x] : cmin;
            cmax = cnt[x] > cmax ? cnt[x] : cmax;
        }
        if (cmax - cmin > 1) FAIL("xcd_remap: n = %d: range sizes %d .. %d", n, cmin, cmax);
    }
    std::printf("xcd_remap: bijection, XCD-contiguous, balanced for every grid 1..700\n");
}

// persistent_units: grids that are multiples of 8 (launch_gemm_h2q and launch_gemm_p44 round theirs, the dwconv7_lnb launch uses 256), 0..400 units: covered once
static void check_persistent() {
    for (int n = 8; n <= 320; n += 8)
        for (int units = 0; units <= 400; ++units) {
            std::vector<int> hit(units, 0);
            for (int b = 0; b < n; ++b) {
                struct { int first, stride, count; } u;
                persistent_units(b, n, units, u.first, u.stride, u.count);
                if (u.count < 0 || u.stride != n / 8) FAIL("persistent_units(%d, %d, %d): count %d stride %d", b, n, units, u.count, u.stride);
                for (int t = 0; t < u.count; ++t) {
                    const int w = u.first + t * u.stride;
                    if (w < 0 || w >= units || hit[w]++) FAIL("persistent_units(%d, %d, %d): unit %d outside [0, units) or taken twice", b, n, units, w);
                }
            }
            for (int w = 0; w < units; ++w)
                if (!hit[w]) FAIL("persistent_units: grid %d, %d units: unit %d is nobody's", n, units, w);
        }
    std::printf("persistent_units: every unit exactly once for grids 8..320 (multiples of 8) x 0..400 units\n");
}

static void check_supertile() {
    for (int nbm = 1; nbm <= 40; ++nbm)
        for (int nbn = 1; nbn <= 40; ++nbn) {
            std::vector<int> hit(nbm * nbn, 0);
            for (int L = 0; L < nbm * nbn; ++L) {
                const TilePos t = supertile_pos(L, nbm, nbn);
                if (t.bm < 0 || t.bm >= nbm || t.bn < 0 || t.bn >= nbn || hit[t.bm * nbn + t.bn]++)
                    FAIL("supertile_pos(%d, %d, %d) = (%d, %d): outside the grid or taken twice", L, nbm, nbn, t.bm, t.bn);
                const TilePos s = supertile_pos(L, nbm, nbn, 256, 192);
                if (s.bm != t.bm * 256 || s.bn != t.bn * 192) FAIL("supertile_pos(%d, %d, %d, 256, 192): not the scaled position", L, nbm, nbn);
            }
            for (int splits = 1; splits <= 4; ++splits) {
                std::vector<int> h2(splits * nbm * nbn, 0);
                for (int u = 0; u < splits * nbm * nbn; ++u) {
                    const SplitTilePos t = supertile_split_pos(u, nbm, nbn);
                    const TilePos ref = supertile_pos(u % (nbm * nbn), nbm, nbn);
                    if (t.split != u / (nbm * nbn) || t.bm != ref.bm || t.bn != ref.bn || h2[(t.split * nbm + t.bm) * nbn + t.bn]++)
                        FAIL("supertile_split_pos(%d, %d, %d) = (%d, %d, %d)", u, nbm, nbn, t.split, t.bm, t.bn);
                }
            }
        }
    std::printf("supertile_pos: bijection onto nbm x nbn for nbm, nbn in 1..40; supertile_split_pos onto (split, tile) for 1..4 splits\n");
}

static void check_splitk() {
    for (int nk = 1; nk <= 300; ++nk)
        for (int sk = 2; sk <= 16; ++sk) {
            int next = 0;
            for (int y = 0; y < sk; ++y) {
                const KRange r = splitk_range(nk, sk, y);
                if (r.kt0 < r.nk) {      // not empty
                    if (r.kt0 != next || r.nk > nk) FAIL("splitk_range(%d, %d, %d) = [%d, %d): expected to start at %d", nk, sk, y, r.kt0, r.nk, next);
                    next = r.nk;
                } else if (next != nk) {
                    FAIL("splitk_range(%d, %d, %d): empty range [%d, %d) before the K steps are used up (%d)", nk, sk, y, r.kt0, r.nk, next);
                }
            }
            if (next != nk) FAIL("splitk_range: nk = %d, splitk = %d: the ranges end at %d", nk, sk, next);
        }
    std::printf("splitk_range: the ranges tile [0, nk) in order for nk in 1..300, splitk in 2..16\n");
}

// first K step < 9 cs that the multiplications decode differently from / and %, or -1
static int tap_counter_example(int cs, int KW) {
    for (int kt = 0; kt < 9 * cs; ++kt) {
        const Tap t = tap_of(kt, cs, KW);
        const int tap = kt / cs;
        if (t.tap != tap || t.cstep != kt % cs || t.ky != tap / KW || t.kx != tap % KW) return kt;
    }
    return -1;
}
static void check_tap() {
    for (int KW = 1; KW <= 3; ++KW)
        for (int cs = 1; cs <= TAP_DECODE_MAX_CS; ++cs) {
            const int kt = tap_counter_example(cs, KW);
            if (kt >= 0) FAIL("tap_of: cs = %d, KW = %d, K step %d is not decoded as / and %% do", cs, KW, kt);
        }
    const int kt = tap_counter_example(TAP_DECODE_MAX_CS + 1, 3);
    if (kt < 0) FAIL("tap_of is exact at cs = %d too: TAP_DECODE_MAX_CS is not the largest exact bound", TAP_DECODE_MAX_CS + 1);
    const Tap t = tap_of(kt, TAP_DECODE_MAX_CS + 1, 3);
    std::printf("tap_of: equal to / and %% for KW in 1..3, cs in 1..%d, every K step < 9 cs; proved bound TAP_DECODE_MAX_CS = %d\n", TAP_DECODE_MAX_CS,
                TAP_DECODE_MAX_CS);
    std::printf("tap_of: cs = %d, K step %d decodes as tap %d, channel step %d (true: tap %d, step %d)\n", TAP_DECODE_MAX_CS + 1, kt, t.tap, t.cstep,
                kt / (TAP_DECODE_MAX_CS + 1), kt % (TAP_DECODE_MAX_CS + 1));
}

static void check_pixel() {
    const int bs[] = {0, 1, 63, 126, 127}, cs[] = {0, 1, 2047, 2048, 4094, 4095};      // launch_gemm: M / Mper < 128; Wout < 4096, Mper / Wout < 4096
    for (int b : bs)
        for (int oy : cs)
            for (int ox : cs) {
                const int w = pixel_pack(b, oy, ox);
                if (w < 0 || pixel_sample(w) != b || pixel_oy(w) != oy || pixel_ox(w) != ox) FAIL("pixel word of (%d, %d, %d) = %d does not round-trip", b, oy, ox, w);
            }
    std::printf("pixel_pack: round trip at the extremes (sample 0..127, oy / ox 0..4095)\n");
}

int main() {
    check_remap();
    check_persistent();
    check_supertile();
    check_splitk();
    check_tap();
    check_pixel();
    std::printf("tile_index_check: OK\n");
    return 0;
}
