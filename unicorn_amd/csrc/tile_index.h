// Integer index arithmetic shared by the GEMM kernels (gemm*.hip) and the strip kernels of norm.hip: which tile a block works on,
// which K steps, which filter tap a K step belongs to.  Plain integers only, so the same text compiles for the device, for the host
// launchers and for tools/tile_index_check.cpp, which checks every function below over its stated domain by exhaustion
// (tests/test_tile_order_cpu.py runs it).
#pragma once

#if defined(__HIPCC__)
#define UNI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UNI_HD inline
#endif

// ---- block -> position.  Block b of a grid runs on XCD b % 8 (private L2).  xcd_remap is a bijection of [0, nwg) that gives the blocks of
// one XCD (equal b % 8) one contiguous range of positions; the eight range sizes differ by at most one.  Domain: nwg >= 1, 0 <= b < nwg.
UNI_HD int xcd_remap(int b, int nwg) {
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// ---- persistent form: the work units first, first + stride, ... (count of them) of block b.  The units are cut into eight XCD-contiguous
// ranges as above and the nwg / 8 blocks of an XCD walk their range round-robin, so over all blocks every unit of [0, units) is taken
// exactly once.  Domain: nwg a positive multiple of 8 (the launchers round their grids to it), 0 <= b < nwg, units >= 0.
// (Results through references: returned as a struct, the values are packed and unpacked again and reach hipcc's scheduler in another order.)
UNI_HD void persistent_units(int b, int nwg, int units, int& first, int& stride, int& count) {
    const int x = b & 7, slot = (int)((unsigned)b >> 3), nslots = (int)((unsigned)nwg >> 3);      // (the unsigned shifts of blockIdx / gridDim)
    const int q = units >> 3, r = units & 7;
    const int start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    const int cnt = q + (x < r ? 1 : 0);
    first = start + slot;
    stride = nslots;
    count = slot < cnt ? (cnt - slot + nslots - 1) / nslots : 0;
}

// ---- position -> tile, L2-friendly: N is cut into chunks of 8 tiles and inside a chunk the tiles run M-major, so the ~64 blocks resident
// on one XCD form an (8 M panels x 8 N tiles) super-tile that shares 16 operand K slices per step.  A bijection of [0, nbm nbn) onto
// nbm x nbn.  (sm, sn) scale the result: tile indices by default, the tile's first row / column with the tile shape (BM, BN).
// Domain: nbm, nbn >= 1, 0 <= L < nbm nbn.
struct TilePos { int bm, bn; };
UNI_HD TilePos supertile_pos(int L, int nbm, int nbn, int sm = 1, int sn = 1) {
    constexpr int GN = 8;
    const int per_chunk = nbm * GN;
    const int c = L / per_chunk;
    const int left = nbn - c * GN, wc = GN < left ? GN : left;
    const int rem = L - c * per_chunk;
    const int bm = rem / wc;
    return {bm * sm, (c * GN + rem - bm * wc) * sn};
}
// work unit u of a split-K launch = (K range u / ntiles, tile u % ntiles): neighbouring units are different tiles of the same K range
// (shared operand panels).  Domain: 0 <= u < splits nbm nbn.
struct SplitTilePos { int split, bm, bn; };
UNI_HD SplitTilePos supertile_split_pos(int u, int nbm, int nbn, int sm = 1, int sn = 1) {
    const int ntiles = nbm * nbn;
    const int split = u / ntiles;
    const TilePos t = supertile_pos(u - split * ntiles, nbm, nbn, sm, sn);
    return {split, t.bm, t.bn};
}

// ---- split-K: the K steps [kt0, nk) of range y out of `splitk`.  The ranges tile [0, nk) in order; the last ones may be empty
// (kt0 >= nk).  Domain: nk >= 1, splitk >= 2, 0 <= y < splitk.
struct KRange { int kt0, nk; };
UNI_HD KRange splitk_range(int nk, int splitk, int y) {
    const int per = (nk + splitk - 1) / splitk;
    const int kt0 = y * per, end = kt0 + per;
    return {kt0, nk < end ? nk : end};
}

// ---- tap decode of the descriptor-addressed implicit GEMMs (gemm_h2d.hip, gemm_h2q.hip): a K step kt covers the channels
// [cstep ks, (cstep + 1) ks) of ONE filter tap (ky, kx), cs = Cin / ks steps per tap, kt = tap cs + cstep.  The kernels divide by
// multiplication: tap = (kt csm) >> 16 with csm = 65536 / cs + 1, ky = (tap kwm) >> 5.  Domain: 1 <= KW <= 3, tap < 9 (at most 3 x 3 taps),
// 1 <= cs <= TAP_DECODE_MAX_CS, 0 <= kt < 9 cs.  TAP_DECODE_MAX_CS is the largest cs such that the decode equals / and % for every
// cs' <= cs over that range (at cs = 103 step 9 * 103 - 1 decodes as tap 9, channel step -1); the launchers refuse wider inputs.
constexpr int TAP_DECODE_MAX_CS = 102;
UNI_HD int tap_csm(int cs) { return 65536 / cs + 1; }                       // kt / cs = (kt * csm) >> 16
UNI_HD int tap_kwm(int KW) { return KW == 3 ? 11 : KW == 2 ? 16 : 32; }     // tap / KW = (tap * kwm) >> 5
UNI_HD int tap_index(int kt, int csm) { return (kt * csm) >> 16; }
UNI_HD int tap_row(int tap, int kwm) { return (tap * kwm) >> 5; }
// the whole decode, as the kernels compose it from the four functions above (scalar pieces: through a struct the kernels' code moves)
struct Tap { int tap, cstep, ky, kx; };
UNI_HD Tap tap_of(int kt, int cs, int KW) {
    const int tap = tap_index(kt, tap_csm(cs)), cstep = kt - tap * cs;
    const int ky = tap_row(tap, tap_kwm(KW)), kx = tap - ky * KW;
    return {tap, cstep, ky, kx};
}

// ---- output pixel of the direct-addressed implicit GEMMs (gemm.hip, gemm_h2.hip) in one register: sample (8 bits) | oy (12) | ox (12).
// Domain: 0 <= b < 128 (launch_gemm: M / Mper < 128; the word stays positive), 0 <= oy, ox < 4096 (the launchers: Wout < 4096,
// Mper / Wout < 4096).
UNI_HD int pixel_pack(int b, int oy, int ox) { return (b << 24) | (oy << 12) | ox; }
UNI_HD int pixel_sample(int w) { return w >> 24; }
UNI_HD int pixel_oy(int w) { return (w >> 12) & 0xfff; }
UNI_HD int pixel_ox(int w) { return w & 0xfff; }
