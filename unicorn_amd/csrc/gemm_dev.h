// Device primitives of the MFMA GEMM units (gemm.hip, gemm_h2.hip, gemm_h2d.hip, gemm_h2q.hip, gemm_p44.hip) and the A side of
// their implicit GEMMs, each stated once.  The integer index arithmetic they rest on is tile_index.h.
#pragma once
#include "kernels.h"
#include "tile_index.h"

#define UNI_AS1 __attribute__((address_space(1)))
#define UNI_AS3 __attribute__((address_space(3)))

// ---- LDS-DMA, 16 bytes per lane: global -> LDS without a VGPR round trip; the LDS side is lane-linear (lptr + lane * 16)
__device__ __forceinline__ void lds_dma16(const void* gptr, void* lptr) {      // global_load_lds_dwordx4
    __builtin_amdgcn_global_load_lds((const UNI_AS1 void*)(gptr), (UNI_AS3 void*)(lptr), 16, 0, 0);
}
// buffer_load_dwordx4 ... lds: descriptor + per-lane offset + scalar offset; an offset beyond num_records reads zeros.  (Arguments in the
// builtin's order: the order in which a caller's argument expressions are evaluated reaches the instruction schedule.)
__device__ __forceinline__ void lds_dma16_buf(__amdgpu_buffer_rsrc_t rs, void* lptr, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (UNI_AS3 void*)(lptr), 16, voff, soff, 0, 0);
}
// ds_read_b128 from a 32-bit LDS address
__device__ __forceinline__ f16x8 lds_read_f16x8(int addr) { return *reinterpret_cast<const UNI_AS3 f16x8*>((size_t)(addr)); }
// counted wait: at most N vector-memory requests of this wave stay in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// hides a 64-bit value from the optimiser: keeps ONE DMA per piece (hipcc otherwise splits the select in front of it into exec-masked branches)
__device__ __forceinline__ void opaque64(long& x) {
    int lo = (int)x, hi = (int)(x >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    x = ((long)hi << 32) | (unsigned)lo;
}
// zeroes the accumulators f32x16 acc[TM][TN].  A macro: through a function that takes the array by reference hipcc schedules the kernels
// differently (tools/kernel_diff.py, profiles/gemm_shared_index.txt).
#define ACC_CLEAR(acc, TM, TN)                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < (TM); ++i_)                   \
        _Pragma("unroll") for (int j_ = 0; j_ < (TN); ++j_)               \
            _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) acc[i_][j_][r_] = 0.f

// ---- the two raw workgroup barriers of the counted-vmcnt kernels.  They differ on purpose.
// gemm_h2d.hip: the K step's order is pinned by the sched_barriers of the loop body itself, so the barrier only has to keep the
// IR optimiser from moving memory accesses across it.
__device__ __forceinline__ void d_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// gemm_h2q.hip: a phase IS what stands between two barriers (the other wave group issues its MFMAs meanwhile), so neither the IR
// optimiser nor the machine scheduler may move anything across it.
__device__ __forceinline__ void phase_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
}

// ---- implicit-GEMM A side, direct addressing (gemm_bf16_kernel, gemm_f32_kernel, gemm_h2_kernel): every lane computes the address of its
// 16 bytes per K step.  The output pixel of GEMM row m travels as one packed word (tile_index.h: pixel_pack).
__device__ __forceinline__ int conv_pixel(const GemmArgs& p, int m) {
    int b = m / p.Mper, q = m - b * p.Mper;        // sample, pixel within the sample
    int oy = q / p.Wout, ox = q - oy * p.Wout;
    return pixel_pack(b, oy, ox);
}
// byte offset from A of channel c of the input pixel that tap (ky, kx) of output pixel `pix` reads; EB = bytes per element, half = 1 for the
// lo halves of an f16x2 group, 16 bytes behind the hi halves (0 for the other formats); zoff (the zero page) outside the image or past K
template <int EB>
__device__ __forceinline__ long conv_src_offset(const GemmArgs& p, int pix, int ky, int kx, int c, bool kok, int half, long zoff) {
    int bb = pixel_sample(pix), oy = pixel_oy(pix), ox = pixel_ox(pix);
    int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
    bool ok = kok && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
    return ok ? (long)(((size_t)((bb * p.Hin + iy) * p.Win + ix) * p.lda + c) * EB + half * 16) : zoff;
}

// ---- implicit-GEMM A side, descriptor addressing (gemm_h2d_kernel, gemm_h2q_kernel; Cin a multiple of the k of a step, so a K step is a
// channel block of ONE tap).  One buffer descriptor per row tile starts (pad, pad) pixels before the tile's first input pixel; the per-lane
// word is the lane's pixel relative to that as a byte offset (< 2^26, the launchers check) | 6 validity bits << 26: bit ky = input row of
// tap row ky inside the image, bit 3 + kx the same for the column, all clear for a row past M.  The tap (ky, kx) and the channel block
// travel in the scalar offset ((ky Win + kx) lda + c, never negative; the decode of a K step: tile_index.h, tap_*), and a lane whose tap
// falls outside the image or whose row is past M presents an offset beyond num_records: the buffer load returns zeros, which IS the
// zero padding.  The two kernels build descriptor and words with the same statements, each in its own text: moved into functions
// here, hipcc orders the prologue of every implicit-GEMM build of both kernels differently (profiles/gemm_shared_index.txt).
constexpr int DESC_OFFSET_MASK = 0x03ffffff, DESC_OUT_OF_RANGE = 0x7fffffff;      // the word's offset bits; a per-lane offset beyond num_records
