// Internal launcher interface between the HIP kernels (*.hip) and the engine / C-ABI (engine.hip, api.hip).
#pragma once
#include "common.h"

// ---------------------------------------------------------------- gemm.hip
struct GemmArgs {
    const bf16* A = nullptr; int lda = 0;     // NHWC bf16 activations, lda = elements per pixel row
    const bf16* W = nullptr;                  // packed [Npad][Kpad] bf16
    int M = 0, N = 0, K = 0, Kpad = 0;
    // conv geometry (1x1/s1/p0 => plain GEMM)
    int Hin = 0, Win = 0, Cin = 0, KH = 1, KW = 1, stride = 1, pad = 0, Wout = 0;
    int Mper = 0;                             // output pixels per sample (M = B * Mper); GN stats slot b lives at stats + 64*b
    int out_hw = 0, out_stride = 0, out_off = 0;   // optional outF row remap: (row/out_hw)*out_stride + out_off + row%out_hw
    // epilogue
    const float* bias = nullptr;              // [N]
    int act = ACT_NONE; int act_col0 = 0;     // activation on columns >= act_col0
    const float* res = nullptr; int ldr = 0;  // fp32 residual added after the activation
    float* outF = nullptr; int ldf = 0;
    bf16* outB = nullptr; int ldb = 0;
    double* stats = nullptr; int cpg = 0;     // GroupNorm group sums [G][2] of (acc+bias), cpg = channels/group
    int force_cfg = 0;                        // 0 = heuristic, else 22 / 12 / 21 / 11
    int b32 = 0;                              // operand format (ActFmt): FMT_BF16, FMT_F32 (A, W, outB fp32; v_mfma_f32_32x32x2_f32) or FMT_H2 (split f16, gemm_h2.hip)
    float wscale = 1.f;                       // FMT_H2: the packed weights carry a power-of-two scale; the accumulator is multiplied by wscale
    // FMT_H2, single-frame problems (few tiles): splitk > 1 cuts the K loop into `splitk` ranges (gridDim.y); every range stores its partial
    // tile into slab [splitk][M][N] fp32 and a reduce kernel (launched by launch_gemm_h2) sums the ranges and applies bias / residual /
    // GroupNorm sums -> outF.  No activation, no operand-format output in this mode.
    int splitk = 0; float* slab = nullptr;
    int dbg = 0;                              // ablation switches for tools/gemm_bench.py (1 = no DMA after tile 0, 2 = no MFMA)
    int epi = 0;                              // set by launch_gemm: 1 = LDS-staged, row-coalesced epilogue stores
};
// implicit GEMM (gathered A operand) as opposed to a plain one (1x1 / stride 1 / no padding)
static inline bool gemm_is_conv(const GemmArgs& a) { return a.KH != 1 || a.KW != 1 || a.stride != 1 || a.pad != 0; }
// variant trace tag of one GEMM launch (common.h: uni_variant_note).  family = the kernel, cfg = its tile configuration; then every
// launch-uniform switch that changes index arithmetic or the store path: implicit conv, GroupNorm statistics, K ranges, staged epilogue,
// which outputs exist, residual, activation (+ column window), outF row remap, stacked samples.
static inline void uni_note_gemm(const char* family, int cfg, bool conv, bool stats, const GemmArgs& a) {
    if (!g_uni_variant_trace.load(std::memory_order_relaxed)) return;
    uni_variant_record("gemm:%s cfg=%d fmt=%s conv=%d stats=%d splitk=%d epi=%d outF=%d outB=%d res=%d act=%d%s remap=%d stacked=%d", family, cfg,
                       uni_fmt_name(a.b32), (int)conv, (int)stats, a.splitk > 1 ? 1 : 0, a.epi, a.outF != nullptr, a.outB != nullptr,
                       a.res != nullptr, a.act, a.act_col0 ? "w" : "", a.out_hw != 0, a.Mper > 0 && a.M != a.Mper);
}
int launch_gemm(const GemmArgs& a, hipStream_t s);
int launch_gemm_h2(const GemmArgs& a, hipStream_t s);     // gemm_h2.hip (reached through launch_gemm when a.b32 == FMT_H2)
uint16_t f32_to_f16_host(float f);
float f16_to_f32_host(uint16_t h);
float h2_weight_scale(float maxabs);
void pack_weight_h2_host(const float* w, int N, int Cin, int KH, int KW, const float* row_scale, float scale, uint16_t* out,
                         int Npad, int Kpad);
int launch_gemm_p44(const GemmArgs& a, hipStream_t s);    // gemm_p44.hip: persistent 256x256 tiles (bf16), next tile prefetched before the drain
bool gemm_p44_supported(const GemmArgs& a);
// deep-pipeline 4-wave tiles for launches with <= ~1 block per CU (gemm_h2d.hip); cfg 322 / 323 / 321 / 312 / 311
bool gemm_h2d_has_cfg(int cfg);
bool gemm_h2d_supported(const GemmArgs& a, int cfg);
int gemm_h2d_choice(const GemmArgs& a);      // 0 or the deep tile configuration the launcher takes for this problem
int launch_gemm_h2d(const GemmArgs& a, int cfg, bool conv, hipStream_t s);
GemmArgs gemm_splitk_partial_args(const GemmArgs& a);    // the launch that fills the slab: fp32 partial tiles only (no bias / residual / statistics / remap)
int launch_splitk_reduce(const GemmArgs& a, hipStream_t s);
int launch_gemm_h2q(const GemmArgs& a, hipStream_t s);    // gemm_h2q.hip: persistent 256x256, two wave groups ping-pong MFMA / LDS phases, counted-vmcnt DMA stream
bool gemm_h2q_supported(const GemmArgs& a);

// ---------------------------------------------------------------- mlp_fused.hip
// Fused ConvNeXt MLP (pwconv1 -> GELU -> pwconv2 (gamma folded) -> + residual), f16x2 operands, hidden kept in registers
struct MlpArgs {
    const void* A = nullptr; int lda = 0;     // [M][C] f16x2 operand rows (dwconv7 + LayerNorm output)
    const void* blob = nullptr;               // weight stream of mlp_pack_host (mlp_blob_bytes(C) bytes)
    const float* b1 = nullptr;                // [4C]
    const float* b2 = nullptr;                // [C], layer scale folded in
    float ws1 = 1.f, ws2 = 1.f;               // accumulator factors (1 / power-of-two weight scale)
    const float* res = nullptr; int ldr = 0;  // fp32 residual rows (may alias out)
    float* out = nullptr; int ldo = 0;        // fp32 [M][C]
    void* outB = nullptr; int ldb = 0;        // optional f16x2 copy of the result
    int M = 0, C = 0;
    int layout = 0;                           // 0: 32-row waves (4 per block, blob of mlp_pack_host); 1: 16-row waves (8 per block, mlp_pack16_host)
};
int launch_mlp_fused(const MlpArgs& a, hipStream_t s);
bool mlp_fused_supported(int C);
size_t mlp_blob_bytes(int C);
void mlp_pack_host(const float* w1, const float* w2, const float* gamma, int C, uint16_t* out, float* ws1, float* ws2);
void mlp_pack16_host(const float* w1, const float* w2, const float* gamma, int C, uint16_t* out, float* ws1, float* ws2);
bool mlp_fused16_supported(int C);

// ---------------------------------------------------------------- norm.hip
// Row LayerNorm over C (biased var, eps inside sqrt): fp32 [M][ldx] -> bf16 and/or fp32.
struct LnArgs {
    const float* x = nullptr; int ldx = 0;
    const float* gamma = nullptr; const float* beta = nullptr; float eps = 1e-6f;
    int M = 0, C = 0;
    float* outF = nullptr; int ldf = 0;
    bf16* outB = nullptr; int ldb = 0;
    // optional PixelShuffle(2) scatter of the bf16 output (unicorn.py:41): row=(y,x) of an (h,w) map,
    // channel c -> pixel (2y+dy, 2x+dx), channel c/4 of a (2h,2w,C/4) map
    int ps_h = 0, ps_w = 0;
    int b32 = 0;                              // outB holds fp32 instead of bf16
    // optional fp32 row remap of the interaction stage: rows are tokens [B][2 frames][pair_hw]; frame 0 rows go to outF, frame 1 rows to
    // outF2, both as [B][pair_hw] maps (one launch instead of 2 B)
    float* outF2 = nullptr; int pair_hw = 0;
};
int launch_layernorm(const LnArgs& a, hipStream_t s);

// GroupNorm apply from group sums + activation (+ prior fusion), fp32 [M][C] raw -> bf16 / fp32 (+2x nearest copy)
struct GnApplyArgs {
    const float* x = nullptr; int ldx = 0;
    const double* stats = nullptr;            // [G][2] sum, sumsq
    const float* gamma = nullptr; const float* beta = nullptr; float eps = 1e-3f;
    int M = 0, C = 0, G = 16, act = ACT_SILU;    // M = rows PER SAMPLE
    int B = 1;                                   // samples; x/out rows are [B*M], stats slot b at stats + 64*b
    const float* prior = nullptr; const float* prior_beta = nullptr;   // y += prior[m] * prior_beta[c]
    float* outF = nullptr; int ldf = 0;
    bf16* outB = nullptr; int ldb = 0;
    bf16* outUp = nullptr; int ldu = 0; int W = 0;   // 2x nearest upsampled copy into a (2H,2W) map
    int b32 = 0;
};
int launch_gn_apply(const GnApplyArgs& a, hipStream_t s);

// depthwise 7x7 (+bias) + LayerNorm(C): fp32 NHWC -> bf16 [M][C]
struct DwLnArgs {
    const float* x = nullptr;                 // [H][W][C]
    const float* w = nullptr;                 // [49][C]
    const float* bias = nullptr; const float* gamma = nullptr; const float* beta = nullptr;
    float eps = 1e-6f;
    int H = 0, W = 0, C = 0, B = 1;            // B images of (H,W,C) stacked
    bf16* out = nullptr;
    int b32 = 0;
};
int launch_dwconv7_ln(const DwLnArgs& a, hipStream_t s);

// stem: conv4x4/s4 (3->C) + bias + LN_cf: NCHW fp32 image -> fp32 NHWC
struct StemArgs {
    const float* img = nullptr; int H = 0, W = 0, B = 1;   // (B,3,H,W)
    const float* w = nullptr;                       // [48][C]  (k = c*16 + ky*4 + kx)
    const float* bias = nullptr; const float* gamma = nullptr; const float* beta = nullptr;
    int C = 0; float* out = nullptr;                // [H/4][W/4][C]
};
int launch_stem(const StemArgs& a, hipStream_t s);

// ---------------------------------------------------------------- msda.hip
// reference-compatible op (ops/src/vision.cpp:13-16): value [N,S,M,D], loc [N,Lq,M,L,P,2], attn [N,Lq,M,L,P]
// T = float | double (the reference dispatches both, ms_deform_attn_cuda.cu:64,134)
template <typename T>
int launch_msda(const T* value, const int64_t* shapes_host, const int64_t* lsi_host, const T* loc,
                const T* attn, T* out, int N, int S, int M, int D, int Lq, int L, int P, hipStream_t s);
// backward (ms_deform_attn_cuda.cu:83-153): zeroes grad_value on the stream, then scatter-adds into it with float atomics;
// grad_loc [N,Lq,M,L,P,2] and grad_attn [N,Lq,M,L,P] are written by plain stores, every element
template <typename T>
int launch_msda_bwd(const T* value, const int64_t* shapes_host, const int64_t* lsi_host, const T* loc, const T* attn,
                    const T* grad_out, T* grad_value, T* grad_loc, T* grad_attn, int N, int S, int M, int D, int Lq, int L, int P,
                    hipStream_t s);
// fused engine variant: raw offsets / attention logits -> softmax, loc = ref + off/(W,H), sample, bf16 out
struct MsdaFusedArgs {
    const float* value = nullptr;             // [2*hw][256] fp32
    const float* offaw = nullptr; int ldo = 0;   // [Lq][192]: 128 offsets (m,l,p,xy) | 64 logits (m,l,p)
    int h = 0, w = 0;                         // both levels (h,w); Lq = 2*h*w
    bf16* out = nullptr;                      // [Lq][256]
    int b32 = 0;
    int B = 1;                                // batch: tokens [B][2][hw]
};
int launch_msda_fused(const MsdaFusedArgs& a, hipStream_t s);

// ---------------------------------------------------------------- corr.hip
// out[k][q] = sum_r V[k][r] softmax_r(<Eref[r], Ecur[q]>);  Eref [R][D], Ecur [Q][D] fp32 row-major, V [K][R]
// lse (optional, [Q] / [B][Q]): the log-sum-exp over the reference axis the kernels hold anyway, lse[q] = m + log l; one more store,
// `out` is bitwise what the call without it returns
int launch_corr(const float* eref, const float* ecur, const float* v, float* out, int R, int Q, int D, int K,
                int precision, void* workspace, size_t ws_bytes, hipStream_t s, float* lse = nullptr);
size_t corr_workspace_bytes(int R, int Q, int K);
int launch_corr_batched(const float* eref, const float* ecur, const float* v, float* out, int B, int R, int Q, int D, int K,
                        int values_per_frame, int precision, void* workspace, size_t ws_bytes, hipStream_t s, float* lse = nullptr);
size_t corr_workspace_bytes_batched(int B, int R, int Q, int K);

// ---------------------------------------------------------------- corr_bwd.hip
// gradient of the operator above (unicorn/models/unicorn.py:321-326 under autograd), flash-style: P is recomputed tile by tile from the
// embeddings and lse.  gref / gcur / gv may each be NULL (not computed); every non-NULL output is written completely, one writer per element.
size_t corr_bwd_workspace_bytes(int B, int R, int Q, int K);      // >= corr_workspace_bytes_batched: one scratch serves forward and backward
int launch_corr_bwd(const float* eref, const float* ecur, const float* v, const float* out, const float* lse, const float* gout,
                    float* gref, float* gcur, float* gv, int B, int R, int Q, int D, int K, int values_per_frame, int precision,
                    void* workspace, size_t ws_bytes, hipStream_t s);
// plain double-precision pair (FMA loops, one wave per output row, one writer per element; small problems, no performance claim)
int launch_corr_f64(const double* eref, const double* ecur, const double* v, double* out, double* lse, int B, int R, int Q, int D, int K,
                    int values_per_frame, hipStream_t s);
int launch_corr_bwd_f64(const double* eref, const double* ecur, const double* v, const double* out, const double* lse, const double* gout,
                        double* gref, double* gcur, double* gv, int B, int R, int Q, int D, int K, int values_per_frame, hipStream_t s);

// ---------------------------------------------------------------- misc.hip
int launch_cast_operand(const float* x, int ldx, bf16* out, int ldo, int M, int C, hipStream_t s, int b32 = 0);
// x0 / x1 [B][hw][C] fp32 (two frames) -> out [B][2][hw][C] in the operand format (the token layout of the interaction stage), one launch
int launch_cast_operand_pair(const float* x0, const float* x1, bf16* out, int hw, int C, int B, hipStream_t s, int b32);
int launch_pixel_shuffle_bf16(const float* x, bf16* out, int h, int w, int C, hipStream_t s, int b32 = 0, int B = 1);
int launch_prior_pyramid(const float* p8, float* p16, float* p32, int K, int H8, int W8, hipStream_t s);
int launch_decode(const float* raw, float* out, int A0, int W0, int A1, int W1, int A2, int W2, int nch, hipStream_t s, int B = 1);
int launch_add_aligned_bilinear(const float* src, int h, int w, int C, int factor, float* dst, hipStream_t s, int B = 1);
int launch_pos_embed(const float* row, const float* col, int sz, int nf, float* out, int h, int w, hipStream_t s);
int launch_sample_embed(const float* emb, int H, int W, int C, const float* boxes, int ldbox, int n, float stride,
                        float* out, hipStream_t s);
struct CondInstArgs {
    const float* mask_feats = nullptr;        // [H][W][8] fp32
    const float* up_masks = nullptr;          // [H][W][9*r*r] fp32
    const float* params = nullptr; int ldp = 0;   // [n][169]
    const float* inst_loc = nullptr;          // [n][2]
    const int* inst_lvl = nullptr;            // [n]
    int n = 0, H = 0, W = 0, r = 4, d_rate = 2;
    float* logits_ws = nullptr;               // [n][H][W] workspace
    float* coarse_ws = nullptr;               // [n][rH][rW] workspace (sigmoid scores at 1/d_rate res)
    float* out = nullptr;                     // [n][d_rate*r*H][d_rate*r*W]
};
int launch_condinst(const CondInstArgs& a, hipStream_t s);
int launch_label_map_s8(const float* box_xyxy, float* out, int H, int W, hipStream_t s);
// condinst_loss.hip: the CondInst dice loss for training (dynamic_mask_head.py:247-278), forward + recomputing backward, fp32 and fp64.
// mf [H][W][8], um [H][W][9 r r], params [n][ldp >= 169], loc [n][2], lvl [n], gt [n][rH][rW] -> loss [n], sums [n][3] = (sum s g, sum s^2,
// sum g^2).  The backward writes gmf [H][W][8], gum [H][W][9 r r], gpar [n][ldp] (169 columns); each may be NULL (not computed).
// Workspace: condinst_loss_workspace_bytes for fp32, twice that for fp64; scratch between calls (the backward recomputes the logits).
size_t condinst_loss_workspace_bytes(int n, int H, int W, int r);
template <typename T>
struct ClArgs {
    const T *mf, *um, *params; int ldp;
    const T* loc; const int* lvl; const T* gt;
    int n, H, W, r;
    void* ws; size_t ws_bytes;
};
template <typename T>
int launch_condinst_loss_fwd(const ClArgs<T>& a, T* loss, T* sums, hipStream_t s);
template <typename T>
int launch_condinst_loss_bwd(const ClArgs<T>& a, const T* sums, const T* gout, T* gmf, T* gum, T* gpar, hipStream_t s);
// simota.hip: SimOTA label assignment of the head loss (unicorn_head_mask.py:754-983) for a batch, four launches, no host read-back.
// outputs [B][A][ld >= 5 + C] (cx, cy, w, h, obj, cls logits), labels [B][M][5] (class, cx, cy, w, h), num_gt [B] device,
// xs / ys / st [A] -> fg_mask [B][A], matched_gt [B][A] (-1 = background), matched_iou [B][A], num_fg [B], all completely written.
size_t simota_workspace_bytes(int B, int A, int M, int C);
int launch_simota_assign(const float* outputs, int ld, const float* labels, const int* num_gt, int M, const float* xs, const float* ys,
                         const float* st, int B, int A, int C, int img_h, int img_w, unsigned char* fg_mask, int* matched_gt,
                         float* matched_iou, int* num_fg, void* ws, size_t ws_bytes, hipStream_t s);
// mot_corr.hip: the MOT instance-contrastive loss of training (unicorn.py:407-466) for a batch, forward + backward, fp32 and fp64, a constant
// number of launches and no host read-back.  e0 / e1 (B, C, H, W) through element strides, targets [B][2][M][6] fp32 -> loss [B]; the backward
// writes the dense g0 / g1 completely through their own strides (NULL: not computed).  Workspace: mot_corr_workspace_bytes for fp32, twice
// that for fp64; scratch between the calls (the backward recomputes).  flags: 1 = bidirect, 2 = grid_sample.
struct McStride { long long b, c, y, x; };      // element strides of a (B, C, H, W) map
size_t mot_corr_workspace_bytes(int B, int M, int C);
struct McArgs {                                 // e0 / e1 hold T (the launcher's type)
    const void *e0, *e1;
    McStride s0, s1;
    const float* targets;
    int B, C, H, W, M;
    float stride;
    int flags;
    void* ws;
    size_t ws_bytes;
};
template <typename T>
int launch_mot_corr_fwd(const McArgs& a, T* loss, hipStream_t s);
template <typename T>
int launch_mot_corr_bwd(const McArgs& a, const T* gout, T* g0, McStride gs0, T* g1, McStride gs1, hipStream_t s);
// prop_loss.hip: what stands around the label propagation in the SOT / VOS training losses (unicorn.py:315-390), fp32 and fp64, no host read.
// launch_prop_labels: targets [B][2][M][6] fp32 (+ masks [B][2][M][r H8][r W8] fp32 / uint8, or NULL: boxes) -> matched [B][Kc][2],
// num_matched [B], gt0 / gt1 [B][Kc][H8 W8], all completely written; sot: one slot (0, 0) per sample.  launch_prop_dice_pyramid_fwd: pred, gt1
// [B][Kc][H8][W8] -> p16, p32, loss ([B][Kc], or ONE value when num_matched is NULL: the SOT Dice over the batch), sums [groups][3] double
// (I, X2, T2).  _bwd: g_pred [B][Kc][H8][W8] completely written from the upstream gradients (each may be NULL).  Workspace (forward only):
// prop_workspace_bytes in both precisions.
size_t prop_workspace_bytes(int B, int Kc, int Q);
struct PlLabelArgs {
    const float* targets; const void* masks;
    int mask_u8, B, M, Kc, sot, H8, W8, r;
    int *matched, *num_matched;
};
template <typename T>
struct PlDiceArgs {
    const T *pred, *gt1; const int* num_matched;
    int B, Kc, H8, W8;
};
template <typename T>
int launch_prop_labels(const PlLabelArgs& a, T* gt0, T* gt1, hipStream_t s);
template <typename T>
int launch_prop_dice_pyramid_fwd(const PlDiceArgs<T>& a, T* p16, T* p32, T* loss, double* sums, void* ws, size_t ws_bytes, hipStream_t s);
template <typename T>
int launch_prop_dice_pyramid_bwd(const PlDiceArgs<T>& a, const double* sums, const T* g8, const T* g16, const T* g32, const T* gl, T* gpred,
                                 hipStream_t s);
// opt_step.hip: GradScaler.step + torch.optim.AdamW + GradScaler.update + ModelEMA.update (trainer.py:260-275, utils/ema.py:50-63) over a list of
// fp32 tensors through a tensor table and a block map in device memory (layouts: include/unicorn_hip.h), at most three launches, no host read.
int opt_chunk_elems();
size_t opt_table_bytes(int n_tensors, long long total_chunks);
int launch_opt_step(const void* table, size_t table_bytes, const void* block_map, size_t map_bytes, int n_tensors, int vec_chunks, int total_chunks,
                    float* step, float* scale, int* growth_tracker, float* found_inf, double lr, double beta1, double beta2, double eps,
                    double ema_decay, double growth_factor, double backoff_factor, int growth_interval, hipStream_t s);
// head_loss.hip: the four detection losses of get_losses (unicorn_head_mask.py:646-745) for a batch from the device-side results of
// launch_simota_assign, forward + backward, fp32 and fp64, two launches each way and no host read-back.  outputs [B][A][ld >= 5 + C],
// origin [B][A][ldo >= 4] or NULL, labels [B][M][5], fg / mg / miou [B][A], num_fg / num_gt [B] device, xs / ys / st [A] ->
// out[5] = reg_weight x iou, obj, cls, l1 losses and max(sum num_fg, 1) / max(sum num_gt, 1); the backward writes g_out [B][A][ldg >= 5 + C]
// (columns 0 .. 4 + C) and g_org [B][A][4] completely (NULL: not computed).  Workspace: head_loss_workspace_bytes in both precisions.
size_t head_loss_workspace_bytes(int B, int A, int C);
template <typename T>
struct HlIn {                                   // passed by value to the kernels
    const T* outputs; int ld;
    const T* origin; int ldo;
    const T* labels; int M;
    const unsigned char* fg; const int* mg; const T* miou;
    const T *xs, *ys, *st;
    int A, C;
};
template <typename T>
struct HlArgs {
    HlIn<T> in;
    const int *num_fg, *num_gt;
    int B;
    double reg_weight;
    void* ws;
    size_t ws_bytes;
};
template <typename T>
int launch_head_loss_fwd(const HlArgs<T>& a, T* out, hipStream_t s);
template <typename T>
int launch_head_loss_bwd(const HlArgs<T>& a, const T* gout, T* g_out, int ldg, T* g_org, hipStream_t s);
// head_assemble.hip: the lines between the head's prediction convolutions and get_losses (unicorn_head_mask.py:339-366, :476-500 and the level
// cats :396-401, :554-558; n_anchors == 1) for a batch and up to HA_MAX_L levels, one launch forward and one backward, fp32 (maps fp32, fp16 or
// bf16) and fp64, no host read-back, no workspace, one writer per element.  Per level l the maps reg (B,4,h,w), obj (B,1,h,w), cls (B,C,h,w)
// and ctrl (B,P,h,w), each NCHW-contiguous (bit 0 .. 3 of layouts[l] set) or channels-last; anchor a = off_l + y w_l + x.
//   forward   outputs [B][A][ld >= 5 + C], origin [B][A][4], xs / ys / st [A], params [B][A][ldp >= P], levels [B][A] (each may be NULL)
//   backward  g_out [B][A][ldg], g_org [B][A][4], g_par [B][A][ldgp] (NULL = zero) -> per level g_reg / g_obj / g_cls / g_ctrl in the element type
//             and layout of their map (an array or an entry may be NULL: not computed); reg is read for exp(reg[2:4]) when g_reg is asked for
// 1 <= L <= 4, 1 <= B <= 65535, 1 <= C <= 256, 1 <= P <= 1024, h, w >= 1, A = sum h w < 2^24, strides > 0.
constexpr int HA_MAX_L = 4;
constexpr int HA_TILE = 64;                     // anchors of one level that a block assembles (and the channels of one pass through LDS)
struct HaShape {
    const int32_t *hs, *ws;                     // host arrays of L
    const double* strides;
    const int32_t* layouts;
    int L, B, C, P, map_dtype;                  // P == 0: no controller maps; map_dtype 0 = T, 1 = fp16, 2 = bf16
};
template <typename T>
struct HaOut {
    T* outputs; int ld;
    T* origin;
    T *xs, *ys, *st;
    T* params; int ldp;
    int32_t* levels;
};
template <typename T>
struct HaGrad {
    const T* g_out; int ldg;
    const T* g_org;
    const T* g_par; int ldgp;
};
template <typename T>
int launch_head_assemble_fwd(const HaShape& sh, const void* const* reg, const void* const* obj, const void* const* cls, const void* const* ctrl,
                             const HaOut<T>& o, hipStream_t s);
template <typename T>
int launch_head_assemble_bwd(const HaShape& sh, const void* const* reg, const HaGrad<T>& g, void* const* g_reg, void* const* g_obj,
                             void* const* g_cls, void* const* g_ctrl, hipStream_t s);
// head_mask_loss.hip: the CondInst mask loss of get_losses (unicorn_head_mask.py:568-569, :675-694, :731-732) for a batch from the device-side
// results of launch_simota_assign, forward + recomputing backward, fp32 and fp64, 5 launches forward and at most 22 backward, no host read-back.
// mf [B][H][W][8], um [B][H][W][9 r r], params [B][A][ldp >= 169], lvl [B][A], masks [B][M][rH][rW] (read in place through mg), fg / mg [B][A],
// xs / ys / st [A] -> out[1 + B] = loss_condinst, loss_mask[B]; sums [cap][3] for the backward.  The backward writes gmf [B][H][W][8],
// gum [B][H][W][9 r r], gpar [B][A][ldg >= 169] (169 columns) completely; each may be NULL.  More foreground anchors than cap: NaN losses, zero
// gradients.  Workspace: head_mask_loss_workspace_bytes for fp32, twice that for fp64; scratch between calls.
size_t head_mask_loss_workspace_bytes(int B, int A, int H, int W, int r, int cap);
template <typename T>
struct HMIn {
    const T *mf, *um, *params;
    int ldp;
    const int* lvl;
    const T* masks;
    int M;
    const unsigned char* fg;
    const int* mg;
    const T *xs, *ys, *st;
    int B, A, H, W, r, cap;
};
template <typename T>
int launch_head_mask_loss_fwd(const HMIn<T>& a, T* out, T* sums, void* ws, size_t ws_bytes, hipStream_t s);
template <typename T>
int launch_head_mask_loss_bwd(const HMIn<T>& a, const T* sums, const T* gout, T* gmf, T* gum, T* gpar, int ldg, void* ws, size_t ws_bytes,
                              hipStream_t s);
// dwln_train.hip: the opening of a ConvNeXt block for TRAINING (convnext.py:32-33,43-45): y = LN_C(dwconv7x7(x) + bias) * gamma + beta, forward +
// recomputing backward, fp32 and fp64, one launch forward and at most four backward, no host read-back, no atomics.  x, y, gy, gx dense
// [B][H][W][C], w [49][C], stats [B H W][2] (mean, rstd) written by the forward for the backward.  The backward writes gx [B][H][W][C], gw [49][C] +
// gb [C], ggamma [C] + gbeta [C] completely; gx, the pair gw / gb and the pair ggamma / gbeta may each be NULL (not computed).  C % 4 == 0,
// C <= 2048, B H W < 2^31.  Workspace (backward only): dwln_train_workspace_bytes for fp32, twice that for fp64; scratch between calls.
size_t dwln_train_workspace_bytes(int B, int H, int W, int C);
template <typename T>
struct DwlnArgs {
    const T *x, *w, *bias, *gamma, *beta;       // beta: forward only
    double eps;                                 // forward only (the backward reads rstd)
    int B, H, W, C;
};
template <typename T>
int launch_dwln_train_fwd(const DwlnArgs<T>& a, T* y, T* stats, hipStream_t s);
template <typename T>
int launch_dwln_train_bwd(const DwlnArgs<T>& a, const T* stats, const T* gy, T* gx, T* gw, T* gb, T* ggamma, T* gbeta, void* ws, size_t ws_bytes,
                          hipStream_t s);
// block_tail.hip: the close of a ConvNeXt block for TRAINING (convnext.py:49-53): out = x + (gamma * y) * s[n] in channels-last memory and its
// backward grad_y = gamma * (x * s[n]), grad_gamma[c] = sum (x * s[n]) * y, fp32 (y / grad_y fp32, fp16 or bf16) and fp64, one launch forward and
// at most two backward, no host read-back, no atomics.  y, grad_y dense [B][H][W][C]; x = residual (forward) / grad_out (backward), dense
// [B][H][W][C] or, with nchw != 0, [B][C][H][W]; gamma [C] and scale [B] may be NULL (= 1); gy and ggamma may be NULL (not computed).
// C % 4 == 0, C <= 2048, B H W < 2^31.  Workspace (backward with ggamma only): block_tail_workspace_bytes for fp32, twice that for fp64.
size_t block_tail_workspace_bytes(int B, int H, int W, int C);
template <typename T>
struct BtArgs {
    const void* y;
    int y_dtype;                                // 0: the type T, 1 fp16, 2 bf16 (fp32 form only)
    const T* x;
    int nchw;
    const T *gamma, *scale;
    int B, H, W, C;
};
template <typename T>
int launch_block_tail_fwd(const BtArgs<T>& a, T* out, hipStream_t s);
template <typename T>
int launch_block_tail_bwd(const BtArgs<T>& a, void* gy, T* ggamma, void* ws, size_t ws_bytes, hipStream_t s);
// lncf_train.hip: the channels-first LayerNorm between the ConvNeXt stages for TRAINING (convnext.py:160-184): y = weight[c] * (x - u) * rstd +
// bias[c] over the channels of every pixel, forward + backward, fp32 (x / grad_x fp32, fp16 or bf16) and fp64, one launch forward and at most
// two backward, no host read-back, no atomics.  x, y, gy, gx are (B, C, H, W) maps in channels-last memory [B][H][W][C] or, with nchw != 0,
// NCHW-contiguous [B][C][H][W], all four in the same layout; y and gy have the type T, gx the type of x; stats [B H W][2] (mean, rstd) is
// written by the forward for the backward.  gx and the pair gw / gb may be NULL (not computed; the workspace is then not touched).
// C % 4 == 0, 4 <= C <= 2048, B H W < 2^31.  Workspace (backward with gw / gb only): lncf_train_workspace_bytes for fp32, twice that for fp64.
size_t lncf_train_workspace_bytes(int B, int H, int W, int C);
template <typename T>
struct LncfArgs {
    const void* x;
    int x_dtype;                                // 0: the type T, 1 fp16, 2 bf16 (fp32 form only)
    int nchw;
    const T *w, *bias;                          // bias: forward only
    double eps;                                 // forward only (the backward reads rstd)
    int B, H, W, C;
};
template <typename T>
int launch_lncf_train_fwd(const LncfArgs<T>& a, T* y, T* stats, hipStream_t s);
template <typename T>
int launch_lncf_train_bwd(const LncfArgs<T>& a, const T* stats, const T* gy, void* gx, T* gw, T* gb, void* ws, size_t ws_bytes, hipStream_t s);
// down_train.hip: the four downsample layers of the ConvNeXt backbone for TRAINING (convnext.py:77-87; the GEMMs stay with the vendor library).
// LN to patches: the channels-first LayerNorm of x dense [B][H][W][C] (fp32, fp16 or bf16; fp64 in the fp64 form) written as the patch matrix
// A [M][4 C] of the 2x2 / stride-2 convolution behind it (row (n Ho + h / 2) Wo + w / 2, column ((h & 1) 2 + (w & 1)) C + c; Ho = H / 2, Wo =
// W / 2, M = B Ho Wo) in the element type a_dtype names, with stats [B H W][2]; `rebuild` reads stats and writes A alone, with the forward's
// bits.  The backward reads gA at the same addresses and is lncf's: gx (the type of x; exact zeros at the pixels an odd H or W drops) and the
// pair gw / gb, each may be NULL.  C % 4 == 0, 4 <= C <= 2048, H, W >= 2, B H W < 2^31.  Workspace (backward with gw / gb only):
// down_train_workspace_bytes for fp32, twice that for fp64.
// Stem patches: x [B][Cin][H][W] -> A [M][Cin 16] (row as above with / 4, column (c 4 + kh) 4 + kw) and back (gx written completely, zeros in
// the margin H % 4 / W % 4 leave).  1 <= Cin <= 4, H, W >= 4, B H W < 2^31.
size_t down_train_workspace_bytes(int B, int H, int W, int C);
template <typename T>
struct DownArgs {
    const void* x;
    int x_dtype, a_dtype;                       // 0: the type T, 1 fp16, 2 bf16 (fp32 form only)
    const T *w, *bias;                          // bias: forward only
    double eps;                                 // forward only (rebuild and backward read rstd)
    int B, H, W, C;
};
template <typename T>
int launch_down_train_fwd(const DownArgs<T>& a, int rebuild, void* A, T* stats, hipStream_t s);
template <typename T>
int launch_down_train_bwd(const DownArgs<T>& a, const T* stats, const void* gA, void* gx, T* gw, T* gb, void* ws, size_t ws_bytes, hipStream_t s);
template <typename T>
int launch_patch4_gather(const void* x, int x_dtype, int B, int Cin, int H, int W, void* A, int a_dtype, hipStream_t s);
template <typename T>
int launch_patch4_scatter(const void* gA, int a_dtype, int B, int Cin, int H, int W, void* gx, int x_dtype, hipStream_t s);
// pw_mlp.hip: the point-wise middle of the ConvNeXt block's MLP for TRAINING (convnext.py:46-48; the GEMMs stay with the vendor library): the
// exact GELU forward a = gelu(h) and a backward that rebuilds a from h: a and / or grad_h = grad_a * gelu'(h) and / or gb1[Hd] = the column sums of
// the unrounded grad_h, plus gb2[Co] = the column sums of grad_y, fp32 (maps fp32, fp16 or bf16) and fp64, one launch forward and at most three
// backward, no host read-back, no atomics.  h, a, ga, gh dense [M][Hd], gy dense [M][Co], all of the element type h_dtype names; a may be h and
// gh may be ga.  Every output may be NULL (not computed).  Hd % 4 == 0, 4 <= Hd <= 8192, the same for Co, 1 <= M < 2^31.  Workspace (with gb1 or
// gb2 only): pw_mlp_workspace_bytes for fp32, twice that for fp64.
size_t pw_mlp_workspace_bytes(int M, int Hd, int Co);
template <typename T>
struct PwBwdArgs {
    const void *h, *ga;
    int h_dtype;                                // 0: the type T, 1 fp16, 2 bf16 (fp32 form only)
    int M, Hd;
    void *a, *gh;
    T* gb1;
    const void* gy;
    int Co;
    T* gb2;
};
template <typename T>
int launch_pw_mlp_act_fwd(const void* h, int h_dtype, int M, int Hd, void* a, hipStream_t s);
template <typename T>
int launch_pw_mlp_act_bwd(const PwBwdArgs<T>& a, void* ws, size_t ws_bytes, hipStream_t s);
// gn_act_train.hip: GroupNorm + activation for TRAINING (network_blocks.py:29-51 after convert_bn_model_to_gn: act(bn(conv(x))) with bn =
// GroupNorm(16, C, eps=1e-3); the CondInst mask branch; unicorn.py:38): y = act((x - mean) * rstd * w[c] + bias[c]) with the statistics of every
// (sample, group), forward + backward (xhat, z and act'(z) are recomputed), fp32 (x / grad_x fp32, fp16 or bf16) and fp64, at most three launches
// forward and three backward, no host read-back, no atomics.  x, y, gy, gx are (B, C, H, W) maps in channels-last memory or, with nchw != 0,
// NCHW-contiguous, all four in the same layout; y and gy have the type T, gx the type of x; stats [B G][2] (mean, rstd).  act: 0 none, 1 ReLU,
// 3 SiLU.  The forward keeps its partial statistics in y until the last launch overwrites it.  gx and the pair gw / gb may be NULL (not computed).
// train_shape_ok(B, H, W, C), 1 <= G <= C, C % G == 0.  Workspace (every backward): gn_act_train_workspace_bytes for fp32, twice that for fp64.
size_t gn_act_train_workspace_bytes(int B, int H, int W, int C, int G);
template <typename T>
struct GnArgs {
    const void* x;
    int x_dtype;                                // 0: the type T, 1 fp16, 2 bf16 (fp32 form only)
    int nchw;
    const T *w, *bias;
    double eps;                                 // forward only (the backward reads rstd)
    int act;
    int B, H, W, C, G;
};
template <typename T>
int launch_gn_act_train_fwd(const GnArgs<T>& a, T* y, T* stats, hipStream_t s);
template <typename T>
int launch_gn_act_train_bwd(const GnArgs<T>& a, const T* stats, const T* gy, void* gx, T* gw, T* gb, void* ws, size_t ws_bytes, hipStream_t s);
// post.hip: utils/boxes.py:33-77 on the device (corners in place, conf filter, (batched) NMS, sorted survivor rows)
int launch_letterbox(const unsigned char* img, int h, int w, int swap_rb, int H, int W, float* out, double* r_out, hipStream_t s);
size_t postprocess_workspace_bytes(int A);
size_t nms_workspace_bytes(int n);
int launch_nms(const float* boxes, const float* scores, int n, float iou_thr, int32_t* keep_idx, int32_t* n_out, void* ws,
               size_t ws_bytes, hipStream_t s);
int launch_postprocess(float* pred, int A, int ld, int num_classes, float conf_thre, float nms_thre, int flags,
                       int max_det, float* det_out, int32_t* keep_idx, int32_t* n_out, void* ws, size_t ws_bytes, hipStream_t s);
// mask_post.hip: mask post-processing of the VOS / MOTS drivers (row N1)
// coarse (N, h, w) CondInst sigmoid scores at 1 / d_rate of the network resolution -> aligned_bilinear(x f) -> resize by 1 / r -> fp32 and / or
// `> thr` bytes at (H, W), without the (N, f h, f w) intermediate (bit-identical to launch_condinst's last pass + launch_mask_resize)
int launch_condinst_resize(const float* coarse, int N, int h, int w, int f, float rscale, int ho, int wo, int H, int W, float thr, float* outF,
                           unsigned char* outU, hipStream_t s);
int launch_mask_resize(const float* masks, int N, int Hn, int Wn, float rscale, int ho, int wo, int H, int W, float thr, float* outF,
                       unsigned char* outU, hipStream_t s);
int launch_vos_merge(const float* probs, const int* prob_ids, int K1, int Hn, int Wn, float rscale, int ho, int wo,
                     const unsigned char* init_masks, const int* init_ids, int K2, int H, int W, unsigned char* out, hipStream_t s);
int launch_overlap_free(const unsigned char* in, int N, int H, int W, unsigned char* out, hipStream_t s);
size_t rle_workspace_bytes(int N, int H, int W, int max_runs);
int launch_rle_encode(const unsigned char* masks, int N, int H, int W, int max_runs, int max_chars, unsigned char* out_chars,
                      int* out_len, unsigned* counts, int* n_runs, void* ws, size_t ws_bytes, hipStream_t s);
int launch_add_pos_bf16(const float* src, const float* pos0, const float* pos1, const float* lvl, bf16* out, int hw,
                        int C, hipStream_t s, int b32 = 0, int B = 1);
