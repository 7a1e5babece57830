/* libunicorn_hip.so — C-ABI of the MI355X-native Unicorn inference hot path (+ the gradient of its one native operator).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  The caller
 * (Python/ctypes in unicorn_amd/, or any other host) owns every input/output buffer (device memory,
 * e.g. torch.Tensor.data_ptr()); the library owns only an opaque uni_ctx holding re-packed weights and
 * its scratch workspace.  Every call is asynchronous on the hipStream_t passed in (no hidden sync), and
 * thread-compatible (one ctx per stream / process).  Return 0 on success, <0 on error
 * (uni_last_error() gives the message).
 *
 * Activation layout: NHWC ("channels_last"), fp32 at the API, i.e. a (1,C,H,W) torch tensor with
 * channels_last strides is passed as-is.  Images enter as the reference's NCHW fp32 0-255 BGR tensor.
 *
 * What each entry point replaces in the reference (paths relative to MasterBin-IIAU/Unicorn):
 *   uni_msda_fwd            MultiScaleDeformableAttention.ms_deform_attn_forward
 *                           (unicorn/models/ops/src/vision.cpp:13-16, ops/src/ms_deform_attn.h:19-38,
 *                            ops/src/cuda/ms_deform_attn_cuda.cu:20-80)
 *   uni_msda_bwd            MultiScaleDeformableAttention.ms_deform_attn_backward
 *                           (ops/src/vision.cpp:13-16, ops/src/ms_deform_attn.h:40-61,
 *                            ops/src/cuda/ms_deform_attn_cuda.cu:83-153, ms_deform_im2col_cuda.cuh:87-234,301-920,956-1326)
 *   uni_msda_fwd_f64 / uni_msda_bwd_f64   the double dispatch of the same two functions (AT_DISPATCH_FLOATING_TYPES,
 *                            ms_deform_attn_cuda.cu:64,134).  Together the four are the whole native boundary of the reference's
 *                            operator, forward and gradient (unicorn_amd.msda_ext offers them under the pybind module's name).
 *                            The model-level entry points below stay inference only.
 *   uni_corr_softmax_pv     simi = E_ref^T E_cur; softmax(dim=0); values @ trans
 *                           (external/lib/test/tracker/unicorn_sot.py:95-100, unicorn_vos.py:166-181)
 *   uni_corr_softmax_pv_lse / uni_corr_softmax_pv_bwd (+ _f64)   the same three lines in the training losses, forward and gradient
 *                           (unicorn/models/unicorn.py:321-326, :342-371)
 *   uni_backbone_fpn        Unicorn.forward(mode="backbone") (unicorn/models/unicorn.py:231-258;
 *                            backbone/convnext.py:141-154, backbone/yolo_pafpn_new.py:113-161)
 *   uni_interaction         Unicorn.forward(mode="interaction") (unicorn.py:260-276,
 *                            deformable_transformer.py:58-131, ops/modules/ms_deform_attn.py:78-115)
 *   uni_upsample            Unicorn.forward(mode="upsample") (unicorn.py:41-44,311-313)
 *   uni_head                UnicornHead.forward / UnicornHeadMask.forward, eval branch
 *                           (unicorn_head.py:249-336,430-482; unicorn_head_mask.py:280-372,451-519;
 *                            condinst/mask_branch.py:77-99,158-162)
 *   uni_condinst_masks      DynamicMaskHead.__call__ + aligned_bilinear(d_rate)
 *                           (condinst/dynamic_mask_head.py:172-225; utils/boxes.py:138-146)
 *   uni_condinst_masks_u8   the same fused with the 1/r resize + `> mask_thres` of the MOTS loop (mot_evaluator.py:804-805)
 *   uni_letterbox           PreprocessorX.process / preproc (unicorn_sot.py:111-123, data/data_augment.py:194-214)
 *   uni_postprocess         postprocess + torchvision nms/batched_nms (utils/boxes.py:33-77)
 *   uni_prior_pyramid       F.interpolate(coarse, 1/2 | 1/4, bilinear) (unicorn_sot.py:103-105)
 *   uni_label_map_s8        get_label_map + F.interpolate(1/8) (unicorn_sot.py:52-53,128-139)
 *   uni_sample_embeddings   per-box F.grid_sample of the embedding map (evaluators/mot_evaluator.py:1024-1034)
 *   uni_pos_embed           PositionEmbeddingLearned.forward (+ identity bicubic) (position_encoding.py:25-36,
 *                            unicorn.py:248-250)
 *   low-level ops (uni_gemm_bf16, uni_layernorm, uni_dwconv7_ln, uni_groupnorm_act, uni_stem)
 *                           building blocks exported for the kernel parity tests.
 */
#ifndef UNICORN_HIP_H
#define UNICORN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uni_ctx uni_ctx;
typedef void* uni_stream_t; /* hipStream_t */

/* Network shape, mirrors exp/unicorn_track.py:31-113 + exps/default/ *.py */
typedef struct uni_model_cfg {
    int32_t dims[4];     /* ConvNeXt stage widths: tiny 96,192,384,768 / large 192,384,768,1536 */
    int32_t depths[4];   /* 3,3,9,3 / 3,3,27,3 */
    int32_t num_classes; /* MOT classes (8 BDD100K, 1 MOT17) */
    int32_t mask;        /* 1 = UnicornHeadMask (+ mask branch, controllers) */
    int32_t n_layer_att; /* 3 */
    int32_t embed_dim;   /* 128 */
    int32_t up_rate;     /* 8 // d_rate (4) */
    int32_t d_rate;      /* 2 */
    int32_t precision;   /* operand format of every dense contraction (fp32 accumulate): 0 = bf16; 1 = exact fp32
                            (v_mfma_f32_32x32x2_f32); 2 = "f16x2" split f16, fp32-equivalent (3 f16 MFMAs per product) */
} uni_model_cfg;

const char* uni_last_error(void);
int uni_version(void);
/* Variant trace (tests / tools): which kernel instantiation did a call run?  Every launcher of the library reports the launch it is about
 * to make as a short tag: launcher, kernel and template arguments, operand format and every launch-uniform switch that changes the
 * index arithmetic or the store path inside the kernel (the tag does not depend on HOW the variant was chosen: heuristic, force_cfg or an
 * environment switch).  Process-global, off by default (then a launch pays one relaxed atomic load), safe to use from several threads.
 * uni_variant_trace(1) clears the recorded tags and starts recording, uni_variant_trace(0) stops (the tags stay readable); returns 0. */
int uni_variant_trace(int on);
/* Writes the recorded tags as "tag\tcount\n" lines, sorted by tag, NUL-terminated and truncated to cap bytes (buf may be NULL);
 * returns the bytes needed for the whole text including the NUL. */
size_t uni_variant_trace_read(char* buf, size_t cap);

/* ---- context / weights ------------------------------------------------------------------------- */
uni_ctx* uni_ctx_create(int device_id, const uni_model_cfg* cfg);
void uni_ctx_destroy(uni_ctx* ctx);
/* Register one reference state-dict tensor (fp32, HOST memory, reference layout e.g. OIHW).  Unknown
 * names are ignored (returns 1), like load_state_dict(strict=False). */
int uni_ctx_load_param(uni_ctx* ctx, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* Deployment artefact for hosts without Python / torch (round 6; the role `tools/export_torchscript.py:51-71` plays for the reference: a file
 * another runtime loads): a FLAT WEIGHTS FILE written by `unicorn_amd.utils.checkpoint.export_flat` (or tools/export_weights.py) --
 * "UNIW1\0\0\0", the uni_model_cfg (15 int32), int32 tensor count, then per tensor: int32 name length, name bytes, int32 ndim, int64 shape[ndim],
 * fp32 data (reference layout, little endian).  uni_weights_file_cfg reads the configuration (precision as exported; the caller may change it before
 * uni_ctx_create), uni_ctx_load_file registers every tensor of the file like uni_ctx_load_param (call uni_ctx_finalize afterwards);
 * *n_loaded = tensors read.  tools/capi_host_demo.cpp runs the SOT step from such a file with nothing but this header and the HIP runtime. */
int uni_weights_file_cfg(const char* path, uni_model_cfg* cfg_out);
int uni_ctx_load_file(uni_ctx* ctx, const char* path, int* n_loaded);
/* Re-pack weights for the device (NHWC / [N][K] bf16, layer-scale folded).  *n_missing = parameters the
 * configured network needs but which were never loaded (left at zero). */
int uni_ctx_finalize(uni_ctx* ctx, int* n_missing);
/* name of the i-th missing parameter after finalize (NULL when out of range) */
const char* uni_ctx_missing_name(uni_ctx* ctx, int i);
/* Pre-size the scratch workspace for an (H,W) input (optional; grows on demand otherwise). */
int uni_ctx_reserve(uni_ctx* ctx, int B, int H, int W);

/* Operand-range check of the "f16x2" mode.  Every fp32 value entering a contraction is stored as hi + lo f16 halves and SATURATES at
 * +-65504 (csrc/common.h h2_split; never inf / NaN).  The synthetic test weights stay far below that, a trained checkpoint cannot be
 * validated offline: uni_ctx_set_check(ctx, 1) (or UNI_CHECK_SAT=1 in the environment at finalize) makes the context scan every
 * operand buffer it produces (one extra pass each; the fused MLP falls back to its two-launch form so the hidden activations exist)
 * and count saturated elements.  uni_ctx_stats synchronises and fills out4 = {saturated operands, operands scanned, buffers scanned,
 * 0} since the last uni_ctx_set_check call. */
int uni_ctx_set_check(uni_ctx* ctx, int on);
int uni_ctx_stats(uni_ctx* ctx, long long* out4);

/* Per-kernel-class timing with HIP events on the launch stream (used by bench.py's roofline leg, off by default).
 * uni_prof_end synchronises the device and fills out16: [5 classes][ms, work, launches] + out16[15] = algorithmic
 * bytes of the GEMM class; classes: 0 GEMM/conv (work = algorithmic FLOPs 2*M*N*K), 1 dwconv7+LN, 2 GroupNorm apply,
 * 3 LayerNorm (work = algorithmic bytes), 4 misc. */
int uni_prof_begin(uni_ctx* ctx);
int uni_prof_end(uni_ctx* ctx, double* out16);

/* ---- stage entry points (one per Unicorn.forward mode) ----------------------------------------------- */
/* Every stage takes a batch B of images (the reference modules are batched too; its inference drivers use B = 1).
 * img: (B,3,H,W) fp32 NCHW.  fpn{0,1,2}: NHWC fp32 (B,H/8,W/8,C1), (B,H/16,W/16,C2), (B,H/32,W/32,C3).
 * feat16: NHWC fp32 (B,H/16,W/16,C2) = seq_dict["feat"].  H, W multiples of 32. */
int uni_backbone_fpn(uni_ctx* ctx, const float* img, int B, int H, int W, float* fpn0, float* fpn1, float* fpn2,
                     float* feat16, uni_stream_t stream);
/* feat_*: NHWC fp32 (B,h,w,C2); pos_*: NHWC fp32 (h,w,256) shared by the batch; out_*: NHWC fp32 (B,h,w,256). */
int uni_interaction(uni_ctx* ctx, const float* feat_ref, const float* pos_ref, const float* feat_cur,
                    const float* pos_cur, int B, int h, int w, float* out_ref, float* out_cur, uni_stream_t stream);
/* feat: NHWC fp32 (B,h,w,256) -> embed: NHWC fp32 (B,2h,2w,embed_dim). */
int uni_upsample(uni_ctx* ctx, const float* feat, int B, int h, int w, float* embed, uni_stream_t stream);
/* fpn*: as produced by uni_backbone_fpn for B (H,W) images; prior*: (B,H/8*W/8), (B,H/16*W/16), (B,H/32*W/32) fp32
 * (one prior per image and level).  mode bit 0: 0 = "sot", 1 = "mot"; bit 1 (value 2): raw rows, i.e. the reference's
 * decode_in_inference = False (unicorn_head.py:436-439, tools/export_torchscript.py:66; not for mask models).
 * out: (B, A, 5+nc) fp32 decoded, A = sum of level
 * sizes, nc = 1 (sot) or num_classes (mot).  Mask models additionally fill dyn_params (B,A,169), mask_feats
 * (B,H/8,W/8,8) NHWC and up_masks (B,H/8,W/8,9*up_rate^2) NHWC (pass NULL for box-only models). */
int uni_head(uni_ctx* ctx, const float* fpn0, const float* fpn1, const float* fpn2, const float* prior8,
             const float* prior16, const float* prior32, int B, int H, int W, int mode, float* out, float* dyn_params,
             float* mask_feats, float* up_masks, uni_stream_t stream);
/* Object-batched head (VOS, external/lib/test/tracker/unicorn_vos.py:178-200 runs the head once per object on the SAME
 * FPN maps): ONE image, K prior sets prior*: (K, H/s*W/s).  The prior enters only at x = stem(fpn) + prior*beta
 * (unicorn_head.py:272-277), so FPN casts, stem convs and the mask branch run once and the rest over K samples.
 * out (K, A, 5+nc), dyn_params (K, A, 169); mask_feats / up_masks are those of the ONE image (1, ...). */
int uni_head_objects(uni_ctx* ctx, const float* fpn0, const float* fpn1, const float* fpn2, const float* prior8,
                     const float* prior16, const float* prior32, int K, int H, int W, int mode, float* out,
                     float* dyn_params, float* mask_feats, float* up_masks, uni_stream_t stream);
int uni_pos_embed(uni_ctx* ctx, int h, int w, float* out_nhwc, uni_stream_t stream);

/* ---- context-free operators ------------------------------------------------------------------------- */
/* value [N,S,M,D] fp32, spatial_shapes [L,2] int64 HOST, level_start_index [L] int64 HOST,
 * sampling_loc [N,Lq,M,L,P,2], attn_weight [N,Lq,M,L,P] -> out [N,Lq,M*D]. */
int uni_msda_fwd(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                 const float* sampling_loc, const float* attn_weight, float* out, int N, int S, int M, int D, int Lq,
                 int L, int P, uni_stream_t stream);
int uni_msda_fwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const double* sampling_loc, const double* attn_weight, double* out, int N, int S, int M, int D,
                     int Lq, int L, int P, uni_stream_t stream);
/* Gradient of uni_msda_fwd (replaces ms_deform_attn_cuda_backward, ms_deform_attn_cuda.cu:83-153, and the col2im kernels
 * ms_deform_im2col_cuda.cuh:301-920,956-1326): the inputs of the forward plus grad_output [N,Lq,M*D] ->
 *   grad_value [N,S,M,D]              scatter-add of w_corner * attn * grad_output into the up-to-four corner rows,
 *   grad_sampling_loc [N,Lq,M,L,P,2]  (W, H) * attn * sum_d grad_output_d * d(bilinear_d)/d(x, y),
 *   grad_attn_weight [N,Lq,M,L,P]     sum_d grad_output_d * bilinear_d,
 * with the forward's rules (pixel coordinates loc*(W,H) - 0.5; a sample outside -1 < x < W, -1 < y < H contributes nothing and gets
 * zero gradients; corners outside the map contribute nothing).  Same limits as the forward (L <= 8, sum(H*W) == S); every level must
 * lie inside [0, S).  All three outputs are written completely: the call zeroes grad_value itself on the stream (hipMemsetAsync) and
 * accumulates into it with hardware float atomics (global_atomic_add_f32 / _f64).  Two consequences for the caller:
 *   - grad_value MUST be ordinary device memory (a hipMalloc-class allocation; torch device tensors are) -- NOT fine-grained,
 *     managed or host-mapped memory, where the hardware float atomic is not performed;
 *   - grad_value depends on the arrival order of the adds in its last bits, run to run, exactly like the reference's atomicAdd;
 *     grad_sampling_loc and grad_attn_weight have one writer per element and are bitwise reproducible.
 * Lq == 0 or N == 0 returns at once with grad_value zeroed. */
int uni_msda_bwd(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                 const float* sampling_loc, const float* attn_weight, const float* grad_output, float* grad_value,
                 float* grad_sampling_loc, float* grad_attn_weight, int N, int S, int M, int D, int Lq, int L, int P,
                 uni_stream_t stream);
int uni_msda_bwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const double* sampling_loc, const double* attn_weight, const double* grad_output, double* grad_value,
                     double* grad_sampling_loc, double* grad_attn_weight, int N, int S, int M, int D, int Lq, int L, int P,
                     uni_stream_t stream);
/* e_ref [R,128], e_cur [Q,128] fp32 row-major (NHWC embedding maps), values [K,R] -> out [K,Q].
 * precision 0 = exact fp32 MFMA, 1 = fp32-equivalent bf16x3 split (6 bf16 MFMAs per product), 2 = fp32-equivalent f16x2 split
 * (3 f16 MFMAs per product; operands must lie inside the f16 range, |x| < 65504 / log2 e), 3 = the reference DRIVER's arithmetic
 * class (unicorn_sot.py:95-100 casts keys, queries, values to fp16): f16-rounded operands, one MFMA per product, f16-rounded scores
 * (not the `.half()` of the normalised softmax).  workspace: device scratch of >= uni_corr_workspace_bytes bytes. */
size_t uni_corr_workspace_bytes(int R, int Q, int K);
int uni_corr_softmax_pv(const float* e_ref, const float* e_cur, const float* values, float* out, int R, int Q, int D,
                        int K, int precision, void* workspace, size_t workspace_bytes, uni_stream_t stream);
/* The same for B frames in ONE launch (the time-batched SOT step, unicorn_sot.py:88-105 per frame): e_ref [B,R,128], e_cur [B,Q,128],
 * values [K,R] shared by the frames (values_per_frame = 0) or [B,K,R] -> out [B,K,Q].  workspace >= uni_corr_workspace_bytes_batched. */
size_t uni_corr_workspace_bytes_batched(int B, int R, int Q, int K);
int uni_corr_softmax_pv_batched(const float* e_ref, const float* e_cur, const float* values, float* out, int B, int R, int Q, int D,
                                int K, int values_per_frame, int precision, void* workspace, size_t workspace_bytes,
                                uni_stream_t stream);
/* The same operator for TRAINING: the label propagation of the reference's losses (unicorn/models/unicorn.py:321-326, compute_loss_sot,
 * and :342-371, compute_loss_vos):  simi_mat = bmm(embed_0^T, embed_1); trans_mat_01 = softmax(simi_mat, dim=1);
 * pred_lbs1 = bmm(gt_lbs_0, trans_mat_01), whose R x Q matrices (1 GB each in fp32 at 800 x 1280, kept by autograd) never exist here.
 *   uni_corr_softmax_pv_lse  = uni_corr_softmax_pv_batched (same kernels, `out` bitwise equal) that also stores
 *                              lse[b,q] = log sum_r exp(S[r,q])   [B,Q]
 *   uni_corr_softmax_pv_bwd  given grad_out = d loss / d out [B,K,Q] and the forward's out / lse, writes
 *                              grad_e_ref [B,R,128], grad_e_cur [B,Q,128], grad_values [B,K,R] ([K,R], summed over the frames, when
 *                              values_per_frame = 0).  Each of the three may be NULL: that gradient is not computed.  P is recomputed
 *                              tile by tile; every output row has ONE writer (two recompute passes, no atomics), so the results are
 *                              bitwise reproducible and completely written by the call.
 * precision: 0 (exact fp32 MFMA) is the only backward arithmetic; any other value is refused by _bwd (the forward accepts 0..3).
 * workspace >= uni_corr_bwd_workspace_bytes (covers both calls), 16-byte aligned like the embeddings.  The _f64 pair is a plain
 * double-precision evaluation (FMA loops, one writer per element, no workspace) for gradcheck and fixtures on small problems. */
size_t uni_corr_bwd_workspace_bytes(int B, int R, int Q, int K);
int uni_corr_softmax_pv_lse(const float* e_ref, const float* e_cur, const float* values, float* out, float* lse, int B, int R, int Q,
                            int D, int K, int values_per_frame, int precision, void* workspace, size_t workspace_bytes,
                            uni_stream_t stream);
int uni_corr_softmax_pv_bwd(const float* e_ref, const float* e_cur, const float* values, const float* out, const float* lse,
                            const float* grad_out, float* grad_e_ref, float* grad_e_cur, float* grad_values, int B, int R, int Q,
                            int D, int K, int values_per_frame, int precision, void* workspace, size_t workspace_bytes,
                            uni_stream_t stream);
int uni_corr_softmax_pv_lse_f64(const double* e_ref, const double* e_cur, const double* values, double* out, double* lse, int B, int R,
                                int Q, int D, int K, int values_per_frame, uni_stream_t stream);
int uni_corr_softmax_pv_bwd_f64(const double* e_ref, const double* e_cur, const double* values, const double* out, const double* lse,
                                const double* grad_out, double* grad_e_ref, double* grad_e_cur, double* grad_values, int B, int R,
                                int Q, int D, int K, int values_per_frame, uni_stream_t stream);
int uni_prior_pyramid(const float* p8, float* p16, float* p32, int K, int H8, int W8, uni_stream_t stream);
int uni_label_map_s8(const float* box_xyxy_dev, float* out, int H, int W, uni_stream_t stream);
int uni_sample_embeddings(const float* embed_nhwc, int H8, int W8, int C, const float* boxes_xyxy, int ld_boxes, int n,
                          float stride, float* out, uni_stream_t stream);
/* mask_feats (H8,W8,8), up_masks (H8,W8,9*r*r) NHWC fp32; params (n,169) row stride ldp; inst_loc (n,2);
 * inst_lvl (n) int32 -> out (n, d_rate*r*H8, d_rate*r*W8) sigmoid scores.  workspace >= n*H8*W8*(1+r*r)*4 bytes */
int uni_condinst_masks(const float* mask_feats, const float* up_masks, const float* params, int ldp,
                       const float* inst_loc, const int32_t* inst_lvl, int n, int H8, int W8, int up_rate, int d_rate,
                       float* out, void* workspace, size_t workspace_bytes, uni_stream_t stream);
/* The CondInst mask loss for TRAINING (unicorn/models/condinst/dynamic_mask_head.py:247-278 with :138-170, :172-225 and dice_coefficient
 * :50-58; called per image on the SimOTA foreground anchors by unicorn_head_mask.py:676-694): the arguments of uni_condinst_masks plus
 * gt [n][r H8][r W8] (0 / 1 maps in the floating type) -> loss [n] = 1 - 2 I / U per instance, sums [n][3] = (I = sum s g, sum s^2,
 * sum g^2), U = sum s^2 + sum g^2 + 1e-5, s = sigmoid of the x r convex-upsampled logits.  No n x rH8 x rW8 map is ever stored.
 *   uni_condinst_loss_bwd  given grad_loss [n] and the forward's sums, recomputes s from the coarse logits and writes
 *                            grad_mask_feats [H8][W8][8], grad_up_masks [H8][W8][9 r r], grad_params [n] rows of pitch ldp (169 columns
 *                            written).  Each may be NULL: that gradient is not computed.  inst_loc / inst_lvl / gt carry no gradient.
 *                            One writer per element, fixed summation orders, no atomics: bitwise reproducible, completely written.
 * inst_lvl outside 0..4 is clamped to that range (the reference's index into sizes_of_interest would fail instead).
 * up_rate 1..16, n <= 65535, H8 W8 r r < 2^30 (uni_condinst_loss_workspace_bytes returns 0 for shapes the calls refuse).
 * workspace: device scratch of >= uni_condinst_loss_workspace_bytes bytes (fp32; the _f64 forms need twice that),
 * 8-byte aligned, O(n H8 W8); nothing is kept in it between the two calls.  n must be > 0.  The _f64 pair is the same templated
 * code in double precision, for gradcheck and fixtures. */
size_t uni_condinst_loss_workspace_bytes(int n, int H8, int W8, int up_rate);
int uni_condinst_loss_fwd(const float* mask_feats, const float* up_masks, const float* params, int ldp, const float* inst_loc,
                          const int32_t* inst_lvl, const float* gt, int n, int H8, int W8, int up_rate, float* loss, float* sums,
                          void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_condinst_loss_bwd(const float* mask_feats, const float* up_masks, const float* params, int ldp, const float* inst_loc,
                          const int32_t* inst_lvl, const float* gt, const float* sums, const float* grad_loss, int n, int H8, int W8,
                          int up_rate, float* grad_mask_feats, float* grad_up_masks, float* grad_params, void* workspace,
                          size_t workspace_bytes, uni_stream_t stream);
int uni_condinst_loss_fwd_f64(const double* mask_feats, const double* up_masks, const double* params, int ldp, const double* inst_loc,
                              const int32_t* inst_lvl, const double* gt, int n, int H8, int W8, int up_rate, double* loss, double* sums,
                              void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_condinst_loss_bwd_f64(const double* mask_feats, const double* up_masks, const double* params, int ldp, const double* inst_loc,
                              const int32_t* inst_lvl, const double* gt, const double* sums, const double* grad_loss, int n, int H8,
                              int W8, int up_rate, double* grad_mask_feats, double* grad_up_masks, double* grad_params, void* workspace,
                              size_t workspace_bytes, uni_stream_t stream);
/* SimOTA label assignment of the head loss for a whole BATCH (unicorn/models/unicorn_head_mask.py:754-983: get_assignments,
 * get_in_boxes_info, dynamic_k_matching, with bboxes_iou of unicorn/utils/boxes.py:154-177), fp32, in four launches whatever the number of
 * boxes or images, without a host synchronisation and without any tensor of size boxes x anchors x classes.
 *   outputs  [B][A] rows of pitch ld_out >= 5 + C: decoded cx, cy, w, h, then the objectness logit and C class logits
 *   labels   [B][M][5]: class, cx, cy, w, h; image b uses its first num_gt[b] rows (num_gt [B] int32 on the DEVICE, clamped to 0..M)
 *   x_shifts, y_shifts, strides [A]: the anchor centre is shift * stride + 0.5 * stride;  img_h, img_w clip the box centres
 *   -> fg_mask [B][A] (1 = anchor matched), matched_gt [B][A] (box index, -1 for background), matched_iou [B][A] (IoU with the matched
 *      box, 0 for background), num_fg [B] (matches per image).  Every output is completely written, also for images with num_gt == 0.
 * An anchor is a candidate when its centre lies strictly inside some box or inside the 2.5-stride square around some (clipped) box centre;
 * cost = sum_c BCE(sqrt(sigmoid(cls) sigmoid(obj)), onehot(class)) + 3 (-log(iou + 1e-8)) + 1e5 (not inside box AND square); box g takes
 * its k_g = max(1, int(sum of its 10 largest IoUs)) cheapest candidates; an anchor taken by several boxes goes to the cheapest of ALL boxes.
 * Ties, which PyTorch leaves open: the lower anchor index wins in both top-k passes, the lower box index in the arg-min.  Only integer
 * atomics are used: two calls give the same bits.  A class outside 0..C-1 is clamped (the reference's one_hot would fail instead).
 * Limits: 1 <= B <= 65535, 1 <= A < 2^24, 0 <= M <= 1024, 1 <= C <= 256; other shapes are refused with an error string and
 * uni_simota_workspace_bytes returns 0 for them.
 * workspace: 4-byte aligned device scratch of >= uni_simota_workspace_bytes(B, A, M, C) bytes, which is at most
 * 3 * B * M * A * 4 bytes (two B x M x A fp32 planes are used: cost and IoU) plus 4 * B * A * (C + 4) bytes plus 2 KiB of alignment;
 * it has no term with M * A * C. */
size_t uni_simota_workspace_bytes(int B, int A, int Gmax, int C);
int uni_simota_assign(const float* outputs, int ld_out, const float* labels, const int32_t* num_gt, int M, const float* x_shifts,
                      const float* y_shifts, const float* strides, int B, int A, int C, int img_h, int img_w, uint8_t* fg_mask,
                      int32_t* matched_gt, float* matched_iou, int32_t* num_fg, void* workspace, size_t workspace_bytes,
                      uni_stream_t stream);
/* The four detection losses of the head for a whole BATCH (the rest of get_losses, unicorn/models/unicorn_head_mask.py:646-745, identically
 * unicorn_head.py:484-681, with IOUloss of unicorn/models/losses.py:15-36, loss_type "iou"), forward and backward, fed by the device-side
 * results of uni_simota_assign: two launches forward and two backward whatever B, A, M, C and the foreground counts, without a host
 * synchronisation, a read-back or an allocation.
 *   outputs      [B][A] rows of pitch ld_out >= 5 + C: decoded cx, cy, w, h, then the objectness logit and C class logits
 *   origin_preds [B][A] rows of pitch ld_org >= 4: the raw regression outputs; NULL = use_l1 False (the L1 loss is 0)
 *   labels       [B][M][5]: class, cx, cy, w, h (may be NULL when M == 0; with M == 0 every anchor is background)
 *   fg_mask [B][A] uint8, matched_gt [B][A] int32, matched_iou [B][A]: what uni_simota_assign wrote
 *   num_fg, num_gt [B] int32 on the DEVICE (clamped to 0..A and 0..M);  x_shifts, y_shifts, strides [A]
 *   -> out[5] = reg_weight x loss_iou, loss_obj, loss_cls, loss_l1, n / max(sum num_gt, 1) (the reference's quirk: its ratio divides the
 *      clamped count, so it is 1.0 with no box at all), every loss divided by n = max(sum_b num_fg[b], 1) read from device memory:
 *      obj  sum over ALL anchors of bce(obj_logit, fg);   iou  sum over foreground anchors of 1 - iou(pred, gt[matched])^2;
 *      cls  sum over foreground anchors and classes of bce(cls_logit_c, c == class ? matched_iou : 0);
 *      l1   sum over foreground anchors and 4 components of |origin - t|, t = (gx / s - x_shift, gy / s - y_shift, log(gw / s + 1e-8),
 *           log(gh / s + 1e-8)) (:747-752);   bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)).
 *      IoU as losses.py:15-36: edges = centre -+ size / 2, tl = max, br = min, en = (tl < br) strictly on both axes,
 *      area_i = (br - tl).prod * en, iou = area_i / (area_p + area_g - area_i + 1e-16).
 *   uni_head_loss_bwd  given grad_out[4] on the device (the weights of out[0..3]) writes grad_outputs [B][A] rows of pitch
 *      ld_grad >= 5 + C, columns 0 .. 4 + C (the pitch padding is not touched), and grad_origin [B][A][4] COMPLETELY, one writer per
 *      element: the objectness column of every anchor (sigmoid(x) - fg) g_obj / n; box and class columns and grad_origin of background
 *      anchors exact zeros; class columns of foreground anchors (sigmoid(x_c) - t_c) g_cls / n; grad_origin sign(origin - t) g_l1 / n
 *      with sign(0) = 0; box columns -2 iou d iou / d (cx, cy, w, h) reg_weight g_iou / n through the max / min of the edges, exactly zero
 *      where en == 0.  Tie rule: where a predicted edge equals the ground-truth edge it is compared with, the gradient is split half and
 *      half, as torch's maximum / minimum do.  Either gradient pointer may be NULL: not computed (grad_origin needs origin_preds).
 *      The backward recomputes from the inputs; nothing is kept in the workspace between the two calls.
 * The kernels never index labels with a matched_gt outside 0..M-1 on a foreground anchor: such a value is clamped; a class outside
 * 0..C-1 is clamped as the assignment does.  The sums are accumulated in double in both precisions, in a fixed order, and the box, IoU and
 * L1 lines of a foreground anchor are evaluated in double in the fp32 form as well (the foreground is sparse); there is no atomic: two
 * calls give the same bits.
 * Limits: 1 <= B <= 65535, 1 <= A < 2^24, 0 <= M <= 1024, 1 <= C <= 256; other shapes are refused with an error string and
 * uni_head_loss_workspace_bytes returns 0 for them.
 * workspace: 8-byte aligned device scratch of >= uni_head_loss_workspace_bytes(B, A, C) = B * ceil(A / 256) * 32 bytes rounded up to a
 * multiple of 256 (four double partial sums per block of 256 anchors), the same in both precisions.
 * The _f64 forms are the same templated code in double precision, for gradcheck and fixtures: every floating-point array is double there
 * (matched_iou included, so that the fp64 run of the reference can be fed exactly); fg_mask, matched_gt, num_fg and num_gt stay as above. */
size_t uni_head_loss_workspace_bytes(int B, int A, int C);
int uni_head_loss_fwd(const float* outputs, int ld_out, const float* origin_preds, int ld_org, const float* labels, int M, const uint8_t* fg_mask,
                      const int32_t* matched_gt, const float* matched_iou, const int32_t* num_fg, const int32_t* num_gt, const float* x_shifts,
                      const float* y_shifts, const float* strides, int B, int A, int C, double reg_weight, float* out, void* workspace,
                      size_t workspace_bytes, uni_stream_t stream);
int uni_head_loss_bwd(const float* outputs, int ld_out, const float* origin_preds, int ld_org, const float* labels, int M, const uint8_t* fg_mask,
                      const int32_t* matched_gt, const float* matched_iou, const int32_t* num_fg, const int32_t* num_gt, const float* x_shifts,
                      const float* y_shifts, const float* strides, const float* grad_out, int B, int A, int C, double reg_weight,
                      float* grad_outputs, int ld_grad, float* grad_origin, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_head_loss_fwd_f64(const double* outputs, int ld_out, const double* origin_preds, int ld_org, const double* labels, int M,
                          const uint8_t* fg_mask, const int32_t* matched_gt, const double* matched_iou, const int32_t* num_fg,
                          const int32_t* num_gt, const double* x_shifts, const double* y_shifts, const double* strides, int B, int A, int C,
                          double reg_weight, double* out, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_head_loss_bwd_f64(const double* outputs, int ld_out, const double* origin_preds, int ld_org, const double* labels, int M,
                          const uint8_t* fg_mask, const int32_t* matched_gt, const double* matched_iou, const int32_t* num_fg,
                          const int32_t* num_gt, const double* x_shifts, const double* y_shifts, const double* strides, const double* grad_out,
                          int B, int A, int C, double reg_weight, double* grad_outputs, int ld_grad, double* grad_origin, void* workspace,
                          size_t workspace_bytes, uni_stream_t stream);
/* Head-output assembly for a whole BATCH: the lines that turn the head's prediction convolutions into what the loss operators above read
 * (unicorn/models/unicorn_head_mask.py:339-366 of forward, get_output_and_grid :476-500 and the level cats :396-401 / :554-558; identically
 * unicorn_head.py, yolo_head_det.py, yolo_head_det_mask.py; n_anchors == 1), forward and backward in ONE launch each whatever B, L, C, P and
 * the layouts, without a host synchronisation, a workspace, a table upload or an atomic: one writer per element, two calls give the same bits.
 *   reg, obj, cls, ctrl   HOST arrays of L DEVICE pointers: the maps (B,4,h_l,w_l), (B,1,h_l,w_l), (B,C,h_l,w_l), (B,P,h_l,w_l) of level l,
 *                         all of the element type map_dtype names (0 = the type of the entry: fp32, fp64 in the _f64 form; 1 = fp16,
 *                         2 = bf16, fp32 form only).  ctrl NULL (then P == 0): no controller maps.
 *   hs, ws, strides       HOST arrays of L: the level sizes and the positive stride of the level
 *   layouts               HOST array of L: bit 0 / 1 / 2 / 3 set = the reg / obj / cls / ctrl map of the level is NCHW-contiguous, clear =
 *                         channels-last memory [B][h][w][channels]
 * Anchor a = off_l + y w_l + x with off_l = sum_{k<l} h_k w_k, A = sum h_l w_l.  uni_head_assemble_fwd writes (a NULL result is skipped)
 *   outputs [B][A] rows of pitch ld_out >= 5 + C: (reg0 + x) * s, (reg1 + y) * s, exp(reg2) * s, exp(reg3) * s, obj, cls[0 .. C-1]; the two
 *                         leading columns as an add and then a multiply, never an fma; exp is the full-precision function
 *   origin_preds [B][A][4] the raw reg channels;   x_shifts, y_shifts, expanded_strides [A]: x, y, s;
 *   dynamic_params [B][A] rows of pitch ld_par >= P: ctrl[b][p][y][x];   fpn_levels [B][A] int32: l.   The pitch padding is never touched.
 * Half maps are read as stored and decoded in fp32: the result has the bits of the fp32 call on the widened maps.
 * uni_head_assemble_bwd reads grad_outputs (pitch ld_gout), grad_origin [B][A][4], grad_params (pitch ld_gpar) -- each may be NULL = zero --
 * and writes, for every non-NULL entry of the HOST arrays grad_reg / grad_obj / grad_cls / grad_ctrl (an array may be NULL as a whole), the
 * gradient of that map COMPLETELY in the element type and layout of the map, rounded once:
 *   g_reg[0:2] = s g_out[0:2] + g_org[0:2];  g_reg[2:4] = s g_out[2:4] exp(reg[2:4]) + g_org[2:4];  g_obj = g_out[4];  g_cls = g_out[5:];
 *   g_ctrl[b][p][y][x] = g_par[b][a][p].   reg is read only where grad_reg asks (it may be NULL otherwise).
 * Limits: 1 <= L <= 4, 1 <= B <= 65535, 1 <= C <= 256, 1 <= P <= 1024 (0 without ctrl), h_l, w_l >= 1, A < 2^24, strides positive and finite;
 * other shapes are refused with an error string before anything is launched.  A block assembles a tile of 64 anchors of one level through LDS.
 * The _f64 forms are the same templated code in double precision for gradcheck and fixtures (maps and results fp64, map_dtype 0). */
int uni_head_assemble_fwd(const void* const* reg, const void* const* obj, const void* const* cls, const void* const* ctrl, const int32_t* hs,
                          const int32_t* ws, const double* strides, const int32_t* layouts, int L, int B, int C, int P, int map_dtype,
                          float* outputs, int ld_out, float* origin_preds, float* x_shifts, float* y_shifts, float* expanded_strides,
                          float* dynamic_params, int ld_par, int32_t* fpn_levels, uni_stream_t stream);
int uni_head_assemble_bwd(const void* const* reg, const int32_t* hs, const int32_t* ws, const double* strides, const int32_t* layouts, int L, int B,
                          int C, int P, int map_dtype, const float* grad_outputs, int ld_gout, const float* grad_origin,
                          const float* grad_params, int ld_gpar, void* const* grad_reg, void* const* grad_obj, void* const* grad_cls,
                          void* const* grad_ctrl, uni_stream_t stream);
int uni_head_assemble_fwd_f64(const void* const* reg, const void* const* obj, const void* const* cls, const void* const* ctrl, const int32_t* hs,
                              const int32_t* ws, const double* strides, const int32_t* layouts, int L, int B, int C, int P, int map_dtype,
                              double* outputs, int ld_out, double* origin_preds, double* x_shifts, double* y_shifts, double* expanded_strides,
                              double* dynamic_params, int ld_par, int32_t* fpn_levels, uni_stream_t stream);
int uni_head_assemble_bwd_f64(const void* const* reg, const int32_t* hs, const int32_t* ws, const double* strides, const int32_t* layouts, int L,
                              int B, int C, int P, int map_dtype, const double* grad_outputs, int ld_gout, const double* grad_origin,
                              const double* grad_params, int ld_gpar, void* const* grad_reg, void* const* grad_obj, void* const* grad_cls,
                              void* const* grad_ctrl, uni_stream_t stream);
/* The CondInst mask loss of the head for a whole BATCH (unicorn/models/unicorn_head_mask.py:568-569, :675-694, :731-732 with
 * dynamic_mask_head.py:247-278), forward and backward, fed by the device-side results of uni_simota_assign: 5 launches forward and at most 22
 * backward whatever the data, B, A, M and capacity, without a host synchronisation, a read-back or an allocation.
 *   mask_feats [B][H8][W8][8], up_masks [B][H8][W8][9 r r] NHWC;  params [B][A] rows of pitch ldp >= 169;  fpn_levels [B][A] int32
 *   masks [B][M][r H8][r W8] (0 / 1 maps in the floating type, M >= 1), READ IN PLACE: no per-instance copy of a ground-truth map exists
 *   fg_mask [B][A] uint8, matched_gt [B][A] int32: what uni_simota_assign wrote (a matched_gt outside 0..M-1 is clamped)
 *   x_shifts, y_shifts, strides [A]: the instance of anchor a is located at stride (shift + 0.5)
 *   -> out[1 + B]: out[1 + b] = loss_mask[b] = the mean of uni_condinst_loss_fwd's per-instance loss over the foreground anchors of image b
 *      in ascending anchor order (an exact 0 without foreground), out[0] = sum_b loss_mask[b] / max(number of images with foreground, 1);
 *      sums [capacity][3]: the three dice sums per instance slot, for the backward.
 * The instance table (slot -> image, anchor, mask row; per-image counts and offsets; the number of valid images) is built on the device by
 * a scan in ascending (image, anchor) order; grids are sized from the geometry and from `capacity`, the number of instance slots the
 * workspace holds, and blocks loop over the counts they read from the table.  If the batch has MORE foreground anchors than capacity,
 * nothing is indexed by a slot: out[0 .. B] are NaN and the backward writes exact zeros (visible in the logged loss; never a silent
 * truncation).  B * min(A, 10 M) can never overflow after uni_simota_assign (a box takes at most 10 anchors).
 *   uni_head_mask_loss_bwd  given grad_out[1] on the device (the weight of out[0]) and the forward's sums, recomputes the logits and
 *      writes grad_mask_feats [B][H8][W8][8], grad_up_masks [B][H8][W8][9 r r] and the DENSE grad_params [B][A] rows of pitch
 *      ld_grad >= 169 (169 columns; background rows and images without foreground: exact zeros) COMPLETELY.  Each may be NULL: that
 *      gradient is not computed.  One writer per element, fixed summation orders, no atomics: bitwise reproducible.
 * Limits: 1 <= B <= 65535, A >= 1, B A <= 2^28, M >= 1, up_rate 1..16, H8 W8 r r < 2^30, 1 <= capacity <= 2^24; other shapes are
 * refused with an error string and uni_head_mask_loss_workspace_bytes returns 0 for them.
 * workspace: 8-byte aligned device scratch of >= uni_head_mask_loss_workspace_bytes bytes (fp32; the _f64 forms need twice that) =
 * 4 (4 + 2 B + 4 capacity + B A) for the table, rounded up to 8, plus 4 bytes x [capacity (2 H8 W8 + 3 ceil(H8 W8 / floor(256 / r^2)) +
 * 169 ceil(H8 W8 / 1024) + 3) + 9 ceil(capacity / 8) H8 W8 + 64 B H8 W8]: O(capacity H8 W8), about 3.5 coarse maps per slot at up_rate 4
 * (the backward stages its 9 tap sums per pixel in 8 passes over the instance range, which is where the launch count comes from).  Nothing
 * is kept in it between the two calls.  The _f64 pair is the same templated code in double precision, for gradcheck and fixtures. */
size_t uni_head_mask_loss_workspace_bytes(int B, int A, int H8, int W8, int up_rate, int capacity);
int uni_head_mask_loss_fwd(const float* mask_feats, const float* up_masks, const float* params, int ldp, const int32_t* fpn_levels, const float* masks, int M,
    const uint8_t* fg_mask, const int32_t* matched_gt, const float* x_shifts, const float* y_shifts, const float* strides, int B, int A, int H8, int W8,
    int up_rate, int capacity, float* out, float* sums, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_head_mask_loss_bwd(const float* mask_feats, const float* up_masks, const float* params, int ldp, const int32_t* fpn_levels, const float* masks, int M,
    const uint8_t* fg_mask, const int32_t* matched_gt, const float* x_shifts, const float* y_shifts, const float* strides, int B, int A, int H8, int W8,
    int up_rate, int capacity, const float* sums, const float* grad_out, float* grad_mask_feats, float* grad_up_masks,
    float* grad_params, int ld_grad, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_head_mask_loss_fwd_f64(const double* mask_feats, const double* up_masks, const double* params, int ldp, const int32_t* fpn_levels, const double* masks, int M,
    const uint8_t* fg_mask, const int32_t* matched_gt, const double* x_shifts, const double* y_shifts, const double* strides, int B, int A, int H8, int W8,
    int up_rate, int capacity, double* out, double* sums, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_head_mask_loss_bwd_f64(const double* mask_feats, const double* up_masks, const double* params, int ldp, const int32_t* fpn_levels, const double* masks, int M,
    const uint8_t* fg_mask, const int32_t* matched_gt, const double* x_shifts, const double* y_shifts, const double* strides, int B, int A, int H8, int W8,
    int up_rate, int capacity, const double* sums, const double* grad_out, double* grad_mask_feats, double* grad_up_masks,
    double* grad_params, int ld_grad, void* workspace, size_t workspace_bytes, uni_stream_t stream);
/* The MOT instance-contrastive loss for TRAINING (unicorn/models/unicorn.py:407-466, compute_loss_mot_corr) for a whole BATCH, forward and
 * backward, in a constant number of launches (5 forward, 8 backward) whatever B, M and the instance counts, without a host
 * synchronisation, a read-back or an allocation.
 *   embed_0, embed_1  (B, C, H, W) maps of the two frames, read through ELEMENT strides strides_f[4] = (batch, channel, row, column) given
 *                     as host arrays: NCHW and NHWC (channels-last) memory both work without a copy.  Strides are >= 0.
 *   targets           [B][2][M][6] fp32, contiguous: rows (class, cx, cy, w, h, track id) of frame 0 and frame 1; fp32 in the _f64 forms too
 *   stride            the reference's `s` (8): input pixels per map pixel;  flags: UNI_MOT_BIDIRECT | UNI_MOT_GRID_SAMPLE
 *   -> loss [B], one value per sample (the reference returns their mean).
 * Per sample: n_f = number of rows of frame f with id != 0, and the instances are the FIRST n_f rows whatever their ids (the reference's
 * range(n_f)); row[i] = smallest j < n1 with id1[j] == id0[i] (fp32 compare), col[j] = LARGEST i < n0 with row[i] == j (the
 * reference's overwrite order), -1 where there is none; E_f[i] = the embedding at the centre of instance i, with GRID_SAMPLE by
 * g = (clamp(c / stride - 0.5, 0, size-1) / (size-1) - 0.5) * 2 (fp32 in both precisions) handed to grid_sample(bilinear, border,
 * align_corners=False), i.e. x = clip(((g + 1) size - 1) / 2, 0, size-1) in the map's precision; without it the one pixel
 * rint(clamp(c / stride, 0, size-1)) (half to even).  S = E_0 E_1^T; loss = 0.5 (CE(S, row) + CE(S^T, col)) with BIDIRECT, else
 * CE(S, row); CE is the mean over the labelled rows (ignore_index = -1) with max-subtracted log-sum-exps.
 * A sample without a matched pair gives NaN and a gradient of exactly zero (as torch's cross_entropy does).  A sample with n0 == 0 or
 * n1 == 0 -- where the reference raises -- gives NaN and a zero gradient as well; other samples are not affected.
 *   uni_mot_corr_loss_bwd  given grad_loss [B], writes the dense gradients grad_embed_f (B, C, H, W) COMPLETELY through grad_strides_f (all
 *                          >= 1 and non-overlapping: refused otherwise): zeros, plus every instance's dE spread over its one to four source pixels with the
 *                          forward's weights.  Either may be NULL: that gradient is not computed.  Targets carry no gradient.
 * One writer per element and fixed summation orders, no float atomics: two calls give the same bits.
 * Limits: 1 <= B <= 65535, 1 <= M <= 1024, 1 <= C <= 1024, C H W < 2^31; other shapes are refused with an error string and
 * uni_mot_corr_workspace_bytes returns 0 for them.
 * workspace: 8-byte aligned device scratch of >= uni_mot_corr_workspace_bytes(B, M, C) bytes (fp32; the _f64 forms need twice that),
 * 4 B M (4 C + M + 14) + 16 B bytes plus at most 9 x 256 of alignment; nothing is kept in it between the two calls (the backward recomputes from the inputs). */
#define UNI_MOT_BIDIRECT 1
#define UNI_MOT_GRID_SAMPLE 2
size_t uni_mot_corr_workspace_bytes(int B, int M, int C);
int uni_mot_corr_loss_fwd(const float* embed_0, const int64_t* strides_0, const float* embed_1, const int64_t* strides_1, const float* targets,
                          int B, int C, int H, int W, int M, float stride, int flags, float* loss, void* workspace, size_t workspace_bytes,
                          uni_stream_t stream);
int uni_mot_corr_loss_bwd(const float* embed_0, const int64_t* strides_0, const float* embed_1, const int64_t* strides_1, const float* targets,
                          const float* grad_loss, int B, int C, int H, int W, int M, float stride, int flags, float* grad_embed_0,
                          const int64_t* grad_strides_0, float* grad_embed_1, const int64_t* grad_strides_1, void* workspace,
                          size_t workspace_bytes, uni_stream_t stream);
int uni_mot_corr_loss_fwd_f64(const double* embed_0, const int64_t* strides_0, const double* embed_1, const int64_t* strides_1,
                              const float* targets, int B, int C, int H, int W, int M, float stride, int flags, double* loss, void* workspace,
                              size_t workspace_bytes, uni_stream_t stream);
int uni_mot_corr_loss_bwd_f64(const double* embed_0, const int64_t* strides_0, const double* embed_1, const int64_t* strides_1,
                              const float* targets, const double* grad_loss, int B, int C, int H, int W, int M, float stride, int flags,
                              double* grad_embed_0, const int64_t* grad_strides_0, double* grad_embed_1, const int64_t* grad_strides_1,
                              void* workspace, size_t workspace_bytes, uni_stream_t stream);

/* The opening of a ConvNeXt block for TRAINING (unicorn/models/backbone/convnext.py:32-33,43-45: dwconv = Conv2d(dim, dim, 7, padding=3,
 * groups=dim), permute to (N, H, W, C), LayerNorm over C with eps inside the square root), forward and recomputing backward for a whole
 * batch: one launch forward, at most four backward whatever the shape, no host synchronisation, no read-back, no allocation.  Operator
 * only: the model-level engine stays inference only.
 *   x, y, grad_y, grad_x  dense [B][H][W][C] (channels-last memory of an (B, C, H, W) tensor)
 *   weight, grad_weight   [49][C], tap t = ky * 7 + kx: the layout uni_dwconv7_ln_ex takes (the module's (C, 1, 7, 7) transposed)
 *   bias, ln_weight, ln_bias and their gradients  [C]
 *   stats                 [B H W][2] = mean and 1 / sqrt(var + eps) of every pixel, written by the forward, read by the backward
 *   uni_dwln_train_fwd  y = (u - mean) * rstd * ln_weight + ln_bias with u = conv7x7(x, zero padding 3) + bias; the variance is the mean of
 *                       (u - mean)^2 (two passes over registers).  Writes y and stats COMPLETELY.
 *   uni_dwln_train_bwd  recomputes u from x, then writes grad_x, grad_weight + grad_bias, grad_ln_weight + grad_ln_bias COMPLETELY.  grad_x,
 *                       the pair grad_weight / grad_bias and the pair grad_ln_weight / grad_ln_bias may each be NULL: that gradient is not
 *                       computed (a pair is given or left out as a whole), and the convolution passes over the workspace are skipped when neither
 *                       grad_x nor grad_weight is wanted.
 * One writer per element, fixed summation orders (partials of a block in ascending wave order, blocks in ascending order in double), no
 * float atomics: two calls give the same bits.  A map may be smaller than the window; nothing of a neighbouring image enters a halo.
 * Limits: B, H, W >= 1, C % 4 == 0, 4 <= C <= 2048, B H W < 2^31 (element offsets are 64-bit), pointers 16-byte aligned; other shapes are
 * refused with an error string and uni_dwln_train_workspace_bytes returns 0 for them.
 * workspace (backward only): 16-byte aligned device scratch of >= uni_dwln_train_workspace_bytes(B, H, W, C) bytes (fp32; the _f64 forms need
 * twice that) = 4 (up(B H W C) + up(2 C RA) + up(50 C RB)), up = round up to 64, RA = min(ceil(B H ceil(W / 2) / NS), 1024) with
 * NS = 512 / (64 ceil(C / 256)) rounded down, RB = ceil(B H ceil(W / slen) / 4) with slen = ceil(W / ceil(W / 128)): du, the per-block partials of
 * grad_ln_weight / grad_ln_bias and of grad_weight / grad_bias.  Nothing is kept in it between calls. */
size_t uni_dwln_train_workspace_bytes(int B, int H, int W, int C);
int uni_dwln_train_fwd(const float* x, const float* weight, const float* bias, const float* ln_weight, const float* ln_bias, double eps, int B,
                       int H, int W, int C, float* y, float* stats, uni_stream_t stream);
int uni_dwln_train_bwd(const float* x, const float* weight, const float* bias, const float* ln_weight, const float* stats, const float* grad_y,
                       int B, int H, int W, int C, float* grad_x, float* grad_weight, float* grad_bias, float* grad_ln_weight,
                       float* grad_ln_bias, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_dwln_train_fwd_f64(const double* x, const double* weight, const double* bias, const double* ln_weight, const double* ln_bias, double eps,
                           int B, int H, int W, int C, double* y, double* stats, uni_stream_t stream);
int uni_dwln_train_bwd_f64(const double* x, const double* weight, const double* bias, const double* ln_weight, const double* stats,
                           const double* grad_y, int B, int H, int W, int C, double* grad_x, double* grad_weight, double* grad_bias,
                           double* grad_ln_weight, double* grad_ln_bias, void* workspace, size_t workspace_bytes, uni_stream_t stream);

/* The close of a ConvNeXt block for TRAINING (unicorn/models/backbone/convnext.py:49-53: layer scale gamma * x, permute to (N, C, H, W),
 * input + drop_path(x)), forward and backward for a whole batch: one launch forward, at most two backward, no host synchronisation, no
 * read-back, no allocation, no atomics.  Operator only: the model-level engine stays inference only.
 *   y, grad_y            dense [B][H][W][C], the output of pwconv2.  y_dtype: 0 = the type of the form (fp32, fp64 in the _f64 form), 1 = fp16,
 *                        2 = bf16 (fp32 form only); grad_y has the type of y.  Conversion in registers, all arithmetic fp32 (fp64).
 *   residual, grad_out   nchw == 0: dense [B][H][W][C] (channels-last memory of a (B, C, H, W) tensor), nchw != 0: dense [B][C][H][W]
 *   out                  dense [B][H][W][C], always
 *   gamma, grad_gamma    [C]; gamma may be NULL (= 1)
 *   scale                [B], the per-sample drop-path factor (0 or 1 / keep); may be NULL (= 1)
 *   uni_block_tail_fwd   out[n][c][h][w] = residual[n][c][h][w] + (gamma[c] * y[n][h][w][c]) * scale[n].  Writes out COMPLETELY.
 *   uni_block_tail_bwd   grad_y[n][h][w][c] = gamma[c] * (grad_out[n][c][h][w] * scale[n]) and grad_gamma[c] = sum over n, h, w of
 *                        (grad_out * scale[n]) * y, each written COMPLETELY; either may be NULL: its work is skipped (and the reduce launch when
 *                        grad_gamma is NULL; the workspace may then be NULL).  The gradient of residual is grad_out itself.
 * A sample with scale[n] == 0 is not read: out = residual, grad_y = 0, and it adds exactly 0 to grad_gamma even where y holds Inf or NaN
 * (the one deliberate difference to the eager lines, which give NaN there).  One writer per element, fixed summation orders (the lanes of a
 * block in ascending order, blocks in ascending order in double): two calls give the same bits.
 * Limits: B, H, W >= 1, C % 4 == 0, 4 <= C <= 2048, B H W < 2^31 (element offsets are 64-bit), the maps and the workspace 16-byte aligned
 * (gamma, scale and grad_gamma need their own type's alignment only); other shapes are refused with an error string and
 * uni_block_tail_workspace_bytes returns 0 for them.
 * workspace (backward with grad_gamma only): 16-byte aligned device scratch of >= uni_block_tail_workspace_bytes(B, H, W, C) bytes (fp32; the
 * _f64 form needs twice that) = 4 * 1024 * C: at most 1024 blocks along the pixels write one row of C partial sums each.  Nothing is kept in
 * it between calls. */
size_t uni_block_tail_workspace_bytes(int B, int H, int W, int C);
int uni_block_tail_fwd(const void* y, int y_dtype, const float* residual, int nchw, const float* gamma, const float* scale, int B, int H, int W,
                       int C, float* out, uni_stream_t stream);
int uni_block_tail_bwd(const void* y, int y_dtype, const float* grad_out, int nchw, const float* gamma, const float* scale, int B, int H, int W,
                       int C, void* grad_y, float* grad_gamma, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_block_tail_fwd_f64(const void* y, int y_dtype, const double* residual, int nchw, const double* gamma, const double* scale, int B, int H,
                           int W, int C, double* out, uni_stream_t stream);
int uni_block_tail_bwd_f64(const void* y, int y_dtype, const double* grad_out, int nchw, const double* gamma, const double* scale, int B, int H,
                           int W, int C, void* grad_y, double* grad_gamma, void* workspace, size_t workspace_bytes, uni_stream_t stream);

/* The channels-first LayerNorm between the ConvNeXt stages for TRAINING (unicorn/models/backbone/convnext.py:160-184, the
 * data_format == "channels_first" branch: u = x.mean(1), s = (x - u).pow(2).mean(1), x = (x - u) / sqrt(s + eps), weight[:, None, None] * x +
 * bias[:, None, None]), forward and backward for a whole batch: one launch forward, at most two backward, no host synchronisation, no
 * read-back, no allocation, no atomics.  Operator only: the model-level engine stays inference only.
 *   x, y, grad_y, grad_x  (B, C, H, W) maps, all four in ONE memory layout: nchw == 0: dense [B][H][W][C] (channels-last memory), nchw != 0:
 *                         dense [B][C][H][W].  Both are read and written in place.  x_dtype: 0 = the type of the form (fp32, fp64 in the _f64
 *                         form), 1 = fp16, 2 = bf16 (fp32 form only) is the type of x and grad_x; y and grad_y have the type of the form.
 *                         Conversion in registers, all arithmetic fp32 (fp64).
 *   weight, bias, grad_weight, grad_bias  [C]
 *   stats                 [B H W][2] = mean and 1 / sqrt(var + eps) of every pixel, written by the forward, read by the backward
 *   uni_lncf_train_fwd  y = weight * (x - mean) * rstd + bias; the variance is the mean of (x - mean)^2: a second pass over registers, and where
 *                       a block's waves share the channels of a pixel (nchw) the pairwise mean / M2 update of such two-pass parts.  Writes y
 *                       and stats COMPLETELY.
 *   uni_lncf_train_bwd  xhat = (x - mean) * rstd, t = grad_y * weight: grad_x = rstd * (t - mean_c t - xhat * mean_c (t * xhat)),
 *                       grad_weight[c] = sum over n, h, w of grad_y * xhat, grad_bias[c] = sum of grad_y, each written COMPLETELY.  grad_x and
 *                       the pair grad_weight / grad_bias may be NULL: that part is skipped (the reduce launch too when the pair is NULL; the
 *                       workspace may then be NULL and is not touched), what is computed has the same bits as in the full call.
 * One writer per element, fixed summation orders (the lanes of a block in a fixed tree, blocks in ascending order in double): two calls give
 * the same bits.
 * Limits: B, H, W >= 1, C % 4 == 0, 4 <= C <= 2048, B H W < 2^31 (element offsets are 64-bit), pointers 16-byte aligned (H W need not be a
 * multiple of anything: the rows of a channel plane are read element-wise); other shapes are refused with an error string and
 * uni_lncf_train_workspace_bytes returns 0 for them.
 * workspace (backward with grad_weight / grad_bias only): 16-byte aligned device scratch of >= uni_lncf_train_workspace_bytes(B, H, W, C) bytes
 * (fp32; the _f64 form needs twice that) = 4 * 1024 * 2 C: at most 1024 blocks write one row of [2][C] partial sums each.  Nothing is kept in
 * it between calls. */
size_t uni_lncf_train_workspace_bytes(int B, int H, int W, int C);
int uni_lncf_train_fwd(const void* x, int x_dtype, int nchw, const float* weight, const float* bias, double eps, int B, int H, int W, int C,
                       float* y, float* stats, uni_stream_t stream);
int uni_lncf_train_bwd(const void* x, int x_dtype, int nchw, const float* weight, const float* stats, const float* grad_y, int B, int H, int W,
                       int C, void* grad_x, float* grad_weight, float* grad_bias, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_lncf_train_fwd_f64(const void* x, int x_dtype, int nchw, const double* weight, const double* bias, double eps, int B, int H, int W,
                           int C, double* y, double* stats, uni_stream_t stream);
int uni_lncf_train_bwd_f64(const void* x, int x_dtype, int nchw, const double* weight, const double* stats, const double* grad_y, int B, int H,
                           int W, int C, void* grad_x, double* grad_weight, double* grad_bias, void* workspace, size_t workspace_bytes,
                           uni_stream_t stream);

/* The four downsample layers of the ConvNeXt backbone for TRAINING (unicorn/models/backbone/convnext.py:77-87: the stem Conv2d(in_chans, C0,
 * 4, stride=4) + channels-first LayerNorm, and three times channels-first LayerNorm + Conv2d(C, Co, 2, stride=2)).  A convolution whose kernel
 * equals its stride is a GEMM over non-overlapping patches: the GEMMs are the caller's (the vendor library), everything around them is here.
 * No host synchronisation, no read-back, no allocation, no atomics.  Operator only: the model-level engine stays inference only.
 *
 * LN to patches (uni_down_train_*)
 *   x, grad_x   the (B, C, H, W) map in channels-last memory, dense [B][H][W][C].  x_dtype: 0 = the type of the form (fp32, fp64 in the _f64
 *               form), 1 = fp16, 2 = bf16 (fp32 form only).  Conversion in registers, all arithmetic fp32 (fp64).
 *   A, grad_A   the patch matrix [M][4 C] of the 2x2 / stride-2 convolution, M = B Ho Wo, Ho = H / 2, Wo = W / 2 (floor): pixel (n, h, w),
 *               channel c is row (n Ho + h / 2) Wo + w / 2, column ((h & 1) 2 + (w & 1)) C + c, the column order of
 *               weight.permute(0, 2, 3, 1).reshape(Co, 4 C).  a_dtype (0 / 1 / 2 as x_dtype) is its element type.  A pixel of a last row or
 *               column that an odd H or W drops has no element in it.
 *   weight, bias, grad_ln_weight, grad_ln_bias  [C] of the LayerNorm
 *   stats       [B H W][2] = mean and 1 / sqrt(var + eps) of EVERY pixel
 *   uni_down_train_fwd  rebuild == 0: mean, rstd (the variance is the mean of (x - mean)^2, a second pass over registers), z = weight *
 *                       (x - mean) * rstd + bias rounded ONCE to the type of A.  Writes A and stats COMPLETELY.  rebuild != 0: the same
 *                       kernel reads stats instead of computing it and writes A alone, COMPLETELY and with the bits of the forward (eps is
 *                       then not read).  One launch.
 *   uni_down_train_bwd  xhat = (x - mean) * rstd, t = grad_A * weight: grad_x = rstd * (t - mean_c t - xhat * mean_c (t * xhat)), written
 *                       COMPLETELY with exact zeros at the dropped pixels, which are not read and take no part in the sums;
 *                       grad_ln_weight[c] = sum of grad_A * xhat, grad_ln_bias[c] = sum of grad_A.  grad_x and the pair grad_ln_weight /
 *                       grad_ln_bias may be NULL: that part is skipped (the reduce launch too when the pair is NULL; the workspace may then be
 *                       NULL and is not touched), what is computed has the same bits as in the full call.  Both NULL: no launch, no error.  At
 *                       most two launches.
 *   Limits: B >= 1, H, W >= 2, C % 4 == 0, 4 <= C <= 2048, B H W < 2^31 (element offsets are 64-bit: A may pass 2^31 elements), pointers
 *   16-byte aligned; other shapes are refused with an error string before any launch and uni_down_train_workspace_bytes returns 0 for them.
 *   workspace (backward with the pair only): 16-byte aligned device scratch of >= uni_down_train_workspace_bytes(B, H, W, C) bytes (fp32; the
 *   _f64 form needs twice that) = uni_lncf_train_workspace_bytes = 4 * 1024 * 2 C.  Nothing is kept in it between calls.
 *
 * Stem patches (uni_patch4_*), one launch each
 *   x, grad_x   (B, Cin, H, W), NCHW-contiguous [B][Cin][H][W], element type x_dtype
 *   A, grad_A   [M][Cin 16], M = B (H / 4) (W / 4), element type a_dtype: row as above with / 4, column (c 4 + kh) 4 + kw, the order of
 *               weight.reshape(Co, Cin 16), so the weight needs no permutation
 *   uni_patch4_gather   A = the patches of x, rounded once to a_dtype.  Writes A COMPLETELY.
 *   uni_patch4_scatter  grad_x = grad_A at the same addresses, zeros in the margin that H % 4 or W % 4 drops.  Writes grad_x COMPLETELY.
 *   Limits: B >= 1, 1 <= Cin <= 4, H, W >= 4, B H W < 2^31, pointers 16-byte aligned (W need not be a multiple of 4: x is accessed
 *   element-wise); other shapes are refused with an error string before any launch.
 * One writer per element, fixed summation orders (as uni_lncf_train_bwd): two calls give the same bits. */
size_t uni_down_train_workspace_bytes(int B, int H, int W, int C);
int uni_down_train_fwd(const void* x, int x_dtype, const float* weight, const float* bias, double eps, int B, int H, int W, int C, int rebuild,
                       void* A, int a_dtype, float* stats, uni_stream_t stream);
int uni_down_train_bwd(const void* x, int x_dtype, const float* weight, const float* stats, const void* grad_A, int a_dtype, int B, int H, int W,
                       int C, void* grad_x, float* grad_ln_weight, float* grad_ln_bias, void* workspace, size_t workspace_bytes,
                       uni_stream_t stream);
int uni_down_train_fwd_f64(const void* x, int x_dtype, const double* weight, const double* bias, double eps, int B, int H, int W, int C,
                           int rebuild, void* A, int a_dtype, double* stats, uni_stream_t stream);
int uni_down_train_bwd_f64(const void* x, int x_dtype, const double* weight, const double* stats, const void* grad_A, int a_dtype, int B, int H,
                           int W, int C, void* grad_x, double* grad_ln_weight, double* grad_ln_bias, void* workspace, size_t workspace_bytes,
                           uni_stream_t stream);
int uni_patch4_gather(const void* x, int x_dtype, int B, int Cin, int H, int W, void* A, int a_dtype, uni_stream_t stream);
int uni_patch4_scatter(const void* grad_A, int a_dtype, int B, int Cin, int H, int W, void* grad_x, int x_dtype, uni_stream_t stream);
int uni_patch4_gather_f64(const void* x, int x_dtype, int B, int Cin, int H, int W, void* A, int a_dtype, uni_stream_t stream);
int uni_patch4_scatter_f64(const void* grad_A, int a_dtype, int B, int Cin, int H, int W, void* grad_x, int x_dtype, uni_stream_t stream);

/* The point-wise middle of the ConvNeXt block's MLP for TRAINING (unicorn/models/backbone/convnext.py:46-48: x = pwconv1(x); x = act(x);
 * x = pwconv2(x) with act = nn.GELU(), the exact erf form): the GELU forward, and a backward that REBUILDS a = gelu(h) from h, so that the
 * caller keeps h (or only the input of pwconv1) instead of h and a.  The two GEMMs are the caller's (the vendor library).  One launch forward,
 * at most three backward, no host synchronisation, no read-back, no allocation, no atomics.  Operator only.
 *   h, a, grad_a, grad_h   dense [M][Hd]: rows = the M = N H W pixels, row pitch Hd;  grad_y dense [M][Co].  h_dtype: 0 = the type of the form
 *                          (fp32, fp64 in the _f64 form), 1 = fp16, 2 = bf16 (fp32 form only) is the element type of all five.  Conversion
 *                          in registers, all arithmetic fp32 (fp64).
 *   grad_b1 [Hd], grad_b2 [Co]   in the type of the form
 *   uni_pw_mlp_act_fwd   a = gelu(h) = h (1 + erf(h / sqrt 2)) / 2, written COMPLETELY.  a == h (in place) is allowed: every element is read and
 *                        then written by the same lane.
 *   uni_pw_mlp_act_bwd   one map kernel reads h and grad_a and writes what is asked for: a = gelu(h) (a == h allowed), grad_h = grad_a *
 *                        gelu'(h) with gelu'(v) = Phi(v) + v phi(v) (grad_h == grad_a allowed), and per-block partial column sums of the
 *                        UNROUNDED grad_h that an ordered reduce turns into grad_b1.  With grad_b2, a column-sum kernel over grad_y runs and
 *                        its partials go through the SAME reduce launch.  a, grad_h, grad_b1 and grad_b2 may each be NULL: that part is
 *                        skipped, what is computed has the same bits as in the full call.  h may be NULL when only grad_b2 is asked for,
 *                        grad_a when neither grad_h nor grad_b1 is, grad_y without grad_b2; the workspace without grad_b1 and grad_b2 (it is
 *                        then not touched).  Nothing asked for: no launch, no error.
 * One writer per element, fixed summation orders (a lane's own rows in the math type; the lanes of a block and the rows of partials in
 * ascending order in double): two calls give the same bits.
 * Limits: 1 <= M < 2^31 (element offsets are 64-bit), Hd % 4 == 0, 4 <= Hd <= 8192, Co % 4 == 0, 4 <= Co <= 8192 (Co is checked even where
 * grad_b2 is NULL), pointers 16-byte aligned; other shapes are refused with an error string and uni_pw_mlp_workspace_bytes returns 0 for them.
 * workspace (backward with grad_b1 or grad_b2 only): 16-byte aligned device scratch of >= uni_pw_mlp_workspace_bytes(M, Hd, Co) bytes (fp32;
 * the _f64 form needs twice that) = 4 * 256 * (Hd + Co): at most 256 blocks along the rows write one row of Hd (Co) partial sums each.  Nothing
 * is kept in it between calls. */
size_t uni_pw_mlp_workspace_bytes(int M, int Hd, int Co);
int uni_pw_mlp_act_fwd(const void* h, int h_dtype, int M, int Hd, void* a, uni_stream_t stream);
int uni_pw_mlp_act_bwd(const void* h, int h_dtype, const void* grad_a, int M, int Hd, void* a, void* grad_h, float* grad_b1, const void* grad_y,
                       int Co, float* grad_b2, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_pw_mlp_act_fwd_f64(const void* h, int h_dtype, int M, int Hd, void* a, uni_stream_t stream);
int uni_pw_mlp_act_bwd_f64(const void* h, int h_dtype, const void* grad_a, int M, int Hd, void* a, void* grad_h, double* grad_b1,
                           const void* grad_y, int Co, double* grad_b2, void* workspace, size_t workspace_bytes, uni_stream_t stream);

/* GroupNorm + activation for TRAINING: what every BaseConv of the YOLOX-PAFPN and of the head runs after convert_bn_model_to_gn
 * (unicorn/models/backbone/network_blocks.py:29-51: act(bn(conv(x))) with bn = GroupNorm(16, C, eps=1e-3), act = SiLU), the CondInst mask
 * branch (GroupNorm(16, C) + ReLU) and unicorn.py:38 (GroupNorm(32, C) alone), forward and backward for a whole batch: at most three launches
 * forward and three backward, no host synchronisation, no read-back, no allocation, no atomics.  The convolution is the caller's.  Operator
 * only: the model-level engine stays inference only.
 *   x, y, grad_y, grad_x  (B, C, H, W) maps, all four in ONE memory layout: nchw == 0: dense [B][H][W][C] (channels-last memory), nchw != 0:
 *                         dense [B][C][H][W].  Both are read and written in place.  x_dtype: 0 = the type of the form (fp32, fp64 in the _f64
 *                         form), 1 = fp16, 2 = bf16 (fp32 form only) is the type of x and grad_x; y and grad_y have the type of the form.
 *                         Conversion in registers, all arithmetic fp32 (fp64).  y must not overlap x.
 *   weight, bias, grad_weight, grad_bias  [C]
 *   G                     groups of cpg = C / G consecutive channels; cpg need not be a multiple of 4
 *   act                   0 none, 1 ReLU, 3 SiLU z * sigmoid(z) (the exact form)
 *   stats                 [B G][2] = mean and 1 / sqrt(var + eps) of every (sample, group), written by the forward, read by the backward
 *   uni_gn_act_train_fwd  mean and the biased variance over the m = cpg H W elements of a (sample, group); z = (x - mean) * rstd * weight[c] +
 *                         bias[c]; y = act(z).  Launch 1: every block takes pixels of ONE image and writes, per channel, the mean over its pixels
 *                         and the sum of squared deviations from THAT mean (a second pass over its pixels: no E[x^2] - E[x]^2); launch 2 combines
 *                         these parts (count, mean, M2; Chan et al.) in a fixed order in double; launch 3 writes y.  Between launch 1
 *                         and launch 3 the parts lie in y (they fit for every admitted shape), so there is no forward workspace.  Writes y and
 *                         stats COMPLETELY.
 *   uni_gn_act_train_bwd  xhat = (x - mean) * rstd, z as above, dz = grad_y * act'(z) with act' = 1, z > 0, s (1 + z (1 - s)) for s = sigmoid(z):
 *                         grad_bias[c] = sum over n, h, w of dz, grad_weight[c] = sum of dz * xhat; with A = sum_{c in g} weight[c] sum_hw dz and
 *                         Bq = sum_{c in g} weight[c] sum_hw dz * xhat: grad_x = rstd * (weight[c] * dz - (A + xhat * Bq) / m).  Launch 1 writes the
 *                         per-(row of partials, channel) sums of dz * xhat and dz, launch 2 forms A / m, Bq / m per (sample, group) and
 *                         grad_weight, grad_bias from them, launch 3 writes grad_x.  grad_x and the pair grad_weight / grad_bias may be NULL: that
 *                         part of launch 2 is skipped, and launch 3 with grad_x; what is computed has the same bits as in the full call.  Both
 *                         NULL: no launch, no error.  Each output is written COMPLETELY.
 * One writer per element, fixed summation orders (a lane's own pixels in the math type, the first-pass sum of x in double; the lanes of a
 * block and the rows of partials in ascending order or a fixed tree in double): two calls give the same bits.
 * Limits: B, H, W >= 1, C % 4 == 0, 4 <= C <= 2048, B H W < 2^31 (element offsets are 64-bit), 1 <= G <= C, C % G == 0, pointers 16-byte
 * aligned (H W need not be a multiple of anything: with nchw != 0 the rows of a channel plane are read element-wise); other shapes are
 * refused with an error string before any launch and uni_gn_act_train_workspace_bytes returns 0 for them.
 * workspace (every backward that computes something): 16-byte aligned device scratch of >= uni_gn_act_train_workspace_bytes(B, H, W, C, G)
 * bytes (fp32; the _f64 form needs twice that) = 4 * (B rpi 2 C rounded up to 64, + 2 B G) with rpi = min(ceil(H W / u), max(1, 1024 / B)) rows
 * of partials per image, u = the power of two >= B H W / 512 within [16, 256].  Nothing is kept in it between calls. */
size_t uni_gn_act_train_workspace_bytes(int B, int H, int W, int C, int G);
int uni_gn_act_train_fwd(const void* x, int x_dtype, int nchw, const float* weight, const float* bias, double eps, int act, int B, int H, int W,
                         int C, int G, float* y, float* stats, uni_stream_t stream);
int uni_gn_act_train_bwd(const void* x, int x_dtype, int nchw, const float* weight, const float* bias, const float* stats, const float* grad_y,
                         int act, int B, int H, int W, int C, int G, void* grad_x, float* grad_weight, float* grad_bias, void* workspace,
                         size_t workspace_bytes, uni_stream_t stream);
int uni_gn_act_train_fwd_f64(const void* x, int x_dtype, int nchw, const double* weight, const double* bias, double eps, int act, int B, int H,
                             int W, int C, int G, double* y, double* stats, uni_stream_t stream);
int uni_gn_act_train_bwd_f64(const void* x, int x_dtype, int nchw, const double* weight, const double* bias, const double* stats,
                             const double* grad_y, int act, int B, int H, int W, int C, int G, void* grad_x, double* grad_weight,
                             double* grad_bias, void* workspace, size_t workspace_bytes, uni_stream_t stream);

/* What stands around the label propagation in the SOT / VOS TRAINING losses (unicorn/models/unicorn.py:315-337 compute_loss_sot, :339-390
 * compute_loss_vos) for a whole BATCH, without a host synchronisation, a read-back or an allocation; the number of launches does not
 * depend on the data.  The propagation itself is uni_corr_softmax_pv_lse / _bwd on the label rows these entries produce.
 *   targets   [B][2][M][6] fp32, contiguous: rows (class, cx, cy, w, h, track id) of frame 0 and frame 1; fp32 in the _f64 forms too.
 *   maps      H8 x W8 pixels (stride 8: the image is 8 H8 x 8 W8), H8, W8 >= 4; Q = H8 W8.
 * uni_prop_labels (2 launches; not differentiable):
 *   sot = 1:  Kc = 1, slot 0 of every sample is (row 0 of frame 0, row 0 of frame 1) whatever the ids (:324, :332); num_matched = 1.
 *   sot = 0:  for i = 0 .. M-1 with id0[i] != 0, j = the first j with id1[j] != 0 && id1[j] == id0[i] (fp32 compare, :352-361); the
 *             matched i fill the slots in the order of i, at most Kc <= M of them (the reference's max_matched_inst).
 *   -> matched [B][Kc][2] int32 = (i, j), -1 in slots >= num_matched[b]; num_matched [B] int32;
 *      gt0, gt1 [B][Kc][Q]: the label rows of frame 0 (row i) and frame 1 (row j), zeros in slots >= num_matched[b]; all completely written.
 *   masks == NULL: F.interpolate(get_label_map(box), 1/8, bilinear) (:521-533) = the mean of the central 2 x 2 of every 8 x 8 block of the
 *             full-resolution box mask, which is never formed.  Corners cx -+ 0.5 w, cy -+ 0.5 h in fp32, rounded half to even; the
 *             start clamped to >= 0; the end by Python's slice rules: above the size it is clipped, negative e means size + e, end <= start is
 *             an empty box.
 *   masks [B][2][M][r H8][r W8], fp32 (mask_u8 = 0) or uint8 (mask_u8 = 1), mask_rate r = 1, 2, 4: init_with_mask (:56-58, :365-366), the
 *             bilinear 1/r of masks[b][0][i] and masks[b][1][j]: the pixel, the 2 x 2 block, the central 2 x 2 of the 4 x 4 block, read in place.
 * uni_prop_dice_pyramid_fwd (2 launches): pred [B][Kc][H8][W8] (the propagated labels), gt1 [B][Kc][Q] ->
 *   p16 [B][Kc][H8/2][W8/2], p32 [B][Kc][H8/4][W8/4] = F.interpolate(pred, 1/2 and 1/4, bilinear) (:329-331, :372-374): rows / columns
 *             2y, 2y+1 and 4y+1, 4y+2; odd sizes keep the floor, trailing rows / columns have no parent;
 *   loss      dice_coefficient (:509-519), 1 - 2 I / (X2 + T2 + 1e-5) with I = sum x t, X2 = sum x^2, T2 = sum t^2.
 *             num_matched != NULL: [B][Kc], one Dice per slot, 0 in slots >= num_matched[b] (read on the device);
 *             num_matched == NULL: ONE value over the whole batch, as compute_loss_sot flattens it;
 *   sums      [B Kc][3] (or [1][3]) double = I, X2, T2, for the backward.  Sums are double in both precisions, in a fixed order.
 * uni_prop_dice_pyramid_bwd (1 launch): grad_pred [B][Kc][H8][W8], completely written, =
 *   grad_p8 + 0.25 grad_p16[parent] + 0.25 grad_p32[parent] + grad_loss (-2 t / U + 4 I x / U^2), U = X2 + T2 + 1e-5.
 *   Each of grad_p8, grad_p16, grad_p32, grad_loss may be NULL (left out).  Slots >= num_matched[b] get exactly zero.  One writer per
 *   element, no atomics: two calls give the same bits.
 * 16-byte accesses are used when W8 % 4 == 0 and the pointers are aligned for them; any other shape / alignment takes the scalar form.
 * Limits: 1 <= Kc <= M <= 1024, B Kc <= 32767, H8, W8 >= 4, B Kc Q < 2^31; other shapes are refused with an error string and
 * uni_prop_workspace_bytes returns 0 for them.  workspace: 8-byte aligned, >= uni_prop_workspace_bytes(B, Kc, Q) = 24 B Kc ceil(Q / 1024)
 * bytes rounded up to 256, in both precisions; the forward's scratch only. */
size_t uni_prop_workspace_bytes(int B, int Kc, int Q);
int uni_prop_labels(const float* targets, const void* masks, int mask_u8, int B, int M, int Kc, int sot, int H8, int W8, int mask_rate,
                    int32_t* matched, int32_t* num_matched, float* gt0, float* gt1, uni_stream_t stream);
int uni_prop_labels_f64(const float* targets, const void* masks, int mask_u8, int B, int M, int Kc, int sot, int H8, int W8, int mask_rate,
                        int32_t* matched, int32_t* num_matched, double* gt0, double* gt1, uni_stream_t stream);
int uni_prop_dice_pyramid_fwd(const float* pred, const float* gt1, const int32_t* num_matched, int B, int Kc, int H8, int W8, float* p16, float* p32,
                              float* loss, double* sums, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_prop_dice_pyramid_fwd_f64(const double* pred, const double* gt1, const int32_t* num_matched, int B, int Kc, int H8, int W8, double* p16,
                                  double* p32, double* loss, double* sums, void* workspace, size_t workspace_bytes, uni_stream_t stream);
int uni_prop_dice_pyramid_bwd(const float* pred, const float* gt1, const int32_t* num_matched, const double* sums, const float* grad_p8,
                              const float* grad_p16, const float* grad_p32, const float* grad_loss, int B, int Kc, int H8, int W8, float* grad_pred,
                              uni_stream_t stream);
int uni_prop_dice_pyramid_bwd_f64(const double* pred, const double* gt1, const int32_t* num_matched, const double* sums, const double* grad_p8,
                                  const double* grad_p16, const double* grad_p32, const double* grad_loss, int B, int Kc, int H8, int W8,
                                  double* grad_pred, uni_stream_t stream);

/* The tail of a TRAINING iteration (unicorn/core/trainer.py:260-275): scaler.step(optimizer) with torch.optim.AdamW (single-tensor form,
 * amsgrad = maximize = False; exp/unicorn_track.py:380-381), scaler.update() and ModelEMA.update (unicorn/utils/ema.py:50-63) over a LIST of fp32
 * tensors in one pass over memory, without a host synchronisation, a read-back or an allocation.  At most three kernel launches with a scaler
 * (check, update, finish) and two without, whatever the number and the sizes of the tensors; with a scaler one 4-byte memset node clears found_inf.
 *   table      n_tensors entries of 64 bytes, 8-byte aligned, in device memory:
 *                offset  0  float*  p        parameter (or, for an EMA-only entry, the model's float buffer / gradient-less parameter: read only)
 *                offset  8  float*  g        gradient, NULL = absent
 *                offset 16  float*  m        exp_avg      (may be NULL in an EMA-only entry)
 *                offset 24  float*  v        exp_avg_sq   (may be NULL in an EMA-only entry)
 *                offset 32  float*  e        the EMA copy
 *                offset 40  int64   n        elements (0 allowed: the entry has no chunk)
 *                offset 48  double  lr_factor   the entry's learning rate is lr x lr_factor (the trainer's param_group["factor"])
 *                offset 56  float   weight_decay
 *                offset 60  int32   flags    UNI_OPT_HAS_GRAD: AdamW + EMA; 0: EMA only
 *              The arrays of an entry are n dense elements each, updated in storage order; arrays of different entries do not overlap.
 *   block_map  total_chunks entries of 8 bytes: int32 tensor, uint32 chunk -> elements [chunk CH, min(n, (chunk + 1) CH)) of that tensor,
 *              CH = uni_opt_chunk_elems() (a multiple of 4).  Every element of every tensor is covered by exactly one entry.  The first
 *              vec_chunks entries are processed with 16-byte accesses (scalar head / tail of at most 3 elements): all non-NULL pointers of
 *              their tensor must share their address modulo 16.  The other entries are processed element by element (pointers misaligned
 *              relative to each other).  Entries that name no tensor of the table, or a chunk behind its end, are skipped.
 *   uni_opt_table_bytes(n_tensors, total_chunks): bytes of ONE upload image that holds both, each part rounded up to 256 bytes: the table
 *              at offset 0, the block map at offset uni_opt_table_bytes(n_tensors, 0).  0 for negative arguments.
 *   state      step (fp32, one word for the list, as torch keeps it per tensor); scale (fp32), growth_tracker (int32), found_inf (fp32): the
 *              scaler's words, all three NULL = no scaler.  found_inf is cleared by the call and holds 1.0 after a skipped step, else 0.
 * The call:  with a scaler inv = float(1 / double(scale)) and found_inf = any(!isfinite(g inv)) over all gradients (the product is tested, as
 *   unscale_ does); without one inv = 1 and there is no check.  If not found_inf, with t = step + 1 and gh = g inv, per element of an entry
 *   with UNI_OPT_HAS_GRAD:  p *= 1 - lr_i wd_i;  m += (gh - m)(1 - beta1);  v = v beta2 + (1 - beta2) gh gh;
 *   p -= (lr_i / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps), the bias corrections in double from the device step.  Then, always
 *   and for every entry, e = fl(fl(e float(ema_decay)) + fl(float(1 - ema_decay) p)) with the p just written: three separate roundings, bit-equal to
 *   the two lines of ModelEMA.update.  Finish: step += 1 unless skipped; torch's _amp_update_scale_ exactly (found_inf: scale *= backoff_factor,
 *   tracker = 0; else tracker += 1 and at growth_interval scale *= growth_factor if that is finite, tracker = 0).  After a skipped step p, m, v
 *   and step keep their bits.  The gradients are left scaled (the unscaled value lives in registers only).
 * One writer per element, no atomics: two calls from the same state give the same bits.  Limits: 0 <= vec_chunks <= total_chunks < 2^31,
 * n < 2^32 CH; errors (-1 and a uni_last_error text): NULL table / block_map / step, negative sizes, table_bytes < 64 n_tensors or map_bytes <
 * 8 total_chunks ("too small"), a scaler without its three words or with growth_interval < 1. */
#define UNI_OPT_HAS_GRAD 1
int uni_opt_chunk_elems(void);
size_t uni_opt_table_bytes(int n_tensors, int total_chunks);
int uni_opt_step(const void* table, size_t table_bytes, const void* block_map, size_t map_bytes, int n_tensors, int vec_chunks, int total_chunks,
                 float* step, float* scale, int32_t* growth_tracker, float* found_inf, double lr, double beta1, double beta2, double eps,
                 double ema_decay, double growth_factor, double backoff_factor, int growth_interval, uni_stream_t stream);

/* Input letterbox on the device (row 0 / N1): PreprocessorX.process (external/lib/test/tracker/unicorn_sot.py:111-123,
 * swap_rb = 1) and preproc (unicorn/data/data_augment.py:194-214, swap_rb = 0).  img_hwc: (h, w, 3) uint8 DEVICE buffer;
 * out_chw: (3, H, W) fp32 = cv2.resize(INTER_LINEAR, 8-bit fixed point) to (int(w r), int(h r)), r = min(H/h, W/w),
 * top-left aligned, padded with 114.  *r_out (host, optional) receives r. */
int uni_letterbox(const uint8_t* img_hwc, int h, int w, int swap_rb, int H, int W, float* out_chw, double* r_out,
                  uni_stream_t stream);

/* UnicornHead.decode_outputs (unicorn_head.py:467-482), in place: outputs (B, A, nch) raw [dx,dy,log w,log h,...] over the three
 * levels (strides 8/16/32 of an HxW input, level-major like the head's concat) -> xy = (xy + grid) * stride, wh = exp(wh) * stride.
 * (uni_head already returns decoded outputs; this entry serves callers that keep decode_in_inference=False.) */
int uni_decode_outputs(float* outputs, int B, int H, int W, int nch, uni_stream_t stream);
/* torchvision.ops.nms on caller boxes (unicorn/utils/boxes.py:58-64): boxes (n,4) xyxy, scores (n) -> keep_idx (n) int32 in
 * descending-score order, *n_out (device int32).  workspace >= uni_nms_workspace_bytes(n). */
size_t uni_nms_workspace_bytes(int n);
int uni_nms(const float* boxes_xyxy, const float* scores, int n, float iou_thr, int32_t* keep_idx, int32_t* n_out, void* workspace,
            size_t workspace_bytes, uni_stream_t stream);

/* Detection post-processing of ONE image on the device (row N1): unicorn/utils/boxes.py:33-77 `postprocess`
 * (+ torchvision.ops.nms / batched_nms semantics).  pred: (A, ld >= 5+num_classes) decoded [cx,cy,w,h,obj,cls...] fp32,
 * converted to corners IN PLACE like the reference (:36-39).  Survivors, in descending obj*cls order:
 * det_out (max_det, 7) rows [x1,y1,x2,y2,obj,cls_conf,cls], keep_idx (max_det) anchor indices, *n_out = row count
 * (device int32, clamped to max_det).  flags: bit 0 = class-agnostic NMS, bit 1 = boxes are already corners (plain
 * torchvision-style nms on caller boxes).  workspace >= uni_postprocess_workspace_bytes(A) device bytes. */
size_t uni_postprocess_workspace_bytes(int A);
int uni_postprocess(float* pred, int A, int ld, int num_classes, float conf_thre, float nms_thre, int flags,
                    int max_det, float* det_out, int32_t* keep_idx, int32_t* n_out, void* workspace, size_t workspace_bytes,
                    uni_stream_t stream);

/* ---- mask post-processing of the VOS / MOTS drivers -------------------------------------------- */
/* masks (N,Hn,Wn) fp32 at network resolution -> F.interpolate(scale_factor=1/r, bilinear, align_corners=False)[:, :H, :W]
 * pasted into zero (N,H,W) maps: out_prob fp32 (external/lib/test/tracker/unicorn_vos.py:146-150) and / or
 * out_bin = prob > thr as bytes (unicorn/evaluators/mot_evaluator.py:804-805).  Either output may be NULL. */
int uni_mask_resize(const float* masks, int N, int Hn, int Wn, double r, int H, int W, float thr, float* out_prob,
                    uint8_t* out_bin, uni_stream_t stream);
/* postprocess_inst's mask half + the MOTS threshold in ONE call, for callers that never look at the network-size maps
 * (unicorn/utils/boxes.py:138-146 -> unicorn/models/condinst/dynamic_mask_head.py:159-225 -> unicorn/evaluators/mot_evaluator.py:804-805;
 * the VOS paste of external/lib/test/tracker/unicorn_vos.py:141-152 with out_prob): arguments of uni_condinst_masks, then
 * F.interpolate(scale_factor=1/r, bilinear)[:, :H, :W] pasted into zero (n,H,W) maps as fp32 (out_prob) and / or `> thr` bytes (out_bin);
 * either may be NULL.  The (n, d_rate*r*H8, d_rate*r*W8) fp32 maps are never written; results are bit-identical to
 * uni_condinst_masks followed by uni_mask_resize.  workspace >= n*H8*W8*(1+r*r)*4 bytes. */
int uni_condinst_masks_u8(const float* mask_feats, const float* up_masks, const float* params, int ldp, const float* inst_loc,
                          const int32_t* inst_lvl, int n, int H8, int W8, int up_rate, int d_rate, double r, int H, int W, float thr,
                          float* out_prob, uint8_t* out_bin, void* workspace, size_t workspace_bytes, uni_stream_t stream);
/* Soft aggregation of unicorn_vos.py:99-120 fused with that resize: probs (K1,Hn,Wn) of the tracked objects (ids prob_ids, in
 * cur_obj_ids order), init_masks (K2,H,W) {0,1} of objects introduced in this frame (ids init_ids); background =
 * prod(1 - p), argmax over [background, ids] (numpy first-maximum rule) -> out (H,W) uint8 id map. */
int uni_vos_merge(const float* probs, const int32_t* prob_ids, int K1, int Hn, int Wn, double r, const uint8_t* init_masks,
                  const int32_t* init_ids, int K2, int H, int W, uint8_t* out, uni_stream_t stream);
/* mot_evaluator.py:860-865: masks (N,H,W) {0,1} in track order -> a pixel stays with the first mask that claims it. */
int uni_mots_overlap_free(const uint8_t* masks, int N, int H, int W, uint8_t* out, uni_stream_t stream);
/* pycocotools rleEncode + rleToString of np.asfortranarray(mask) (mot_evaluator.py:889-892): out_chars (N,max_chars) bytes,
 * out_len (N) string lengths (-1: more than max_runs runs or max_chars chars, retry with larger bounds); optional
 * counts (N,max_runs+1) uint32 run lengths and n_runs (N). */
size_t uni_rle_workspace_bytes(int N, int H, int W, int max_runs);
int uni_rle_encode(const uint8_t* masks, int N, int H, int W, int max_runs, int max_chars, uint8_t* out_chars,
                   int32_t* out_len, uint32_t* counts, int32_t* n_runs, void* workspace, size_t workspace_bytes,
                   uni_stream_t stream);

/* ---- low-level building blocks (exported for kernel parity tests) --------------------------------------- */
/* out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) (+res).  A: bf16 NHWC map (Hin,Win,Cin) row stride lda.
 * w_packed: [roundup(N,256)][roundup(K,64)] bf16, K order (ky,kx,c) (see uni_pack_weight). */
int uni_pack_weight(const float* w_oihw_host, int N, int Cin, int KH, int KW, uint16_t* out_host_bf16);
int uni_gemm_bf16(const uint16_t* A, int lda, const uint16_t* w_packed, int M, int N, int Hin, int Win, int Cin, int KH,
                  int KW, int stride, int pad, const float* bias, int act, const float* residual, int ldr, float* outF,
                  int ldf, uint16_t* outB, int ldb, double* gn_stats, int cpg, int force_cfg, uni_stream_t stream);
int uni_cast_bf16(const float* x, int ldx, uint16_t* out, int ldo, int M, int C, uni_stream_t stream);
/* The same three for the "f16x2" operand format (precision 2: every value split into hi + lo f16 halves, per 8 channels a
 * 32-byte group [8 x hi][8 x lo]; fp32-equivalent contraction as hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16).
 * Buffers are 4 bytes per element.  uni_pack_weight_h2 returns the power-of-two scale the packed tensor carries in
 * *wscale_out (pass it to uni_gemm_h2, which multiplies the accumulator by it). */
int uni_pack_weight_h2(const float* w_oihw_host, int N, int Cin, int KH, int KW, void* out_host, float* wscale_out);
int uni_gemm_h2(const void* A, int lda, const void* w_packed, float wscale, int M, int N, int Hin, int Win, int Cin, int KH,
                int KW, int stride, int pad, const float* bias, int act, const float* residual, int ldr, float* outF,
                int ldf, void* outB, int ldb, double* gn_stats, int cpg, int force_cfg, uni_stream_t stream);
int uni_cast_h2(const float* x, int ldx, void* out, int ldo, int M, int C, uni_stream_t stream);
/* Fused ConvNeXt MLP of the narrow stages (unicorn/models/backbone/convnext.py:47-54; C in {96, 192, 256}):
 *     out[m][:] = residual[m][:] + b2 + diag(gamma) W2 . GELU(W1 . a[m][:] + b1)
 * in one launch with the 4C hidden units kept in registers (csrc/mlp_fused.hip).  uni_mlp_pack lays the nn.Linear weights
 * w1 [4C][C], w2 [C][4C] (host, fp32; gamma [C] or NULL folded into the rows of w2) out as the f16x2 weight stream the kernel
 * consumes (uni_mlp_blob_bytes(C) bytes, host; copy it to the device) and returns the two accumulator factors.  a: f16x2 operand
 * rows (uni_cast_h2 / uni_dwconv7_ln output), b2 must already carry gamma; out may alias residual; out_h2 (optional) receives
 * an f16x2 copy of the result.  layout 0: 4 waves x 32 rows per 128-row tile, one wave per SIMD (C = 96, 192, 256); layout 1: 8 waves x
 * 16 rows, two waves per SIMD, v_mfma_f32_16x16x32_f16 (C = 192, 256; what the engine uses).  The blob is layout specific. */
size_t uni_mlp_blob_bytes(int C);
int uni_mlp_pack(const float* w1_host, const float* w2_host, const float* gamma_host, int C, int layout, void* blob_host,
                 float* ws1_out, float* ws2_out);
int uni_mlp_fused(const void* a_h2, int lda, const void* blob_dev, const float* b1, const float* b2, float ws1, float ws2,
                  const float* residual, int ldr, float* out, int ldo, void* out_h2, int ldb, int M, int C, int layout,
                  uni_stream_t stream);
int uni_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float eps, int M, int C, float* outF,
                  uint16_t* outB, uni_stream_t stream);
/* Every mode of the row LayerNorm the engine uses, without a context (fmt: 0 = bf16, 1 = fp32, 2 = f16x2 operand rows in out_op).
 *   out_f32 (optional, ld ldf): fp32 rows.  pair_hw > 0: the rows are tokens [B][2 frames][pair_hw] and the fp32 rows of frame 0 go to
 *     out_f32, those of frame 1 to out_f32_2, both as [B][pair_hw] maps (M a multiple of 2 pair_hw); otherwise out_f32_2 = NULL.
 *   out_op (optional, ld ldb): operand rows in fmt.  ps_h, ps_w > 0: the rows are the pixels of a map ps_w wide and out_op receives
 *     PixelShuffle(2) of it, a dense (2 M / ps_w, 2 ps_w, C / 4) map (ldb unused; unicorn.py:41).  Only ps_w enters the addressing: the
 *     output row is 2 (row / ps_w), so stacked (ps_h, ps_w) maps simply extend the height; ps_h switches the mode on and M must be a
 *     multiple of ps_h * ps_w. */
int uni_layernorm_ex(const float* x, int ldx, const float* gamma, const float* beta, float eps, int M, int C, float* out_f32, int ldf,
                     float* out_f32_2, int pair_hw, void* out_op, int ldb, int ps_h, int ps_w, int fmt, uni_stream_t stream);
int uni_dwconv7_ln(const float* x_nhwc, const float* w49c, const float* bias, const float* gamma, const float* beta,
                   float eps, int H, int W, int C, uint16_t* out_bf16, uni_stream_t stream);
/* The same for B stacked (H,W,C) maps and any operand format (what the engine calls per ConvNeXt block): fmt 0 = bf16 rows, 1 = fp32
 * rows, 2 = f16x2 rows ([8 hi][8 lo] groups).  convnext.py:30-33,47-49. */
int uni_dwconv7_ln_ex(const float* x_nhwc, const float* w49c, const float* bias, const float* gamma, const float* beta, float eps,
                      int B, int H, int W, int C, void* out, int fmt, uni_stream_t stream);
/* The engine's sampler of the ref <-> cur interaction (csrc/msda.hip msda_wave_kernel: one wave per (token, head), shuffle reductions):
 * Unicorn's fixed geometry -- 8 heads x 32 channels, 2 levels = reference / current frame of identical (h, w), 4 points -- with
 * MSDeformAttn.forward's softmax over the 8 logits and loc = ref + off / (W, H) fused in (ms_deform_attn.py:98-105,
 * deformable_transformer.py:141-153).  value (B, 2 h w, 256) fp32; offaw (B * 2 h w, ldo >= 192): 128 sampling offsets
 * (head, level, point, xy) then 64 attention logits (head, level, point) -> out (B * 2 h w, 256) fp32. */
int uni_msda_tokens(const float* value, const float* offaw, int ldo, int B, int h, int w, float* out, uni_stream_t stream);
int uni_groupnorm_act(const float* x, const double* stats, const float* gamma, const float* beta, float eps, int M,
                      int C, int G, int act, float* outF, uint16_t* outB, uni_stream_t stream);
/* Every mode of the GroupNorm apply the engine uses, without a context: B samples of M rows each (x, outputs: [B * M] rows), the group
 * sums (sum, sum of squares per group, G <= 32) of sample b at stats + 64 b.  y = act(GroupNorm(x)) (+ prior[row] * prior_beta[c] when
 * both are given, unicorn_head.py:272-277) -> out_f32 (fp32, ld ldf) and / or out_op (operand rows in fmt, ld ldb) and / or out_up: the
 * 2x nearest-neighbour copy of every sample's (M / W, W) map into a (2 M / W, 2 W) map of operand rows (ld ldu).  fmt as above; the
 * bf16 / f16x2 formats use the reciprocal-based activations of the GEMM epilogues, fp32 the exact ones. */
int uni_groupnorm_act_ex(const float* x, int ldx, const double* stats, const float* gamma, const float* beta, float eps, int B, int M,
                         int C, int G, int act, const float* prior, const float* prior_beta, float* out_f32, int ldf, void* out_op,
                         int ldb, void* out_up, int ldu, int W, int fmt, uni_stream_t stream);
int uni_stem(const float* img, int H, int W, const float* w48c, const float* bias, const float* gamma,
             const float* beta, int C, float* out_nhwc, uni_stream_t stream);
/* The same for a batch: img (B, 3, H, W) -> out (B, H / 4, W / 4, C) (what the engine calls for B frames). */
int uni_stem_ex(const float* img, int B, int H, int W, const float* w48c, const float* bias, const float* gamma, const float* beta, int C,
                float* out_nhwc, uni_stream_t stream);
/* uni_gemm_bf16 / uni_gemm_h2 for any operand format, plus the activation window the engine uses on the head outputs: fmt 0 = bf16,
 * 1 = exact fp32 (a, out_op: fp32 rows; w_packed: [ceil(N / 256) * 256][ceil(K / 64) * 64] fp32, zero padded, k = (ky * KW + kx) * Cin + c;
 * wscale unused), 2 = f16x2 (uni_cast_h2 / uni_pack_weight_h2).  act applies to the columns >= act_col0 only (0: every column).
 * force_cfg: 0 or a tile configuration (no ablation bits, no split-K: those stay with uni_gemm_h2).  Other arguments as uni_gemm_bf16.
 * uni_cast_f32: the operand cast in the fp32 format (a strided copy). */
int uni_gemm_ex(const void* a, int lda, const void* w_packed, float wscale, int fmt, int M, int N, int Hin, int Win, int Cin, int KH, int KW,
                int stride, int pad, const float* bias, int act, int act_col0, const float* residual, int ldr, float* out_f32, int ldf,
                void* out_op, int ldb, double* gn_stats, int cpg, int force_cfg, uni_stream_t stream);
int uni_cast_f32(const float* x, int ldx, float* out, int ldo, int M, int C, uni_stream_t stream);
/* uni_gemm_ex with the two launch modes the engine sets on a batch, without a context.  Stacked samples: a holds B maps [B][Hin][Win][Cin]
 * (Hin, Win per sample, 1 <= B < 128), M = B * Hout * Wout; a convolution pads every sample on its own and the GroupNorm sums of sample b
 * go to gn_stats + 64 b (gn_stats: 64 B doubles, zeroed by the caller; cpg divides N into at most 32 groups).  Row remap (out_hw > 0):
 * row r of out_f32 is written at (r / out_hw) * out_stride + out_off + r % out_hw, which is how one launch spreads a pyramid level over
 * the anchor rows of several images; out_f32 has outF_rows rows and the call fails when the last remapped row (or, without a remap, M)
 * does not fit.  out_op is never remapped.  splitk > 1 (fmt 2 only): that many K ranges through a slab kept by the library, then the
 * reduce kernel (bias, residual, statistics); fp32 output only, no activation, no remap.  Every argument is checked before a launch. */
int uni_gemm_stacked(const void* a, int lda, const void* w_packed, float wscale, int fmt, int B, int M, int N, int Hin, int Win, int Cin, int KH,
                     int KW, int stride, int pad, const float* bias, int act, int act_col0, const float* residual, int ldr, float* out_f32,
                     int ldf, int out_hw, int out_stride, int out_off, int outF_rows, void* out_op, int ldb, double* gn_stats, int cpg,
                     int splitk, int force_cfg, uni_stream_t stream);
/* The glue launchers the engine runs between its own buffers, without a context.  fmt = operand format of out (0 = bf16, 1 = fp32, 2 = f16x2).
 * uni_cast_operand_pair_ex: x0, x1 [B][hw][C] fp32 (two frames) -> out [B][2][hw][C] operand rows (the token layout of the interaction
 * stage).  uni_pixel_shuffle_ex: x (B, h, w, C) fp32 -> out (B, 2h, 2w, C / 4) operand rows, PixelShuffle(2).  uni_add_pos_ex: tokens src
 * [B][2][hw][C] + pos0 / pos1 [hw][C] (frame 0 / 1, shared by the batch) + lvl[frame][C] -> operand rows (deformable_transformer.py:74,124).
 * uni_add_aligned_bilinear_ex: dst (B, f h, f w, C) += aligned_bilinear(src (B, h, w, C), f) (condinst/comm.py:5-27).  uni_pos_embed_ex:
 * [col_embed(x) | row_embed(y)] of two (sz, nf) tables, bilinear to (h, w) -> out (h w, 2 nf) (position_encoding.py:25-36).
 * uni_msda_tokens_ex: uni_msda_tokens with the output in any operand format. */
int uni_cast_operand_pair_ex(const float* x0, const float* x1, void* out, int B, int hw, int C, int fmt, uni_stream_t stream);
int uni_pixel_shuffle_ex(const float* x, void* out, int B, int h, int w, int C, int fmt, uni_stream_t stream);
int uni_add_pos_ex(const float* src, const float* pos0, const float* pos1, const float* lvl, void* out, int B, int hw, int C, int fmt,
                   uni_stream_t stream);
int uni_add_aligned_bilinear_ex(const float* src, int B, int h, int w, int C, int factor, float* dst, uni_stream_t stream);
int uni_pos_embed_ex(const float* row_embed, const float* col_embed, int sz, int nf, int h, int w, float* out_nhwc, uni_stream_t stream);
int uni_msda_tokens_ex(const float* value, const float* offaw, int ldo, int B, int h, int w, void* out, int fmt, uni_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
