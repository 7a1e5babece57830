// extern "C" surface of libunicorn_hip.so (declared in include/unicorn_hip.h).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine.h"

#include <map>
#include <mutex>
#include <string>
#include <utility>

static thread_local char g_err[1024] = "";
void uni_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
// variant trace (common.h): tag -> number of launches since uni_variant_trace(1)
std::atomic<int> g_uni_variant_trace{0};
static std::mutex g_vt_mu;
static std::map<std::string, long long>& vt_map() { static std::map<std::string, long long> m; return m; }
void uni_variant_record(const char* fmt, ...) {
    char tag[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tag, sizeof(tag), fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_vt_mu);
    ++vt_map()[tag];
}
static inline hipStream_t S(uni_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
static int post_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { uni_set_error("kernel launch failed: %s", hipGetErrorString(e)); return -2; }
    return 0;
}
// what uni_condinst_masks and uni_condinst_masks_u8 share: the workspace check and the argument struct up to `out`
static int condinst_args(CondInstArgs& a, const char* what, const float* mask_feats, const float* up_masks, const float* params, int ldp,
                         const float* inst_loc, const int32_t* inst_lvl, int n, int H8, int W8, int up_rate, int d_rate, void* workspace,
                         size_t workspace_bytes) {
    const size_t need = (size_t)n * H8 * W8 * (1 + up_rate * up_rate) * sizeof(float);
    UNI_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu", what, workspace_bytes, need);
    a.mask_feats = mask_feats; a.up_masks = up_masks; a.params = params; a.ldp = ldp; a.inst_loc = inst_loc; a.inst_lvl = inst_lvl;
    a.n = n; a.H = H8; a.W = W8; a.r = up_rate; a.d_rate = d_rate;
    a.logits_ws = reinterpret_cast<float*>(workspace);
    a.coarse_ws = a.logits_ws + (size_t)n * H8 * W8;
    return 0;
}
// conv geometry of the three GEMM entries (1x1 / s1 / p0 => plain GEMM); M must be its number of output pixels
static int gemm_geometry(GemmArgs& g, const char* what, const void* A, int lda, const void* w_packed, int M, int N, int Hin, int Win, int Cin,
                         int KH, int KW, int stride, int pad) {
    g.A = reinterpret_cast<const bf16*>(A); g.lda = lda; g.W = reinterpret_cast<const bf16*>(w_packed);
    g.N = N; g.K = Cin * KH * KW; g.Kpad = cdiv(g.K, 64) * 64;
    g.Hin = Hin; g.Win = Win; g.Cin = Cin; g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    const int Hout = (Hin + 2 * pad - KH) / stride + 1;
    g.Wout = (Win + 2 * pad - KW) / stride + 1;
    g.M = Hout * g.Wout;
    UNI_REQUIRE(g.M == M, "%s: M=%d does not match conv geometry (%d)", what, M, g.M);
    return 0;
}
// partial-tile slab of the split-K path for the context-free entries (uni_gemm_h2, uni_gemm_stacked): one grow-only buffer PER DEVICE
// (the engine takes its slabs from the context workspace; these entries have no context)
static int gemm_entry_slab(float** slab, size_t need) {
    static std::mutex mu;
    static std::map<int, std::pair<float*, size_t>> slabs;
    int dev = 0;
    UNI_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto& sl = slabs[dev];
    if (need > sl.second) {
        UNI_CHECK_HIP(hipDeviceSynchronize());
        if (sl.first) (void)hipFree(sl.first);
        sl = {nullptr, 0};
        UNI_CHECK_HIP(hipMalloc(&sl.first, need));
        sl.second = need;
    }
    *slab = sl.first;
    return 0;
}
#define API(expr) do { int _rc = (expr); if (_rc) return _rc; return post_launch(); } while (0)

extern "C" {

const char* uni_last_error(void) { return g_err; }
int uni_version(void) { return 1; }

int uni_variant_trace(int on) {
    std::lock_guard<std::mutex> lk(g_vt_mu);
    if (on) vt_map().clear();
    g_uni_variant_trace.store(on ? 1 : 0, std::memory_order_relaxed);
    return 0;
}
size_t uni_variant_trace_read(char* buf, size_t cap) {
    std::string out;
    {
        std::lock_guard<std::mutex> lk(g_vt_mu);
        for (const auto& kv : vt_map()) out += kv.first + "\t" + std::to_string(kv.second) + "\n";      // std::map: sorted by tag
    }
    if (buf && cap) {
        const size_t n = out.size() < cap - 1 ? out.size() : cap - 1;
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return out.size() + 1;
}

uni_ctx* uni_ctx_create(int device_id, const uni_model_cfg* cfg) {
    if (!cfg) { uni_set_error("cfg is NULL"); return nullptr; }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) {
        uni_set_error("no HIP device %d (count %d)", device_id, n);
        return nullptr;
    }
    for (int i = 0; i < 4; ++i)
        if (cfg->dims[i] <= 0 || cfg->dims[i] % 8 || cfg->depths[i] < 0) { uni_set_error("bad cfg dims/depths"); return nullptr; }
    if (cfg->precision < 0 || cfg->precision > 2) { uni_set_error("precision %d unknown (0 = bf16, 1 = fp32, 2 = f16x2)", cfg->precision); return nullptr; }
    if (cfg->embed_dim != 128) { uni_set_error("embed_dim %d unsupported (128)", cfg->embed_dim); return nullptr; }
    uni_ctx* c = new uni_ctx();
    c->device = device_id;
    c->cfg = *cfg;
    c->b32 = cfg->precision;      // ActFmt
    return c;
}
void uni_ctx_destroy(uni_ctx* ctx) { engine_destroy(ctx); }

int uni_ctx_load_param(uni_ctx* ctx, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    UNI_REQUIRE(ctx && name && host_data && (shape || ndim == 0), "load_param: NULL argument");
    UNI_REQUIRE(!ctx->finalized, "load_param after finalize");
    HostParam p;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { p.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    p.data.assign(host_data, host_data + n);
    ctx->host[name] = std::move(p);
    return 0;
}
// ---- flat weights file (include/unicorn_hip.h: "UNIW1", cfg, tensors) ----
namespace {
struct FileCloser { FILE* f; ~FileCloser() { if (f) fclose(f); } };
bool read_exact(FILE* f, void* dst, size_t n) { return fread(dst, 1, n, f) == n; }
int open_weights(const char* path, FILE** out, uni_model_cfg* cfg, int32_t* count) {
    UNI_REQUIRE(path, "weights file: NULL path");
    FILE* f = fopen(path, "rb");
    UNI_REQUIRE(f, "weights file: cannot open %s", path);
    char magic[8];
    int32_t raw[15];
    if (!read_exact(f, magic, 8) || memcmp(magic, "UNIW1\0\0\0", 8) != 0 || !read_exact(f, raw, sizeof(raw)) || !read_exact(f, count, 4) || *count < 0) {
        fclose(f);
        uni_set_error("weights file %s: bad header (not a UNIW1 file)", path);
        return -1;
    }
    static_assert(sizeof(uni_model_cfg) == 15 * sizeof(int32_t), "uni_model_cfg is 15 int32");
    memcpy(cfg, raw, sizeof(raw));
    *out = f;
    return 0;
}
}  // namespace
int uni_weights_file_cfg(const char* path, uni_model_cfg* cfg_out) {
    UNI_REQUIRE(cfg_out, "weights_file_cfg: NULL cfg");
    FILE* f = nullptr;
    int32_t count = 0;
    int rc = open_weights(path, &f, cfg_out, &count);
    if (rc) return rc;
    fclose(f);
    return 0;
}
int uni_ctx_load_file(uni_ctx* ctx, const char* path, int* n_loaded) {
    UNI_REQUIRE(ctx, "load_file: NULL ctx");
    UNI_REQUIRE(!ctx->finalized, "load_file after finalize");
    FILE* f = nullptr;
    uni_model_cfg cfg;
    int32_t count = 0;
    int rc = open_weights(path, &f, &cfg, &count);
    if (rc) return rc;
    FileCloser closer{f};
    for (int i = 0; i < 15; ++i)
        if (i != 14 && reinterpret_cast<const int32_t*>(&cfg)[i] != reinterpret_cast<const int32_t*>(&ctx->cfg)[i]) {      // (precision may differ: the file holds fp32 tensors)
            uni_set_error("weights file %s was exported for another network configuration (field %d: %d, context: %d)", path, i,
                          reinterpret_cast<const int32_t*>(&cfg)[i], reinterpret_cast<const int32_t*>(&ctx->cfg)[i]);
            return -1;
        }
    std::vector<char> name;
    std::vector<float> data;
    for (int32_t t = 0; t < count; ++t) {
        int32_t nl = 0, nd = 0;
        int64_t shape[8];
        if (!read_exact(f, &nl, 4) || nl <= 0 || nl > 4096) { uni_set_error("weights file %s: truncated at tensor %d", path, t); return -1; }
        name.assign((size_t)nl + 1, 0);
        if (!read_exact(f, name.data(), (size_t)nl) || !read_exact(f, &nd, 4) || nd < 0 || nd > 8 || !read_exact(f, shape, sizeof(int64_t) * (size_t)nd)) {
            uni_set_error("weights file %s: truncated at tensor %d", path, t);
            return -1;
        }
        size_t n = 1;
        for (int i = 0; i < nd; ++i) {
            if (shape[i] < 0 || shape[i] > (1 << 28)) { uni_set_error("weights file %s: bad shape of %s", path, name.data()); return -1; }
            n *= (size_t)shape[i];
        }
        data.resize(n);
        if (!read_exact(f, data.data(), n * sizeof(float))) { uni_set_error("weights file %s: truncated data of %s", path, name.data()); return -1; }
        rc = uni_ctx_load_param(ctx, name.data(), data.data(), shape, nd);
        if (rc < 0) return rc;
    }
    if (n_loaded) *n_loaded = count;
    return 0;
}
int uni_ctx_finalize(uni_ctx* ctx, int* n_missing) {
    UNI_REQUIRE(ctx, "ctx is NULL");
    UNI_REQUIRE(!ctx->finalized, "already finalized");
    int rc = engine_finalize(ctx);
    if (rc == 0 && getenv("UNI_CHECK_SAT")) rc = engine_set_check(ctx, 1);
    if (n_missing) *n_missing = (int)ctx->missing.size();
    return rc;
}
const char* uni_ctx_missing_name(uni_ctx* ctx, int i) {
    if (!ctx || i < 0 || i >= (int)ctx->missing.size()) return nullptr;
    return ctx->missing[i].c_str();
}
int uni_ctx_reserve(uni_ctx* ctx, int B, int H, int W) {
    UNI_REQUIRE(ctx && ctx->finalized, "context not finalized");
    return engine_reserve(ctx, B, H, W);
}

int uni_ctx_set_check(uni_ctx* ctx, int on) { return engine_set_check(ctx, on); }
int uni_ctx_stats(uni_ctx* ctx, long long* out4) { return engine_stats(ctx, out4); }
int uni_prof_begin(uni_ctx* ctx) { UNI_REQUIRE(ctx, "ctx is NULL"); return engine_prof_begin(ctx); }
int uni_prof_end(uni_ctx* ctx, double* out16) { UNI_REQUIRE(ctx && out16, "prof_end: NULL argument"); return engine_prof_end(ctx, out16); }

int uni_backbone_fpn(uni_ctx* ctx, const float* img, int B, int H, int W, float* fpn0, float* fpn1, float* fpn2, float* feat16,
                     uni_stream_t stream) {
    UNI_REQUIRE(ctx && img && fpn0 && fpn1 && fpn2 && feat16, "backbone_fpn: NULL argument");
    API(engine_backbone_fpn(ctx, img, B, H, W, fpn0, fpn1, fpn2, feat16, S(stream)));
}
int uni_interaction(uni_ctx* ctx, const float* feat_ref, const float* pos_ref, const float* feat_cur, const float* pos_cur,
                    int B, int h, int w, float* out_ref, float* out_cur, uni_stream_t stream) {
    UNI_REQUIRE(ctx && feat_ref && pos_ref && feat_cur && pos_cur && out_ref && out_cur, "interaction: NULL argument");
    UNI_REQUIRE(h > 0 && w > 0, "interaction: h=%d w=%d", h, w);
    API(engine_interaction(ctx, feat_ref, pos_ref, feat_cur, pos_cur, B, h, w, out_ref, out_cur, S(stream)));
}
int uni_upsample(uni_ctx* ctx, const float* feat, int B, int h, int w, float* embed, uni_stream_t stream) {
    UNI_REQUIRE(ctx && feat && embed && h > 0 && w > 0, "upsample: bad argument");
    API(engine_upsample(ctx, feat, B, h, w, embed, S(stream)));
}
int uni_head(uni_ctx* ctx, const float* fpn0, const float* fpn1, const float* fpn2, const float* prior8, const float* prior16,
             const float* prior32, int B, int H, int W, int mode, float* out, float* dyn_params, float* mask_feats, float* up_masks,
             uni_stream_t stream) {
    UNI_REQUIRE(ctx && fpn0 && fpn1 && fpn2 && prior8 && prior16 && prior32 && out, "head: NULL argument");
    UNI_REQUIRE(mode >= 0 && mode <= 3, "head: mode %d (bit 0: 0 = sot / 1 = mot, bit 1: raw outputs, decode_in_inference = False)", mode);
    API(engine_head(ctx, fpn0, fpn1, fpn2, prior8, prior16, prior32, B, 1, H, W, mode, out, dyn_params, mask_feats, up_masks, S(stream)));
}
int uni_head_objects(uni_ctx* ctx, const float* fpn0, const float* fpn1, const float* fpn2, const float* prior8, const float* prior16,
                     const float* prior32, int K, int H, int W, int mode, float* out, float* dyn_params, float* mask_feats,
                     float* up_masks, uni_stream_t stream) {
    UNI_REQUIRE(ctx && fpn0 && fpn1 && fpn2 && prior8 && prior16 && prior32 && out, "head_objects: NULL argument");
    UNI_REQUIRE(mode >= 0 && mode <= 3, "head_objects: mode %d", mode);
    API(engine_head(ctx, fpn0, fpn1, fpn2, prior8, prior16, prior32, 1, K, H, W, mode, out, dyn_params, mask_feats, up_masks, S(stream)));
}
int uni_pos_embed(uni_ctx* ctx, int h, int w, float* out_nhwc, uni_stream_t stream) {
    UNI_REQUIRE(ctx && out_nhwc && h > 0 && w > 0, "pos_embed: bad argument");
    API(engine_pos_embed(ctx, h, w, out_nhwc, S(stream)));
}

// ---- fp32 / fp64 operator pairs: ONE definition each, expanded for (symbol suffix, element type) = (, float) and (_f64, double).  A body checks
// for NULL, fills the unit's argument struct (kernels.h) and calls the templated launcher; everything else lives in the unit.
#define UNI_PAIR(DEF) DEF(, float) DEF(_f64, double)
#define DEF_MSDA(SFX, T)                                                                                                                 \
    int uni_msda_fwd##SFX(const T* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const T* sampling_loc,        \
                          const T* attn_weight, T* out, int N, int S_, int M, int D, int Lq, int L, int P, uni_stream_t stream) {        \
        UNI_REQUIRE(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && out, "msda: NULL argument");          \
        API(launch_msda<T>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, out, N, S_, M, D, Lq, L, P, S(stream))); \
    }                                                                                                                                    \
    int uni_msda_bwd##SFX(const T* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const T* sampling_loc,        \
                          const T* attn_weight, const T* grad_output, T* grad_value, T* grad_sampling_loc, T* grad_attn_weight, int N,   \
                          int S_, int M, int D, int Lq, int L, int P, uni_stream_t stream) {                                             \
        UNI_REQUIRE(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && grad_output && grad_value &&          \
                    grad_sampling_loc && grad_attn_weight, "msda_bwd: NULL argument");                                                   \
        API(launch_msda_bwd<T>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, grad_value,             \
                               grad_sampling_loc, grad_attn_weight, N, S_, M, D, Lq, L, P, S(stream)));                                  \
    }
UNI_PAIR(DEF_MSDA)
size_t uni_corr_workspace_bytes(int R, int Q, int K) { return corr_workspace_bytes(R, Q, K); }
int uni_corr_softmax_pv(const float* e_ref, const float* e_cur, const float* values, float* out, int R, int Q, int D, int K,
                        int precision, void* workspace, size_t workspace_bytes, uni_stream_t stream) {
    UNI_REQUIRE(e_ref && e_cur && values && out && workspace, "corr: NULL argument");
    API(launch_corr(e_ref, e_cur, values, out, R, Q, D, K, precision, workspace, workspace_bytes, S(stream)));
}
size_t uni_corr_workspace_bytes_batched(int B, int R, int Q, int K) { return corr_workspace_bytes_batched(B, R, Q, K); }
int uni_corr_softmax_pv_batched(const float* e_ref, const float* e_cur, const float* values, float* out, int B, int R, int Q, int D, int K,
                                int values_per_frame, int precision, void* workspace, size_t workspace_bytes, uni_stream_t stream) {
    UNI_REQUIRE(e_ref && e_cur && values && out && workspace, "corr: NULL argument");
    API(launch_corr_batched(e_ref, e_cur, values, out, B, R, Q, D, K, values_per_frame, precision, workspace, workspace_bytes, S(stream)));
}
size_t uni_corr_bwd_workspace_bytes(int B, int R, int Q, int K) { return corr_bwd_workspace_bytes(B, R, Q, K); }
int uni_corr_softmax_pv_lse(const float* e_ref, const float* e_cur, const float* values, float* out, float* lse, int B, int R, int Q, int D,
                            int K, int values_per_frame, int precision, void* workspace, size_t workspace_bytes, uni_stream_t stream) {
    UNI_REQUIRE(e_ref && e_cur && values && out && lse && workspace, "corr_lse: NULL argument");
    UNI_REQUIRE(B > 0 && R > 0 && Q > 0 && K > 0, "corr_lse: empty problem B=%d R=%d Q=%d K=%d", B, R, Q, K);
    UNI_REQUIRE(workspace_bytes >= corr_bwd_workspace_bytes(B, R, Q, K), "corr_lse: workspace too small (uni_corr_bwd_workspace_bytes)");
    API(launch_corr_batched(e_ref, e_cur, values, out, B, R, Q, D, K, values_per_frame, precision, workspace, workspace_bytes, S(stream), lse));
}
int uni_corr_softmax_pv_bwd(const float* e_ref, const float* e_cur, const float* values, const float* out, const float* lse,
                            const float* grad_out, float* grad_e_ref, float* grad_e_cur, float* grad_values, int B, int R, int Q, int D,
                            int K, int values_per_frame, int precision, void* workspace, size_t workspace_bytes, uni_stream_t stream) {
    UNI_REQUIRE(e_ref && e_cur && values && out && lse && grad_out && workspace, "corr_bwd: NULL argument");
    API(launch_corr_bwd(e_ref, e_cur, values, out, lse, grad_out, grad_e_ref, grad_e_cur, grad_values, B, R, Q, D, K, values_per_frame,
                        precision, workspace, workspace_bytes, S(stream)));
}
int uni_corr_softmax_pv_lse_f64(const double* e_ref, const double* e_cur, const double* values, double* out, double* lse, int B, int R,
                                int Q, int D, int K, int values_per_frame, uni_stream_t stream) {
    UNI_REQUIRE(e_ref && e_cur && values && out && lse, "corr_lse_f64: NULL argument");
    API(launch_corr_f64(e_ref, e_cur, values, out, lse, B, R, Q, D, K, values_per_frame, S(stream)));
}
int uni_corr_softmax_pv_bwd_f64(const double* e_ref, const double* e_cur, const double* values, const double* out, const double* lse,
                                const double* grad_out, double* grad_e_ref, double* grad_e_cur, double* grad_values, int B, int R,
                                int Q, int D, int K, int values_per_frame, uni_stream_t stream) {
    UNI_REQUIRE(e_ref && e_cur && values && out && lse && grad_out, "corr_bwd_f64: NULL argument");
    API(launch_corr_bwd_f64(e_ref, e_cur, values, out, lse, grad_out, grad_e_ref, grad_e_cur, grad_values, B, R, Q, D, K, values_per_frame,
                            S(stream)));
}
int uni_prior_pyramid(const float* p8, float* p16, float* p32, int K, int H8, int W8, uni_stream_t stream) {
    UNI_REQUIRE(p8 && p16 && p32, "prior_pyramid: NULL argument");
    API(launch_prior_pyramid(p8, p16, p32, K, H8, W8, S(stream)));
}
int uni_label_map_s8(const float* box_xyxy_dev, float* out, int H, int W, uni_stream_t stream) {
    UNI_REQUIRE(box_xyxy_dev && out && H % 8 == 0 && W % 8 == 0, "label_map: bad argument");
    API(launch_label_map_s8(box_xyxy_dev, out, H, W, S(stream)));
}
int uni_sample_embeddings(const float* embed_nhwc, int H8, int W8, int C, const float* boxes_xyxy, int ld_boxes, int n, float stride,
                          float* out, uni_stream_t stream) {
    UNI_REQUIRE(embed_nhwc && (n == 0 || (boxes_xyxy && out)), "sample_embeddings: NULL argument");
    API(launch_sample_embed(embed_nhwc, H8, W8, C, boxes_xyxy, ld_boxes, n, stride, out, S(stream)));
}
int uni_letterbox(const uint8_t* img_hwc, int h, int w, int swap_rb, int H, int W, float* out_chw, double* r_out, uni_stream_t stream) {
    UNI_REQUIRE(img_hwc && out_chw, "letterbox: NULL argument");
    API(launch_letterbox(img_hwc, h, w, swap_rb, H, W, out_chw, r_out, S(stream)));
}
size_t uni_nms_workspace_bytes(int n) { return nms_workspace_bytes(n); }
int uni_nms(const float* boxes_xyxy, const float* scores, int n, float iou_thr, int32_t* keep_idx, int32_t* n_out, void* workspace,
            size_t workspace_bytes, uni_stream_t stream) {
    UNI_REQUIRE(n_out && (n == 0 || (boxes_xyxy && scores && keep_idx && workspace)), "nms: NULL argument");
    API(launch_nms(boxes_xyxy, scores, n, iou_thr, keep_idx, n_out, workspace, workspace_bytes, S(stream)));
}
int uni_decode_outputs(float* outputs, int B, int H, int W, int nch, uni_stream_t stream) {
    UNI_REQUIRE(outputs && B >= 1 && H % 32 == 0 && W % 32 == 0 && nch >= 5, "decode_outputs: bad argument");
    const int w0 = W / 8, w1 = W / 16, w2 = W / 32;
    API(launch_decode(outputs, outputs, (H / 8) * w0, w0, (H / 16) * w1, w1, (H / 32) * w2, w2, nch, S(stream), B));
}
size_t uni_postprocess_workspace_bytes(int A) { return postprocess_workspace_bytes(A); }
int uni_postprocess(float* pred, int A, int ld, int num_classes, float conf_thre, float nms_thre, int flags, int max_det,
                    float* det_out, int32_t* keep_idx, int32_t* n_out, void* workspace, size_t workspace_bytes,
                    uni_stream_t stream) {
    UNI_REQUIRE(n_out && (A == 0 || (pred && workspace)) && (max_det == 0 || (det_out && keep_idx)), "postprocess: NULL argument");
    API(launch_postprocess(pred, A, ld, num_classes, conf_thre, nms_thre, flags, max_det, det_out, keep_idx, n_out,
                           workspace, workspace_bytes, S(stream)));
}
int uni_condinst_masks(const float* mask_feats, const float* up_masks, const float* params, int ldp, const float* inst_loc,
                       const int32_t* inst_lvl, int n, int H8, int W8, int up_rate, int d_rate, float* out, void* workspace,
                       size_t workspace_bytes, uni_stream_t stream) {
    if (n == 0) return 0;
    UNI_REQUIRE(mask_feats && up_masks && params && inst_loc && inst_lvl && out && workspace, "condinst: NULL argument");
    CondInstArgs a;
    if (int rc = condinst_args(a, "condinst", mask_feats, up_masks, params, ldp, inst_loc, inst_lvl, n, H8, W8, up_rate, d_rate, workspace,
                               workspace_bytes)) return rc;
    a.out = out;
    API(launch_condinst(a, S(stream)));
}
size_t uni_condinst_loss_workspace_bytes(int n, int H8, int W8, int up_rate) { return condinst_loss_workspace_bytes(n, H8, W8, up_rate); }
#define DEF_CONDINST_LOSS(SFX, T)                                                                                                                \
    int uni_condinst_loss_fwd##SFX(const T* mask_feats, const T* up_masks, const T* params, int ldp, const T* inst_loc, const int32_t* inst_lvl, \
                                   const T* gt, int n, int H8, int W8, int up_rate, T* loss, T* sums, void* workspace, size_t workspace_bytes,   \
                                   uni_stream_t stream) {                                                                                        \
        UNI_REQUIRE(mask_feats && up_masks && params && inst_loc && inst_lvl && gt && loss && sums && workspace,                                 \
                    "condinst_loss_fwd" #SFX ": NULL argument");                                                                                 \
        const ClArgs<T> a{mask_feats, up_masks, params, ldp, inst_loc, inst_lvl, gt, n, H8, W8, up_rate, workspace, workspace_bytes};            \
        API(launch_condinst_loss_fwd<T>(a, loss, sums, S(stream)));                                                                              \
    }                                                                                                                                            \
    int uni_condinst_loss_bwd##SFX(const T* mask_feats, const T* up_masks, const T* params, int ldp, const T* inst_loc, const int32_t* inst_lvl, \
                                   const T* gt, const T* sums, const T* grad_loss, int n, int H8, int W8, int up_rate, T* grad_mask_feats,       \
                                   T* grad_up_masks, T* grad_params, void* workspace, size_t workspace_bytes, uni_stream_t stream) {             \
        UNI_REQUIRE(mask_feats && up_masks && params && inst_loc && inst_lvl && gt && sums && grad_loss && workspace,                            \
                    "condinst_loss_bwd" #SFX ": NULL argument");                                                                                 \
        const ClArgs<T> a{mask_feats, up_masks, params, ldp, inst_loc, inst_lvl, gt, n, H8, W8, up_rate, workspace, workspace_bytes};            \
        API(launch_condinst_loss_bwd<T>(a, sums, grad_loss, grad_mask_feats, grad_up_masks, grad_params, S(stream)));                            \
    }
UNI_PAIR(DEF_CONDINST_LOSS)
size_t uni_simota_workspace_bytes(int B, int A, int Gmax, int C) { return simota_workspace_bytes(B, A, Gmax, C); }
int uni_simota_assign(const float* outputs, int ld_out, const float* labels, const int32_t* num_gt, int M, const float* x_shifts,
                      const float* y_shifts, const float* strides, int B, int A, int C, int img_h, int img_w, uint8_t* fg_mask,
                      int32_t* matched_gt, float* matched_iou, int32_t* num_fg, void* workspace, size_t workspace_bytes,
                      uni_stream_t stream) {
    UNI_REQUIRE(outputs && (labels || M == 0) && num_gt && x_shifts && y_shifts && strides && fg_mask && matched_gt && matched_iou && num_fg &&
                workspace, "simota_assign: NULL argument");
    API(launch_simota_assign(outputs, ld_out, labels, num_gt, M, x_shifts, y_shifts, strides, B, A, C, img_h, img_w, fg_mask, matched_gt,
                             matched_iou, num_fg, workspace, workspace_bytes, S(stream)));
}
static inline McStride mc_stride(const int64_t* s) { return McStride{s[0], s[1], s[2], s[3]}; }
static const int64_t mc_no_stride[4] = {0, 0, 0, 0};
size_t uni_head_mask_loss_workspace_bytes(int B, int A, int H8, int W8, int up_rate, int capacity) {
    return head_mask_loss_workspace_bytes(B, A, H8, W8, up_rate, capacity);
}
#define DEF_HEAD_MASK_LOSS(SFX, T)                                                                                                               \
    int uni_head_mask_loss_fwd##SFX(const T* mask_feats, const T* up_masks, const T* params, int ldp, const int32_t* fpn_levels, const T* masks, \
                                    int M, const uint8_t* fg_mask, const int32_t* matched_gt, const T* x_shifts, const T* y_shifts,              \
                                    const T* strides, int B, int A, int H8, int W8, int up_rate, int capacity, T* out, T* sums, void* workspace, \
                                    size_t workspace_bytes, uni_stream_t stream) {                                                               \
        UNI_REQUIRE(mask_feats && up_masks && params && fpn_levels && masks && fg_mask && matched_gt && x_shifts && y_shifts && strides &&       \
                    workspace && out && sums, "head_mask_loss_fwd" #SFX ": NULL argument");                                                      \
        const HMIn<T> a{mask_feats, up_masks, params, ldp, fpn_levels, masks, M, fg_mask, matched_gt, x_shifts, y_shifts, strides, B, A, H8, W8, \
                        up_rate, capacity};                                                                                                      \
        API(launch_head_mask_loss_fwd<T>(a, out, sums, workspace, workspace_bytes, S(stream)));                                                  \
    }                                                                                                                                            \
    int uni_head_mask_loss_bwd##SFX(const T* mask_feats, const T* up_masks, const T* params, int ldp, const int32_t* fpn_levels, const T* masks, \
                                    int M, const uint8_t* fg_mask, const int32_t* matched_gt, const T* x_shifts, const T* y_shifts,              \
                                    const T* strides, int B, int A, int H8, int W8, int up_rate, int capacity, const T* sums, const T* grad_out, \
                                    T* grad_mask_feats, T* grad_up_masks, T* grad_params, int ld_grad, void* workspace, size_t workspace_bytes,  \
                                    uni_stream_t stream) {                                                                                       \
        UNI_REQUIRE(mask_feats && up_masks && params && fpn_levels && masks && fg_mask && matched_gt && x_shifts && y_shifts && strides &&       \
                    workspace && sums && grad_out, "head_mask_loss_bwd" #SFX ": NULL argument");                                                 \
        const HMIn<T> a{mask_feats, up_masks, params, ldp, fpn_levels, masks, M, fg_mask, matched_gt, x_shifts, y_shifts, strides, B, A, H8, W8, \
                        up_rate, capacity};                                                                                                      \
        API(launch_head_mask_loss_bwd<T>(a, sums, grad_out, grad_mask_feats, grad_up_masks, grad_params, ld_grad, workspace, workspace_bytes,    \
                                         S(stream)));                                                                                            \
    }
UNI_PAIR(DEF_HEAD_MASK_LOSS)
size_t uni_prop_workspace_bytes(int B, int Kc, int Q) { return prop_workspace_bytes(B, Kc, Q); }
#define DEF_PROP_LOSS(SFX, T)                                                                                                                    \
    int uni_prop_labels##SFX(const float* targets, const void* masks, int mask_u8, int B, int M, int Kc, int sot, int H8, int W8, int mask_rate, \
                             int32_t* matched, int32_t* num_matched, T* gt0, T* gt1, uni_stream_t stream) {                                      \
        UNI_REQUIRE(targets && matched && num_matched && gt0 && gt1, "prop_labels" #SFX ": NULL argument");                                      \
        const PlLabelArgs a{targets, masks, mask_u8, B, M, Kc, sot, H8, W8, mask_rate, matched, num_matched};                                    \
        API(launch_prop_labels<T>(a, gt0, gt1, S(stream)));                                                                                      \
    }                                                                                                                                            \
    int uni_prop_dice_pyramid_fwd##SFX(const T* pred, const T* gt1, const int32_t* num_matched, int B, int Kc, int H8, int W8, T* p16, T* p32,   \
                                       T* loss, double* sums, void* workspace, size_t workspace_bytes, uni_stream_t stream) {                    \
        UNI_REQUIRE(pred && gt1 && p16 && p32 && loss && sums && workspace, "prop_dice_pyramid_fwd" #SFX ": NULL argument");                     \
        const PlDiceArgs<T> a{pred, gt1, num_matched, B, Kc, H8, W8};                                                                            \
        API(launch_prop_dice_pyramid_fwd<T>(a, p16, p32, loss, sums, workspace, workspace_bytes, S(stream)));                                    \
    }                                                                                                                                            \
    int uni_prop_dice_pyramid_bwd##SFX(const T* pred, const T* gt1, const int32_t* num_matched, const double* sums, const T* grad_p8,            \
                                       const T* grad_p16, const T* grad_p32, const T* grad_loss, int B, int Kc, int H8, int W8, T* grad_pred,    \
                                       uni_stream_t stream) {                                                                                    \
        UNI_REQUIRE(pred && gt1 && sums && grad_pred, "prop_dice_pyramid_bwd" #SFX ": NULL argument");                                           \
        const PlDiceArgs<T> a{pred, gt1, num_matched, B, Kc, H8, W8};                                                                            \
        API(launch_prop_dice_pyramid_bwd<T>(a, sums, grad_p8, grad_p16, grad_p32, grad_loss, grad_pred, S(stream)));                             \
    }
UNI_PAIR(DEF_PROP_LOSS)
int uni_opt_chunk_elems(void) { return opt_chunk_elems(); }
size_t uni_opt_table_bytes(int n_tensors, int total_chunks) { return opt_table_bytes(n_tensors, total_chunks); }
int uni_opt_step(const void* table, size_t table_bytes, const void* block_map, size_t map_bytes, int n_tensors, int vec_chunks, int total_chunks,
                 float* step, float* scale, int32_t* growth_tracker, float* found_inf, double lr, double beta1, double beta2, double eps,
                 double ema_decay, double growth_factor, double backoff_factor, int growth_interval, uni_stream_t stream) {
    UNI_REQUIRE(table && block_map && step, "opt_step: NULL argument");
    API(launch_opt_step(table, table_bytes, block_map, map_bytes, n_tensors, vec_chunks, total_chunks, step, scale, growth_tracker, found_inf, lr, beta1,
                        beta2, eps, ema_decay, growth_factor, backoff_factor, growth_interval, S(stream)));
}
size_t uni_mot_corr_workspace_bytes(int B, int M, int C) { return mot_corr_workspace_bytes(B, M, C); }
#define DEF_MOT_CORR_LOSS(SFX, T)                                                                                                                \
    int uni_mot_corr_loss_fwd##SFX(const T* embed_0, const int64_t* strides_0, const T* embed_1, const int64_t* strides_1, const float* targets, \
                                   int B, int C, int H, int W, int M, float stride, int flags, T* loss, void* workspace, size_t workspace_bytes, \
                                   uni_stream_t stream) {                                                                                        \
        UNI_REQUIRE(embed_0 && strides_0 && embed_1 && strides_1 && targets && loss && workspace, "mot_corr_loss_fwd" #SFX ": NULL argument");   \
        const McArgs a{embed_0, embed_1, mc_stride(strides_0), mc_stride(strides_1), targets, B, C, H, W, M, stride, flags, workspace,           \
                       workspace_bytes};                                                                                                         \
        API(launch_mot_corr_fwd<T>(a, loss, S(stream)));                                                                                         \
    }                                                                                                                                            \
    int uni_mot_corr_loss_bwd##SFX(const T* embed_0, const int64_t* strides_0, const T* embed_1, const int64_t* strides_1, const float* targets, \
                                   const T* grad_loss, int B, int C, int H, int W, int M, float stride, int flags, T* grad_embed_0,              \
                                   const int64_t* grad_strides_0, T* grad_embed_1, const int64_t* grad_strides_1, void* workspace,               \
                                   size_t workspace_bytes, uni_stream_t stream) {                                                                \
        UNI_REQUIRE(embed_0 && strides_0 && embed_1 && strides_1 && targets && grad_loss && workspace && (!grad_embed_0 || grad_strides_0) &&    \
                    (!grad_embed_1 || grad_strides_1), "mot_corr_loss_bwd" #SFX ": NULL argument");                                              \
        const McArgs a{embed_0, embed_1, mc_stride(strides_0), mc_stride(strides_1), targets, B, C, H, W, M, stride, flags, workspace,           \
                       workspace_bytes};                                                                                                         \
        API(launch_mot_corr_bwd<T>(a, grad_loss, grad_embed_0, mc_stride(grad_embed_0 ? grad_strides_0 : mc_no_stride), grad_embed_1,            \
                                   mc_stride(grad_embed_1 ? grad_strides_1 : mc_no_stride), S(stream)));                                         \
    }
UNI_PAIR(DEF_MOT_CORR_LOSS)
size_t uni_head_loss_workspace_bytes(int B, int A, int C) { return head_loss_workspace_bytes(B, A, C); }
#define DEF_HEAD_LOSS(SFX, T)                                                                                                                      \
    int uni_head_loss_fwd##SFX(const T* outputs, int ld_out, const T* origin_preds, int ld_org, const T* labels, int M, const uint8_t* fg_mask,    \
                               const int32_t* matched_gt, const T* matched_iou, const int32_t* num_fg, const int32_t* num_gt, const T* x_shifts,   \
                               const T* y_shifts, const T* strides, int B, int A, int C, double reg_weight, T* out, void* workspace,               \
                               size_t workspace_bytes, uni_stream_t stream) {                                                                      \
        UNI_REQUIRE(outputs && (labels || M == 0) && fg_mask && matched_gt && matched_iou && num_fg && num_gt && x_shifts && y_shifts &&           \
                    strides && out && workspace, "head_loss_fwd" #SFX ": NULL argument");                                                          \
        const HlArgs<T> a{{outputs, ld_out, origin_preds, ld_org, labels, M, fg_mask, matched_gt, matched_iou, x_shifts, y_shifts, strides, A, C}, \
                          num_fg, num_gt, B, reg_weight, workspace, workspace_bytes};                                                              \
        API(launch_head_loss_fwd<T>(a, out, S(stream)));                                                                                           \
    }                                                                                                                                              \
    int uni_head_loss_bwd##SFX(const T* outputs, int ld_out, const T* origin_preds, int ld_org, const T* labels, int M, const uint8_t* fg_mask,    \
                               const int32_t* matched_gt, const T* matched_iou, const int32_t* num_fg, const int32_t* num_gt, const T* x_shifts,   \
                               const T* y_shifts, const T* strides, const T* grad_out, int B, int A, int C, double reg_weight, T* grad_outputs,    \
                               int ld_grad, T* grad_origin, void* workspace, size_t workspace_bytes, uni_stream_t stream) {                        \
        UNI_REQUIRE(outputs && (labels || M == 0) && fg_mask && matched_gt && matched_iou && num_fg && num_gt && x_shifts && y_shifts &&           \
                    strides && grad_out && workspace, "head_loss_bwd" #SFX ": NULL argument");                                                     \
        const HlArgs<T> a{{outputs, ld_out, origin_preds, ld_org, labels, M, fg_mask, matched_gt, matched_iou, x_shifts, y_shifts, strides, A, C}, \
                          num_fg, num_gt, B, reg_weight, workspace, workspace_bytes};                                                              \
        API(launch_head_loss_bwd<T>(a, grad_out, grad_outputs, ld_grad, grad_origin, S(stream)));                                                  \
    }
UNI_PAIR(DEF_HEAD_LOSS)
#define DEF_HEAD_ASSEMBLE(SFX, T)                                                                                                                  \
    int uni_head_assemble_fwd##SFX(const void* const* reg, const void* const* obj, const void* const* cls, const void* const* ctrl,               \
                                   const int32_t* hs, const int32_t* ws, const double* strides, const int32_t* layouts, int L, int B, int C,      \
                                   int P, int map_dtype, T* outputs, int ld_out, T* origin_preds, T* x_shifts, T* y_shifts, T* expanded_strides,  \
                                   T* dynamic_params, int ld_par, int32_t* fpn_levels, uni_stream_t stream) {                                     \
        UNI_REQUIRE(reg && obj && cls && hs && ws && strides && layouts, "head_assemble_fwd" #SFX ": NULL argument");                             \
        const HaShape sh{hs, ws, strides, layouts, L, B, C, P, map_dtype};                                                                         \
        const HaOut<T> o{outputs, ld_out, origin_preds, x_shifts, y_shifts, expanded_strides, dynamic_params, ld_par, fpn_levels};                 \
        API(launch_head_assemble_fwd<T>(sh, reg, obj, cls, ctrl, o, S(stream)));                                                                   \
    }                                                                                                                                              \
    int uni_head_assemble_bwd##SFX(const void* const* reg, const int32_t* hs, const int32_t* ws, const double* strides, const int32_t* layouts,   \
                                   int L, int B, int C, int P, int map_dtype, const T* grad_outputs, int ld_gout, const T* grad_origin,           \
                                   const T* grad_params, int ld_gpar, void* const* grad_reg, void* const* grad_obj, void* const* grad_cls,        \
                                   void* const* grad_ctrl, uni_stream_t stream) {                                                                 \
        UNI_REQUIRE(hs && ws && strides && layouts, "head_assemble_bwd" #SFX ": NULL argument");                                                  \
        const HaShape sh{hs, ws, strides, layouts, L, B, C, P, map_dtype};                                                                         \
        const HaGrad<T> g{grad_outputs, ld_gout, grad_origin, grad_params, ld_gpar};                                                               \
        API(launch_head_assemble_bwd<T>(sh, reg, g, grad_reg, grad_obj, grad_cls, grad_ctrl, S(stream)));                                          \
    }
UNI_PAIR(DEF_HEAD_ASSEMBLE)
size_t uni_dwln_train_workspace_bytes(int B, int H, int W, int C) { return dwln_train_workspace_bytes(B, H, W, C); }
#define DEF_DWLN_TRAIN(SFX, T)                                                                                                                     \
    int uni_dwln_train_fwd##SFX(const T* x, const T* weight, const T* bias, const T* ln_weight, const T* ln_bias, double eps, int B, int H, int W, \
                                int C, T* y, T* stats, uni_stream_t stream) {                                                                      \
        UNI_REQUIRE(x && weight && bias && ln_weight && ln_bias && y && stats, "dwln_train_fwd" #SFX ": NULL argument");                           \
        const DwlnArgs<T> a{x, weight, bias, ln_weight, ln_bias, eps, B, H, W, C};                                                                 \
        API(launch_dwln_train_fwd<T>(a, y, stats, S(stream)));                                                                                     \
    }                                                                                                                                              \
    int uni_dwln_train_bwd##SFX(const T* x, const T* weight, const T* bias, const T* ln_weight, const T* stats, const T* grad_y, int B, int H,     \
                                int W, int C, T* grad_x, T* grad_weight, T* grad_bias, T* grad_ln_weight, T* grad_ln_bias, void* workspace,        \
                                size_t workspace_bytes, uni_stream_t stream) {                                                                     \
        UNI_REQUIRE(x && weight && bias && ln_weight && stats && grad_y && workspace, "dwln_train_bwd" #SFX ": NULL argument");                    \
        const DwlnArgs<T> a{x, weight, bias, ln_weight, nullptr, 0.0, B, H, W, C};                                                                 \
        API(launch_dwln_train_bwd<T>(a, stats, grad_y, grad_x, grad_weight, grad_bias, grad_ln_weight, grad_ln_bias, workspace, workspace_bytes,   \
                                     S(stream)));                                                                                                  \
    }
UNI_PAIR(DEF_DWLN_TRAIN)
size_t uni_block_tail_workspace_bytes(int B, int H, int W, int C) { return block_tail_workspace_bytes(B, H, W, C); }
#define DEF_BLOCK_TAIL(SFX, T)                                                                                                                     \
    int uni_block_tail_fwd##SFX(const void* y, int y_dtype, const T* residual, int nchw, const T* gamma, const T* scale, int B, int H, int W,      \
                                int C, T* out, uni_stream_t stream) {                                                                              \
        UNI_REQUIRE(y && residual && out, "block_tail_fwd" #SFX ": NULL argument");                                                                \
        const BtArgs<T> a{y, y_dtype, residual, nchw, gamma, scale, B, H, W, C};                                                                   \
        API(launch_block_tail_fwd<T>(a, out, S(stream)));                                                                                          \
    }                                                                                                                                              \
    int uni_block_tail_bwd##SFX(const void* y, int y_dtype, const T* grad_out, int nchw, const T* gamma, const T* scale, int B, int H, int W,      \
                                int C, void* grad_y, T* grad_gamma, void* workspace, size_t workspace_bytes, uni_stream_t stream) {                \
        UNI_REQUIRE(y && grad_out, "block_tail_bwd" #SFX ": NULL argument");                                                                       \
        const BtArgs<T> a{y, y_dtype, grad_out, nchw, gamma, scale, B, H, W, C};                                                                   \
        API(launch_block_tail_bwd<T>(a, grad_y, grad_gamma, workspace, workspace_bytes, S(stream)));                                               \
    }
UNI_PAIR(DEF_BLOCK_TAIL)
size_t uni_lncf_train_workspace_bytes(int B, int H, int W, int C) { return lncf_train_workspace_bytes(B, H, W, C); }
#define DEF_LNCF_TRAIN(SFX, T)                                                                                                                     \
    int uni_lncf_train_fwd##SFX(const void* x, int x_dtype, int nchw, const T* weight, const T* bias, double eps, int B, int H, int W, int C,      \
                                T* y, T* stats, uni_stream_t stream) {                                                                             \
        UNI_REQUIRE(x && weight && bias && y && stats, "lncf_train_fwd" #SFX ": NULL argument");                                                   \
        const LncfArgs<T> a{x, x_dtype, nchw, weight, bias, eps, B, H, W, C};                                                                      \
        API(launch_lncf_train_fwd<T>(a, y, stats, S(stream)));                                                                                     \
    }                                                                                                                                              \
    int uni_lncf_train_bwd##SFX(const void* x, int x_dtype, int nchw, const T* weight, const T* stats, const T* grad_y, int B, int H, int W,       \
                                int C, void* grad_x, T* grad_weight, T* grad_bias, void* workspace, size_t workspace_bytes,                        \
                                uni_stream_t stream) {                                                                                             \
        UNI_REQUIRE(x && weight && stats && grad_y, "lncf_train_bwd" #SFX ": NULL argument");                                                      \
        const LncfArgs<T> a{x, x_dtype, nchw, weight, nullptr, 0.0, B, H, W, C};                                                                   \
        API(launch_lncf_train_bwd<T>(a, stats, grad_y, grad_x, grad_weight, grad_bias, workspace, workspace_bytes, S(stream)));                    \
    }
UNI_PAIR(DEF_LNCF_TRAIN)
size_t uni_down_train_workspace_bytes(int B, int H, int W, int C) { return down_train_workspace_bytes(B, H, W, C); }
#define DEF_DOWN_TRAIN(SFX, T)                                                                                                                     \
    int uni_down_train_fwd##SFX(const void* x, int x_dtype, const T* weight, const T* bias, double eps, int B, int H, int W, int C, int rebuild,   \
                                void* A, int a_dtype, T* stats, uni_stream_t stream) {                                                             \
        UNI_REQUIRE(x && weight && bias && A && stats, "down_train_fwd" #SFX ": NULL argument");                                                   \
        const DownArgs<T> a{x, x_dtype, a_dtype, weight, bias, eps, B, H, W, C};                                                                   \
        API(launch_down_train_fwd<T>(a, rebuild, A, stats, S(stream)));                                                                            \
    }                                                                                                                                              \
    int uni_down_train_bwd##SFX(const void* x, int x_dtype, const T* weight, const T* stats, const void* grad_A, int a_dtype, int B, int H, int W, \
                                int C, void* grad_x, T* grad_ln_weight, T* grad_ln_bias, void* workspace, size_t workspace_bytes,                  \
                                uni_stream_t stream) {                                                                                             \
        UNI_REQUIRE(x && weight && stats && grad_A, "down_train_bwd" #SFX ": NULL argument");                                                      \
        const DownArgs<T> a{x, x_dtype, a_dtype, weight, nullptr, 0.0, B, H, W, C};                                                                \
        API(launch_down_train_bwd<T>(a, stats, grad_A, grad_x, grad_ln_weight, grad_ln_bias, workspace, workspace_bytes, S(stream)));              \
    }                                                                                                                                              \
    int uni_patch4_gather##SFX(const void* x, int x_dtype, int B, int Cin, int H, int W, void* A, int a_dtype, uni_stream_t stream) {              \
        UNI_REQUIRE(x && A, "patch4_gather" #SFX ": NULL argument");                                                                               \
        API(launch_patch4_gather<T>(x, x_dtype, B, Cin, H, W, A, a_dtype, S(stream)));                                                             \
    }                                                                                                                                              \
    int uni_patch4_scatter##SFX(const void* grad_A, int a_dtype, int B, int Cin, int H, int W, void* grad_x, int x_dtype, uni_stream_t stream) {   \
        UNI_REQUIRE(grad_A && grad_x, "patch4_scatter" #SFX ": NULL argument");                                                                    \
        API(launch_patch4_scatter<T>(grad_A, a_dtype, B, Cin, H, W, grad_x, x_dtype, S(stream)));                                                  \
    }
UNI_PAIR(DEF_DOWN_TRAIN)
size_t uni_pw_mlp_workspace_bytes(int M, int Hd, int Co) { return pw_mlp_workspace_bytes(M, Hd, Co); }
#define DEF_PW_MLP(SFX, T)                                                                                                                         \
    int uni_pw_mlp_act_fwd##SFX(const void* h, int h_dtype, int M, int Hd, void* a, uni_stream_t stream) {                                         \
        UNI_REQUIRE(h && a, "pw_mlp_act_fwd" #SFX ": NULL argument");                                                                              \
        API(launch_pw_mlp_act_fwd<T>(h, h_dtype, M, Hd, a, S(stream)));                                                                            \
    }                                                                                                                                              \
    int uni_pw_mlp_act_bwd##SFX(const void* h, int h_dtype, const void* grad_a, int M, int Hd, void* a, void* grad_h, T* grad_b1,                  \
                                const void* grad_y, int Co, T* grad_b2, void* workspace, size_t workspace_bytes, uni_stream_t stream) {            \
        const PwBwdArgs<T> args{h, grad_a, h_dtype, M, Hd, a, grad_h, grad_b1, grad_y, Co, grad_b2};                                               \
        API(launch_pw_mlp_act_bwd<T>(args, workspace, workspace_bytes, S(stream)));                                                                \
    }
UNI_PAIR(DEF_PW_MLP)
size_t uni_gn_act_train_workspace_bytes(int B, int H, int W, int C, int G) { return gn_act_train_workspace_bytes(B, H, W, C, G); }
#define DEF_GN_ACT_TRAIN(SFX, T)                                                                                                                   \
    int uni_gn_act_train_fwd##SFX(const void* x, int x_dtype, int nchw, const T* weight, const T* bias, double eps, int act, int B, int H, int W,  \
                                  int C, int G, T* y, T* stats, uni_stream_t stream) {                                                             \
        UNI_REQUIRE(x && weight && bias && y && stats, "gn_act_train_fwd" #SFX ": NULL argument");                                                 \
        const GnArgs<T> a{x, x_dtype, nchw, weight, bias, eps, act, B, H, W, C, G};                                                                \
        API(launch_gn_act_train_fwd<T>(a, y, stats, S(stream)));                                                                                   \
    }                                                                                                                                              \
    int uni_gn_act_train_bwd##SFX(const void* x, int x_dtype, int nchw, const T* weight, const T* bias, const T* stats, const T* grad_y, int act,  \
                                  int B, int H, int W, int C, int G, void* grad_x, T* grad_weight, T* grad_bias, void* workspace,                  \
                                  size_t workspace_bytes, uni_stream_t stream) {                                                                   \
        UNI_REQUIRE(x && weight && bias && stats && grad_y, "gn_act_train_bwd" #SFX ": NULL argument");                                            \
        const GnArgs<T> a{x, x_dtype, nchw, weight, bias, 0.0, act, B, H, W, C, G};                                                                \
        API(launch_gn_act_train_bwd<T>(a, stats, grad_y, grad_x, grad_weight, grad_bias, workspace, workspace_bytes, S(stream)));                  \
    }
UNI_PAIR(DEF_GN_ACT_TRAIN)

// F.interpolate(scale_factor = 1/r): output size floor(in * (1/r)), source scale (float)(1 / (1/r)) (ATen compute_scales_value)
static void resize_geometry(int Hn, int Wn, double r, int* ho, int* wo, float* rscale) {
    const double sf = 1.0 / r;
    *ho = (int)floor((double)Hn * sf);
    *wo = (int)floor((double)Wn * sf);
    *rscale = (float)(1.0 / sf);
}
int uni_mask_resize(const float* masks, int N, int Hn, int Wn, double r, int H, int W, float thr, float* out_prob, uint8_t* out_bin,
                    uni_stream_t stream) {
    UNI_REQUIRE((N == 0 || masks) && (out_prob || out_bin) && r > 0, "mask_resize: bad argument");
    int ho, wo; float rs;
    resize_geometry(Hn, Wn, r, &ho, &wo, &rs);
    API(launch_mask_resize(masks, N, Hn, Wn, rs, ho, wo, H, W, thr, out_prob, out_bin, S(stream)));
}
int uni_condinst_masks_u8(const float* mask_feats, const float* up_masks, const float* params, int ldp, const float* inst_loc,
                          const int32_t* inst_lvl, int n, int H8, int W8, int up_rate, int d_rate, double r, int H, int W, float thr,
                          float* out_prob, uint8_t* out_bin, void* workspace, size_t workspace_bytes, uni_stream_t stream) {
    if (n == 0) return 0;
    UNI_REQUIRE(mask_feats && up_masks && params && inst_loc && inst_lvl && (out_prob || out_bin) && workspace && r > 0, "condinst_u8: bad argument");
    CondInstArgs a;      // a.out stays NULL: stop after the convex upsample, coarse_ws holds (n, r H8, r W8) sigmoid scores
    if (int rc = condinst_args(a, "condinst_u8", mask_feats, up_masks, params, ldp, inst_loc, inst_lvl, n, H8, W8, up_rate, d_rate, workspace,
                               workspace_bytes)) return rc;
    int rc = launch_condinst(a, S(stream));
    if (rc) return rc;
    int ho, wo; float rs;
    resize_geometry(d_rate * up_rate * H8, d_rate * up_rate * W8, r, &ho, &wo, &rs);
    API(launch_condinst_resize(a.coarse_ws, n, up_rate * H8, up_rate * W8, d_rate, rs, ho, wo, H, W, thr, out_prob, out_bin, S(stream)));
}
int uni_vos_merge(const float* probs, const int32_t* prob_ids, int K1, int Hn, int Wn, double r, const uint8_t* init_masks,
                  const int32_t* init_ids, int K2, int H, int W, uint8_t* out, uni_stream_t stream) {
    UNI_REQUIRE(out && (K1 == 0 || (probs && prob_ids)) && (K2 == 0 || (init_masks && init_ids)) && r > 0, "vos_merge: bad argument");
    int ho = 0, wo = 0; float rs = 1.f;
    if (K1) resize_geometry(Hn, Wn, r, &ho, &wo, &rs);
    API(launch_vos_merge(probs, prob_ids, K1, Hn, Wn, rs, ho, wo, init_masks, init_ids, K2, H, W, out, S(stream)));
}
int uni_mots_overlap_free(const uint8_t* masks, int N, int H, int W, uint8_t* out, uni_stream_t stream) {
    UNI_REQUIRE(N == 0 || (masks && out), "overlap_free: NULL argument");
    API(launch_overlap_free(masks, N, H, W, out, S(stream)));
}
size_t uni_rle_workspace_bytes(int N, int H, int W, int max_runs) { return rle_workspace_bytes(N, H, W, max_runs); }
int uni_rle_encode(const uint8_t* masks, int N, int H, int W, int max_runs, int max_chars, uint8_t* out_chars, int32_t* out_len,
                   uint32_t* counts, int32_t* n_runs, void* workspace, size_t workspace_bytes, uni_stream_t stream) {
    UNI_REQUIRE(N == 0 || (masks && out_chars && out_len && workspace), "rle_encode: NULL argument");
    API(launch_rle_encode(masks, N, H, W, max_runs, max_chars, out_chars, out_len, counts, n_runs, workspace, workspace_bytes, S(stream)));
}

int uni_pack_weight(const float* w, int N, int Cin, int KH, int KW, uint16_t* out) {
    UNI_REQUIRE(w && out && N > 0 && Cin > 0, "pack_weight: bad argument");
    pack_weight_host(w, N, Cin, KH, KW, nullptr, out, cdiv(N, 256) * 256, cdiv(Cin * KH * KW, 64) * 64);
    return 0;
}
int uni_gemm_bf16(const uint16_t* A, int lda, const uint16_t* w_packed, int M, int N, int Hin, int Win, int Cin, int KH, int KW,
                  int stride, int pad, const float* bias, int act, const float* residual, int ldr, float* outF, int ldf,
                  uint16_t* outB, int ldb, double* gn_stats, int cpg, int force_cfg, uni_stream_t stream) {
    UNI_REQUIRE(A && w_packed && (outF || outB), "gemm: NULL argument");
    GemmArgs g;
    if (int rc = gemm_geometry(g, "gemm", A, lda, w_packed, M, N, Hin, Win, Cin, KH, KW, stride, pad)) return rc;
    g.bias = bias; g.act = act; g.res = residual; g.ldr = ldr; g.outF = outF; g.ldf = ldf;
    g.outB = reinterpret_cast<bf16*>(outB); g.ldb = ldb; g.stats = gn_stats; g.cpg = cpg; g.force_cfg = force_cfg; g.dbg = force_cfg / 1000;
    API(launch_gemm(g, S(stream)));
}
int uni_gemm_ex(const void* A, int lda, const void* w_packed, float wscale, int fmt, int M, int N, int Hin, int Win, int Cin, int KH, int KW, int stride,
                int pad, const float* bias, int act, int act_col0, const float* residual, int ldr, float* outF, int ldf, void* outB, int ldb,
                double* gn_stats, int cpg, int force_cfg, uni_stream_t stream) {
    UNI_REQUIRE(A && w_packed && (outF || outB), "gemm_ex: NULL argument");
    UNI_REQUIRE(fmt >= 0 && fmt <= 2 && KH > 0 && KW > 0 && stride > 0 && pad >= 0 && Cin > 0 && N > 0, "gemm_ex: fmt=%d / bad geometry", fmt);
    UNI_REQUIRE(act_col0 >= 0 && act_col0 <= N && force_cfg >= 0 && force_cfg < 1000, "gemm_ex: act_col0=%d force_cfg=%d (tile configuration only)", act_col0, force_cfg);
    GemmArgs g;
    if (int rc = gemm_geometry(g, "gemm_ex", A, lda, w_packed, M, N, Hin, Win, Cin, KH, KW, stride, pad)) return rc;
    g.Mper = g.M;
    g.bias = bias; g.act = act; g.act_col0 = act_col0; g.res = residual; g.ldr = ldr; g.outF = outF; g.ldf = ldf;
    g.outB = reinterpret_cast<bf16*>(outB); g.ldb = ldb; g.stats = gn_stats; g.cpg = cpg; g.force_cfg = force_cfg; g.b32 = fmt;
    g.wscale = fmt == FMT_H2 ? wscale : 1.f;
    API(launch_gemm(g, S(stream)));
}
int uni_gemm_stacked(const void* A, int lda, const void* w_packed, float wscale, int fmt, int B, int M, int N, int Hin, int Win, int Cin, int KH, int KW,
                     int stride, int pad, const float* bias, int act, int act_col0, const float* residual, int ldr, float* outF, int ldf, int out_hw,
                     int out_stride, int out_off, int outF_rows, void* outB, int ldb, double* gn_stats, int cpg, int splitk, int force_cfg,
                     uni_stream_t stream) {
    UNI_REQUIRE(A && w_packed && (outF || outB), "gemm_stacked: NULL argument");
    UNI_REQUIRE(fmt >= 0 && fmt <= 2 && KH > 0 && KW > 0 && stride > 0 && pad >= 0 && Cin > 0 && N > 0 && Hin > 0 && Win > 0, "gemm_stacked: fmt=%d / bad geometry", fmt);
    UNI_REQUIRE(act_col0 >= 0 && act_col0 <= N && force_cfg >= 0 && force_cfg < 1000, "gemm_stacked: act_col0=%d force_cfg=%d (tile configuration only)", act_col0, force_cfg);
    UNI_REQUIRE(B >= 1 && B < 128, "gemm_stacked: B=%d (1 .. 127 samples)", B);
    UNI_REQUIRE(M > 0 && M % B == 0, "gemm_stacked: M=%d is not a multiple of B=%d", M, B);
    GemmArgs g;
    if (int rc = gemm_geometry(g, "gemm_stacked", A, lda, w_packed, M / B, N, Hin, Win, Cin, KH, KW, stride, pad)) return rc;      // Hin, Win: per sample
    g.Mper = g.M; g.M = M;
    UNI_REQUIRE(lda >= Cin && (!residual || ldr >= N) && (!outF || ldf >= N) && (!outB || ldb >= N), "gemm_stacked: lda=%d ldr=%d ldf=%d ldb=%d", lda, ldr, ldf, ldb);
    UNI_REQUIRE(out_hw >= 0 && out_stride >= 0 && out_off >= 0 && outF_rows >= 0, "gemm_stacked: out_hw=%d out_stride=%d out_off=%d outF_rows=%d", out_hw, out_stride, out_off, outF_rows);
    if (out_hw > 0) {     // the engine's remap rule: row -> (row / out_hw) * out_stride + out_off + row % out_hw
        UNI_REQUIRE(outF && M % out_hw == 0 && out_stride >= out_hw, "gemm_stacked: row remap needs out_f32, M=%d a multiple of out_hw=%d and out_stride=%d >= out_hw", M, out_hw, out_stride);
        UNI_REQUIRE((long)(M / out_hw - 1) * out_stride + out_off + out_hw <= (long)outF_rows, "gemm_stacked: the remapped rows end behind outF_rows=%d", outF_rows);
    } else if (outF) {
        UNI_REQUIRE(outF_rows >= M, "gemm_stacked: outF_rows=%d < M=%d", outF_rows, M);
    }
    if (gn_stats) UNI_REQUIRE(cpg > 0 && N % cpg == 0 && N / cpg <= 32 && act == ACT_NONE, "gemm_stacked: statistics need cpg=%d to divide N into at most 32 groups and no activation", cpg);
    UNI_REQUIRE(splitk >= 0 && splitk <= 64, "gemm_stacked: splitk=%d", splitk);
    g.bias = bias; g.act = act; g.act_col0 = act_col0; g.res = residual; g.ldr = ldr; g.outF = outF; g.ldf = ldf;
    g.out_hw = out_hw; g.out_stride = out_hw ? out_stride : 0; g.out_off = out_hw ? out_off : 0;
    g.outB = reinterpret_cast<bf16*>(outB); g.ldb = ldb; g.stats = gn_stats; g.cpg = cpg; g.force_cfg = force_cfg; g.b32 = fmt;
    g.wscale = fmt == FMT_H2 ? wscale : 1.f;
    if (splitk > 1) {     // launch_gemm_h2's conditions, before the slab is taken
        UNI_REQUIRE(fmt == FMT_H2 && outF && !outB && act == ACT_NONE && !out_hw, "gemm_stacked: split-K needs f16x2 operands, fp32 output only, no activation, no row remap");
        UNI_REQUIRE(N % 8 == 0 && ldf % 4 == 0 && ((uintptr_t)outF & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0) &&
                    (!residual || (ldr % 4 == 0 && ((uintptr_t)residual & 15) == 0)), "gemm_stacked: split-K needs the staged epilogue (N %% 8, ldf / ldr %% 4, 16-byte aligned pointers)");
        g.splitk = splitk;
        if (int rc = gemm_entry_slab(&g.slab, (size_t)splitk * M * N * sizeof(float))) return rc;
    }
    API(launch_gemm(g, S(stream)));
}
int uni_pack_weight_h2(const float* w, int N, int Cin, int KH, int KW, void* out, float* wscale_out) {
    UNI_REQUIRE(w && out && wscale_out && N > 0 && Cin > 0, "pack_weight_h2: bad argument");
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)N * Cin * KH * KW; ++i) mx = fmaxf(mx, fabsf(w[i]));
    const float scale = h2_weight_scale(mx);
    pack_weight_h2_host(w, N, Cin, KH, KW, nullptr, scale, reinterpret_cast<uint16_t*>(out), cdiv(N, 256) * 256, cdiv(Cin * KH * KW, 64) * 64);
    *wscale_out = 1.f / scale;
    return 0;
}
int uni_gemm_h2(const void* A, int lda, const void* w_packed, float wscale, int M, int N, int Hin, int Win, int Cin, int KH, int KW,
                int stride, int pad, const float* bias, int act, const float* residual, int ldr, float* outF, int ldf,
                void* outB, int ldb, double* gn_stats, int cpg, int force_cfg, uni_stream_t stream) {
    UNI_REQUIRE(A && w_packed && (outF || outB), "gemm_h2: NULL argument");
    GemmArgs g;
    if (int rc = gemm_geometry(g, "gemm_h2", A, lda, w_packed, M, N, Hin, Win, Cin, KH, KW, stride, pad)) return rc;
    g.bias = bias; g.act = act; g.res = residual; g.ldr = ldr; g.outF = outF; g.ldf = ldf;
    g.outB = reinterpret_cast<bf16*>(outB); g.ldb = ldb; g.stats = gn_stats; g.cpg = cpg; g.force_cfg = force_cfg;
    // tests / tools: force_cfg = tile cfg (< 1000) + 1000 * ablation bits (0..255: gemm_epi.h `dbg & 128`, gemm.hip `& 64`, ...) + 1000000 * K ranges
    g.b32 = FMT_H2; g.wscale = wscale; g.dbg = (force_cfg / 1000) % 1000;
    g.splitk = force_cfg / 1000000;
    g.force_cfg = force_cfg % 1000;
    g.Mper = g.M;
    if (g.splitk > 1)
        if (int rc = gemm_entry_slab(&g.slab, (size_t)g.splitk * g.M * g.N * sizeof(float))) return rc;
    API(launch_gemm(g, S(stream)));
}
size_t uni_mlp_blob_bytes(int C) { return mlp_fused_supported(C) ? mlp_blob_bytes(C) : 0; }
int uni_mlp_pack(const float* w1, const float* w2, const float* gamma, int C, int layout, void* blob_out, float* ws1_out, float* ws2_out) {
    UNI_REQUIRE(w1 && w2 && blob_out && ws1_out && ws2_out, "mlp_pack: NULL argument");
    UNI_REQUIRE(layout == 0 || layout == 1, "mlp_pack: layout %d (0 = 32-row waves, 1 = 16-row waves)", layout);
    UNI_REQUIRE(layout ? mlp_fused16_supported(C) : mlp_fused_supported(C), "mlp_pack: C=%d unsupported by layout %d (0: 96, 192, 256; 1: 192, 256)", C, layout);
    if (layout) mlp_pack16_host(w1, w2, gamma, C, reinterpret_cast<uint16_t*>(blob_out), ws1_out, ws2_out);
    else mlp_pack_host(w1, w2, gamma, C, reinterpret_cast<uint16_t*>(blob_out), ws1_out, ws2_out);
    return 0;
}
int uni_mlp_fused(const void* A, int lda, const void* blob, const float* b1, const float* b2, float ws1, float ws2, const float* residual,
                  int ldr, float* out, int ldo, void* outB, int ldb, int M, int C, int layout, uni_stream_t stream) {
    MlpArgs a;
    a.layout = layout;
    a.A = A; a.lda = lda; a.blob = blob; a.b1 = b1; a.b2 = b2; a.ws1 = ws1; a.ws2 = ws2; a.res = residual; a.ldr = ldr;
    a.out = out; a.ldo = ldo; a.outB = outB; a.ldb = ldb; a.M = M; a.C = C;
    API(launch_mlp_fused(a, S(stream)));
}
int uni_cast_h2(const float* x, int ldx, void* out, int ldo, int M, int C, uni_stream_t stream) {
    UNI_REQUIRE(x && out, "cast_h2: NULL argument");
    API(launch_cast_operand(x, ldx, reinterpret_cast<bf16*>(out), ldo, M, C, S(stream), FMT_H2));
}
int uni_cast_f32(const float* x, int ldx, float* out, int ldo, int M, int C, uni_stream_t stream) {
    UNI_REQUIRE(x && out, "cast_f32: NULL argument");
    API(launch_cast_operand(x, ldx, reinterpret_cast<bf16*>(out), ldo, M, C, S(stream), FMT_F32));
}
int uni_cast_bf16(const float* x, int ldx, uint16_t* out, int ldo, int M, int C, uni_stream_t stream) {
    UNI_REQUIRE(x && out, "cast: NULL argument");
    API(launch_cast_operand(x, ldx, reinterpret_cast<bf16*>(out), ldo, M, C, S(stream)));
}
int uni_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float eps, int M, int C, float* outF, uint16_t* outB,
                  uni_stream_t stream) {
    UNI_REQUIRE(x && gamma && beta && (outF || outB), "layernorm: NULL argument");
    LnArgs a;
    a.x = x; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.eps = eps; a.M = M; a.C = C;
    a.outF = outF; a.ldf = C; a.outB = reinterpret_cast<bf16*>(outB); a.ldb = C;
    API(launch_layernorm(a, S(stream)));
}
int uni_layernorm_ex(const float* x, int ldx, const float* gamma, const float* beta, float eps, int M, int C, float* outF, int ldf,
                     float* outF2, int pair_hw, void* outB, int ldb, int ps_h, int ps_w, int fmt, uni_stream_t stream) {
    UNI_REQUIRE(x && gamma && beta && (outF || outB), "layernorm_ex: NULL argument");
    UNI_REQUIRE(M > 0 && C > 0 && ldx >= C && fmt >= 0 && fmt <= 2, "layernorm_ex: M=%d C=%d ldx=%d fmt=%d", M, C, ldx, fmt);
    if (outF) UNI_REQUIRE(ldf >= C && ldf % 4 == 0 && ((uintptr_t)outF & 15) == 0, "layernorm_ex: ldf=%d / outF must be 16-byte aligned", ldf);
    UNI_REQUIRE(pair_hw >= 0 && (pair_hw > 0) == (outF2 != nullptr), "layernorm_ex: outF2 and pair_hw=%d go together", pair_hw);
    if (pair_hw) UNI_REQUIRE(outF && ((uintptr_t)outF2 & 15) == 0 && M % (2 * pair_hw) == 0, "layernorm_ex: pair mode needs outF, outF2 and M=%d a multiple of 2 * pair_hw=%d", M, pair_hw);
    UNI_REQUIRE(ps_h >= 0 && ps_w >= 0 && (ps_h > 0) == (ps_w > 0), "layernorm_ex: ps_h=%d ps_w=%d", ps_h, ps_w);
    if (ps_h) UNI_REQUIRE(outB && M % (ps_h * ps_w) == 0 && (fmt != FMT_H2 || C % 32 == 0), "layernorm_ex: PixelShuffle needs outB, M=%d a multiple of ps_h * ps_w, C / 4 a multiple of 8 in f16x2", M);
    if (outB && !ps_h) UNI_REQUIRE(ldb >= C && ldb % (fmt == FMT_H2 ? 8 : 4) == 0, "layernorm_ex: ldb=%d", ldb);
    if (outB) UNI_REQUIRE(((uintptr_t)outB & 15) == 0, "layernorm_ex: outB must be 16-byte aligned");
    LnArgs a;
    a.x = x; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.eps = eps; a.M = M; a.C = C;
    a.outF = outF; a.ldf = ldf; a.outF2 = outF2; a.pair_hw = pair_hw;
    a.outB = reinterpret_cast<bf16*>(outB); a.ldb = ldb; a.ps_h = ps_h; a.ps_w = ps_w; a.b32 = fmt;
    API(launch_layernorm(a, S(stream)));
}
int uni_groupnorm_act_ex(const float* x, int ldx, const double* stats, const float* gamma, const float* beta, float eps, int B, int M, int C,
                         int G, int act, const float* prior, const float* prior_beta, float* outF, int ldf, void* outB, int ldb, void* outUp,
                         int ldu, int W, int fmt, uni_stream_t stream) {
    UNI_REQUIRE(x && stats && gamma && beta && (outF || outB || outUp), "groupnorm_act_ex: NULL argument");
    UNI_REQUIRE(B > 0 && B < 65536 && M > 0 && C > 0 && C <= 8192 && G > 0 && G <= 32 && fmt >= 0 && fmt <= 2, "groupnorm_act_ex: B=%d M=%d C=%d G=%d fmt=%d", B, M, C, G, fmt);
    UNI_REQUIRE(ldx >= C && ((uintptr_t)x & 15) == 0, "groupnorm_act_ex: ldx=%d / x must be 16-byte aligned", ldx);
    UNI_REQUIRE((prior != nullptr) == (prior_beta != nullptr), "groupnorm_act_ex: prior and prior_beta go together");
    if (outF) UNI_REQUIRE(ldf >= C && ldf % 4 == 0 && ((uintptr_t)outF & 15) == 0, "groupnorm_act_ex: ldf=%d / outF must be 16-byte aligned", ldf);
    if (outB) UNI_REQUIRE(ldb >= C, "groupnorm_act_ex: ldb=%d", ldb);
    if (outUp) UNI_REQUIRE(ldu >= C && W > 0 && M % W == 0, "groupnorm_act_ex: outUp needs ldu=%d >= C and M=%d a multiple of W=%d", ldu, M, W);
    GnApplyArgs a;
    a.x = x; a.ldx = ldx; a.stats = stats; a.gamma = gamma; a.beta = beta; a.eps = eps; a.M = M; a.C = C; a.G = G; a.act = act; a.B = B;
    a.prior = prior; a.prior_beta = prior_beta; a.outF = outF; a.ldf = ldf; a.outB = reinterpret_cast<bf16*>(outB); a.ldb = ldb;
    a.outUp = reinterpret_cast<bf16*>(outUp); a.ldu = ldu; a.W = W; a.b32 = fmt;
    API(launch_gn_apply(a, S(stream)));
}
int uni_dwconv7_ln(const float* x, const float* w49c, const float* bias, const float* gamma, const float* beta, float eps, int H, int W,
                   int C, uint16_t* out, uni_stream_t stream) {
    UNI_REQUIRE(x && w49c && bias && gamma && beta && out, "dwconv7_ln: NULL argument");
    DwLnArgs d;
    d.x = x; d.w = w49c; d.bias = bias; d.gamma = gamma; d.beta = beta; d.eps = eps; d.H = H; d.W = W; d.C = C;
    d.out = reinterpret_cast<bf16*>(out);
    API(launch_dwconv7_ln(d, S(stream)));
}
int uni_dwconv7_ln_ex(const float* x, const float* w49c, const float* bias, const float* gamma, const float* beta, float eps, int B, int H,
                      int W, int C, void* out, int fmt, uni_stream_t stream) {
    UNI_REQUIRE(x && w49c && bias && gamma && beta && out, "dwconv7_ln_ex: NULL argument");
    UNI_REQUIRE(B > 0 && H > 0 && W > 0 && fmt >= 0 && fmt <= 2, "dwconv7_ln_ex: B=%d H=%d W=%d fmt=%d", B, H, W, fmt);
    DwLnArgs d;
    d.x = x; d.w = w49c; d.bias = bias; d.gamma = gamma; d.beta = beta; d.eps = eps; d.H = H; d.W = W; d.C = C; d.B = B;
    d.out = reinterpret_cast<bf16*>(out); d.b32 = fmt;
    API(launch_dwconv7_ln(d, S(stream)));
}
int uni_msda_tokens(const float* value, const float* offaw, int ldo, int B, int h, int w, float* out, uni_stream_t stream) {
    UNI_REQUIRE(value && offaw && out && B > 0 && h > 0 && w > 0 && ldo >= 192, "msda_tokens: bad argument");
    MsdaFusedArgs m;
    m.value = value; m.offaw = offaw; m.ldo = ldo; m.h = h; m.w = w; m.B = B;
    m.out = reinterpret_cast<bf16*>(out); m.b32 = FMT_F32;
    API(launch_msda_fused(m, S(stream)));
}
// ---- context-free entries of the glue launchers the engine runs between context buffers (arguments as the launchers of kernels.h; fmt =
// operand format of `out`).  The divisibility and alignment the kernels rely on are checked here: the launchers themselves trust the engine.
int uni_cast_operand_pair_ex(const float* x0, const float* x1, void* out, int B, int hw, int C, int fmt, uni_stream_t stream) {
    UNI_REQUIRE(x0 && x1 && out && B > 0 && hw > 0 && C > 0 && C % 8 == 0 && fmt >= 0 && fmt <= 2, "cast_operand_pair_ex: B=%d hw=%d C=%d fmt=%d", B, hw, C, fmt);
    UNI_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)out) & 15) == 0, "cast_operand_pair_ex: pointers must be 16-byte aligned");
    API(launch_cast_operand_pair(x0, x1, reinterpret_cast<bf16*>(out), hw, C, B, S(stream), fmt));
}
int uni_pixel_shuffle_ex(const float* x, void* out, int B, int h, int w, int C, int fmt, uni_stream_t stream) {
    UNI_REQUIRE(x && out && B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && fmt >= 0 && fmt <= 2, "pixel_shuffle_ex: B=%d h=%d w=%d C=%d fmt=%d", B, h, w, C, fmt);
    UNI_REQUIRE(fmt != FMT_H2 || C % 32 == 0, "pixel_shuffle_ex: f16x2 rows need C / 4 = %d a multiple of 8", C / 4);
    API(launch_pixel_shuffle_bf16(x, reinterpret_cast<bf16*>(out), h, w, C, S(stream), fmt, B));
}
int uni_add_pos_ex(const float* src, const float* pos0, const float* pos1, const float* lvl, void* out, int B, int hw, int C, int fmt,
                   uni_stream_t stream) {
    UNI_REQUIRE(src && pos0 && pos1 && lvl && out && B > 0 && hw > 0 && C > 0 && C % 8 == 0 && fmt >= 0 && fmt <= 2, "add_pos_ex: B=%d hw=%d C=%d fmt=%d", B, hw, C, fmt);
    UNI_REQUIRE((((uintptr_t)src | (uintptr_t)pos0 | (uintptr_t)pos1 | (uintptr_t)lvl | (uintptr_t)out) & 15) == 0, "add_pos_ex: pointers must be 16-byte aligned");
    API(launch_add_pos_bf16(src, pos0, pos1, lvl, reinterpret_cast<bf16*>(out), hw, C, S(stream), fmt, B));
}
int uni_add_aligned_bilinear_ex(const float* src, int B, int h, int w, int C, int factor, float* dst, uni_stream_t stream) {
    UNI_REQUIRE(src && dst && B > 0 && B < 65536 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && factor >= 1, "add_aligned_bilinear_ex: B=%d h=%d w=%d C=%d factor=%d", B, h, w, C, factor);
    UNI_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "add_aligned_bilinear_ex: pointers must be 16-byte aligned");
    API(launch_add_aligned_bilinear(src, h, w, C, factor, dst, S(stream), B));
}
int uni_pos_embed_ex(const float* row_embed, const float* col_embed, int sz, int nf, int h, int w, float* out_nhwc, uni_stream_t stream) {
    UNI_REQUIRE(row_embed && col_embed && out_nhwc && sz > 0 && nf > 0 && h > 0 && w > 0 && (long)h * w * 2 * nf < (1L << 31), "pos_embed_ex: sz=%d nf=%d h=%d w=%d", sz, nf, h, w);
    API(launch_pos_embed(row_embed, col_embed, sz, nf, out_nhwc, h, w, S(stream)));
}
int uni_msda_tokens_ex(const float* value, const float* offaw, int ldo, int B, int h, int w, void* out, int fmt, uni_stream_t stream) {
    UNI_REQUIRE(value && offaw && out && B > 0 && h > 0 && w > 0 && ldo >= 192 && fmt >= 0 && fmt <= 2, "msda_tokens_ex: bad argument (fmt=%d)", fmt);
    UNI_REQUIRE((((uintptr_t)value | (uintptr_t)out) & 15) == 0, "msda_tokens_ex: value / out must be 16-byte aligned");
    MsdaFusedArgs m;
    m.value = value; m.offaw = offaw; m.ldo = ldo; m.h = h; m.w = w; m.B = B;
    m.out = reinterpret_cast<bf16*>(out); m.b32 = fmt;
    API(launch_msda_fused(m, S(stream)));
}
int uni_groupnorm_act(const float* x, const double* stats, const float* gamma, const float* beta, float eps, int M, int C, int G,
                      int act, float* outF, uint16_t* outB, uni_stream_t stream) {
    UNI_REQUIRE(x && stats && gamma && beta && (outF || outB), "groupnorm: NULL argument");
    GnApplyArgs a;
    a.x = x; a.ldx = C; a.stats = stats; a.gamma = gamma; a.beta = beta; a.eps = eps; a.M = M; a.C = C; a.G = G; a.act = act;
    a.outF = outF; a.ldf = C; a.outB = reinterpret_cast<bf16*>(outB); a.ldb = C;
    API(launch_gn_apply(a, S(stream)));
}
int uni_stem(const float* img, int H, int W, const float* w48c, const float* bias, const float* gamma, const float* beta, int C,
             float* out, uni_stream_t stream) {
    UNI_REQUIRE(img && w48c && bias && gamma && beta && out, "stem: NULL argument");
    StemArgs a;
    a.img = img; a.H = H; a.W = W; a.w = w48c; a.bias = bias; a.gamma = gamma; a.beta = beta; a.C = C; a.out = out;
    API(launch_stem(a, S(stream)));
}
int uni_stem_ex(const float* img, int B, int H, int W, const float* w48c, const float* bias, const float* gamma, const float* beta, int C,
                float* out, uni_stream_t stream) {
    UNI_REQUIRE(img && w48c && bias && gamma && beta && out && B > 0, "stem_ex: bad argument");
    StemArgs a;
    a.img = img; a.H = H; a.W = W; a.B = B; a.w = w48c; a.bias = bias; a.gamma = gamma; a.beta = beta; a.C = C; a.out = out;
    API(launch_stem(a, S(stream)));
}

}  // extern "C"
