// The C ABI entries of the masked attention family without score modifiers (include/kfunca_hip.h: kf_attn_full_*, kf_attn_prefix_*,
// kf_attn_window_*, kf_attn_doc_*). The kernels and the host path they share with kf_attn_ext_* (attn_ext.hip) are in attn_full_kernels.h.
#include "attn_full_kernels.h"

int kf::full::plain_fwd(const char *who, const Problem &pr, const MaskPlan &p, const FwdOps &x, void *stream) {
    return full_fwd<X_NONE>(who, pr, p, Mods{0.f, nullptr}, x, stream);
}
int kf::full::plain_bwd(const char *who, const char *size_query, const Problem &pr, const MaskPlan &p, const BwdOps &x, void *stream) {
    return full_bwd<false>(who, size_query, pr, p, Mods{0.f, nullptr}, x, stream);
}

// Every entry below: the mask its arguments describe (the fields of the other kinds neutral), the one check of it, the plain path.
static int family_fwd(const char *who, const Problem &pr, const kf_attn_mask &m, const FwdOps &x, void *stream) {
    MaskPlan p;
    int rc = mask_check(who, &m, pr.Sq, pr.Skv, p);
    return rc != KF_OK ? rc : plain_fwd(who, pr, p, x, stream);
}
static int family_bwd(const char *who, const Problem &pr, const kf_attn_mask &m, const BwdOps &x, void *stream) {
    MaskPlan p;
    int rc = mask_check(who, &m, pr.Sq, pr.Skv, p);
    return rc != KF_OK ? rc : plain_bwd(who, "kf_attn_full_bwd_workspace_bytes", pr, p, x, stream);
}

extern "C" int kf_attn_full_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                                void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    return family_fwd("kf_attn_full_fwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_FULL, .kv_len = kv_len, .window_left = -1, .window_right = -1},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse}, stream);
}

extern "C" int kf_attn_full_bwd_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, size_t *bytes) {
    return ws_query("kf_attn_full_bwd_workspace_bytes", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = 1.f}, bytes);
}

extern "C" int kf_attn_full_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                                const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq,
                                const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return family_bwd("kf_attn_full_bwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_FULL, .kv_len = kv_len, .window_left = -1, .window_right = -1},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse, .d_o = d_o, .ldo = ldo, .dq = dq, .ldq = ldq,
                       .dk = dk, .ldk = ldk, .dv = dv, .ldv = ldv, .workspace = workspace, .workspace_bytes = workspace_bytes}, stream);
}

extern "C" int kf_attn_prefix_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  const int64_t *prefix_len, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v,
                                  const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    return family_fwd("kf_attn_prefix_fwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_PREFIX, .kv_len = kv_len, .prefix_len = prefix_len, .window_left = -1, .window_right = -1},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse}, stream);
}

extern "C" int kf_attn_prefix_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  const int64_t *prefix_len, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v,
                                  const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                                  const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                                  const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream) {
    return family_bwd("kf_attn_prefix_bwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_PREFIX, .kv_len = kv_len, .prefix_len = prefix_len, .window_left = -1, .window_right = -1},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse, .d_o = d_o, .ldo = ldo, .dq = dq, .ldq = ldq,
                       .dk = dk, .ldk = ldk, .dv = dv, .ldv = ldv, .workspace = workspace, .workspace_bytes = workspace_bytes}, stream);
}

extern "C" int kf_attn_window_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  int64_t window_left, int64_t window_right, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                                  const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    return family_fwd("kf_attn_window_fwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_WINDOW, .kv_len = kv_len, .window_left = window_left, .window_right = window_right},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse}, stream);
}

extern "C" int kf_attn_window_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  int64_t window_left, int64_t window_right, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                                  const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                                  const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                                  const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream) {
    return family_bwd("kf_attn_window_bwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_WINDOW, .kv_len = kv_len, .window_left = window_left, .window_right = window_right},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse, .d_o = d_o, .ldo = ldo, .dq = dq, .ldq = ldq,
                       .dk = dk, .ldk = ldk, .dv = dv, .ldv = ldv, .workspace = workspace, .workspace_bytes = workspace_bytes}, stream);
}

// ---- the document variant: several sequences packed end to end in one row (kf_attn_doc_*) ----
extern "C" int kf_attn_doc_table(int64_t B, int64_t S, int64_t n_docs, const int64_t *cu_doclens, int64_t *kv_len, int32_t *doc_start, int32_t *doc_end,
                                 void *stream) {
    KF_REQUIRE(B >= 0 && S >= 0, KF_ERR_INVALID, "kf_attn_doc_table: negative extent");
    KF_REQUIRE(n_docs >= 1, KF_ERR_INVALID, "kf_attn_doc_table: n_docs %lld must be at least 1", (long long)n_docs);
    KF_REQUIRE(cu_doclens && kv_len && doc_start && doc_end, KF_ERR_INVALID, "kf_attn_doc_table: null pointer");
    if (B == 0 || S == 0) return KF_OK;
    KF_REQUIRE(S < (1ll << 31) && (B * S + NT - 1) / NT < (1ll << 31) && B <= (1ll << 31), KF_ERR_UNSUPPORTED,
               "kf_attn_doc_table: the tables are 32-bit and the grid holds 2^31 workgroups: S must be below 2^31 and B S below 2^39");
    hipStream_t st = as_stream(stream);
    KF_PROF("attn_doc_table", st);
    return launch(attn_doc_table_kernel, (unsigned)((B * S + NT - 1) / NT), NT, 0, st, cu_doclens, B, S, n_docs, kv_len, doc_start, doc_end);
}

extern "C" int kf_attn_doc_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, int causal, const int64_t *kv_len,
                               const int32_t *doc_start, const int32_t *doc_end, const void *q, const kf_attn_layout *lq, const void *k,
                               const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    return family_fwd("kf_attn_doc_fwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = S, .Skv = S, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_DOC, .kv_len = kv_len, .window_left = -1, .window_right = -1, .doc_start = doc_start, .doc_end = doc_end, .causal = causal},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse}, stream);
}

extern "C" int kf_attn_doc_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, int causal, const int64_t *kv_len,
                               const int32_t *doc_start, const int32_t *doc_end, const void *q, const kf_attn_layout *lq, const void *k,
                               const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse,
                               const void *d_o, const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                               const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream) {
    return family_bwd("kf_attn_doc_bwd", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = S, .Skv = S, .D = D, .scale = scale},
                      {.kind = KF_ATTN_MASK_DOC, .kv_len = kv_len, .window_left = -1, .window_right = -1, .doc_start = doc_start, .doc_end = doc_end, .causal = causal},
                      {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse, .d_o = d_o, .ldo = ldo, .dq = dq, .ldq = ldq,
                       .dk = dk, .ldk = ldk, .dv = dv, .ldv = ldv, .workspace = workspace, .workspace_bytes = workspace_bytes}, stream);
}
