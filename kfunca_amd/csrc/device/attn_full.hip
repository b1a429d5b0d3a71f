// The C ABI entries of the masked attention family without score modifiers (include/kfunca_hip.h: kf_attn_full_*, kf_attn_prefix_*,
// kf_attn_window_*, kf_attn_doc_*). The kernels and the host path they share with kf_attn_ext_* (attn_ext.hip) are in attn_full_kernels.h.
#include "attn_full_kernels.h"

extern "C" int kf_attn_full_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                                void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    return full_fwd("kf_attn_full_fwd", M_FULL, Window{-1, -1}, dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, nullptr, q, lq, k, lk, v, lv, o, lo, lse, stream);
}

extern "C" int kf_attn_full_bwd_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_attn_full_bwd_workspace_bytes: null out pointer");
    FullArgs a;
    Plan plan;
    int rc = full_check("kf_attn_full_bwd_workspace_bytes", dtype, B, Hq, Hkv, Sq, Skv, D, 1.f, nullptr, nullptr, 0, a, plan);
    if (rc != KF_OK) return rc;
    *bytes = ws_bytes(B, Hq, Sq);
    return KF_OK;
}

extern "C" int kf_attn_full_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv,
                                const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq,
                                const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return full_bwd("kf_attn_full_bwd", M_FULL, Window{-1, -1}, dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, nullptr, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq, dk,
                    ldk, dv, ldv, workspace, workspace_bytes, stream);
}

extern "C" int kf_attn_prefix_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  const int64_t *prefix_len, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v,
                                  const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    return full_fwd("kf_attn_prefix_fwd", M_PREFIX, Window{-1, -1}, dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, prefix_len, q, lq, k, lk, v, lv, o, lo, lse, stream);
}

extern "C" int kf_attn_prefix_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  const int64_t *prefix_len, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v,
                                  const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                                  const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                                  const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream) {
    return full_bwd("kf_attn_prefix_bwd", M_PREFIX, Window{-1, -1}, dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, prefix_len, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq,
                    dk, ldk, dv, ldv, workspace, workspace_bytes, stream);
}

extern "C" int kf_attn_window_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  int64_t window_left, int64_t window_right, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                                  const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    KF_REQUIRE(window_left >= -1 && window_right >= -1, KF_ERR_INVALID, "kf_attn_window_fwd: a window side is a key count >= 0 or -1 (unbounded), not (%lld, %lld)",
               (long long)window_left, (long long)window_right);
    return full_fwd("kf_attn_window_fwd", window_mode(window_left, window_right), Window{window_left, window_right}, dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len,
                    nullptr, q, lq, k, lk, v, lv, o, lo, lse, stream);
}

extern "C" int kf_attn_window_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const int64_t *kv_len,
                                  int64_t window_left, int64_t window_right, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                                  const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                                  const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                                  const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream) {
    KF_REQUIRE(window_left >= -1 && window_right >= -1, KF_ERR_INVALID, "kf_attn_window_bwd: a window side is a key count >= 0 or -1 (unbounded), not (%lld, %lld)",
               (long long)window_left, (long long)window_right);
    return full_bwd("kf_attn_window_bwd", window_mode(window_left, window_right), Window{window_left, window_right}, dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len,
                    nullptr, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq, dk, ldk, dv, ldv, workspace, workspace_bytes, stream);
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
    KF_REQUIRE(causal == 0 || causal == 1, KF_ERR_INVALID, "kf_attn_doc_fwd: causal is 0 or 1, not %d", causal);
    return full_fwd("kf_attn_doc_fwd", M_DOC, Window{-1, -1}, dtype, B, Hq, Hkv, S, S, D, scale, kv_len, nullptr, q, lq, k, lk, v, lv, o, lo, lse, stream,
                    DocTables{doc_start, doc_end, causal});
}

extern "C" int kf_attn_doc_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, int causal, const int64_t *kv_len,
                               const int32_t *doc_start, const int32_t *doc_end, const void *q, const kf_attn_layout *lq, const void *k,
                               const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse,
                               const void *d_o, const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                               const kf_attn_layout *ldv, void *workspace, size_t workspace_bytes, void *stream) {
    KF_REQUIRE(causal == 0 || causal == 1, KF_ERR_INVALID, "kf_attn_doc_bwd: causal is 0 or 1, not %d", causal);
    return full_bwd("kf_attn_doc_bwd", M_DOC, Window{-1, -1}, dtype, B, Hq, Hkv, S, S, D, scale, kv_len, nullptr, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq,
                    dk, ldk, dv, ldv, workspace, workspace_bytes, stream, DocTables{doc_start, doc_end, causal});
}
