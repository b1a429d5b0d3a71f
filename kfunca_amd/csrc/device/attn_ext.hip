// The masked attention family with modifiers of the scores (include/kfunca_hip.h: kf_attn_ext_*): logit
// soft-capping, s = cap tanh(scale <q, k> / cap), and attention sinks, one learned logit per query head that joins the softmax
// denominator and owns no value row. One descriptor-based trio serves the four masks. The kernels are those of attn_full_kernels.h
// compiled with the modifier; this translation unit holds every modified instantiation and none of the others:
//   softcap = 0 and no sink   the unmodified host path of attn_full.hip is called (plain_fwd, plain_bwd: the families' kernels, labels
//                             and bits) with this entry's name, so every check runs once and a refusal carries that name
//   a sink, softcap = 0       forward: the kernels without the cap compiled with the sink epilogue (X_SINK), under the labels of the
//                             family; backward: the unmodified host path of attn_full.hip - P is formed from lse, which holds the
//                             sink - followed by attn_sink_grad
//   softcap > 0               the _cap_ instantiations (the sink, if any, read in the forward epilogue), then attn_sink_grad
//
// kf_attn_span_*  are here too: the document mask with a causal rule, per-document prefixes and a window baked
// into its tables by kf_attn_span_table. They add no attention kernel: the M_DOC instantiations above and those of attn_full.hip run with
// causal = 0 on (key_lo, key_hi), the two dK/dV launches on (query_lo, query_hi).
#include "attn_full_kernels.h"

static int modifier_check(const char *who, float softcap) {
    KF_REQUIRE(softcap >= 0.f && softcap < INFINITY, KF_ERR_INVALID, "%s: softcap must be 0 (off) or positive and finite", who);
    return KF_OK;
}

extern "C" int kf_attn_ext_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const kf_attn_mask *mask,
                               float softcap, const float *sink, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                               const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    const char *who = "kf_attn_ext_fwd";
    const Problem pr = {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale};
    const FwdOps x = {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse};
    const Mods mod = {.softcap = softcap, .sink = sink};
    MaskPlan p;
    int rc = mask_check(who, mask, Sq, Skv, p);
    if (rc != KF_OK) return rc;
    rc = modifier_check(who, softcap);
    if (rc != KF_OK) return rc;
    if (softcap > 0.f) return full_fwd<X_CAP>(who, pr, p, mod, x, stream);
    if (sink) return full_fwd<X_SINK>(who, pr, p, Mods{.softcap = 0.f, .sink = sink}, x, stream);
    return plain_fwd(who, pr, p, x, stream);
}

extern "C" int kf_attn_ext_bwd_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, size_t *bytes) {
    return ws_query("kf_attn_ext_bwd_workspace_bytes", {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = 1.f}, bytes);
}

extern "C" int kf_attn_ext_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const kf_attn_mask *mask,
                               float softcap, const float *sink, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                               const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                               const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                               const kf_attn_layout *ldv, float *dsink, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_attn_ext_bwd", *size_query = "kf_attn_ext_bwd_workspace_bytes";
    const Problem pr = {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = Sq, .Skv = Skv, .D = D, .scale = scale};
    const BwdOps x = {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse, .d_o = d_o, .ldo = ldo, .dq = dq, .ldq = ldq,
                      .dk = dk, .ldk = ldk, .dv = dv, .ldv = ldv, .workspace = workspace, .workspace_bytes = workspace_bytes};
    MaskPlan p;
    int rc = mask_check(who, mask, Sq, Skv, p);
    if (rc != KF_OK) return rc;
    rc = modifier_check(who, softcap);
    if (rc != KF_OK) return rc;
    KF_REQUIRE((sink != nullptr) == (dsink != nullptr), KF_ERR_INVALID, "%s: dsink is required exactly when sink is given", who);
    rc = softcap > 0.f ? full_bwd<true>(who, size_query, pr, p, Mods{.softcap = softcap, .sink = sink}, x, stream) : plain_bwd(who, size_query, pr, p, x, stream);
    if (rc != KF_OK || !sink || B == 0 || Hq == 0 || Sq == 0) return rc; // (an empty problem launched nothing and has no dsink to write)
    // the workspace holds delta [B, Hq, Sq] (the pre-pass of the launches above); one workgroup per head (Hq <= 2^24: full_check)
    hipStream_t st = as_stream(stream);
    KF_PROF("attn_sink_grad", st);
    return launch(attn_sink_grad_kernel, (unsigned)Hq, NT, 0, st, sink, lse, (const float *)workspace, dsink, B, Hq, Sq);
}

// ---- the span variant: documents with a causal rule, per-document prefixes and a window (kf_attn_span_*) ----
extern "C" int kf_attn_span_table(int64_t B, int64_t S, int64_t n_docs, const int64_t *cu_doclens, const int64_t *doc_prefix, int causal, int64_t window_left,
                                  int64_t window_right, int64_t *kv_len, int32_t *key_lo, int32_t *key_hi, int32_t *query_lo, int32_t *query_hi, void *stream) {
    KF_REQUIRE(B >= 0 && S >= 0, KF_ERR_INVALID, "kf_attn_span_table: negative extent");
    KF_REQUIRE(n_docs >= 1, KF_ERR_INVALID, "kf_attn_span_table: n_docs %lld must be at least 1", (long long)n_docs);
    KF_REQUIRE(cu_doclens && kv_len && key_lo && key_hi && query_lo && query_hi, KF_ERR_INVALID, "kf_attn_span_table: null pointer");
    KF_REQUIRE(causal == 0 || causal == 1, KF_ERR_INVALID, "kf_attn_span_table: causal is 0 or 1, not %d", causal);
    KF_REQUIRE(window_left >= -1 && window_right >= -1, KF_ERR_INVALID,
               "kf_attn_span_table: a window side is a key count >= 0 or -1 (unbounded), not (%lld, %lld)", (long long)window_left, (long long)window_right);
    KF_REQUIRE(!doc_prefix || causal == 1, KF_ERR_INVALID, "kf_attn_span_table: doc_prefix belongs to causal = 1 (without the causal rule a prefix changes nothing)");
    if (B == 0 || S == 0) return KF_OK;
    KF_REQUIRE(S < (1ll << 31) && (B * S + NT - 1) / NT < (1ll << 31) && B <= (1ll << 31), KF_ERR_UNSUPPORTED,
               "kf_attn_span_table: the tables are 32-bit and the grid holds 2^31 workgroups: S must be below 2^31 and B S below 2^39");
    hipStream_t st = as_stream(stream);
    KF_PROF("attn_span_table", st);
    // a side of S or more reaches past every document: clamped, so that the kernel's m - wl and m + wr + 1 cannot overflow
    return launch(attn_span_table_kernel, (unsigned)((B * S + NT - 1) / NT), NT, 0, st, cu_doclens, doc_prefix, B, S, n_docs, causal,
                  window_left > S ? S : window_left, window_right > S ? S : window_right, kv_len, key_lo, key_hi, query_lo, query_hi);
}

// The mask of the two entries below: M_DOC without its causal rule (the tables hold it), keyed (full_bwd hands the dK/dV launches the second pair)
static MaskPlan span_plan(const int64_t *kv_len, const int32_t *key_lo, const int32_t *key_hi, const int32_t *query_lo, const int32_t *query_hi) {
    return MaskPlan{M_DOC, kv_len, nullptr, Window{-1, -1}, DocTables{key_lo, key_hi, 0, query_lo, query_hi, true}};
}

extern "C" int kf_attn_span_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, const int64_t *kv_len, const int32_t *key_lo,
                                const int32_t *key_hi, float softcap, const float *sink, const void *q, const kf_attn_layout *lq, const void *k,
                                const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    const char *who = "kf_attn_span_fwd";
    const Problem pr = {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = S, .Skv = S, .D = D, .scale = scale};
    const FwdOps x = {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse};
    const MaskPlan p = span_plan(kv_len, key_lo, key_hi, nullptr, nullptr);
    int rc = modifier_check(who, softcap);
    if (rc != KF_OK) return rc;
    if (softcap > 0.f) return full_fwd<X_CAP>(who, pr, p, Mods{.softcap = softcap, .sink = sink}, x, stream);
    if (sink) return full_fwd<X_SINK>(who, pr, p, Mods{.softcap = 0.f, .sink = sink}, x, stream);
    return plain_fwd(who, pr, p, x, stream);
}

extern "C" int kf_attn_span_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, float scale, const int64_t *kv_len, const int32_t *key_lo,
                                const int32_t *key_hi, const int32_t *query_lo, const int32_t *query_hi, float softcap, const float *sink, const void *q,
                                const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk, const void *v, const kf_attn_layout *lv, const void *o,
                                const kf_attn_layout *lo, const float *lse, const void *d_o, const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq,
                                void *dk, const kf_attn_layout *ldk, void *dv, const kf_attn_layout *ldv, float *dsink, void *workspace, size_t workspace_bytes,
                                void *stream) {
    const char *who = "kf_attn_span_bwd", *size_query = "kf_attn_full_bwd_workspace_bytes";
    const Problem pr = {.dtype = dtype, .B = B, .Hq = Hq, .Hkv = Hkv, .Sq = S, .Skv = S, .D = D, .scale = scale};
    const BwdOps x = {.q = q, .lq = lq, .k = k, .lk = lk, .v = v, .lv = lv, .o = o, .lo = lo, .lse = lse, .d_o = d_o, .ldo = ldo, .dq = dq, .ldq = ldq,
                      .dk = dk, .ldk = ldk, .dv = dv, .ldv = ldv, .workspace = workspace, .workspace_bytes = workspace_bytes};
    const MaskPlan p = span_plan(kv_len, key_lo, key_hi, query_lo, query_hi);
    int rc = modifier_check(who, softcap);
    if (rc != KF_OK) return rc;
    KF_REQUIRE((sink != nullptr) == (dsink != nullptr), KF_ERR_INVALID, "%s: dsink is required exactly when sink is given", who);
    rc = softcap > 0.f ? full_bwd<true>(who, size_query, pr, p, Mods{.softcap = softcap, .sink = sink}, x, stream) : plain_bwd(who, size_query, pr, p, x, stream);
    if (rc != KF_OK || !sink || B == 0 || Hq == 0 || S == 0) return rc; // (as kf_attn_ext_bwd: an empty problem has no dsink to write)
    hipStream_t st = as_stream(stream);
    KF_PROF("attn_sink_grad", st);
    return launch(attn_sink_grad_kernel, (unsigned)Hq, NT, 0, st, sink, lse, (const float *)workspace, dsink, B, Hq, S);
}
