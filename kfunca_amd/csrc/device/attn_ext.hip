// The masked attention family with modifiers of the scores (include/kfunca_hip.h: kf_attn_ext_*): logit
// soft-capping, s = cap tanh(scale <q, k> / cap), and attention sinks, one learned logit per query head that joins the softmax
// denominator and owns no value row. One descriptor-based trio serves the four masks. The kernels are those of attn_full_kernels.h
// compiled with the modifier; this translation unit holds every modified instantiation and none of the others:
//   softcap = 0 and no sink   the entries of attn_full.hip are called (their kernels, labels and bits); the checks run here first, so a
//                             refusal carries this entry's name
//   a sink, softcap = 0       forward: the kernels without the cap compiled with the sink epilogue (X_SINK), under the labels of the
//                             family; backward: the entries of attn_full.hip - P is formed from lse, which holds the sink - followed
//                             by attn_sink_grad
//   softcap > 0               the _cap_ instantiations (the sink, if any, read in the forward epilogue), then attn_sink_grad
#include "attn_full_kernels.h"

namespace {

struct MaskPlan {
    Mode mode;
    Window win;
    DocTables doc;
};

// kind and the fields that belong to it; a field of another kind must hold its neutral value (NULL, -1, 0), as the per-family entries
// have no such argument at all
int mask_check(const char *who, const kf_attn_mask *m, int64_t Sq, int64_t Skv, MaskPlan &p) {
    KF_REQUIRE(m, KF_ERR_INVALID, "%s: null mask", who);
    KF_REQUIRE(m->kind >= KF_ATTN_MASK_FULL && m->kind <= KF_ATTN_MASK_DOC, KF_ERR_INVALID, "%s: unknown mask kind %d", who, m->kind);
    KF_REQUIRE(m->kind == KF_ATTN_MASK_PREFIX || !m->prefix_len, KF_ERR_INVALID, "%s: prefix_len belongs to KF_ATTN_MASK_PREFIX, the kind is %d", who, m->kind);
    KF_REQUIRE(m->kind == KF_ATTN_MASK_WINDOW || (m->window_left == -1 && m->window_right == -1), KF_ERR_INVALID,
               "%s: a window (%lld, %lld) belongs to KF_ATTN_MASK_WINDOW, the kind is %d (other kinds: -1, -1)", who, (long long)m->window_left,
               (long long)m->window_right, m->kind);
    KF_REQUIRE(m->kind == KF_ATTN_MASK_DOC || (!m->doc_start && !m->doc_end && m->causal == 0), KF_ERR_INVALID,
               "%s: doc_start, doc_end and causal belong to KF_ATTN_MASK_DOC, the kind is %d", who, m->kind);
    p = MaskPlan{(Mode)m->kind, Window{-1, -1}, DocTables{nullptr, nullptr, 0}};
    if (m->kind == KF_ATTN_MASK_WINDOW) {
        KF_REQUIRE(m->window_left >= -1 && m->window_right >= -1, KF_ERR_INVALID, "%s: a window side is a key count >= 0 or -1 (unbounded), not (%lld, %lld)", who,
                   (long long)m->window_left, (long long)m->window_right);
        p.win = Window{m->window_left, m->window_right};
        p.mode = window_mode(m->window_left, m->window_right);
    } else if (m->kind == KF_ATTN_MASK_DOC) {
        KF_REQUIRE(m->causal == 0 || m->causal == 1, KF_ERR_INVALID, "%s: causal is 0 or 1, not %d", who, m->causal);
        KF_REQUIRE(Sq == Skv, KF_ERR_INVALID, "%s: a document mask is self-attention, Sq %lld must equal Skv %lld", who, (long long)Sq, (long long)Skv);
        p.doc = DocTables{m->doc_start, m->doc_end, m->causal};
    }
    return KF_OK;
}

int modifier_check(const char *who, float softcap) {
    KF_REQUIRE(softcap >= 0.f && softcap < INFINITY, KF_ERR_INVALID, "%s: softcap must be 0 (off) or positive and finite", who);
    return KF_OK;
}

} // namespace

extern "C" int kf_attn_ext_fwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const kf_attn_mask *mask,
                               float softcap, const float *sink, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                               const void *v, const kf_attn_layout *lv, void *o, const kf_attn_layout *lo, float *lse, void *stream) {
    const char *who = "kf_attn_ext_fwd";
    MaskPlan p;
    int rc = mask_check(who, mask, Sq, Skv, p);
    if (rc != KF_OK) return rc;
    rc = modifier_check(who, softcap);
    if (rc != KF_OK) return rc;
    if (softcap > 0.f)
        return full_fwd<X_CAP>(who, p.mode, p.win, dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->prefix_len, q, lq, k, lk, v, lv, o, lo, lse, stream, p.doc,
                               softcap, sink);
    if (sink)
        return full_fwd<X_SINK>(who, p.mode, p.win, dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->prefix_len, q, lq, k, lk, v, lv, o, lo, lse, stream, p.doc,
                                0.f, sink);
    { // modifiers off: this entry's checks (and name), then the family's own entry
        const void *ops[4] = {q, k, v, o};
        const kf_attn_layout *lay[4] = {lq, lk, lv, lo};
        FullArgs a;
        Plan plan;
        rc = full_check(who, dtype, B, Hq, Hkv, Sq, Skv, D, scale, ops, lay, 4, a, plan);
        if (rc != KF_OK || plan == PLAN_NONE) return rc;
        rc = set_doc(who, a, p.mode, p.doc);
        if (rc != KF_OK) return rc;
    }
    switch (mask->kind) {
    case KF_ATTN_MASK_FULL: return kf_attn_full_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, q, lq, k, lk, v, lv, o, lo, lse, stream);
    case KF_ATTN_MASK_PREFIX: return kf_attn_prefix_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->prefix_len, q, lq, k, lk, v, lv, o, lo, lse, stream);
    case KF_ATTN_MASK_WINDOW:
        return kf_attn_window_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->window_left, mask->window_right, q, lq, k, lk, v, lv, o, lo, lse, stream);
    default:
        return kf_attn_doc_fwd(dtype, B, Hq, Hkv, Sq, D, scale, mask->causal, mask->kv_len, mask->doc_start, mask->doc_end, q, lq, k, lk, v, lv, o, lo, lse, stream);
    }
}

extern "C" int kf_attn_ext_bwd_workspace_bytes(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_attn_ext_bwd_workspace_bytes: null out pointer");
    FullArgs a;
    Plan plan;
    int rc = full_check("kf_attn_ext_bwd_workspace_bytes", dtype, B, Hq, Hkv, Sq, Skv, D, 1.f, nullptr, nullptr, 0, a, plan);
    if (rc != KF_OK) return rc;
    *bytes = ws_bytes(B, Hq, Sq);
    return KF_OK;
}

extern "C" int kf_attn_ext_bwd(int dtype, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, float scale, const kf_attn_mask *mask,
                               float softcap, const float *sink, const void *q, const kf_attn_layout *lq, const void *k, const kf_attn_layout *lk,
                               const void *v, const kf_attn_layout *lv, const void *o, const kf_attn_layout *lo, const float *lse, const void *d_o,
                               const kf_attn_layout *ldo, void *dq, const kf_attn_layout *ldq, void *dk, const kf_attn_layout *ldk, void *dv,
                               const kf_attn_layout *ldv, float *dsink, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_attn_ext_bwd";
    MaskPlan p;
    int rc = mask_check(who, mask, Sq, Skv, p);
    if (rc != KF_OK) return rc;
    rc = modifier_check(who, softcap);
    if (rc != KF_OK) return rc;
    KF_REQUIRE((sink != nullptr) == (dsink != nullptr), KF_ERR_INVALID, "%s: dsink is required exactly when sink is given", who);
    {
        const void *ops[8] = {q, k, v, o, d_o, dq, dk, dv};
        const kf_attn_layout *lay[8] = {lq, lk, lv, lo, ldo, ldq, ldk, ldv};
        FullArgs a;
        Plan plan;
        rc = full_check(who, dtype, B, Hq, Hkv, Sq, Skv, D, scale, ops, lay, 8, a, plan);
        if (rc != KF_OK || plan == PLAN_NONE) return rc;
        KF_REQUIRE(lse, KF_ERR_INVALID, "%s: null operand", who);
        const size_t need = ws_bytes(B, Hq, Sq);
        KF_REQUIRE(workspace && workspace_bytes >= need && (uintptr_t)workspace % sizeof(float) == 0, KF_ERR_INVALID,
                   "%s: workspace of at least %zu bytes required (kf_attn_ext_bwd_workspace_bytes), got %zu", who, need, workspace_bytes);
        rc = set_doc(who, a, p.mode, p.doc);
        if (rc != KF_OK) return rc;
    }
    if (softcap > 0.f) {
        rc = full_bwd<true>(who, p.mode, p.win, dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->prefix_len, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq,
                            ldq, dk, ldk, dv, ldv, workspace, workspace_bytes, stream, p.doc, softcap);
    } else {
        switch (mask->kind) {
        case KF_ATTN_MASK_FULL:
            rc = kf_attn_full_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq, dk, ldk, dv, ldv, workspace,
                                  workspace_bytes, stream);
            break;
        case KF_ATTN_MASK_PREFIX:
            rc = kf_attn_prefix_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->prefix_len, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq, dk, ldk,
                                    dv, ldv, workspace, workspace_bytes, stream);
            break;
        case KF_ATTN_MASK_WINDOW:
            rc = kf_attn_window_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, mask->kv_len, mask->window_left, mask->window_right, q, lq, k, lk, v, lv, o, lo, lse, d_o,
                                    ldo, dq, ldq, dk, ldk, dv, ldv, workspace, workspace_bytes, stream);
            break;
        default:
            rc = kf_attn_doc_bwd(dtype, B, Hq, Hkv, Sq, D, scale, mask->causal, mask->kv_len, mask->doc_start, mask->doc_end, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo,
                                 dq, ldq, dk, ldk, dv, ldv, workspace, workspace_bytes, stream);
            break;
        }
    }
    if (rc != KF_OK || !sink) return rc;
    // the workspace holds delta [B, Hq, Sq] (the pre-pass of the launches above); one workgroup per head (Hq <= 2^24: full_check)
    hipStream_t st = as_stream(stream);
    KF_PROF("attn_sink_grad", st);
    return launch(attn_sink_grad_kernel, (unsigned)Hq, NT, 0, st, sink, lse, (const float *)workspace, dsink, B, Hq, Sq);
}
