// namespace gpu: the attention operators over the C ABI's attention entries - causal_attention, causal_attention_gqa and
// causal_attention_qkv (ops.h; nn_ops.cpp:6-8 + the checks of causal_attention_kernel.cu:9-20), attention and attention_qkv (attn_full.h).
// Seven families of entries (the causal pair, full attention and its prefix-LM, sliding-window and document-masked forms, the last also with a window and prefixes inside the documents), one host path: check, plan the padding, pad,
// allocate, call, un-pad.
#include <cmath>

#include "allocator.h"
#include "attn_full.h"
#include "device_api.h"
#include "ops.h"

namespace gpu {

using utils::memory::DataPtr;
using utils::memory::DeviceAllocator;

namespace {

int code(ScalarType t) { return static_cast<int>(t); }
bool h16(ScalarType t) { return t == ScalarType::Half || t == ScalarType::BFloat16; }

enum class Family {
    CausalMha, // kf_attn_fwd / kf_attn_bwd, their _scaled forms for padded operands, their _strided forms for the packed projection
    CausalGqa, // kf_attn_fwd_gqa / kf_attn_bwd_gqa: query head h reads K/V head h / (Hq / Hkv)
    Full,      // kf_attn_full_fwd / kf_attn_full_bwd: no mask but an optional per-batch key length
    Prefix,    // kf_attn_prefix_fwd / kf_attn_prefix_bwd: Full's operands and checks; causal beyond an optional per-batch prefix
    Window,    // kf_attn_window_fwd / kf_attn_window_bwd: Full's operands and checks; keys m - left .. m + right of query m
    Doc,       // kf_attn_doc_fwd / kf_attn_doc_bwd: Full's operands and checks, Sq = Skv; the keys of the query's own document
    Span,      // kf_attn_span_fwd / kf_attn_span_bwd: Doc's, the mask's causal rule, prefixes and window baked into two pairs of tables
};
bool full_like(Family f) { return f == Family::Full || f == Family::Prefix || f == Family::Window || f == Family::Doc || f == Family::Span; }
// the length arrays of attention / attention_qkv: undefined tensors for the other families; with them the window of Family::Window
// (-1: unbounded on that side), which the backward keeps beside the lengths
// and the tables of Family::Doc (a DocMask's, kv among them) with its causal flag
struct Lens {
    Tensor kv, prefix;
    int64_t wl = -1, wr = -1;
    Tensor doc_start, doc_end;
    bool doc_causal = false;
    // Family::Span: doc_start and doc_end are the mask's key_lo and key_hi, these its key-indexed pair (the causal rule is in the tables)
    Tensor query_lo, query_hi;
    // the score modifiers of attention / attention_qkv (kf_attn_ext_*): the cap (0: off) and the sinks, Float [Hq] (undefined: none)
    float softcap = 0.f;
    Tensor sinks;
    bool modified() const { return softcap > 0.f || sinks.defined(); }
};

// One call as the C ABI takes it: the sizes handed down (padded ones where the host pads), the scale of the REAL head size, and the
// layouts of q, k, v and their gradients (lx) and of out and its gradient (lo); NULL: contiguous [B, H, S, D].
struct Call {
    Family family;
    int dt, device;
    int64_t B, Hq, Hkv, Sq, Skv, D;
    float scale;
    kf_attn_mask mask; // the full-like families: the one form of the mask, built once from Family + Lens (call_mask)
    const kf_attn_layout *lx, *lo;
    bool padded;
    // the score modifiers (full-like families only): with either one the call goes to kf_attn_ext_*, without them to the family's entries
    float softcap = 0.f;
    const float *sink = nullptr;
    const int32_t *query_lo = nullptr, *query_hi = nullptr; // Family::Span: the tables the dK/dV kernels read (mask.doc_start / doc_end: key_lo / key_hi)
    bool modified() const { return softcap > 0.f || sink; }
};

void run_fwd(const Call &c, const void *q, const void *k, const void *v, void *o, float *lse) {
    void *st = dev::stream(c.device);
    const kf_attn_mask &m = c.mask;
    if (c.family == Family::Span) { // one entry with and without modifiers
        DEV_CALL(kf_attn_span_fwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.D, c.scale, m.kv_len, m.doc_start, m.doc_end, c.softcap, c.sink, q, c.lx, k, c.lx, v, c.lx, o,
                                  c.lo, lse, st));
        return;
    }
    if (c.modified()) {
        DEV_CALL(kf_attn_ext_fwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, &m, c.softcap, c.sink, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, st));
        return;
    }
    switch (c.family) {
    case Family::CausalMha:
        if (c.lx) DEV_CALL(kf_attn_fwd_strided(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, c.scale, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, st));
        else if (c.padded) DEV_CALL(kf_attn_fwd_scaled(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, c.scale, q, k, v, o, lse, st));
        else DEV_CALL(kf_attn_fwd(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, q, k, v, o, lse, st));
        break;
    case Family::CausalGqa:
        DEV_CALL(kf_attn_fwd_gqa(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, st));
        break;
    case Family::Full:
        DEV_CALL(kf_attn_full_fwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, m.kv_len, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, st));
        break;
    case Family::Prefix:
        DEV_CALL(kf_attn_prefix_fwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, m.kv_len, m.prefix_len, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, st));
        break;
    case Family::Window:
        DEV_CALL(kf_attn_window_fwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, m.kv_len, m.window_left, m.window_right, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, st));
        break;
    case Family::Span: // (served above)
        break;
    case Family::Doc:
        DEV_CALL(kf_attn_doc_fwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.D, c.scale, m.causal, m.kv_len, m.doc_start, m.doc_end, q, c.lx, k, c.lx, v, c.lx, o, c.lo,
                                 lse, st));
        break;
    }
}

void run_bwd(const Call &c, const void *q, const void *k, const void *v, const void *o, const float *lse, const void *go, void *dq, void *dk, void *dv,
             void *ws, size_t bytes, float *dsink = nullptr) {
    void *st = dev::stream(c.device);
    const kf_attn_mask &m = c.mask;
    if (c.family == Family::Span) {
        DEV_CALL(kf_attn_span_bwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.D, c.scale, m.kv_len, m.doc_start, m.doc_end, c.query_lo, c.query_hi, c.softcap, c.sink, q, c.lx,
                                  k, c.lx, v, c.lx, o, c.lo, lse, go, c.lo, dq, c.lx, dk, c.lx, dv, c.lx, dsink, ws, bytes, st));
        return;
    }
    if (c.modified()) { // (the workspace is kf_attn_full_bwd_workspace_bytes': the two size queries agree)
        DEV_CALL(kf_attn_ext_bwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, &m, c.softcap, c.sink, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, go, c.lo, dq,
                                 c.lx, dk, c.lx, dv, c.lx, dsink, ws, bytes, st));
        return;
    }
    switch (c.family) {
    case Family::CausalMha:
        if (c.lx)
            DEV_CALL(kf_attn_bwd_strided(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, c.scale, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, go, c.lo, dq, c.lx, dk, c.lx,
                                         dv, c.lx, ws, bytes, st));
        else if (c.padded) DEV_CALL(kf_attn_bwd_scaled(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, c.scale, q, k, v, o, lse, go, dq, dk, dv, ws, bytes, st));
        else DEV_CALL(kf_attn_bwd(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, q, k, v, o, lse, go, dq, dk, dv, ws, bytes, st));
        break;
    case Family::CausalGqa:
        DEV_CALL(kf_attn_bwd_gqa(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, go, c.lo, dq, c.lx, dk, c.lx,
                                 dv, c.lx, ws, bytes, st));
        break;
    case Family::Full:
        DEV_CALL(kf_attn_full_bwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, m.kv_len, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, go, c.lo, dq, c.lx,
                                  dk, c.lx, dv, c.lx, ws, bytes, st));
        break;
    case Family::Prefix:
        DEV_CALL(kf_attn_prefix_bwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, m.kv_len, m.prefix_len, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, go,
                                    c.lo, dq, c.lx, dk, c.lx, dv, c.lx, ws, bytes, st));
        break;
    case Family::Window:
        DEV_CALL(kf_attn_window_bwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, c.scale, m.kv_len, m.window_left, m.window_right, q, c.lx, k, c.lx, v, c.lx, o, c.lo, lse, go, c.lo,
                                    dq, c.lx, dk, c.lx, dv, c.lx, ws, bytes, st));
        break;
    case Family::Span: // (served above)
        break;
    case Family::Doc:
        DEV_CALL(kf_attn_doc_bwd(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.D, c.scale, m.causal, m.kv_len, m.doc_start, m.doc_end, q, c.lx, k, c.lx, v, c.lx, o, c.lo,
                                 lse, go, c.lo, dq, c.lx, dk, c.lx, dv, c.lx, ws, bytes, st));
        break;
    }
}

// Backward scratch of the causal families: the size the device library recommends (statistics + dS of as many (batch, head) pairs as
// its cap allows); when the allocator cannot supply that, halve the part above `floor_` (the dS part) until it can - the library accepts
// anything down to its minimum (then the recomputing dQ kernel runs: kf_attn_bwd, include/kfunca_hip.h).
DataPtr alloc_shrinking(size_t need, size_t floor_, int device, size_t &bytes) {
    for (;;) {
        try {
            bytes = need;
            return DeviceAllocator::GetInstance()->allocate(need, device);
        } catch (const utils::OutOfMemory &) { // only that: any other failure is not cured by asking for less
            if (need <= floor_) throw;
            need = floor_ + (need - floor_) / 2;
            if (need - floor_ < ((size_t)1 << 20)) need = floor_;
        }
    }
}
DataPtr bwd_scratch(const Call &c, size_t &bytes) {
    size_t need = 0, floor_ = 0;
    switch (c.family) {
    case Family::CausalMha:
        DEV_CALL(kf_attn_bwd_workspace_bytes(c.dt, c.B, c.Hq, c.Sq, c.Skv, c.D, &need));
        floor_ = 3 * (((size_t)c.B * c.Hq * c.Sq * sizeof(float) + 255) / 256 * 256);
        break;
    case Family::CausalGqa: // the library's minimum (statistics + the dK / dV partials) is the floor of the OOM retries
        DEV_CALL(kf_attn_bwd_gqa_workspace_bytes(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, &need, &floor_));
        break;
    case Family::Full: // one size, no smaller form to retry with
    case Family::Prefix:
    case Family::Window:
    case Family::Doc:
    case Family::Span:
        DEV_CALL(kf_attn_full_bwd_workspace_bytes(c.dt, c.B, c.Hq, c.Hkv, c.Sq, c.Skv, c.D, &bytes));
        return DeviceAllocator::GetInstance()->allocate(bytes > 0 ? bytes : 1, c.device);
    }
    return alloc_shrinking(need, floor_, c.device, bytes);
}

// The refusals of causal_attention_gqa and attention carry their operator's name; causal_attention's carry no text but the dtype's.
void check_operands(Family f, const Tensor &q, const Tensor &k, const Tensor &v) {
    const char *op = full_like(f) ? "attention" : "causal_attention_gqa";
    auto text = [&](auto... parts) { return f == Family::CausalMha ? std::string() : utils::concat(op, parts...); };
    CHECK_FAIL(q.defined() && k.defined() && v.defined() && q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
               text(" expects q [B, Hq, Sq, D] and k, v [B, Hkv, Skv, D]"));
    CHECK_FAIL(k.shape(0) == q.shape(0) && k.shape(3) == q.shape(3) && k.sizes() == v.sizes(), text(": shapes of q, k, v do not match"));
    CHECK_FAIL(f == Family::CausalMha ? k.shape(1) == q.shape(1) : k.shape(1) >= 1 && k.shape(1) <= q.shape(1) && q.shape(1) % k.shape(1) == 0,
               text(": the K/V head count ", k.shape(1), " must divide the query head count ", q.shape(1)));
    CHECK_FAIL(q.dtype() == k.dtype() && q.dtype() == v.dtype(), text(": q, k, v must share a dtype"));
    CHECK_FAIL(q.dtype() == ScalarType::Float || h16(q.dtype()),
               full_like(f) ? std::string("attention supports float, half and bfloat16") : utils::concat("Unsupported ScalarType ", q.dtype()));
    if (full_like(f)) {
        CHECK_FAIL(q.shape(3) >= 1 && q.shape(3) <= 256, "attention: head size ", q.shape(3), " outside [1, 256]");
        CHECK_FAIL(k.shape(2) >= 1, "attention: keys are empty");
    }
    CHECK_FAIL(q.is_dense() && k.is_dense() && v.is_dense(), text(" expects dense tensors"));
    CHECK_FAIL(q.device() == k.device() && q.device() == v.device(), text(": q, k, v must be on one device"));
}
// the kernels read kv_len and prefix_len as dense int64 arrays
Tensor check_len(const Tensor &kv_len, int64_t B, int device, const char *name = "kv_len") {
    if (!kv_len.defined()) return Tensor();
    CHECK_FAIL(kv_len.dtype() == ScalarType::Long, "attention: ", name, " must be of type Long");
    CHECK_FAIL(kv_len.numel() == B && kv_len.device() == device, "attention: ", name, " must hold B = ", B, " elements on the operands' device");
    return kv_len.dense();
}
Lens check_lens(const Lens &l, int64_t B, int device) {
    Lens r = l;
    r.kv = check_len(l.kv, B, device);
    r.prefix = check_len(l.prefix, B, device, "prefix_len");
    return r;
}
// the sinks of attention / attention_qkv: Float [Hq], dense, on the operands' device (the tensor itself is kept: it receives the gradient)
void check_modifiers(const char *op, const Lens &l, int64_t Hq, int device) {
    if (!l.sinks.defined()) return;
    CHECK_FAIL(l.sinks.dtype() == ScalarType::Float, op, ": sinks must be of type Float");
    CHECK_FAIL(l.sinks.dim() == 1 && l.sinks.shape(0) == Hq && l.sinks.is_dense(), op, ": sinks must be a dense tensor of shape [Hq] = [", Hq, "]");
    CHECK_FAIL(l.sinks.device() == device, op, ": sinks must be on the operands' device");
}
const float *sink_ptr(const Tensor &t) { return t.defined() ? static_cast<const float *>(t.data_ptr()) : nullptr; }
const int64_t *len_ptr(const Tensor &kv_len) { return kv_len.defined() ? static_cast<const int64_t *>(kv_len.data_ptr()) : nullptr; }
const int32_t *tab_ptr(const Tensor &t) { return t.defined() ? static_cast<const int32_t *>(t.data_ptr()) : nullptr; }
// the mask of a full-like family as the C ABI has it, the fields of another kind neutral (the causal families read none of it)
kf_attn_mask call_mask(Family f, const Lens &len) {
    kf_attn_mask m{KF_ATTN_MASK_FULL, len_ptr(len.kv), nullptr, -1, -1, nullptr, nullptr, 0};
    if (f == Family::Prefix) {
        m.kind = KF_ATTN_MASK_PREFIX;
        m.prefix_len = len_ptr(len.prefix);
    } else if (f == Family::Window) {
        m.kind = KF_ATTN_MASK_WINDOW;
        m.window_left = len.wl;
        m.window_right = len.wr;
    } else if (f == Family::Doc) {
        m.kind = KF_ATTN_MASK_DOC;
        m.doc_start = tab_ptr(len.doc_start);
        m.doc_end = tab_ptr(len.doc_end);
        m.causal = len.doc_causal;
    } else if (f == Family::Span) { // as kf_attn_span_* read it: the document tables without a causal rule of their own
        m.kind = KF_ATTN_MASK_DOC;
        m.doc_start = tab_ptr(len.doc_start);
        m.doc_end = tab_ptr(len.doc_end);
    }
    return m;
}

// The extents handed down. The MFMA kernels want D = 64 or 128 (and, f32, whole tiles of 32 rows); everything else takes the generic
// vector-ALU kernel (two orders of magnitude slower). Zero columns change neither Q K^T nor P V (the softmax scale stays 1 / sqrt(D) of
// the real head size), so a 16-bit head size up to 128 is padded in every family; f32 is padded in the causal families only (the
// exact-f32 MFMA kernels), and only there rows are padded, when Skv >= Sq > 0: a padded key n >= Skv >= Sq > m is above the diagonal
// of every real query; a padded query has q = 0 and dO = 0, so it contributes exactly zero to dK and dV. The 16-bit kernels take any
// sequence lengths themselves (rows beyond a tensor's end are zero-filled / dropped by their buffer descriptors).
struct PadPlan { int64_t Sq, Skv, D; };
PadPlan pad_plan(Family f, const Tensor &q, const Tensor &k) {
    const int64_t Sq = q.shape(2), Skv = k.shape(2), D = q.shape(3);
    PadPlan p{Sq, Skv, D};
    if (full_like(f)) {
        if (h16(q.dtype()) && D != 64 && D <= 128) p.D = D < 64 ? 64 : 128;
        return p;
    }
    if (!(D > 0 && D <= 128 && Skv >= Sq && Sq > 0) || !(h16(q.dtype()) || q.dtype() == ScalarType::Float)) return p;
    const int64_t rows = h16(q.dtype()) ? 1 : 32;
    return {(Sq + rows - 1) / rows * rows, (Skv + rows - 1) / rows * rows, D <= 64 ? 64 : 128};
}
bool same_extents(const Tensor &t, int64_t rows, int64_t cols) { return t.shape(2) == rows && (t.dim() == 3 || t.shape(3) == cols); }
Tensor pad(const Tensor &t, int64_t rows, int64_t cols) { // [B,H,S,D] -> [B,H,rows,cols] (or [B,H,S] -> [B,H,rows]), zero-filled; t itself when nothing grows
    if (same_extents(t, rows, cols)) return t;
    auto shape = t.sizes();
    shape[2] = rows;
    if (shape.size() == 4) shape[3] = cols;
    Tensor p = zeros(shape, t.dtype(), t.device());
    Tensor head = p.narrow(2, 0, t.shape(2));
    if (shape.size() == 4) head = head.narrow(3, 0, t.shape(3));
    copy_(head, t);
    return p;
}
Tensor unpad(const Tensor &t, int64_t rows, int64_t cols) {
    if (same_extents(t, rows, cols)) return t;
    Tensor v = t.narrow(2, 0, rows);
    if (t.dim() == 4) v = v.narrow(3, 0, cols);
    return v.dense();
}

Call contiguous_call(Family f, const Tensor &q, const Tensor &k, const PadPlan &pp, const Lens &len) {
    const bool padded = pp.Sq != q.shape(2) || pp.Skv != k.shape(2) || pp.D != q.shape(3);
    return {.family = f, .dt = code(q.dtype()), .device = q.device(), .B = q.shape(0), .Hq = q.shape(1), .Hkv = k.shape(1), .Sq = pp.Sq, .Skv = pp.Skv,
            .D = pp.D, .scale = 1.0f / std::sqrt((float)q.shape(3)), .mask = call_mask(f, len), .lx = nullptr, .lo = nullptr, .padded = padded,
            .softcap = len.softcap, .sink = sink_ptr(len.sinks), .query_lo = tab_ptr(len.query_lo), .query_hi = tab_ptr(len.query_hi)};
}

std::tuple<Tensor, Tensor> attention_forward(Family f, const Tensor &q, const Tensor &k, const Tensor &v, const Lens &len) {
    const int64_t B = q.shape(0), Hq = q.shape(1), Sq = q.shape(2), D = q.shape(3);
    if (f == Family::CausalGqa) {
        if (q.numel() == 0) return {empty_like(q), empty({B, Hq, Sq}, ScalarType::Float, q.device())};
        CHECK_FAIL(k.shape(2) > 0, "causal_attention_gqa: keys are empty");
    }
    const PadPlan pp = pad_plan(f, q, k);
    Tensor qp = pad(q, pp.Sq, pp.D), kp = pad(k, pp.Skv, pp.D), vp = pad(v, pp.Skv, pp.D);
    Tensor outp = empty_like(qp);
    Tensor lsep = empty({B, Hq, pp.Sq}, ScalarType::Float, q.device());
    run_fwd(contiguous_call(f, q, k, pp, len), qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), outp.data_ptr(), static_cast<float *>(lsep.data_ptr()));
    return {unpad(outp, Sq, D), unpad(lsep, Sq, 0)};
}

// dsink: with sinks, where their gradient goes (Float [Hq]; zeros when there is no query to sum over)
std::tuple<Tensor, Tensor, Tensor> attention_backward(Family f, const Tensor &q, const Tensor &k, const Tensor &v, const Lens &len, const Tensor &out,
                                                      const Tensor &lse, const Tensor &grad_out, Tensor *dsink = nullptr) {
    if (dsink) *dsink = zeros(len.sinks.sizes(), ScalarType::Float, q.device());
    if (f == Family::CausalMha) check_operands(f, q, k, v); // causal_attention_bwd is an operator of its own (ops.h)
    CHECK_FAIL(grad_out.sizes() == q.sizes() && grad_out.dtype() == q.dtype(), full_like(f) ? "attention: the gradient does not match the output" : "");
    const int64_t Sq = q.shape(2), Skv = k.shape(2), D = q.shape(3);
    if (f == Family::CausalGqa && (q.numel() == 0 || k.numel() == 0)) // nothing attends: every gradient is zero
        return {zeros(q.sizes(), q.dtype(), q.device()), zeros(k.sizes(), k.dtype(), k.device()), zeros(v.sizes(), v.dtype(), v.device())};
    const PadPlan pp = pad_plan(f, q, k);
    Tensor qp = pad(q, pp.Sq, pp.D), kp = pad(k, pp.Skv, pp.D), vp = pad(v, pp.Skv, pp.D), op = pad(out, pp.Sq, pp.D);
    Tensor lp = pad(lse, pp.Sq, 0), gp = pad(grad_out.dense(), pp.Sq, pp.D);
    Tensor dqp = empty_like(qp), dkp = empty_like(kp), dvp = empty_like(vp);
    if (full_like(f) && dqp.numel() == 0) // no query: dk and dv are zero
        return {unpad(dqp, Sq, D), unpad(zeros(kp.sizes(), k.dtype(), k.device()), Skv, D), unpad(zeros(vp.sizes(), v.dtype(), v.device()), Skv, D)};
    const Call c = contiguous_call(f, q, k, pp, len);
    size_t bytes = 0;
    DataPtr scratch = bwd_scratch(c, bytes);
    run_bwd(c, qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), op.data_ptr(), static_cast<const float *>(lp.data_ptr()), gp.data_ptr(), dqp.data_ptr(),
            dkp.data_ptr(), dvp.data_ptr(), scratch.get(), bytes, dsink ? static_cast<float *>(dsink->data_ptr()) : nullptr);
    return {unpad(dqp, Sq, D), unpad(dkp, Skv, D), unpad(dvp, Skv, D)};
}

class AttentionGradFunction : public GradFunction {
public:
    AttentionGradFunction(Family f, const Tensor &q, const Tensor &k, const Tensor &v, const Lens &len, const Tensor &out, const Tensor &lse)
        : family_(f), len_(len), out_(out), lse_(lse) {
        inputs = {q, k, v};
        if (len.sinks.defined()) inputs.push_back(len.sinks); // a fourth differentiable input
    }
    std::vector<Tensor> backward(Tensor g) override {
        Tensor dsink;
        auto [dq, dk, dv] = attention_backward(family_, inputs[0], inputs[1], inputs[2], len_, out_, lse_, g, len_.sinks.defined() ? &dsink : nullptr);
        if (len_.sinks.defined()) return {dq, dk, dv, dsink};
        return {dq, dk, dv};
    }

private:
    Family family_;
    Lens len_;
    Tensor out_, lse_;
};

// kv_len and prefix_len are checked and made dense once; the backward keeps those tensors
Tensor contiguous_attention(Family f, const Tensor &q, const Tensor &k, const Tensor &v, const Lens &lens) {
    check_operands(f, q, k, v);
    Lens len = check_lens(lens, q.shape(0), q.device());
    check_modifiers("attention", len, q.shape(1), q.device());
    auto [out, lse] = attention_forward(f, q, k, v, len);
    out.set_requires_grad(q.requires_grad() || k.requires_grad() || v.requires_grad() || (len.sinks.defined() && len.sinks.requires_grad()));
    if (out.requires_grad()) out.set_grad_fn(new AttentionGradFunction(f, q, k, v, len, out, lse));
    return out;
}

// ---- the packed QKV projection (README.md:32), read in place: [B*S, W], W = (H + 2 Hkv) D, columns q | k | v; the output is [B*S, H D] ----
struct PackedLay { kf_attn_layout qkv, flat; };
PackedLay packed_layouts(int64_t S, int64_t H, int64_t Hkv, int64_t D) {
    const int64_t d = H * D, W = (H + 2 * Hkv) * D;
    return {{S * W, D, W}, {S * d, D, d}};
}
// family CausalMha is Hkv = H here: K at column H D, V at 2 H D (the strided entries); otherwise K at H D, V at (H + Hkv) D
Call packed_call(Family f, const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t Hkv, int64_t D, const PackedLay &L, const Lens &len) {
    return {.family = f, .dt = code(qkv.dtype()), .device = qkv.device(), .B = B, .Hq = H, .Hkv = Hkv, .Sq = S, .Skv = S, .D = D,
            .scale = 1.0f / std::sqrt((float)D), .mask = call_mask(f, len), .lx = &L.qkv, .lo = &L.flat, .padded = false,
            .softcap = len.softcap, .sink = sink_ptr(len.sinks), .query_lo = tab_ptr(len.query_lo), .query_hi = tab_ptr(len.query_hi)};
}

class PackedAttentionGradFunction : public GradFunction {
public:
    PackedAttentionGradFunction(Family f, const Tensor &qkv, const Lens &len, const Tensor &out, const Tensor &lse, int64_t B, int64_t S, int64_t H,
                                int64_t Hkv)
        : family_(f), len_(len), out_(out), lse_(lse), B_(B), S_(S), H_(H), Hkv_(Hkv) {
        inputs = {qkv};
        if (len.sinks.defined()) inputs.push_back(len.sinks);
    }
    std::vector<Tensor> backward(Tensor g) override { // one packed gradient; dk, dv summed over each group
        const Tensor &qkv = inputs[0];
        const int64_t D = qkv.shape(1) / (H_ + 2 * Hkv_), es = qkv.element_size_in_bytes(), k_at = H_ * D * es, v_at = (H_ + Hkv_) * D * es;
        Tensor gc = g.dense();
        Tensor dqkv = empty(qkv.sizes(), qkv.dtype(), qkv.device());
        const PackedLay L = packed_layouts(S_, H_, Hkv_, D);
        const Call c = packed_call(family_, qkv, B_, S_, H_, Hkv_, D, L, len_);
        const char *p = static_cast<const char *>(qkv.data_ptr());
        char *gp = static_cast<char *>(dqkv.data_ptr());
        size_t bytes = 0;
        DataPtr scratch = bwd_scratch(c, bytes);
        Tensor dsink;
        if (len_.sinks.defined()) dsink = zeros(len_.sinks.sizes(), ScalarType::Float, qkv.device());
        run_bwd(c, p, p + k_at, p + v_at, out_.data_ptr(), static_cast<const float *>(lse_.data_ptr()), gc.data_ptr(), gp, gp + k_at, gp + v_at,
                scratch.get(), bytes, dsink.defined() ? static_cast<float *>(dsink.data_ptr()) : nullptr);
        if (dsink.defined()) return {dqkv, dsink};
        return {dqkv};
    }

private:
    Family family_;
    Lens len_;
    Tensor out_, lse_;
    int64_t B_, S_, H_, Hkv_;
};

// f: CausalMha for causal_attention_qkv(qkv, B, S, H) (Hkv = H, the [B*S, 3*H*D] texts), CausalGqa for its kv_heads form, Full, Prefix,
// Window, Doc and Span for attention_qkv
Tensor packed_attention(Family f, const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t Hkv, const Lens &lens) {
    const char *op = full_like(f) ? "attention_qkv" : "causal_attention_qkv";
    CHECK_FAIL(qkv.defined() && qkv.dim() == 2 && qkv.is_dense(), op,
               f == Family::CausalMha ? " expects a contiguous [B*S, 3*H*D] tensor" : " expects a contiguous [B*S, (H + 2*kv_heads)*D] tensor");
    if (f == Family::CausalMha) {
        CHECK_FAIL(B > 0 && S > 0 && H > 0 && qkv.shape(0) == B * S && qkv.shape(1) % (3 * H) == 0, "causal_attention_qkv: shape does not match B, S, H");
    } else {
        CHECK_FAIL(B > 0 && S > 0 && H > 0 && Hkv > 0 && H % Hkv == 0, op, ": kv_heads ", Hkv, " must divide H ", H);
        CHECK_FAIL(qkv.shape(0) == B * S && (!full_like(f) || qkv.shape(1) > 0) && qkv.shape(1) % (H + 2 * Hkv) == 0, op,
                   ": shape does not match B, S, H, kv_heads");
    }
    const int64_t D = qkv.shape(1) / (H + 2 * Hkv), d = H * D, dkv = Hkv * D;
    if (!(h16(qkv.dtype()) && (D == 64 || D == 128))) {
        // off the strided kernels' shapes: split heads and the contiguous operator of the family (which carries its own autograd)
        auto parts = tensor_split(qkv, {d, dkv, dkv}, 1);
        const int64_t nh[3] = {H, Hkv, Hkv};
        std::vector<Tensor> heads;
        for (int i = 0; i < 3; ++i) heads.push_back(parts[i].dense().view({B, S, nh[i], D}).permute({0, 2, 1, 3}).dense());
        Tensor a = contiguous_attention(f, heads[0], heads[1], heads[2], lens);
        return a.permute({0, 2, 1, 3}).dense().view({B * S, d});
    }
    Lens len = check_lens(lens, B, qkv.device());
    check_modifiers("attention_qkv", len, H, qkv.device());
    const int64_t es = qkv.element_size_in_bytes();
    Tensor out = empty({B * S, d}, qkv.dtype(), qkv.device());
    Tensor lse = empty({B, H, S}, ScalarType::Float, qkv.device());
    const PackedLay L = packed_layouts(S, H, Hkv, D);
    const char *p = static_cast<const char *>(qkv.data_ptr());
    run_fwd(packed_call(f, qkv, B, S, H, Hkv, D, L, len), p, p + d * es, p + (d + dkv) * es, out.data_ptr(), static_cast<float *>(lse.data_ptr()));
    if (qkv.requires_grad() || (len.sinks.defined() && len.sinks.requires_grad())) {
        out.set_requires_grad(true);
        out.set_grad_fn(new PackedAttentionGradFunction(f, qkv, len, out, lse, B, S, H, Hkv));
    }
    return out;
}

} // namespace

std::tuple<Tensor, Tensor> causal_attention_fwd(const Tensor &q, const Tensor &k, const Tensor &v) {
    check_operands(Family::CausalMha, q, k, v);
    return attention_forward(Family::CausalMha, q, k, v, Lens());
}
std::tuple<Tensor, Tensor, Tensor> causal_attention_bwd(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse,
                                                        const Tensor &grad_out) {
    return attention_backward(Family::CausalMha, q, k, v, Lens(), out, lse, grad_out);
}
Tensor causal_attention(const Tensor &q, const Tensor &k, const Tensor &v) { return contiguous_attention(Family::CausalMha, q, k, v, Lens()); }
Tensor causal_attention_gqa(const Tensor &q, const Tensor &k, const Tensor &v) { return contiguous_attention(Family::CausalGqa, q, k, v, Lens()); }
// A document mask is a family of its own: the mask carries its key lengths, so kv_len beside it is refused - like a prefix or a window
// given to the call: inside documents those are built into the mask (doc_mask(..., window, prefix_lens, causal)) - and so is a mask
// built for another batch, length or device (B_, S_, device: the operands'; Sq: the query length, Sq != Skv being cross-attention between
// packed rows). A mask built with a window, prefixes or causal holds the causal rule in its tables: the call's flag must repeat it.
static Family doc_family(const char *op, bool causal, const Tensor &prefix_len, const AttentionWindow *window, Lens &lens, const DocMask *doc, int64_t B_,
                         int64_t Sq, int64_t S_, int device) {
    CHECK_FAIL(!lens.kv.defined() && !prefix_len.defined() && !window, op,
               ": doc_mask cannot be combined with kv_len, prefix_len or window (the mask carries the rows' lengths; a window or prefixes inside "
               "documents belong to the mask: doc_mask(cu_doclens, S, window=..., prefix_lens=..., causal=...))");
    CHECK_FAIL(doc->kv_len.defined() && doc->doc_start.defined() && doc->doc_end.defined(), op, ": doc_mask is empty (build it with doc_mask(cu_doclens, S))");
    CHECK_FAIL(Sq == S_, op, ": doc_mask needs self-attention, Sq = Skv (got Sq = ", Sq, ", Skv = ", S_, ")");
    CHECK_FAIL(doc->B == B_ && doc->S == S_, op, ": doc_mask was built for B = ", doc->B, ", S = ", doc->S, ", the operands have B = ", B_, ", S = ", S_);
    CHECK_FAIL(doc->kv_len.device() == device, op, ": doc_mask must be on the operands' device");
    lens.kv = doc->kv_len;
    lens.doc_start = doc->doc_start;
    lens.doc_end = doc->doc_end;
    if (doc->span) {
        CHECK_FAIL(doc->query_lo.defined() && doc->query_hi.defined(), op, ": doc_mask is empty (build it with doc_mask(cu_doclens, S, ...))");
        CHECK_FAIL(causal == doc->causal, op, ": causal = ", causal ? "true" : "false", " but doc_mask was built with causal = ", doc->causal ? "true" : "false",
                   " (a mask with a window or prefixes holds the causal rule in its tables: pass the same value to both)");
        lens.query_lo = doc->query_lo;
        lens.query_hi = doc->query_hi;
        return Family::Span;
    }
    lens.doc_causal = causal;
    return Family::Doc;
}
// causal = false is the full family's path, call for call; a prefix belongs to the causal mask. Without a window the calls are those
// made before windows existed. With one: causal closes its right side (right = 0), so another right side contradicts it, and a window
// beside a prefix is no mask this package has.
static Family masked_family(const char *op, bool causal, const Tensor &prefix_len, const AttentionWindow *window, Lens &lens) {
    if (window) {
        CHECK_FAIL(!prefix_len.defined(), op, ": window and prefix_len cannot be combined (a window inside a prefix-LM mask is not supported)");
        CHECK_FAIL(window->left >= -1 && window->right >= -1, op, ": window sizes must be non-negative (-1 / None: unbounded on that side)");
        CHECK_FAIL(!causal || window->right <= 0, op, ": causal = true means window right = 0, got right = ", window->right);
        lens.wl = window->left;
        lens.wr = causal ? 0 : window->right;
        return Family::Window;
    }
    CHECK_FAIL(causal || !prefix_len.defined(), op, ": prefix_len needs causal = true (without the causal mask every key is visible already)");
    return causal ? Family::Prefix : Family::Full;
}
// softcap (0: off) and sinks as the operators take them; the cap is refused here with the operator's name, the sinks once Hq is known
static void set_modifiers(const char *op, Lens &lens, const AttentionModifiers *mods) {
    if (!mods) return;
    if (mods->has_softcap) {
        CHECK_FAIL(mods->softcap > 0.0 && std::isfinite(mods->softcap) && std::isfinite((float)mods->softcap), op, ": softcap must be positive and finite, got ",
                   mods->softcap);
        lens.softcap = (float)mods->softcap;
    }
    lens.sinks = mods->sinks;
}
Tensor attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len, bool causal, const Tensor &prefix_len,
                 const AttentionWindow *window, const DocMask *doc_mask, const AttentionModifiers *mods) {
    Lens lens{kv_len, prefix_len};
    set_modifiers("attention", lens, mods);
    if (doc_mask) check_operands(Family::Doc, q, k, v); // the shapes the mask is compared with
    const Family f = doc_mask ? doc_family("attention", causal, prefix_len, window, lens, doc_mask, q.shape(0), q.shape(2), k.shape(2), q.device())
                              : masked_family("attention", causal, prefix_len, window, lens);
    return contiguous_attention(f, q, k, v, lens);
}

// What both forms of doc_mask share: the checks of cu_doclens and S, the dense list (cu) and the mask's B, S and kv_len.
static DocMask doc_mask_head(const Tensor &cu_doclens, int64_t S, Tensor &cu) {
    CHECK_FAIL(cu_doclens.defined() && cu_doclens.dim() == 2 && cu_doclens.dtype() == ScalarType::Long && cu_doclens.shape(1) >= 2,
               "doc_mask expects cu_doclens of type Long and shape [B, n_docs + 1] with n_docs >= 1");
    CHECK_FAIL(S >= 0 && S < (int64_t(1) << 31), "doc_mask: S ", S, " outside [0, 2^31)");
    cu = cu_doclens.dense();
    DocMask m;
    m.B = cu.shape(0);
    m.S = S;
    m.kv_len = zeros({m.B}, ScalarType::Long, cu.device()); // (S = 0 launches nothing: every length is 0)
    return m;
}
// One launch (kf_attn_doc_table); the three tensors are dense and live on cu_doclens' device.
DocMask doc_mask(const Tensor &cu_doclens, int64_t S) {
    Tensor cu;
    DocMask m = doc_mask_head(cu_doclens, S, cu);
    const int64_t B = m.B, n = cu.shape(1) - 1;
    const int device = cu.device();
    m.doc_start = empty({B, S}, ScalarType::Int, device);
    m.doc_end = empty({B, S}, ScalarType::Int, device);
    if (B > 0 && S > 0)
        DEV_CALL(kf_attn_doc_table(B, S, n, static_cast<const int64_t *>(cu.data_ptr()), static_cast<int64_t *>(m.kv_len.data_ptr()),
                                   static_cast<int32_t *>(m.doc_start.data_ptr()), static_cast<int32_t *>(m.doc_end.data_ptr()), dev::stream(device)));
    return m;
}
// The mask with a window, per-document prefixes or the causal rule inside the documents: one launch (kf_attn_span_table) writes the keys
// each query sees (doc_start, doc_end) and the queries that see each key (query_lo, query_hi). The window is attention's: a side is a
// key count or -1; causal closes the right side (0, or -1 read as 0). Prefixes open it again - a token sees its whole prefix - so with
// them the table is built without a right side: the causal rule alone bounds it.
DocMask doc_mask(const Tensor &cu_doclens, int64_t S, const AttentionWindow *window, const Tensor &prefix_lens, bool causal) {
    Tensor cu;
    DocMask m = doc_mask_head(cu_doclens, S, cu);
    const int64_t B = m.B, n = cu.shape(1) - 1;
    const int device = cu.device();
    int64_t wl = -1, wr = -1;
    if (window) {
        CHECK_FAIL(window->left >= -1 && window->right >= -1, "doc_mask: window sizes must be non-negative (-1 / None: unbounded on that side)");
        CHECK_FAIL(!causal || window->right <= 0, "doc_mask: causal = true means window right = 0, got right = ", window->right);
        wl = window->left;
        wr = window->right;
    }
    if (causal) wr = 0;
    Tensor prefix;
    if (prefix_lens.defined()) {
        CHECK_FAIL(causal, "doc_mask: prefix_lens needs causal = true (without the causal mask every key of the document is visible already)");
        CHECK_FAIL(prefix_lens.dtype() == ScalarType::Long && prefix_lens.dim() == 2 && prefix_lens.shape(0) == B && prefix_lens.shape(1) == n,
                   "doc_mask: prefix_lens must be of type Long and shape [B, n_docs] = [", B, ", ", n, "]");
        CHECK_FAIL(prefix_lens.device() == device, "doc_mask: prefix_lens must be on cu_doclens' device");
        prefix = prefix_lens.dense();
    }
    m.span = true;
    m.causal = causal;
    m.window_left = wl;
    m.window_right = wr;
    Tensor *tab[4] = {&m.doc_start, &m.doc_end, &m.query_lo, &m.query_hi};
    for (Tensor *t : tab) *t = empty({B, S}, ScalarType::Int, device);
    if (B > 0 && S > 0)
        DEV_CALL(kf_attn_span_table(B, S, n, static_cast<const int64_t *>(cu.data_ptr()), len_ptr(prefix), causal, wl, prefix.defined() ? -1 : wr,
                                    static_cast<int64_t *>(m.kv_len.data_ptr()), static_cast<int32_t *>(m.doc_start.data_ptr()),
                                    static_cast<int32_t *>(m.doc_end.data_ptr()), static_cast<int32_t *>(m.query_lo.data_ptr()),
                                    static_cast<int32_t *>(m.query_hi.data_ptr()), dev::stream(device)));
    return m;
}

Tensor causal_attention_qkv(const Tensor &qkv, int64_t B, int64_t S, int64_t H) { return packed_attention(Family::CausalMha, qkv, B, S, H, H, Lens()); }
Tensor causal_attention_qkv(const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t kv_heads) {
    if (kv_heads >= 0 && kv_heads != H) return packed_attention(Family::CausalGqa, qkv, B, S, H, kv_heads, Lens());
    return causal_attention_qkv(qkv, B, S, H);
}
Tensor attention_qkv(const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t kv_heads, const Tensor &kv_len, bool causal, const Tensor &prefix_len,
                     const AttentionWindow *window, const DocMask *doc_mask, const AttentionModifiers *mods) {
    Lens lens{kv_len, prefix_len};
    set_modifiers("attention_qkv", lens, mods);
    const Family f = doc_mask ? doc_family("attention_qkv", causal, prefix_len, window, lens, doc_mask, B, S, S, qkv.defined() ? qkv.device() : 0)
                              : masked_family("attention_qkv", causal, prefix_len, window, lens);
    return packed_attention(f, qkv, B, S, H, kv_heads < 0 ? H : kv_heads, lens);
}

} // namespace gpu
