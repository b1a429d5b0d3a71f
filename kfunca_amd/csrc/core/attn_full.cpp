// namespace gpu: full attention over kf_attn_full_fwd / kf_attn_full_bwd (attn_full.h).
#include "attn_full.h"

#include <cmath>

#include "allocator.h"
#include "device_api.h"
#include "ops.h"

namespace gpu {

using utils::memory::DataPtr;
using utils::memory::DeviceAllocator;

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool h16(ScalarType t) { return t == ScalarType::Half || t == ScalarType::BFloat16; }

void check_operands(const Tensor &q, const Tensor &k, const Tensor &v) {
    CHECK_FAIL(q.defined() && k.defined() && v.defined() && q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
               "attention expects q [B, Hq, Sq, D] and k, v [B, Hkv, Skv, D]");
    CHECK_FAIL(k.shape(0) == q.shape(0) && k.shape(3) == q.shape(3) && k.sizes() == v.sizes(), "attention: shapes of q, k, v do not match");
    CHECK_FAIL(k.shape(1) >= 1 && k.shape(1) <= q.shape(1) && q.shape(1) % k.shape(1) == 0, "attention: the K/V head count ", k.shape(1),
               " must divide the query head count ", q.shape(1));
    CHECK_FAIL(q.dtype() == k.dtype() && q.dtype() == v.dtype(), "attention: q, k, v must share a dtype");
    CHECK_FAIL(q.dtype() == ScalarType::Float || h16(q.dtype()), "attention supports float, half and bfloat16");
    CHECK_FAIL(q.shape(3) >= 1 && q.shape(3) <= 256, "attention: head size ", q.shape(3), " outside [1, 256]");
    CHECK_FAIL(k.shape(2) >= 1, "attention: keys are empty");
    CHECK_FAIL(q.is_dense() && k.is_dense() && v.is_dense(), "attention expects dense tensors");
    CHECK_FAIL(q.device() == k.device() && q.device() == v.device(), "attention: q, k, v must be on one device");
}
// the kernels read kv_len as a dense int64 array
Tensor check_len(const Tensor &kv_len, int64_t B, int device) {
    if (!kv_len.defined()) return Tensor();
    CHECK_FAIL(kv_len.dtype() == ScalarType::Long, "attention: kv_len must be of type Long");
    CHECK_FAIL(kv_len.numel() == B && kv_len.device() == device, "attention: kv_len must hold B = ", B, " elements on the operands' device");
    return kv_len.dense();
}
const int64_t *len_ptr(const Tensor &kv_len) { return kv_len.defined() ? static_cast<const int64_t *>(kv_len.data_ptr()) : nullptr; }

// 16-bit head sizes off 64 / 128: zero columns change neither Q K^T nor P V, and the scale stays that of the real head size
int64_t padded_head(const Tensor &q) {
    const int64_t D = q.shape(3);
    if (!h16(q.dtype()) || D == 64 || D > 128) return D;
    return D < 64 ? 64 : 128;
}
Tensor pad_cols(const Tensor &t, int64_t cols) { // [B, H, S, D] -> [B, H, S, cols], zero-filled
    if (t.shape(3) == cols) return t;
    auto shape = t.sizes();
    shape[3] = cols;
    Tensor p = zeros(shape, t.dtype(), t.device());
    Tensor head = p.narrow(3, 0, t.shape(3));
    copy_(head, t);
    return p;
}
Tensor unpad_cols(const Tensor &t, int64_t cols) { return t.shape(3) == cols ? t : t.narrow(3, 0, cols).dense(); }

DataPtr bwd_scratch(int dt, int64_t B, int64_t Hq, int64_t Hkv, int64_t Sq, int64_t Skv, int64_t D, int device, size_t &bytes) {
    DEV_CALL(kf_attn_full_bwd_workspace_bytes(dt, B, Hq, Hkv, Sq, Skv, D, &bytes));
    return DeviceAllocator::GetInstance()->allocate(bytes > 0 ? bytes : 1, device);
}

std::tuple<Tensor, Tensor> attention_fwd(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len) {
    const int64_t B = q.shape(0), Hq = q.shape(1), Sq = q.shape(2), D = q.shape(3), Hkv = k.shape(1), Skv = k.shape(2), Dp = padded_head(q);
    const Tensor qp = pad_cols(q, Dp), kp = pad_cols(k, Dp), vp = pad_cols(v, Dp);
    Tensor outp = empty_like(qp);
    Tensor lse = empty({B, Hq, Sq}, ScalarType::Float, q.device());
    DEV_CALL(kf_attn_full_fwd(code(q.dtype()), B, Hq, Hkv, Sq, Skv, Dp, 1.0f / std::sqrt((float)D), len_ptr(kv_len), qp.data_ptr(), nullptr, kp.data_ptr(),
                              nullptr, vp.data_ptr(), nullptr, outp.data_ptr(), nullptr, static_cast<float *>(lse.data_ptr()), dev::stream(q.device())));
    return {unpad_cols(outp, D), lse};
}

std::tuple<Tensor, Tensor, Tensor> attention_bwd(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len, const Tensor &out, const Tensor &lse,
                                                 const Tensor &grad_out) {
    CHECK_FAIL(grad_out.sizes() == q.sizes() && grad_out.dtype() == q.dtype(), "attention: the gradient does not match the output");
    const int64_t B = q.shape(0), Hq = q.shape(1), Sq = q.shape(2), D = q.shape(3), Hkv = k.shape(1), Skv = k.shape(2), Dp = padded_head(q);
    const int dt = code(q.dtype());
    const Tensor qp = pad_cols(q, Dp), kp = pad_cols(k, Dp), vp = pad_cols(v, Dp), op = pad_cols(out, Dp), gp = pad_cols(grad_out.dense(), Dp);
    Tensor dqp = empty_like(qp), dkp = empty_like(kp), dvp = empty_like(vp);
    if (dqp.numel() == 0) return {unpad_cols(dqp, D), unpad_cols(zeros(kp.sizes(), k.dtype(), k.device()), D), unpad_cols(zeros(vp.sizes(), v.dtype(), v.device()), D)};
    size_t need = 0;
    DataPtr scratch = bwd_scratch(dt, B, Hq, Hkv, Sq, Skv, Dp, q.device(), need);
    DEV_CALL(kf_attn_full_bwd(dt, B, Hq, Hkv, Sq, Skv, Dp, 1.0f / std::sqrt((float)D), len_ptr(kv_len), qp.data_ptr(), nullptr, kp.data_ptr(), nullptr,
                              vp.data_ptr(), nullptr, op.data_ptr(), nullptr, static_cast<const float *>(lse.data_ptr()), gp.data_ptr(), nullptr,
                              dqp.data_ptr(), nullptr, dkp.data_ptr(), nullptr, dvp.data_ptr(), nullptr, scratch.get(), need, dev::stream(q.device())));
    return {unpad_cols(dqp, D), unpad_cols(dkp, D), unpad_cols(dvp, D)};
}

class FullAttentionGradFunction : public GradFunction {
public:
    FullAttentionGradFunction(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len, const Tensor &out, const Tensor &lse)
        : kv_len_(kv_len), out_(out), lse_(lse) {
        inputs = {q, k, v};
    }
    std::vector<Tensor> backward(Tensor g) override {
        auto [dq, dk, dv] = attention_bwd(inputs[0], inputs[1], inputs[2], kv_len_, out_, lse_, g);
        return {dq, dk, dv};
    }

private:
    Tensor kv_len_, out_, lse_;
};

struct PackedLay { kf_attn_layout qkv, flat; };
PackedLay packed_layouts(int64_t S, int64_t H, int64_t Hkv, int64_t D) { // the projection [B*S, W], W = (H + 2 Hkv) D; the output [B*S, H D]
    const int64_t d = H * D, W = (H + 2 * Hkv) * D;
    return {{S * W, D, W}, {S * d, D, d}};
}

class PackedFullAttentionGradFunction : public GradFunction {
public:
    PackedFullAttentionGradFunction(const Tensor &qkv, const Tensor &kv_len, const Tensor &out, const Tensor &lse, int64_t B, int64_t S, int64_t H, int64_t Hkv)
        : kv_len_(kv_len), out_(out), lse_(lse), B_(B), S_(S), H_(H), Hkv_(Hkv) {
        inputs = {qkv};
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &qkv = inputs[0];
        const int64_t D = qkv.shape(1) / (H_ + 2 * Hkv_), d = H_ * D, dkv = (H_ + Hkv_) * D;
        const int es = (int)qkv.element_size_in_bytes(), dt = code(qkv.dtype());
        Tensor gc = g.dense();
        Tensor dqkv = empty(qkv.sizes(), qkv.dtype(), qkv.device());
        const PackedLay L = packed_layouts(S_, H_, Hkv_, D);
        const char *p = static_cast<const char *>(qkv.data_ptr());
        char *gp = static_cast<char *>(dqkv.data_ptr());
        size_t need = 0;
        DataPtr scratch = bwd_scratch(dt, B_, H_, Hkv_, S_, S_, D, qkv.device(), need);
        DEV_CALL(kf_attn_full_bwd(dt, B_, H_, Hkv_, S_, S_, D, 1.0f / std::sqrt((float)D), len_ptr(kv_len_), p, &L.qkv, p + d * es, &L.qkv, p + dkv * es,
                                  &L.qkv, out_.data_ptr(), &L.flat, static_cast<const float *>(lse_.data_ptr()), gc.data_ptr(), &L.flat, gp, &L.qkv,
                                  gp + d * es, &L.qkv, gp + dkv * es, &L.qkv, scratch.get(), need, dev::stream(qkv.device())));
        return {dqkv};
    }

private:
    Tensor kv_len_, out_, lse_;
    int64_t B_, S_, H_, Hkv_;
};
} // namespace

Tensor attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len) {
    check_operands(q, k, v);
    const Tensor len = check_len(kv_len, q.shape(0), q.device());
    auto [out, lse] = attention_fwd(q, k, v, len);
    out.set_requires_grad(q.requires_grad() || k.requires_grad() || v.requires_grad());
    if (out.requires_grad()) out.set_grad_fn(new FullAttentionGradFunction(q, k, v, len, out, lse));
    return out;
}

Tensor attention_qkv(const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t kv_heads, const Tensor &kv_len) {
    const int64_t Hkv = kv_heads < 0 ? H : kv_heads;
    CHECK_FAIL(qkv.defined() && qkv.dim() == 2 && qkv.is_dense(), "attention_qkv expects a contiguous [B*S, (H + 2*kv_heads)*D] tensor");
    CHECK_FAIL(B > 0 && S > 0 && H > 0 && Hkv > 0 && H % Hkv == 0, "attention_qkv: kv_heads ", Hkv, " must divide H ", H);
    CHECK_FAIL(qkv.shape(0) == B * S && qkv.shape(1) > 0 && qkv.shape(1) % (H + 2 * Hkv) == 0, "attention_qkv: shape does not match B, S, H, kv_heads");
    const int64_t D = qkv.shape(1) / (H + 2 * Hkv), d = H * D, dkv = Hkv * D;
    if (!(h16(qkv.dtype()) && (D == 64 || D == 128))) {
        // off the strided kernels' shapes: split heads and the contiguous operator (which carries its own autograd)
        auto parts = tensor_split(qkv, {d, dkv, dkv}, 1);
        const int64_t nh[3] = {H, Hkv, Hkv};
        std::vector<Tensor> heads;
        for (int i = 0; i < 3; ++i) heads.push_back(parts[i].dense().view({B, S, nh[i], D}).permute({0, 2, 1, 3}).dense());
        Tensor a = attention(heads[0], heads[1], heads[2], kv_len);
        return a.permute({0, 2, 1, 3}).dense().view({B * S, d});
    }
    const Tensor len = check_len(kv_len, B, qkv.device());
    const int es = (int)qkv.element_size_in_bytes();
    Tensor out = empty({B * S, d}, qkv.dtype(), qkv.device());
    Tensor lse = empty({B, H, S}, ScalarType::Float, qkv.device());
    const PackedLay L = packed_layouts(S, H, Hkv, D);
    const char *p = static_cast<const char *>(qkv.data_ptr());
    DEV_CALL(kf_attn_full_fwd(code(qkv.dtype()), B, H, Hkv, S, S, D, 1.0f / std::sqrt((float)D), len_ptr(len), p, &L.qkv, p + d * es, &L.qkv,
                              p + (d + dkv) * es, &L.qkv, out.data_ptr(), &L.flat, static_cast<float *>(lse.data_ptr()), dev::stream(qkv.device())));
    if (qkv.requires_grad()) {
        out.set_requires_grad(true);
        out.set_grad_fn(new PackedFullAttentionGradFunction(qkv, len, out, lse, B, S, H, Hkv));
    }
    return out;
}

} // namespace gpu
