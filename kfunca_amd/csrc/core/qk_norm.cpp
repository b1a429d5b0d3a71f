// namespace gpu: per-head QK-norm fused with the rotary embedding over kf_qk_norm_rope_fwd / kf_qk_norm_rope_bwd (qk_norm.h).
#include "qk_norm.h"

#include <cmath>

#include "allocator.h"
#include "device_api.h"

namespace gpu {

using utils::memory::DataPtr;
using utils::memory::DeviceAllocator;

namespace {
int code(ScalarType t) { return static_cast<int>(t); }

// what one call needs besides the operands
struct QkNormCall {
    int64_t B, S, Hq, Hk, Hv, D, R;
    bool interleaved;
    double eps;
    Tensor cos, sin, positions;
    const float *table(const Tensor &t) const { return t.defined() ? static_cast<const float *>(t.data_ptr()) : nullptr; }
    const int64_t *pos() const { return positions.defined() ? static_cast<const int64_t *>(positions.data_ptr()) : nullptr; }
    int64_t table_rows() const { return cos.defined() ? cos.shape(0) : 0; }
    int64_t W() const { return (Hq + Hk + Hv) * D; }
};

const void *ptr_or_null(const Tensor &t) { return t.defined() ? t.data_ptr() : nullptr; }

// keeps the input, the weights, the tables and the positions: rstd and xhat are recomputed from x
class QkNormRopeGradFunction : public GradFunction {
public:
    QkNormRopeGradFunction(const Tensor &x, const Tensor &wq, const Tensor &wk, const QkNormCall &call)
        : call_(call), has_q_(wq.defined()), has_k_(wk.defined()) {
        inputs = {x};
        if (has_q_) inputs.push_back(wq);
        if (has_k_) inputs.push_back(wk);
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &x = inputs[0];
        const int iq = 1, ik = has_q_ ? 2 : 1;
        const Tensor wq = has_q_ ? inputs[iq] : Tensor(), wk = has_k_ ? inputs[ik] : Tensor();
        const bool want_q = has_q_ && wq.requires_grad(), want_k = has_k_ && wk.requires_grad();
        Tensor gc = g.dense();
        Tensor dx = empty(x.sizes(), x.dtype(), x.device());
        Tensor dwq, dwk;
        if (want_q) dwq = empty({call_.D}, x.dtype(), x.device());
        if (want_k) dwk = empty({call_.D}, x.dtype(), x.device());
        size_t need = 0;
        DataPtr scratch;
        if (want_q || want_k) {
            DEV_CALL(kf_qk_norm_rope_bwd_workspace_bytes(code(x.dtype()), call_.B, call_.S, call_.Hq, call_.Hk, call_.Hv, call_.D, &need));
            if (need) scratch = DeviceAllocator::GetInstance()->allocate(need, x.device());
        }
        const int64_t W = call_.W();
        DEV_CALL(kf_qk_norm_rope_bwd(code(x.dtype()), call_.B, call_.S, call_.Hq, call_.Hk, call_.Hv, call_.D, call_.R, call_.interleaved ? 1 : 0,
                                     call_.eps, ptr_or_null(wq), ptr_or_null(wk), call_.table(call_.cos), call_.table(call_.sin), call_.table_rows(),
                                     call_.pos(), x.data_ptr(), W, gc.data_ptr(), W, dx.data_ptr(), W, dwq.defined() ? dwq.data_ptr() : nullptr,
                                     dwk.defined() ? dwk.data_ptr() : nullptr, scratch.get(), need, dev::stream(x.device())));
        std::vector<Tensor> out(inputs.size());
        if (x.requires_grad()) out[0] = dx;
        if (want_q) out[iq] = dwq;
        if (want_k) out[ik] = dwk;
        return out;
    }

private:
    QkNormCall call_;
    bool has_q_, has_k_;
};
} // namespace

Tensor qk_norm_rope(const Tensor &qkv, const Tensor &q_weight, const Tensor &k_weight, const Tensor &cos, const Tensor &sin, int64_t B, int64_t S,
                    int64_t H, int64_t kv_heads, const Tensor &positions, bool interleaved, double eps) {
    const int64_t kv = kv_heads < 0 ? H : kv_heads;
    CHECK_FAIL(qkv.defined() && qkv.dim() == 2 && qkv.is_dense(), "qk_norm_rope expects a contiguous [B*S, (H + 2*kv_heads)*D] tensor");
    CHECK_FAIL(qkv.dtype() == ScalarType::Float || qkv.dtype() == ScalarType::Half || qkv.dtype() == ScalarType::BFloat16,
               "qk_norm_rope supports float, half and bfloat16");
    CHECK_FAIL(B > 0 && S > 0 && H > 0 && qkv.shape(0) == B * S && qkv.shape(1) > 0 && qkv.shape(1) % (H + 2 * kv) == 0,
               "qk_norm_rope: shape does not match B, S, H, kv_heads");
    CHECK_FAIL(std::isfinite(eps) && eps >= 0.0, "qk_norm_rope: eps ", eps, " must be finite and not negative");
    const int64_t W = qkv.shape(1), D = W / (H + 2 * kv);
    for (const Tensor *w : {&q_weight, &k_weight})
        if (w->defined())
            CHECK_FAIL(w->dim() == 1 && w->shape(0) == D && w->dtype() == qkv.dtype() && w->is_dense() && w->device() == qkv.device(),
                       "qk_norm_rope: q_weight / k_weight must be contiguous 1-D tensors of the head dimension D = ", D, " and of qkv's dtype, on its device");
    CHECK_FAIL(cos.defined() == sin.defined(), "qk_norm_rope: cos and sin must be given together (both None: the norm alone)");
    int64_t R = 0;
    if (cos.defined()) {
        CHECK_FAIL(cos.dim() == 2 && cos.sizes() == sin.sizes() && cos.is_dense() && sin.is_dense(),
                   "qk_norm_rope: cos and sin must be contiguous 2-D tables of one shape [positions, rotary_dim / 2]");
        CHECK_FAIL(cos.dtype() == ScalarType::Float && sin.dtype() == ScalarType::Float, "qk_norm_rope: cos and sin must be float tables");
        CHECK_FAIL(cos.shape(0) >= 1 && cos.shape(1) >= 1 && 2 * cos.shape(1) <= D, "qk_norm_rope: the tables' rotary_dim ", 2 * cos.shape(1),
                   " must lie in [2, D = ", D, "]");
        CHECK_FAIL(cos.device() == qkv.device() && sin.device() == qkv.device(), "qk_norm_rope: the tables must be on the operand's device");
        R = 2 * cos.shape(1);
        if (positions.defined()) {
            CHECK_FAIL(positions.dtype() == ScalarType::Long, "qk_norm_rope: positions must be of type Long");
            CHECK_FAIL(positions.numel() == B * S && positions.device() == qkv.device(), "qk_norm_rope: positions must hold B*S = ", B * S,
                       " elements on the operand's device");
        } else {
            CHECK_FAIL(S <= cos.shape(0), "qk_norm_rope: without positions the tables need S = ", S, " rows, they have ", cos.shape(0));
        }
    }
    // the kernel reads positions as a dense int64 array in token order; without tables they are not read at all
    const QkNormCall call{B, S, H, kv, kv, D, R, interleaved, eps, cos, sin, (R > 0 && positions.defined()) ? positions.dense() : Tensor()};
    Tensor out = empty(qkv.sizes(), qkv.dtype(), qkv.device());
    DEV_CALL(kf_qk_norm_rope_fwd(code(qkv.dtype()), B, S, H, kv, kv, D, R, interleaved ? 1 : 0, eps, ptr_or_null(q_weight), ptr_or_null(k_weight),
                                 call.table(cos), call.table(sin), call.table_rows(), call.pos(), qkv.data_ptr(), W, out.data_ptr(), W,
                                 dev::stream(qkv.device())));
    if (qkv.requires_grad() || (q_weight.defined() && q_weight.requires_grad()) || (k_weight.defined() && k_weight.requires_grad())) {
        out.set_requires_grad(true);
        out.set_grad_fn(new QkNormRopeGradFunction(qkv, q_weight, k_weight, call));
    }
    return out;
}

} // namespace gpu
