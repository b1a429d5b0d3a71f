// namespace gpu: linear attention with a scalar decay over kf_linear_attn_* (linear_attn.h).
#include "linear_attn.h"

#include <cmath>

#include "allocator.h"
#include "device_api.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }

// keeps q, k, v, g (contiguous) and runs the three backward kernels in one call; the workspace comes from the caching allocator
class LinearAttentionGradFunction : public GradFunction {
public:
    LinearAttentionGradFunction(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, float scale) : scale_(scale) { inputs = {q, k, v, g}; }
    std::vector<Tensor> backward(Tensor grad) override {
        const Tensor &q = inputs[0], &k = inputs[1], &v = inputs[2], &g = inputs[3];
        const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.dense(), go = grad.dense();
        const int64_t B = q.shape(0), H = q.shape(1), S = q.shape(2), D = q.shape(3);
        const int device = q.device();
        Tensor dq = empty(q.sizes(), q.dtype(), device), dk = empty(q.sizes(), q.dtype(), device), dv = empty(q.sizes(), q.dtype(), device);
        Tensor dg = empty(g.sizes(), ScalarType::Float, device);
        size_t need = 0;
        DEV_CALL(kf_linear_attn_bwd_workspace_bytes(code(q.dtype()), B, H, S, D, D, &need));
        utils::memory::DataPtr scratch = utils::memory::DeviceAllocator::GetInstance()->allocate(need, device);
        DEV_CALL(kf_linear_attn_bwd(code(q.dtype()), B, H, S, D, D, scale_, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                    static_cast<const float *>(gc.data_ptr()), go.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                    static_cast<float *>(dg.data_ptr()), scratch.get(), need, dev::stream(device)));
        return {dq, dk, dv, dg};
    }

private:
    float scale_;
};
} // namespace

Tensor linear_attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, std::optional<float> scale) {
    const char *who = "linear_attention";
    CHECK_FAIL(q.defined() && k.defined() && v.defined() && g.defined() && q.dim() == 4 && k.dim() == 4 && v.dim() == 4 && g.dim() == 3, who,
               " expects q, k, v [B, H, S, D] and g [B, H, S]");
    CHECK_FAIL(q.dtype() == ScalarType::Half || q.dtype() == ScalarType::BFloat16, who, " supports half and bfloat16 q, k, v");
    CHECK_FAIL(k.dtype() == q.dtype() && v.dtype() == q.dtype(), who, ": q, k and v must have one dtype");
    CHECK_FAIL(g.dtype() == ScalarType::Float, who, ": g must be float");
    const int64_t B = q.shape(0), H = q.shape(1), S = q.shape(2), D = q.shape(3);
    CHECK_FAIL(k.sizes() == q.sizes() && v.shape(0) == B && v.shape(1) == H && v.shape(2) == S, who, ": q, k and v must agree in B, H and S");
    CHECK_FAIL(v.shape(3) == D, who, ": Dk ", D, " != Dv ", v.shape(3), " is not supported");
    CHECK_FAIL(D == 64 || D == 128, who, ": head size ", D, " not supported (64, 128)");
    CHECK_FAIL(g.shape(0) == B && g.shape(1) == H && g.shape(2) == S, who, ": g must be [B, H, S]");
    CHECK_FAIL(B > 0 && H > 0 && S > 0, who, ": empty operands");
    const int device = q.device();
    CHECK_FAIL(k.device() == device && v.device() == device && g.device() == device, who, ": operands on different devices");
    const float sc = scale ? *scale : 1.f / std::sqrt((float)D);
    const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.dense();
    Tensor out = empty(q.sizes(), q.dtype(), device);
    DEV_CALL(kf_linear_attn_fwd(code(q.dtype()), B, H, S, D, D, sc, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), static_cast<const float *>(gc.data_ptr()),
                                out.data_ptr(), dev::stream(device)));
    if (q.requires_grad() || k.requires_grad() || v.requires_grad() || g.requires_grad()) {
        out.set_requires_grad(true);
        out.set_grad_fn(new LinearAttentionGradFunction(q, k, v, g, sc));
    }
    return out;
}

} // namespace gpu
