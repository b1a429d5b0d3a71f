// namespace gpu: linear attention with a scalar decay over kf_linear_attn_* (linear_attn.h).
#include "linear_attn.h"

#include <cmath>

#include "allocator.h"
#include "device_api.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
const float *fptr(const Tensor &t) { return t.defined() ? static_cast<const float *>(t.data_ptr()) : nullptr; }

// keeps q, k, v, g (and the initial state, when there is one) and runs the three backward kernels in one call; the workspace comes
// from the caching allocator. The engine's nodes have one output each, so with a returned state o and the final state each get a node
// of this class: the o node (of_state false) takes d_o with no d_hT, the state node takes d_hT with a zero d_o. The backward is linear
// in (d_o, d_hT), so the engine's sum of the two nodes' gradients is the gradient of both.
class LinearAttentionGradFunction : public GradFunction {
public:
    LinearAttentionGradFunction(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, const Tensor &h0, float scale, bool of_state)
        : scale_(scale), of_state_(of_state) {
        inputs = {q, k, v, g};
        if (h0.defined()) inputs.push_back(h0);
    }
    std::vector<Tensor> backward(Tensor grad) override {
        const Tensor &q = inputs[0], &k = inputs[1], &v = inputs[2], &g = inputs[3];
        const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.dense(), h0 = inputs.size() > 4 ? inputs[4].dense() : Tensor();
        const int64_t B = q.shape(0), H = q.shape(1), S = q.shape(2), D = q.shape(3);
        const int device = q.device();
        const Tensor go = of_state_ ? zeros(q.sizes(), q.dtype(), device) : grad.dense(), dhT = of_state_ ? grad.dense() : Tensor();
        Tensor dq = empty(q.sizes(), q.dtype(), device), dk = empty(q.sizes(), q.dtype(), device), dv = empty(q.sizes(), q.dtype(), device);
        Tensor dg = empty(g.sizes(), ScalarType::Float, device);
        Tensor dh0 = h0.defined() && inputs[4].requires_grad() ? empty(h0.sizes(), ScalarType::Float, device) : Tensor();
        size_t need = 0;
        if (!h0.defined() && !of_state_) { // no state anywhere: the stateless entries
            DEV_CALL(kf_linear_attn_bwd_workspace_bytes(code(q.dtype()), B, H, S, D, D, &need));
            utils::memory::DataPtr scratch = utils::memory::DeviceAllocator::GetInstance()->allocate(need, device);
            DEV_CALL(kf_linear_attn_bwd(code(q.dtype()), B, H, S, D, D, scale_, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                        static_cast<const float *>(gc.data_ptr()), go.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                        static_cast<float *>(dg.data_ptr()), scratch.get(), need, dev::stream(device)));
            return {dq, dk, dv, dg};
        }
        DEV_CALL(kf_linear_attn_state_bwd_workspace_bytes(code(q.dtype()), B, H, S, D, D, &need));
        utils::memory::DataPtr scratch = utils::memory::DeviceAllocator::GetInstance()->allocate(need, device);
        DEV_CALL(kf_linear_attn_state_bwd(code(q.dtype()), B, H, S, D, D, scale_, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                          static_cast<const float *>(gc.data_ptr()), fptr(h0), go.data_ptr(), fptr(dhT), dq.data_ptr(), dk.data_ptr(),
                                          dv.data_ptr(), static_cast<float *>(dg.data_ptr()), const_cast<float *>(fptr(dh0)), scratch.get(), need,
                                          dev::stream(device)));
        std::vector<Tensor> out = {dq, dk, dv, dg};
        if (h0.defined()) out.push_back(dh0);
        return out;
    }

private:
    float scale_;
    bool of_state_;
};

void check_state(const char *who, const char *name, const Tensor &s, int64_t B, int64_t H, int64_t D, int device) {
    CHECK_FAIL(s.dim() == 4 && s.shape(0) == B && s.shape(1) == H && s.shape(2) == D && s.shape(3) == D, who, ": ", name, " must be [B, H, D, D]");
    CHECK_FAIL(s.dtype() == ScalarType::Float, who, ": ", name, " must be float");
    CHECK_FAIL(s.device() == device, who, ": operands on different devices");
}
} // namespace

std::pair<Tensor, Tensor> linear_attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, std::optional<float> scale,
                                           const Tensor &initial_state, bool return_state) {
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
    if (initial_state.defined()) check_state(who, "initial_state", initial_state, B, H, D, device);
    const float sc = scale ? *scale : 1.f / std::sqrt((float)D);
    const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.dense(), h0 = initial_state.defined() ? initial_state.dense() : Tensor();
    Tensor out = empty(q.sizes(), q.dtype(), device), hT;
    if (!h0.defined() && !return_state) {
        DEV_CALL(kf_linear_attn_fwd(code(q.dtype()), B, H, S, D, D, sc, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), static_cast<const float *>(gc.data_ptr()),
                                    out.data_ptr(), dev::stream(device)));
    } else {
        if (return_state) hT = empty({B, H, D, D}, ScalarType::Float, device);
        DEV_CALL(kf_linear_attn_state_fwd(code(q.dtype()), B, H, S, D, D, sc, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                          static_cast<const float *>(gc.data_ptr()), fptr(h0), out.data_ptr(), const_cast<float *>(fptr(hT)),
                                          dev::stream(device)));
    }
    if (q.requires_grad() || k.requires_grad() || v.requires_grad() || g.requires_grad() || (initial_state.defined() && initial_state.requires_grad())) {
        out.set_requires_grad(true);
        out.set_grad_fn(new LinearAttentionGradFunction(q, k, v, g, initial_state, sc, false));
        if (return_state) {
            hT.set_requires_grad(true);
            hT.set_grad_fn(new LinearAttentionGradFunction(q, k, v, g, initial_state, sc, true));
        }
    }
    return {out, hT};
}

Tensor linear_attention_step(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, Tensor &state, std::optional<float> scale) {
    const char *who = "linear_attention_step";
    CHECK_FAIL(q.defined() && k.defined() && v.defined() && g.defined() && state.defined() && q.dim() == 4 && k.dim() == 4 && v.dim() == 4 && g.dim() == 3,
               who, " expects q, k, v [B, H, T, D], g [B, H, T] and state [B, H, D, D]");
    CHECK_FAIL(q.dtype() == ScalarType::Half || q.dtype() == ScalarType::BFloat16, who, " supports half and bfloat16 q, k, v");
    CHECK_FAIL(k.dtype() == q.dtype() && v.dtype() == q.dtype(), who, ": q, k and v must have one dtype");
    CHECK_FAIL(g.dtype() == ScalarType::Float, who, ": g must be float");
    const int64_t B = q.shape(0), H = q.shape(1), T = q.shape(2), D = q.shape(3);
    CHECK_FAIL(k.sizes() == q.sizes() && v.sizes() == q.sizes(), who, ": q, k and v must agree in shape (Dk != Dv is not supported)");
    CHECK_FAIL(D == 64 || D == 128, who, ": head size ", D, " not supported (64, 128)");
    CHECK_FAIL(g.shape(0) == B && g.shape(1) == H && g.shape(2) == T, who, ": g must be [B, H, T]");
    CHECK_FAIL(B > 0 && H > 0 && T > 0, who, ": empty operands");
    const int device = q.device();
    CHECK_FAIL(k.device() == device && v.device() == device && g.device() == device, who, ": operands on different devices");
    check_state(who, "state", state, B, H, D, device);
    CHECK_FAIL(state.is_contiguous(), who, ": state is updated in place and must be contiguous");
    const float sc = scale ? *scale : 1.f / std::sqrt((float)D);
    const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.dense();
    Tensor out = empty(q.sizes(), q.dtype(), device);
    DEV_CALL(kf_linear_attn_step(code(q.dtype()), B, H, T, D, D, sc, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), static_cast<const float *>(gc.data_ptr()),
                                 static_cast<float *>(state.data_ptr()), out.data_ptr(), dev::stream(device)));
    return out;
}

} // namespace gpu
