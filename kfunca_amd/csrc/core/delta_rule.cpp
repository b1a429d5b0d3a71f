// namespace gpu: the gated delta rule over kf_delta_rule_* (delta_rule.h).
#include "delta_rule.h"

#include <cmath>

#include "allocator.h"
#include "device_api.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
const float *fptr(const Tensor &t) { return t.defined() ? static_cast<const float *>(t.data_ptr()) : nullptr; }

// the checks both operators share; returns the scale that goes to the kernels
float check_operands(const char *who, const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, const Tensor &beta, const Tensor &state,
                     const char *state_name, std::optional<float> scale) {
    CHECK_FAIL(q.defined() && k.defined() && v.defined() && beta.defined() && q.dim() == 4 && k.dim() == 4 && v.dim() == 4 && beta.dim() == 3, who,
               " expects q, k, v [B, H, S, D] and beta [B, H, S]");
    CHECK_FAIL(q.dtype() == ScalarType::Half || q.dtype() == ScalarType::BFloat16, who, " supports half and bfloat16 q, k, v");
    CHECK_FAIL(k.dtype() == q.dtype() && v.dtype() == q.dtype(), who, ": q, k and v must have one dtype");
    const int64_t B = q.shape(0), H = q.shape(1), S = q.shape(2), D = q.shape(3);
    CHECK_FAIL(k.sizes() == q.sizes() && v.sizes() == q.sizes(), who, ": q, k and v must agree in shape (Dk != Dv is not supported)");
    CHECK_FAIL(D == 64 || D == 128, who, ": head size ", D, " not supported (64, 128)");
    CHECK_FAIL(B > 0 && H > 0 && S > 0, who, ": empty operands");
    const int device = q.device();
    CHECK_FAIL(k.device() == device && v.device() == device && beta.device() == device, who, ": operands on different devices");
    CHECK_FAIL(beta.dtype() == ScalarType::Float && beta.shape(0) == B && beta.shape(1) == H && beta.shape(2) == S, who, ": beta must be float [B, H, S]");
    if (g.defined()) {
        CHECK_FAIL(g.dtype() == ScalarType::Float && g.dim() == 3 && g.shape(0) == B && g.shape(1) == H && g.shape(2) == S && g.device() == device, who,
                   ": g must be float [B, H, S] on the operands' device");
    }
    if (state.defined()) {
        CHECK_FAIL(state.dim() == 4 && state.shape(0) == B && state.shape(1) == H && state.shape(2) == D && state.shape(3) == D, who, ": ", state_name,
                   " must be [B, H, D, D]");
        CHECK_FAIL(state.dtype() == ScalarType::Float, who, ": ", state_name, " must be float");
        CHECK_FAIL(state.device() == device, who, ": operands on different devices");
    }
    return scale ? *scale : 1.f / std::sqrt((float)D);
}
} // namespace

std::pair<Tensor, Tensor> gated_delta_rule(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, const Tensor &beta, std::optional<float> scale,
                                           const Tensor &initial_state, bool return_state) {
    const float sc = check_operands("gated_delta_rule", q, k, v, g, beta, initial_state, "initial_state", scale);
    const int64_t B = q.shape(0), H = q.shape(1), S = q.shape(2), D = q.shape(3);
    const int device = q.device();
    const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.defined() ? g.dense() : Tensor(), bc = beta.dense();
    const Tensor h0 = initial_state.defined() ? initial_state.dense() : Tensor();
    Tensor out = empty(q.sizes(), q.dtype(), device), hT;
    if (return_state) hT = empty({B, H, D, D}, ScalarType::Float, device);
    size_t need = 0;
    DEV_CALL(kf_delta_rule_fwd_workspace_bytes(code(q.dtype()), B, H, S, D, D, &need));
    utils::memory::DataPtr scratch = utils::memory::DeviceAllocator::GetInstance()->allocate(need, device);
    DEV_CALL(kf_delta_rule_fwd(code(q.dtype()), B, H, S, D, D, sc, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), fptr(gc), fptr(bc), fptr(h0), out.data_ptr(),
                               const_cast<float *>(fptr(hT)), scratch.get(), need, dev::stream(device)));
    return {out, hT};
}

Tensor gated_delta_rule_step(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, const Tensor &beta, Tensor &state, std::optional<float> scale) {
    const char *who = "gated_delta_rule_step";
    CHECK_FAIL(state.defined(), who, " expects a state [B, H, D, D]");
    const float sc = check_operands(who, q, k, v, g, beta, state, "state", scale);
    CHECK_FAIL(state.is_contiguous(), who, ": state is updated in place and must be contiguous");
    const int64_t B = q.shape(0), H = q.shape(1), T = q.shape(2), D = q.shape(3);
    const int device = q.device();
    const Tensor qc = q.dense(), kc = k.dense(), vc = v.dense(), gc = g.defined() ? g.dense() : Tensor(), bc = beta.dense();
    Tensor out = empty(q.sizes(), q.dtype(), device);
    DEV_CALL(kf_delta_rule_step(code(q.dtype()), B, H, T, D, D, sc, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), fptr(gc), fptr(bc),
                                static_cast<float *>(state.data_ptr()), out.data_ptr(), dev::stream(device)));
    return out;
}

} // namespace gpu
