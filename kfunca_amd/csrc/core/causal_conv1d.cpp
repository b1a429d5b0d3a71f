// namespace gpu: the causal depthwise conv1d over kf_causal_conv1d_* (causal_conv1d.h).
#include "causal_conv1d.h"

#include "allocator.h"
#include "device_api.h"
#include "row_view.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
const void *cptr(const Tensor &t) { return t.defined() ? t.data_ptr() : nullptr; }

// x as the kernel reads it: in place through its row stride when that is whole 16-byte packs from an aligned base, else a dense copy
RowView conv_rows(const Tensor &t) {
    const RowView v = rows_of(t);
    const int64_t pack = 16 / t.element_size_in_bytes();
    if (v.ld % pack == 0 && reinterpret_cast<uintptr_t>(v.t.data_ptr()) % 16 == 0) return v;
    Tensor d = t.dense();
    return {d, v.rows, t.shape(-1)};
}

int act_code(const char *who, const std::string &activation) {
    CHECK_FAIL(activation.empty() || activation == "silu", who, ": activation must be None or \"silu\", not \"", activation, "\"");
    return activation.empty() ? KF_CONV1D_ACT_NONE : KF_CONV1D_ACT_SILU;
}

// what both entries ask of x, weight and bias; returns K
int64_t check_operands(const char *who, const Tensor &x, const Tensor &weight, const Tensor &bias) {
    CHECK_FAIL(x.defined() && weight.defined() && x.dim() == 3 && weight.dim() == 2, who, " expects x [B, S, C] and weight [K, C]");
    CHECK_FAIL(x.dtype() == ScalarType::Float || x.dtype() == ScalarType::Half || x.dtype() == ScalarType::BFloat16, who,
               " supports float, half and bfloat16");
    const int64_t C = x.shape(2), K = weight.shape(0);
    CHECK_FAIL(x.shape(0) > 0 && x.shape(1) > 0 && C > 0, who, ": empty operands");
    CHECK_FAIL(weight.shape(1) == C && weight.dtype() == x.dtype() && weight.device() == x.device(), who, ": weight must be [K, ", C,
               "] in the dtype and on the device of x");
    CHECK_FAIL(K >= 2 && K <= 4, who, ": K ", K, " not supported (2, 3, 4)");
    CHECK_FAIL(C % (16 / x.element_size_in_bytes()) == 0, who, ": C ", C, " must be a multiple of ", 16 / x.element_size_in_bytes());
    if (bias.defined())
        CHECK_FAIL(bias.dim() == 1 && bias.shape(0) == C && bias.dtype() == x.dtype() && bias.device() == x.device(), who, ": bias must be [", C,
                   "] in the dtype and on the device of x");
    return K;
}

void check_state(const char *who, const char *name, const Tensor &s, const Tensor &x, int64_t K) {
    CHECK_FAIL(s.dim() == 3 && s.shape(0) == x.shape(0) && s.shape(1) == K - 1 && s.shape(2) == x.shape(2), who, ": ", name, " must be [B, K - 1, C]");
    CHECK_FAIL(s.dtype() == x.dtype() && s.device() == x.device(), who, ": ", name, " must have the dtype and the device of x");
}

// keeps x, weight (and bias and the initial state, when given) and runs the backward and its reduction in one call; the workspace comes
// from the caching allocator. As for linear attention, y and the returned state each get a node of this class: the y node takes dy with
// no d_hT, the state node takes d_hT with a zero dy. The backward is linear in (dy, d_hT), so the engine's sum of the two nodes'
// gradients is the gradient of both.
class CausalConv1dGradFunction : public GradFunction {
public:
    CausalConv1dGradFunction(const Tensor &x, const Tensor &weight, const Tensor &bias, const Tensor &h0, int act, bool of_state)
        : act_(act), has_bias_(bias.defined()), has_h0_(h0.defined()), of_state_(of_state) {
        inputs = {x, weight};
        if (has_bias_) inputs.push_back(bias);
        if (has_h0_) inputs.push_back(h0);
    }
    std::vector<Tensor> backward(Tensor grad) override {
        const Tensor &x = inputs[0];
        const Tensor w = inputs[1].dense(), bias = has_bias_ ? inputs[2].dense() : Tensor(), h0 = has_h0_ ? inputs[2 + has_bias_].dense() : Tensor();
        const int64_t B = x.shape(0), S = x.shape(1), C = x.shape(2), K = w.shape(0);
        const int device = x.device();
        const RowView vx = conv_rows(x), vdy = conv_rows(of_state_ ? zeros(x.sizes(), x.dtype(), device) : grad);
        const Tensor dhT = of_state_ ? grad.dense() : Tensor();
        Tensor dx = empty(x.sizes(), x.dtype(), device), dw = empty(w.sizes(), x.dtype(), device);
        Tensor dbias = has_bias_ ? empty({C}, x.dtype(), device) : Tensor(), dh0 = has_h0_ ? empty({B, K - 1, C}, x.dtype(), device) : Tensor();
        size_t need = 0;
        DEV_CALL(kf_causal_conv1d_bwd_workspace_bytes(code(x.dtype()), B, S, C, K, &need));
        utils::memory::DataPtr scratch = utils::memory::DeviceAllocator::GetInstance()->allocate(need, device);
        DEV_CALL(kf_causal_conv1d_bwd(code(x.dtype()), act_, B, S, C, K, vx.t.data_ptr(), vx.ld, w.data_ptr(), cptr(bias), cptr(h0), vdy.t.data_ptr(),
                                      vdy.ld, cptr(dhT), dx.data_ptr(), C, dw.data_ptr(), const_cast<void *>(cptr(dbias)),
                                      const_cast<void *>(cptr(dh0)), scratch.get(), need, dev::stream(device)));
        std::vector<Tensor> out = {dx, dw};
        if (has_bias_) out.push_back(dbias);
        if (has_h0_) out.push_back(dh0);
        return out;
    }

private:
    int act_;
    bool has_bias_, has_h0_, of_state_;
};
} // namespace

std::pair<Tensor, Tensor> causal_conv1d(const Tensor &x, const Tensor &weight, const Tensor &bias, const std::string &activation,
                                        const Tensor &initial_state, bool return_state) {
    const char *who = "causal_conv1d";
    const int act = act_code(who, activation);
    const int64_t K = check_operands(who, x, weight, bias);
    if (initial_state.defined()) check_state(who, "initial_state", initial_state, x, K);
    const int64_t B = x.shape(0), S = x.shape(1), C = x.shape(2);
    const int device = x.device();
    const RowView vx = conv_rows(x);
    const Tensor w = weight.dense(), bc = bias.defined() ? bias.dense() : Tensor(), h0 = initial_state.defined() ? initial_state.dense() : Tensor();
    Tensor y = empty(x.sizes(), x.dtype(), device), hT = return_state ? empty({B, K - 1, C}, x.dtype(), device) : Tensor();
    DEV_CALL(kf_causal_conv1d_fwd(code(x.dtype()), act, B, S, C, K, vx.t.data_ptr(), vx.ld, w.data_ptr(), cptr(bc), cptr(h0), y.data_ptr(), C,
                                  const_cast<void *>(cptr(hT)), dev::stream(device)));
    if (x.requires_grad() || weight.requires_grad() || (bias.defined() && bias.requires_grad()) ||
        (initial_state.defined() && initial_state.requires_grad())) {
        y.set_requires_grad(true);
        y.set_grad_fn(new CausalConv1dGradFunction(x, weight, bias, initial_state, act, false));
        if (return_state) {
            hT.set_requires_grad(true);
            hT.set_grad_fn(new CausalConv1dGradFunction(x, weight, bias, initial_state, act, true));
        }
    }
    return {y, hT};
}

Tensor causal_conv1d_step(const Tensor &x, const Tensor &weight, const Tensor &bias, Tensor &state, const std::string &activation) {
    const char *who = "causal_conv1d_step";
    const int act = act_code(who, activation);
    const int64_t K = check_operands(who, x, weight, bias);
    CHECK_FAIL(state.defined(), who, " expects a state [B, K - 1, C]");
    check_state(who, "state", state, x, K);
    CHECK_FAIL(state.is_contiguous(), who, ": state is updated in place and must be contiguous");
    const int64_t B = x.shape(0), T = x.shape(1), C = x.shape(2);
    CHECK_FAIL(T <= KF_CONV1D_STEP_MAX, who, ": T ", T, " > ", (int)KF_CONV1D_STEP_MAX, " tokens belong to causal_conv1d");
    const int device = x.device();
    const RowView vx = conv_rows(x);
    const Tensor w = weight.dense(), bc = bias.defined() ? bias.dense() : Tensor();
    Tensor y = empty(x.sizes(), x.dtype(), device);
    DEV_CALL(kf_causal_conv1d_fwd(code(x.dtype()), act, B, T, C, K, vx.t.data_ptr(), vx.ld, w.data_ptr(), cptr(bc), state.data_ptr(), y.data_ptr(), C,
                                  state.data_ptr(), dev::stream(device)));
    return y;
}

} // namespace gpu
