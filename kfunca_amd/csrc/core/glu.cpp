// namespace gpu: gated activations over kf_glu_fwd / kf_glu_bwd (glu.h).
#include "glu.h"

#include "device_api.h"
#include "row_view.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool glu_dtype_ok(ScalarType t) { return t == ScalarType::Float || t == ScalarType::Half || t == ScalarType::BFloat16; }

char *at(const RowView &v, int64_t col) { return static_cast<char *>(v.t.data_ptr()) + col * v.t.element_size_in_bytes(); }

// The backward of h = act(gate) * up recomputed from the kept inputs. packed: inputs = {x}, x = gate | up, one [..., 2F] gradient;
// otherwise inputs = {gate, up} or, ungated, {x}.
class GluGradFunction : public GradFunction {
public:
    GluGradFunction(int act, std::vector<Tensor> in, const RowView &gate, const RowView &up, bool packed, int64_t F)
        : act_(act), gate_(gate), up_(up), packed_(packed), F_(F) {
        inputs = std::move(in);
    }
    std::vector<Tensor> backward(Tensor g) override {
        const RowView dh = rows_of(g);
        const Tensor &x = inputs[0];
        void *st = dev::stream(x.device());
        if (packed_) {
            Tensor dx = empty(x.sizes(), x.dtype(), x.device());
            char *p = static_cast<char *>(dx.data_ptr());
            DEV_CALL(kf_glu_bwd(act_, code(x.dtype()), gate_.rows, F_, at(gate_, 0), gate_.ld, at(gate_, F_), gate_.ld, at(dh, 0), dh.ld, p, 2 * F_,
                                p + F_ * x.element_size_in_bytes(), 2 * F_, st));
            return {dx};
        }
        Tensor dgate = empty(x.sizes(), x.dtype(), x.device());
        if (!up_.t.defined()) {
            DEV_CALL(kf_glu_bwd(act_, code(x.dtype()), gate_.rows, F_, at(gate_, 0), gate_.ld, nullptr, 0, at(dh, 0), dh.ld, dgate.data_ptr(), F_, nullptr,
                                0, st));
            return {dgate};
        }
        Tensor dup = empty(inputs[1].sizes(), x.dtype(), x.device());
        DEV_CALL(kf_glu_bwd(act_, code(x.dtype()), gate_.rows, F_, at(gate_, 0), gate_.ld, at(up_, 0), up_.ld, at(dh, 0), dh.ld, dgate.data_ptr(), F_,
                            dup.data_ptr(), F_, st));
        return {inputs[0].requires_grad() ? dgate : Tensor(), inputs[1].requires_grad() ? dup : Tensor()};
    }

private:
    int act_;
    RowView gate_, up_;
    bool packed_;
    int64_t F_;
};

void check_act(int act, const char *who) {
    CHECK_FAIL(act == KF_ACT_SILU || act == KF_ACT_GELU_TANH || act == KF_ACT_GELU_ERF, who, ": unknown activation ", act);
}
} // namespace

Tensor glu(int act, const Tensor &gate, const Tensor &up) {
    check_act(act, "glu");
    CHECK_FAIL(gate.defined() && gate.dim() >= 1, "glu expects gate [..., F] (or the packed [..., 2F] without up)");
    CHECK_FAIL(glu_dtype_ok(gate.dtype()), "glu supports float, half and bfloat16");
    const bool packed = !up.defined();
    if (packed) CHECK_FAIL(gate.shape(-1) % 2 == 0, "glu: the packed width ", gate.shape(-1), " must be even (gate | up)");
    else CHECK_FAIL(up.sizes() == gate.sizes() && up.dtype() == gate.dtype() && up.device() == gate.device(),
                    "glu: gate and up must have one shape, dtype and device");
    const int64_t F = packed ? gate.shape(-1) / 2 : gate.shape(-1);
    std::vector<int64_t> shape = gate.sizes();
    shape.back() = F;
    Tensor out = empty(shape, gate.dtype(), gate.device());
    const RowView vg = rows_of(gate), vu = packed ? RowView{} : rows_of(up);
    if (out.numel() > 0)
        DEV_CALL(kf_glu_fwd(act, code(gate.dtype()), vg.rows, F, at(vg, 0), vg.ld, packed ? at(vg, F) : at(vu, 0), packed ? vg.ld : vu.ld,
                            out.data_ptr(), F, dev::stream(gate.device())));
    if (gate.requires_grad() || (!packed && up.requires_grad())) {
        out.set_requires_grad(true);
        out.set_grad_fn(new GluGradFunction(act, packed ? std::vector<Tensor>{gate} : std::vector<Tensor>{gate, up}, vg, vu, packed, F));
    }
    return out;
}

Tensor activation(int act, const Tensor &x) {
    check_act(act, "activation");
    CHECK_FAIL(x.defined() && x.dim() >= 1, "activation expects x [..., F]");
    CHECK_FAIL(glu_dtype_ok(x.dtype()), "activation supports float, half and bfloat16");
    const int64_t F = x.shape(-1);
    Tensor out = empty(x.sizes(), x.dtype(), x.device());
    const RowView vx = rows_of(x);
    if (out.numel() > 0)
        DEV_CALL(kf_glu_fwd(act, code(x.dtype()), vx.rows, F, at(vx, 0), vx.ld, nullptr, 0, out.data_ptr(), F, dev::stream(x.device())));
    if (x.requires_grad()) {
        out.set_requires_grad(true);
        out.set_grad_fn(new GluGradFunction(act, {x}, vx, RowView{}, false, F));
    }
    return out;
}

} // namespace gpu
