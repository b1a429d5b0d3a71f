// namespace gpu: softmax / log_softmax over kf_softmax_fwd / kf_softmax_bwd (softmax.h).
#include "softmax.h"

#include <cmath>

#include "device_api.h"
#include "row_view.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }

// dx from the kept result y and the incoming gradient
class SoftmaxGradFunction : public GradFunction {
public:
    SoftmaxGradFunction(int kind, float scale, const Tensor &x, const Tensor &y) : kind_(kind), scale_(scale), y_(y) { inputs = {x}; }
    std::vector<Tensor> backward(Tensor g) override {
        const int64_t V = y_.shape(-1);
        const RowView dy = rows_of(g);
        Tensor dx = empty(y_.sizes(), y_.dtype(), y_.device());
        if (dx.numel() > 0)
            DEV_CALL(kf_softmax_bwd(kind_, code(y_.dtype()), dy.rows, V, scale_, y_.data_ptr(), V, dy.t.data_ptr(), dy.ld, dx.data_ptr(), V,
                                    dev::stream(y_.device())));
        return {dx};
    }

private:
    int kind_;
    float scale_;
    Tensor y_;   // a second handle on the result's storage: the result itself would hold its own grad function alive
};

Tensor softmax_last(int kind, const Tensor &x, float scale) {
    const int64_t V = x.shape(-1);
    Tensor out = empty(x.sizes(), x.dtype(), x.device());
    const RowView vx = rows_of(x);
    if (out.numel() > 0)
        DEV_CALL(kf_softmax_fwd(kind, code(x.dtype()), vx.rows, V, scale, vx.t.data_ptr(), vx.ld, out.data_ptr(), V, dev::stream(x.device())));
    if (x.requires_grad()) {
        Tensor kept = out.as_strided(out.sizes(), out.strides(), out.storage_offset());
        out.set_requires_grad(true);
        out.set_grad_fn(new SoftmaxGradFunction(kind, scale, x, kept));
    }
    return out;
}

Tensor softmax_any(int kind, const char *who, const Tensor &x, int64_t dim, float scale) {
    CHECK_FAIL(x.defined(), who, " expects a tensor");
    CHECK_FAIL(x.dim() >= 1, who, " expects at least one dimension");
    CHECK_FAIL(x.dtype() == ScalarType::Float || x.dtype() == ScalarType::Half || x.dtype() == ScalarType::BFloat16, who,
               " supports float, half and bfloat16");
    const int nd = x.dim();
    CHECK_FAIL(dim >= -nd && dim < nd, who, ": dim ", dim, " out of range for ", nd, " dimensions");
    CHECK_FAIL(std::isfinite(scale) && scale > 0.f, who, ": scale ", scale, " must be finite and greater than 0");
    const int d = (int)(dim < 0 ? dim + nd : dim);
    if (d == nd - 1) return softmax_last(kind, x, scale);
    std::vector<int64_t> perm(nd);   // d and the last dimension change places: the permutation is its own inverse
    for (int i = 0; i < nd; ++i) perm[i] = i;
    std::swap(perm[d], perm[nd - 1]);
    return softmax_last(kind, x.permute(perm).contiguous(), scale).permute(perm);
}
} // namespace

Tensor softmax(const Tensor &x, int64_t dim, float scale) { return softmax_any(KF_SOFTMAX, "softmax", x, dim, scale); }
Tensor log_softmax(const Tensor &x, int64_t dim, float scale) { return softmax_any(KF_LOG_SOFTMAX, "log_softmax", x, dim, scale); }

} // namespace gpu
