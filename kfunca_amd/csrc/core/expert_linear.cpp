// namespace gpu: segment_offsets and expert_linear over kf_segment_offsets / kf_gemm_segmented / kf_gemm_segmented_wgrad (expert_linear.h).
#include "expert_linear.h"

#include "allocator.h"
#include "device_api.h"
#include "ops.h"
#include "row_view.h"

namespace gpu {

using utils::memory::DataPtr;
using utils::memory::DeviceAllocator;

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool expert_dtype_ok(ScalarType t) { return t == ScalarType::Float || t == ScalarType::Half || t == ScalarType::BFloat16; }

struct Scratch {
    DataPtr ptr;
    size_t bytes = 0;
};
Scratch plan_scratch(ScalarType dt, int64_t T, int64_t E, int device) {
    Scratch s;
    DEV_CALL(kf_gemm_segmented_workspace_bytes(code(dt), T, E, &s.bytes));
    s.ptr = DeviceAllocator::GetInstance()->allocate(s.bytes, device);
    return s;
}

// Where dw is written: the bucket slot of a bucketed leaf whose gradient starts empty, handed out once per backward pass (GradSink::take_slot,
// as gemm's weight gradient takes it) when the slot has the weight's dtype; a fresh tensor otherwise.
Tensor dw_target(const Tensor &w) {
    TensorImpl *wi = w.impl();
    if (!w.has_grad_fn())
        if (std::shared_ptr<GradSink> sink = wi->sink_.lock())
            if (!wi->grad_ && sink->slot(wi).dtype() == w.dtype())
                if (Tensor s = sink->take_slot(wi); s.defined()) return s;
    return empty(w.sizes(), w.dtype(), w.device());
}

class ExpertLinearGradFunction : public GradFunction {
public:
    ExpertLinearGradFunction(const Tensor &x, const Tensor &w, const Tensor &offsets, const RowView &vx) : offsets_(offsets), vx_(vx) { inputs = {x, w}; }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &x = inputs[0], &w = inputs[1];
        const int64_t E = w.shape(0), Din = w.shape(1), Dout = w.shape(2), T = vx_.rows;
        const RowView dy = rows_of(g);
        const int64_t *off = static_cast<const int64_t *>(offsets_.data_ptr());
        void *st = dev::stream(x.device());
        const Scratch ws = plan_scratch(x.dtype(), T, E, x.device());
        std::vector<Tensor> out(2);
        if (x.requires_grad()) {
            out[0] = empty(x.sizes(), x.dtype(), x.device());
            if (T > 0)
                DEV_CALL(kf_gemm_segmented(code(x.dtype()), 1, T, Din, Dout, E, off, 1.f, dy.t.data_ptr(), dy.ld, w.data_ptr(), Dout, Din * Dout, 0.f,
                                           out[0].data_ptr(), Din, ws.ptr.get(), ws.bytes, st));
        }
        if (w.requires_grad()) {
            Tensor dw = T > 0 ? dw_target(w) : zeros(w.sizes(), w.dtype(), w.device());
            if (T > 0)
                DEV_CALL(kf_gemm_segmented_wgrad(code(x.dtype()), T, Din, Dout, E, off, 1.f, vx_.t.data_ptr(), vx_.ld, dy.t.data_ptr(), dy.ld, 0.f,
                                                 dw.data_ptr(), Dout, Din * Dout, ws.ptr.get(), ws.bytes, st));
            // a bucket that keeps another dtype (float behind 16-bit weights) receives the rounded gradient in its own dtype
            if (!w.has_grad_fn())
                if (std::shared_ptr<GradSink> sink = w.impl()->sink_.lock())
                    if (ScalarType sd = sink->slot(w.impl()).dtype(); sd != dw.dtype()) dw = convert(dw, sd);
            out[1] = dw;
        }
        return out;
    }

private:
    Tensor offsets_;
    RowView vx_;
};
} // namespace

Tensor segment_offsets(const Tensor &sorted_ids, int64_t num_experts) {
    CHECK_FAIL(sorted_ids.defined() && sorted_ids.dtype() == ScalarType::Long, "segment_offsets expects a Long tensor of ascending expert ids");
    CHECK_FAIL(num_experts >= 1, "segment_offsets: num_experts ", num_experts, " must be at least 1");
    Tensor ids = sorted_ids.dense();
    Tensor out = empty({num_experts + 1}, ScalarType::Long, sorted_ids.device());
    DEV_CALL(kf_segment_offsets(static_cast<const int64_t *>(ids.data_ptr()), ids.numel(), num_experts, static_cast<int64_t *>(out.data_ptr()),
                                dev::stream(sorted_ids.device())));
    return out;
}

Tensor expert_linear(const Tensor &x, const Tensor &w, const Tensor &offsets) {
    CHECK_FAIL(x.defined() && x.dim() == 2, "expert_linear expects x [T, Din]");
    CHECK_FAIL(w.defined() && w.dim() == 3 && w.is_dense(), "expert_linear expects a contiguous w [E, Din, Dout]");
    CHECK_FAIL(expert_dtype_ok(x.dtype()), "expert_linear supports float, half and bfloat16");
    CHECK_FAIL(w.dtype() == x.dtype() && w.device() == x.device(), "expert_linear: x and w must have one dtype and device");
    const int64_t T = x.shape(0), Din = x.shape(1), E = w.shape(0), Dout = w.shape(2);
    CHECK_FAIL(E >= 1 && Din >= 1 && Dout >= 1 && w.shape(1) == Din, "expert_linear: w must be [E >= 1, Din = ", Din, ", Dout >= 1]");
    CHECK_FAIL(offsets.defined() && offsets.dtype() == ScalarType::Long && offsets.is_dense() && offsets.numel() == E + 1 && offsets.device() == x.device(),
               "expert_linear: offsets must be a contiguous Long tensor of E + 1 = ", E + 1, " entries on x's device");
    Tensor out = empty({T, Dout}, x.dtype(), x.device());
    const RowView vx = rows_of(x);
    if (T > 0) {
        const Scratch ws = plan_scratch(x.dtype(), T, E, x.device());
        DEV_CALL(kf_gemm_segmented(code(x.dtype()), 0, T, Dout, Din, E, static_cast<const int64_t *>(offsets.data_ptr()), 1.f, vx.t.data_ptr(), vx.ld,
                                   w.data_ptr(), Dout, Din * Dout, 0.f, out.data_ptr(), Dout, ws.ptr.get(), ws.bytes, dev::stream(x.device())));
    }
    if (x.requires_grad() || w.requires_grad()) {
        out.set_requires_grad(true);
        out.set_grad_fn(new ExpertLinearGradFunction(x, w, offsets, vx));
    }
    return out;
}

} // namespace gpu
