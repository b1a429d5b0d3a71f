// namespace gpu: moe_plan, moe_gate, moe_dispatch and moe_combine over the kf_moe_* entries (moe.h).
#include "moe.h"

#include "allocator.h"
#include "device_api.h"
#include "row_view.h"

namespace gpu {

using utils::memory::DataPtr;
using utils::memory::DeviceAllocator;

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool moe_dtype_ok(ScalarType t) { return t == ScalarType::Float || t == ScalarType::Half || t == ScalarType::BFloat16; }

const int32_t *i32(const Tensor &t) { return static_cast<const int32_t *>(t.data_ptr()); }
const int64_t *i64(const Tensor &t) { return static_cast<const int64_t *>(t.data_ptr()); }
// offsets[E] on the device: the number of live pairs
const int64_t *n_valid(const MoePlan &plan) { return i64(plan.offsets) + plan.E; }

// a plan as moe_plan builds it, on the operand's device
void check_plan(const char *op, const MoePlan &plan, int device) {
    const int64_t n = plan.T * plan.k;
    CHECK_FAIL(plan.T >= 0 && plan.k >= 1 && plan.E >= 1 && plan.offsets.defined() && plan.row_pair.defined() && plan.pair_row.defined() &&
                   plan.ids.defined(),
               op, ": the plan is empty (build it with moe_plan(ids, num_experts))");
    CHECK_FAIL(plan.offsets.dtype() == ScalarType::Long && plan.offsets.is_dense() && plan.offsets.numel() == plan.E + 1, op,
               ": plan.offsets must be a contiguous Long tensor of E + 1 = ", plan.E + 1, " entries");
    CHECK_FAIL(plan.row_pair.dtype() == ScalarType::Int && plan.row_pair.is_dense() && plan.row_pair.numel() == n, op,
               ": plan.row_pair must be a contiguous Int tensor of T k = ", n, " entries");
    CHECK_FAIL(plan.pair_row.dtype() == ScalarType::Int && plan.pair_row.is_dense() && plan.pair_row.numel() == n, op,
               ": plan.pair_row must be a contiguous Int tensor of T k = ", n, " entries");
    CHECK_FAIL(plan.ids.dtype() == ScalarType::Long && plan.ids.is_dense() && plan.ids.numel() == n, op,
               ": plan.ids must be a contiguous Long tensor of T k = ", n, " entries");
    CHECK_FAIL(plan.offsets.device() == device && plan.row_pair.device() == device && plan.pair_row.device() == device && plan.ids.device() == device, op,
               ": the plan must be on the operand's device");
}

class MoeGateGradFunction : public GradFunction {
public:
    MoeGateGradFunction(const Tensor &p, const MoePlan &plan, bool normalize, const RowView &vp, const Tensor &gate)
        : plan_(plan), normalize_(normalize), vp_(vp), gate_(gate) {
        inputs = {p};
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &p = inputs[0];
        const RowView dg = rows_of(g);
        Tensor dp = empty({plan_.T, plan_.E}, p.dtype(), p.device());
        if (plan_.T > 0)
            DEV_CALL(kf_moe_gate_bwd(code(p.dtype()), plan_.T, plan_.k, plan_.E, i64(plan_.ids), vp_.t.data_ptr(), vp_.ld, normalize_ ? 1 : 0,
                                     gate_.data_ptr(), plan_.k, dg.t.data_ptr(), dg.ld, dp.data_ptr(), plan_.E, dev::stream(p.device())));
        return {dp};
    }

private:
    MoePlan plan_;
    bool normalize_;
    RowView vp_;
    Tensor gate_;   // a second handle on the result's storage: the result itself would hold its own grad function alive
};

// dx[t] = sum_j dxs[pair_row[t, j]]: every sorted row holds a copy of a token's row, the dropped pairs' rows too
class MoeDispatchGradFunction : public GradFunction {
public:
    MoeDispatchGradFunction(const Tensor &x, const MoePlan &plan) : plan_(plan) { inputs = {x}; }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &x = inputs[0];
        const int64_t d = x.shape(1);
        const RowView dxs = rows_of(g);
        Tensor dx = empty({plan_.T, d}, x.dtype(), x.device());
        if (dx.numel() > 0)
            DEV_CALL(kf_moe_combine(code(x.dtype()), plan_.T, plan_.k, d, i32(plan_.pair_row), nullptr, nullptr, 0, dxs.t.data_ptr(), dxs.ld, dx.data_ptr(),
                                    d, dev::stream(x.device())));
        return {dx};
    }

private:
    MoePlan plan_;
};

class MoeCombineGradFunction : public GradFunction {
public:
    MoeCombineGradFunction(const Tensor &ys, const Tensor &gate, const MoePlan &plan, const RowView &vys, const RowView &vg)
        : plan_(plan), vys_(vys), vg_(vg), has_gate_(gate.defined()) {
        inputs = {ys};
        if (has_gate_) inputs.push_back(gate);
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &ys = inputs[0];
        const int64_t d = ys.shape(1), n = plan_.T * plan_.k;
        const RowView dy = rows_of(g);
        const bool want_gate = has_gate_ && inputs[1].requires_grad();
        std::vector<Tensor> out(inputs.size());
        Tensor dys = empty({n, d}, ys.dtype(), ys.device());   // the plan's tables are a permutation: every row is written
        Tensor dgate;
        if (want_gate) dgate = empty({plan_.T, plan_.k}, ys.dtype(), ys.device());
        if (plan_.T > 0 && (d > 0 || want_gate))
            DEV_CALL(kf_moe_combine_bwd(code(ys.dtype()), plan_.T, plan_.k, d, i32(plan_.pair_row), n_valid(plan_), has_gate_ ? vg_.t.data_ptr() : nullptr,
                                        has_gate_ ? vg_.ld : 0, want_gate ? vys_.t.data_ptr() : nullptr, vys_.ld, dy.t.data_ptr(), dy.ld, dys.data_ptr(), d,
                                        want_gate ? dgate.data_ptr() : nullptr, plan_.k, dev::stream(ys.device())));
        if (ys.requires_grad()) out[0] = dys;
        if (want_gate) out[1] = dgate;
        return out;
    }

private:
    MoePlan plan_;
    RowView vys_, vg_;
    bool has_gate_;
};
// dlogits from logits, ids and the incoming gradient: the row is recomputed, the gate is not kept
class MoeRouteGradFunction : public GradFunction {
public:
    MoeRouteGradFunction(const Tensor &logits, const Tensor &ids, int64_t k, int score, bool normalize, const RowView &vl)
        : ids_(ids), k_(k), score_(score), normalize_(normalize), vl_(vl) {
        inputs = {logits};
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &l = inputs[0];
        const int64_t T = l.shape(0), E = l.shape(1);
        const RowView dg = rows_of(g);
        Tensor dl = empty({T, E}, l.dtype(), l.device());
        if (T > 0)
            DEV_CALL(kf_moe_router_bwd(code(l.dtype()), T, E, k_, score_, normalize_ ? 1 : 0, vl_.t.data_ptr(), vl_.ld, i64(ids_), dg.t.data_ptr(), dg.ld,
                                       dl.data_ptr(), E, dev::stream(l.device())));
        return {dl};
    }

private:
    Tensor ids_;
    int64_t k_;
    int score_;
    bool normalize_;
    RowView vl_;
};

class MoeAuxLossGradFunction : public GradFunction {
public:
    MoeAuxLossGradFunction(const Tensor &logits, const MoePlan &plan, float balance_coef, float z_coef, const RowView &vl)
        : plan_(plan), balance_coef_(balance_coef), z_coef_(z_coef), vl_(vl) {
        inputs = {logits};
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &l = inputs[0];
        Tensor gc = g.dense();
        CHECK_FAIL(gc.dtype() == ScalarType::Float && gc.numel() == 1, "moe_aux_loss backward: unexpected gradient");
        Tensor dl = empty({plan_.T, plan_.E}, l.dtype(), l.device());
        DEV_CALL(kf_moe_aux_loss_bwd(code(l.dtype()), plan_.T, plan_.E, plan_.k, vl_.t.data_ptr(), vl_.ld, i64(plan_.offsets), balance_coef_, z_coef_,
                                     static_cast<const float *>(gc.data_ptr()), dl.data_ptr(), plan_.E, dev::stream(l.device())));
        return {dl};
    }

private:
    MoePlan plan_;
    float balance_coef_, z_coef_;
    RowView vl_;
};
} // namespace

std::pair<Tensor, Tensor> moe_route(const Tensor &logits, int64_t k, int score, bool normalize) {
    CHECK_FAIL(logits.defined() && logits.dim() == 2, "moe_route expects logits [T, E]");
    CHECK_FAIL(moe_dtype_ok(logits.dtype()), "moe_route supports float, half and bfloat16");
    CHECK_FAIL(score == KF_MOE_SCORE_SOFTMAX || score == KF_MOE_SCORE_SIGMOID, "moe_route: score must be softmax or sigmoid");
    const int64_t T = logits.shape(0), E = logits.shape(1);
    CHECK_FAIL(E >= 1 && E <= 1024, "moe_route: E = ", E, " experts, one wave holds a token's row (1 <= E <= 1024)");
    CHECK_FAIL(k >= 1 && k <= E && k <= 64, "moe_route: k = ", k, " must lie in [1, min(E, 64)] with E = ", E);
    const int device = logits.device();
    Tensor ids = empty({T, k}, ScalarType::Long, device);
    Tensor gate = empty({T, k}, logits.dtype(), device);
    const RowView vl = rows_of(logits);
    if (T > 0)
        DEV_CALL(kf_moe_router_fwd(code(logits.dtype()), T, E, k, score, normalize ? 1 : 0, vl.t.data_ptr(), vl.ld, static_cast<int64_t *>(ids.data_ptr()),
                                   gate.data_ptr(), k, dev::stream(device)));
    if (logits.requires_grad()) {
        gate.set_requires_grad(true);
        gate.set_grad_fn(new MoeRouteGradFunction(logits, ids, k, score, normalize, vl));
    }
    return {ids, gate};
}

Tensor moe_aux_loss(const Tensor &logits, const MoePlan &plan, double balance_coef, double z_coef, Tensor *parts) {
    CHECK_FAIL(logits.defined() && logits.dim() == 2, "moe_aux_loss expects logits [T, E]");
    CHECK_FAIL(moe_dtype_ok(logits.dtype()), "moe_aux_loss supports float, half and bfloat16");
    check_plan("moe_aux_loss", plan, logits.device());
    CHECK_FAIL(logits.shape(0) == plan.T && logits.shape(1) == plan.E, "moe_aux_loss: the plan was built for T = ", plan.T, ", E = ", plan.E, ", logits is [",
               logits.shape(0), ", ", logits.shape(1), "]");
    CHECK_FAIL(plan.T >= 1, "moe_aux_loss: no tokens");
    CHECK_FAIL(plan.E <= 1024 && plan.k <= 64 && plan.k <= plan.E, "moe_aux_loss: E = ", plan.E, ", k = ", plan.k, " (E <= 1024, k <= min(E, 64))");
    const int device = logits.device();
    Tensor loss = empty({1}, ScalarType::Float, device);
    if (parts) *parts = empty({2}, ScalarType::Float, device);
    const RowView vl = rows_of(logits);
    size_t need = 0;
    DEV_CALL(kf_moe_aux_loss_workspace_bytes(plan.T, plan.E, &need));
    DataPtr scratch;
    if (need) scratch = DeviceAllocator::GetInstance()->allocate(need, device);
    DEV_CALL(kf_moe_aux_loss_fwd(code(logits.dtype()), plan.T, plan.E, plan.k, vl.t.data_ptr(), vl.ld, i64(plan.offsets), (float)balance_coef, (float)z_coef,
                                 static_cast<float *>(loss.data_ptr()), parts ? static_cast<float *>(parts->data_ptr()) : nullptr, scratch.get(), need,
                                 dev::stream(device)));
    if (logits.requires_grad()) {
        loss.set_requires_grad(true);
        loss.set_grad_fn(new MoeAuxLossGradFunction(logits, plan, (float)balance_coef, (float)z_coef, vl));
    }
    return loss;
}

MoePlan moe_plan(const Tensor &ids, int64_t num_experts) {
    CHECK_FAIL(ids.defined() && ids.dtype() == ScalarType::Long && ids.dim() == 2, "moe_plan expects ids of type Long and shape [T, k] (the indices of a topk)");
    CHECK_FAIL(num_experts >= 1, "moe_plan: num_experts ", num_experts, " must be at least 1");
    MoePlan plan;
    plan.T = ids.shape(0);
    plan.k = ids.shape(1);
    plan.E = num_experts;
    CHECK_FAIL(plan.k >= 1, "moe_plan: ids must be [T, k >= 1]");
    CHECK_FAIL(plan.T == 0 || plan.k <= 0x7fffffffLL / plan.T, "moe_plan: T k = ", plan.T, " x ", plan.k, " pairs do not fit the 32-bit tables");
    const int device = ids.device();
    plan.ids = ids.dense();
    plan.offsets = empty({plan.E + 1}, ScalarType::Long, device);
    plan.row_pair = empty({plan.T * plan.k}, ScalarType::Int, device);
    plan.pair_row = empty({plan.T, plan.k}, ScalarType::Int, device);
    size_t bytes = 0;
    DEV_CALL(kf_moe_plan_workspace_bytes(plan.T, plan.k, plan.E, &bytes));
    DataPtr ws;
    if (bytes > 0) ws = DeviceAllocator::GetInstance()->allocate(bytes, device);
    DEV_CALL(kf_moe_plan(i64(plan.ids), plan.T, plan.k, plan.E, static_cast<int64_t *>(plan.offsets.data_ptr()),
                         static_cast<int32_t *>(plan.row_pair.data_ptr()), static_cast<int32_t *>(plan.pair_row.data_ptr()), bytes > 0 ? ws.get() : nullptr,
                         bytes, dev::stream(device)));
    return plan;
}

Tensor moe_gate(const Tensor &p, const MoePlan &plan, bool normalize) {
    CHECK_FAIL(p.defined() && p.dim() == 2, "moe_gate expects p [T, E]");
    CHECK_FAIL(moe_dtype_ok(p.dtype()), "moe_gate supports float, half and bfloat16");
    check_plan("moe_gate", plan, p.device());
    CHECK_FAIL(p.shape(0) == plan.T && p.shape(1) == plan.E, "moe_gate: the plan was built for T = ", plan.T, ", E = ", plan.E, ", p is [", p.shape(0), ", ",
               p.shape(1), "]");
    Tensor gate = empty({plan.T, plan.k}, p.dtype(), p.device());
    const RowView vp = rows_of(p);
    if (plan.T > 0)
        DEV_CALL(kf_moe_gate_fwd(code(p.dtype()), plan.T, plan.k, plan.E, i64(plan.ids), vp.t.data_ptr(), vp.ld, normalize ? 1 : 0, gate.data_ptr(), plan.k,
                                 dev::stream(p.device())));
    if (p.requires_grad()) {
        Tensor kept = gate.as_strided(gate.sizes(), gate.strides(), gate.storage_offset());
        gate.set_requires_grad(true);
        gate.set_grad_fn(new MoeGateGradFunction(p, plan, normalize, vp, kept));
    }
    return gate;
}

Tensor moe_dispatch(const Tensor &x, const MoePlan &plan) {
    CHECK_FAIL(x.defined() && x.dim() == 2, "moe_dispatch expects x [T, d]");
    CHECK_FAIL(moe_dtype_ok(x.dtype()), "moe_dispatch supports float, half and bfloat16");
    check_plan("moe_dispatch", plan, x.device());
    CHECK_FAIL(x.shape(0) == plan.T, "moe_dispatch: the plan was built for T = ", plan.T, ", x has ", x.shape(0), " rows");
    const int64_t d = x.shape(1), n = plan.T * plan.k;
    Tensor xs = empty({n, d}, x.dtype(), x.device());
    const RowView vx = rows_of(x);
    if (xs.numel() > 0)
        DEV_CALL(kf_moe_dispatch(code(x.dtype()), plan.T, plan.k, d, i32(plan.row_pair), vx.t.data_ptr(), vx.ld, xs.data_ptr(), d, dev::stream(x.device())));
    if (x.requires_grad()) {
        xs.set_requires_grad(true);
        xs.set_grad_fn(new MoeDispatchGradFunction(x, plan));
    }
    return xs;
}

Tensor moe_combine(const Tensor &ys, const MoePlan &plan, const Tensor &gate) {
    CHECK_FAIL(ys.defined() && ys.dim() == 2, "moe_combine expects ys [T k, d]");
    CHECK_FAIL(moe_dtype_ok(ys.dtype()), "moe_combine supports float, half and bfloat16");
    check_plan("moe_combine", plan, ys.device());
    const int64_t d = ys.shape(1), n = plan.T * plan.k;
    CHECK_FAIL(ys.shape(0) == n, "moe_combine: the plan was built for T k = ", plan.T, " x ", plan.k, " = ", n, " rows, ys has ", ys.shape(0));
    if (gate.defined()) {
        CHECK_FAIL(gate.dim() == 2 && gate.shape(0) == plan.T && gate.shape(1) == plan.k, "moe_combine: gate must be [T = ", plan.T, ", k = ", plan.k, "]");
        CHECK_FAIL(gate.dtype() == ys.dtype() && gate.device() == ys.device(), "moe_combine: ys and gate must have one dtype and device");
    }
    Tensor y = empty({plan.T, d}, ys.dtype(), ys.device());
    const RowView vys = rows_of(ys);
    const RowView vg = gate.defined() ? rows_of(gate) : RowView{Tensor(), 0, 0};
    if (y.numel() > 0)
        DEV_CALL(kf_moe_combine(code(ys.dtype()), plan.T, plan.k, d, i32(plan.pair_row), n_valid(plan), gate.defined() ? vg.t.data_ptr() : nullptr, vg.ld,
                                vys.t.data_ptr(), vys.ld, y.data_ptr(), d, dev::stream(ys.device())));
    if (ys.requires_grad() || (gate.defined() && gate.requires_grad())) {
        y.set_requires_grad(true);
        y.set_grad_fn(new MoeCombineGradFunction(ys, gate, plan, vys, vg));
    }
    return y;
}

} // namespace gpu
