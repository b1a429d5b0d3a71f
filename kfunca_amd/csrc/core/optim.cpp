// namespace gpu: the fused AdamW optimizer over kf_adamw_step (optim.h).
#include "optim.h"

#include <cmath>

#include "allocator.h"
#include "device_api.h"
#include "ops.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool is_16bit(ScalarType t) { return t == ScalarType::Half || t == ScalarType::BFloat16; }
} // namespace

AdamW::AdamW(const std::vector<Group> &groups, double lr, double beta1, double beta2, double eps, double max_grad_norm, double grad_scale,
             bool master_weights)
    : lr_value_(lr), beta1_(beta1), beta2_(beta2), eps_(eps), max_grad_norm_((float)max_grad_norm), grad_scale_((float)grad_scale) {
    CHECK_FAIL(lr >= 0.0 && std::isfinite(lr), "AdamW: invalid learning rate ", lr);
    CHECK_FAIL(beta1 >= 0.0 && beta1 < 1.0, "AdamW: invalid beta parameter at index 0: ", beta1);
    CHECK_FAIL(beta2 >= 0.0 && beta2 < 1.0, "AdamW: invalid beta parameter at index 1: ", beta2);
    CHECK_FAIL(eps >= 0.0 && std::isfinite(eps), "AdamW: invalid epsilon value ", eps);
    CHECK_FAIL(std::isfinite(grad_scale), "AdamW: grad_scale must be finite, got ", grad_scale);
    CHECK_FAIL(!std::isnan(max_grad_norm), "AdamW: max_grad_norm is NaN");
    for (const Group &g : groups) {
        CHECK_FAIL(g.weight_decay >= 0.0 && std::isfinite(g.weight_decay), "AdamW: invalid weight_decay value ", g.weight_decay);
        for (const Tensor &p : g.params) {
            CHECK_FAIL(p.defined() && !p.has_grad_fn(), "AdamW: can't optimize a non-leaf tensor");
            CHECK_FAIL(p.dtype() == ScalarType::Float || is_16bit(p.dtype()), "AdamW: params must be float, half or bfloat16");
            CHECK_FAIL(p.is_dense(), "AdamW: params must be contiguous");
            CHECK_FAIL(index_.emplace(p.impl(), (int)params_.size()).second, "AdamW: some parameters appear in more than one parameter group");
            if (!params_.empty()) CHECK_FAIL(p.device() == params_[0].device(), "AdamW: all params must be on one device");
            params_.push_back(p);
            weight_decay_.push_back((float)g.weight_decay);
        }
    }
    CHECK_FAIL(!params_.empty(), "AdamW: optimizer got an empty parameter list");
    device_ = params_[0].device();
    dev::set_device(device_);
    for (const Tensor &p : params_) {
        exp_avg_.push_back(zeros(p.sizes(), ScalarType::Float, device_));
        exp_avg_sq_.push_back(zeros(p.sizes(), ScalarType::Float, device_));
        master_.push_back(master_weights && is_16bit(p.dtype()) ? convert(p, ScalarType::Float) : Tensor());
    }
    steps_ = zeros({(int64_t)params_.size()}, ScalarType::Float, device_);
    lr_ = empty({1}, ScalarType::Float, device_);
    fill_(lr_, any_t(lr));
    size_t need = 0;
    DEV_CALL(kf_adamw_workspace_bytes((int64_t)params_.size(), max_grad_norm_, &need));
    if (need) {
        workspace_ = empty({(int64_t)need}, ScalarType::Byte, device_);
        norm_ = zeros({1}, ScalarType::Float, device_);
    }
}

Tensor AdamW::step() {
    std::vector<kf_adamw_tensor> ts;
    ts.reserve(params_.size());
    float *steps = static_cast<float *>(steps_.data_ptr());
    for (size_t i = 0; i < params_.size(); ++i) {
        Tensor &p = params_[i];
        Tensor *g = p.grad();
        if (!g || !g->defined()) continue; // no gradient this step: skipped, its state untouched
        CHECK_FAIL(g->numel() == p.numel() && g->is_dense(), "AdamW: the grad of param ", i, " must be a contiguous tensor of its size");
        CHECK_FAIL(g->dtype() == ScalarType::Float || g->dtype() == p.dtype(), "AdamW: the grad of param ", i, " must be float or the param's dtype");
        CHECK_FAIL(g->device() == device_, "AdamW: the grad of param ", i, " is on another device");
        kf_adamw_tensor t{};
        t.numel = p.numel();
        t.param_dtype = code(p.dtype());
        t.grad_dtype = code(g->dtype());
        t.param = p.numel() ? p.data_ptr() : nullptr;
        t.grad = p.numel() ? g->data_ptr() : nullptr;
        t.master = master_[i].defined() && p.numel() ? static_cast<float *>(master_[i].data_ptr()) : nullptr;
        t.exp_avg = p.numel() ? static_cast<float *>(exp_avg_[i].data_ptr()) : nullptr;
        t.exp_avg_sq = p.numel() ? static_cast<float *>(exp_avg_sq_[i].data_ptr()) : nullptr;
        t.step = steps + i;
        t.weight_decay = weight_decay_[i];
        ts.push_back(t);
    }
    const bool clip = workspace_.defined();
    DEV_CALL(kf_adamw_step(ts.data(), (int64_t)ts.size(), beta1_, beta2_, eps_, static_cast<const float *>(lr_.data_ptr()), grad_scale_,
                           max_grad_norm_, clip ? static_cast<float *>(norm_.data_ptr()) : nullptr, clip ? workspace_.data_ptr() : nullptr,
                           clip ? (size_t)workspace_.numel() : 0, dev::stream(device_)));
    return clip ? norm_ : Tensor();
}

void AdamW::zero_grad() {
    for (Tensor &p : params_) p.impl()->grad_.reset();
}

void AdamW::set_lr(double lr) {
    CHECK_FAIL(lr >= 0.0 && std::isfinite(lr), "AdamW: invalid learning rate ", lr);
    CHECK_FAIL(!utils::memory::DeviceAllocator::GetInstance()->capture_open(device_),
               "AdamW.set_lr: a graph capture is open; set the rate between replays, outside the capture");
    fill_(lr_, any_t(lr));
    lr_value_ = lr;
}

std::tuple<Tensor, Tensor, Tensor, Tensor> AdamW::state(const Tensor &param) const {
    auto it = index_.find(param.impl());
    CHECK_FAIL(it != index_.end(), "AdamW.state: this tensor is not one of the optimizer's params");
    const int i = it->second;
    return {exp_avg_[i], exp_avg_sq_[i], steps_.narrow(0, i, 1), master_[i]};
}

} // namespace gpu
