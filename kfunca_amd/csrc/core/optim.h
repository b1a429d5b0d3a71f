// namespace gpu, the optimizer half of the operator API: torch.optim.AdamW as ONE fused device step over a whole model's parameters
// (kf_adamw_step), with torch.nn.utils.clip_grad_norm_ in the same call. No reference counterpart (the reference ends at p.grad()).
#pragma once

#include <cstdint>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "tensor.h"

namespace gpu {

class AdamW {
public:
    struct Group {
        std::vector<Tensor> params;
        double weight_decay;
    };
    // Every piece of state lives on the device and is allocated here: exp_avg and exp_avg_sq (f32, zero), the step counts (one f32
    // each, zero), the f32 master copies of 16-bit params (master_weights, initialised from the params), the lr scalar, the norm and the
    // clipping scratch. step() therefore allocates nothing and reads nothing back: it can be captured in a graph from the first call.
    // max_grad_norm <= 0: no clipping.
    AdamW(const std::vector<Group> &groups, double lr, double beta1, double beta2, double eps, double max_grad_norm, double grad_scale,
          bool master_weights);
    // One step over the params whose grad() is defined (the others and their state are left alone, as torch does). Returns the norm of
    // the (grad_scale-scaled) gradients before clipping - the optimizer's own device [1] f32 tensor, rewritten by every step - when
    // clipping, else an undefined tensor. The grads themselves are not rewritten.
    Tensor step();
    void zero_grad();                     // every param's grad dropped (torch's set_to_none)
    void set_lr(double lr);               // the device scalar, written in stream order; refused while a graph capture is open
    double lr() const { return lr_value_; }
    // (exp_avg, exp_avg_sq, step [1], master or undefined) of one of the params
    std::tuple<Tensor, Tensor, Tensor, Tensor> state(const Tensor &param) const;
    int64_t size() const { return (int64_t)params_.size(); }

private:
    std::vector<Tensor> params_, exp_avg_, exp_avg_sq_, master_;
    std::vector<float> weight_decay_;
    std::unordered_map<TensorImpl *, int> index_;
    Tensor steps_, lr_, norm_, workspace_;
    double lr_value_, beta1_, beta2_, eps_;
    float max_grad_norm_, grad_scale_;
    int device_ = 0;
};

} // namespace gpu
