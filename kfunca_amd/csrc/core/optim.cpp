// namespace gpu: the fused AdamW optimizer over kf_adamw_step, and Muon over kf_muon_* / kf_gemm_sym / kf_gemm (optim.h).
#include "optim.h"

#include <algorithm>
#include <cmath>

#include "allocator.h"
#include "device_api.h"
#include "ops.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool is_16bit(ScalarType t) { return t == ScalarType::Half || t == ScalarType::BFloat16; }
constexpr double kNsA = 3.4445, kNsB = -4.7750, kNsC = 2.0315; // the quintic Muon iterates: X <- (a I + b A + c A A) X
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

// ---- the symmetric product, Newton-Schulz and Muon ------------------------------------------------------------------------------------
namespace {

int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// The wide orientation of a [rows, cols] matrix and its extension to whole 128-tiles: zero rows and columns add nothing to any of the
// iteration's products and stay zero through it, and every product then runs on the matrix cores.
struct NsShape {
    int64_t m, n, mp, np;
    NsShape(int64_t rows, int64_t cols) : m(std::min(rows, cols)), n(std::max(rows, cols)), mp(up(m, 128)), np(up(n, 128)) {}
};

size_t ns_gemm_scratch(const NsShape &s) {
    size_t nt = 0, nn = 0; // A = X X^T (NT) and X <- (a I + B) X (NN)
    DEV_CALL(kf_gemm_workspace_bytes(code(ScalarType::BFloat16), 0, 1, s.mp, s.mp, s.np, &nt));
    DEV_CALL(kf_gemm_workspace_bytes(code(ScalarType::BFloat16), 0, 0, s.mp, s.np, s.mp, &nn));
    return std::max(nt, nn);
}

// `steps` iterations from the X in x[0]; the matrices are bf16: x[0], x[1] [mp, np], A, B [mp, mp]. Returns the index of the x that holds
// the result. Per step: A = X X^T on kf_gemm (NT), a I + b A + c A A on kf_gemm_sym (A A = A A^T; D = A and gamma spare a copy of A and,
// in the third product, a copy of X), then X <- that X on kf_gemm. The dispatch rule for A is measured: at every
// benchmarked shape kf_gemm's 256-tile kernel computes the full X X^T faster than kf_gemm_sym's 128-tile kernel computes its triangle.
int ns_iterate(const NsShape &s, int64_t steps, double a, double b, double c, void *const x[2], void *A, void *B, void *scratch, size_t scratch_bytes,
               int device) {
    const int bf = code(ScalarType::BFloat16);
    void *st = dev::stream(device);
    int cur = 0;
    for (int64_t k = 0; k < steps; ++k, cur ^= 1) {
        DEV_CALL(kf_gemm(bf, 0, 1, s.mp, s.mp, s.np, 1.f, x[cur], s.np, x[cur], s.np, 0.f, A, s.mp, KF_EPI_NONE, nullptr, scratch, scratch_bytes, st));
        DEV_CALL(kf_gemm_sym(bf, s.mp, s.mp, (float)c, A, s.mp, (float)b, A, s.mp, (float)a, B, s.mp, st));
        DEV_CALL(kf_gemm(bf, 0, 0, s.mp, s.np, s.mp, 1.f, B, s.mp, x[cur], s.np, 0.f, x[cur ^ 1], s.np, KF_EPI_NONE, nullptr, scratch, scratch_bytes, st));
    }
    return cur;
}

bool muon_dtype_ok(ScalarType t) { return t == ScalarType::Float || is_16bit(t); }

} // namespace

Tensor gemm_sym(const Tensor &x, float alpha, const Tensor &d, float beta, float gamma) {
    CHECK_FAIL(x.defined() && x.dim() == 2, "gemm_sym: x must be 2-D");
    CHECK_FAIL(muon_dtype_ok(x.dtype()), "gemm_sym: x must be float, half or bfloat16");
    CHECK_FAIL(x.is_dense(), "gemm_sym: x must be contiguous");
    const int64_t M = x.shape(0), K = x.shape(1);
    if (d.defined()) {
        CHECK_FAIL(d.dim() == 2 && d.shape(0) == M && d.shape(1) == M, "gemm_sym: d must be [", M, ", ", M, "]");
        CHECK_FAIL(d.dtype() == x.dtype() && d.device() == x.device() && d.is_dense(), "gemm_sym: d must be a contiguous tensor of x's dtype and device");
    }
    dev::set_device(x.device());
    Tensor out = empty({M, M}, x.dtype(), x.device());
    DEV_CALL(kf_gemm_sym(code(x.dtype()), M, K, alpha, x.numel() ? x.data_ptr() : nullptr, K, beta, d.defined() && M ? d.data_ptr() : nullptr, M, gamma,
                         M ? out.data_ptr() : nullptr, M, dev::stream(x.device())));
    return out;
}

Tensor newton_schulz(const Tensor &x, int64_t steps, double a, double b, double c) {
    CHECK_FAIL(x.defined() && x.dim() == 2, "newton_schulz: x must be 2-D");
    CHECK_FAIL(muon_dtype_ok(x.dtype()), "newton_schulz: x must be float, half or bfloat16");
    CHECK_FAIL(x.is_dense(), "newton_schulz: x must be contiguous");
    CHECK_FAIL(x.numel() > 0, "newton_schulz: x is empty");
    CHECK_FAIL(steps >= 0, "newton_schulz: steps ", steps, " < 0");
    const int device = x.device();
    dev::set_device(device);
    const int64_t rows = x.shape(0), cols = x.shape(1);
    const NsShape s(rows, cols);
    Tensor xs[2] = {empty({s.mp, s.np}, ScalarType::BFloat16, device), empty({s.mp, s.np}, ScalarType::BFloat16, device)};
    Tensor A = empty({s.mp, s.mp}, ScalarType::BFloat16, device), B = empty({s.mp, s.mp}, ScalarType::BFloat16, device);
    size_t pbytes = 0;
    DEV_CALL(kf_muon_prepare_workspace_bytes(rows, cols, &pbytes));
    Tensor partial = empty({(int64_t)pbytes}, ScalarType::Byte, device);
    const size_t gbytes = ns_gemm_scratch(s);
    Tensor scratch = gbytes ? empty({(int64_t)gbytes}, ScalarType::Byte, device) : Tensor();
    DEV_CALL(kf_muon_prepare(code(x.dtype()), rows, cols, x.data_ptr(), nullptr, 0.f, 0, 1.f, xs[0].data_ptr(), s.mp, s.np, s.np, partial.data_ptr(), pbytes,
                             dev::stream(device)));
    void *const xp[2] = {xs[0].data_ptr(), xs[1].data_ptr()};
    const int r = ns_iterate(s, steps, a, b, c, xp, A.data_ptr(), B.data_ptr(), gbytes ? scratch.data_ptr() : nullptr, gbytes, device);
    Tensor wide = xs[r].narrow(0, 0, s.m).narrow(1, 0, s.n);
    Tensor out = empty({rows, cols}, ScalarType::BFloat16, device);
    copy_(out, rows > cols ? wide.permute({1, 0}) : wide);
    return out;
}

Muon::Muon(const std::vector<Tensor> &params, double lr, double momentum, bool nesterov, int64_t ns_steps, double weight_decay, Adjust adjust,
           double grad_scale, bool master_weights)
    : lr_value_(lr), mu_((float)momentum), weight_decay_((float)weight_decay), grad_scale_((float)grad_scale), nesterov_(nesterov), ns_steps_(ns_steps),
      adjust_(adjust) {
    CHECK_FAIL(lr >= 0.0 && std::isfinite(lr), "Muon: invalid learning rate ", lr);
    CHECK_FAIL(momentum >= 0.0 && momentum < 1.0, "Muon: invalid momentum value ", momentum);
    CHECK_FAIL(ns_steps >= 0, "Muon: invalid ns_steps value ", ns_steps);
    CHECK_FAIL(weight_decay >= 0.0 && std::isfinite(weight_decay), "Muon: invalid weight_decay value ", weight_decay);
    CHECK_FAIL(std::isfinite(grad_scale), "Muon: grad_scale must be finite, got ", grad_scale);
    int64_t mp = 0, np = 0;
    size_t gbytes = 0;
    for (const Tensor &p : params) {
        CHECK_FAIL(p.defined() && !p.has_grad_fn(), "Muon: can't optimize a non-leaf tensor");
        CHECK_FAIL(p.dim() == 2, "Muon: params must be 2-D matrices, got a ", p.dim(), "-D tensor; put it in AdamW");
        CHECK_FAIL(muon_dtype_ok(p.dtype()), "Muon: params must be float, half or bfloat16");
        CHECK_FAIL(p.is_dense() && p.numel() > 0, "Muon: params must be contiguous and not empty");
        CHECK_FAIL(index_.emplace(p.impl(), (int)params_.size()).second, "Muon: a parameter appears more than once");
        if (!params_.empty()) CHECK_FAIL(p.device() == params_[0].device(), "Muon: all params must be on one device");
        params_.push_back(p);
        const NsShape s(p.shape(0), p.shape(1));
        mp = std::max(mp, s.mp);
        np = std::max(np, s.np);
        gbytes = std::max(gbytes, ns_gemm_scratch(s));
    }
    CHECK_FAIL(!params_.empty(), "Muon: optimizer got an empty parameter list");
    device_ = params_[0].device();
    dev::set_device(device_);
    for (const Tensor &p : params_) {
        momentum_.push_back(zeros(p.sizes(), ScalarType::Float, device_));
        master_.push_back(master_weights && is_16bit(p.dtype()) ? convert(p, ScalarType::Float) : Tensor());
    }
    // the largest wide matrix need not have the most rows: mp and np are maxima of their own, and every param uses a prefix of each buffer
    for (Tensor &x : x_) x = empty({mp * np}, ScalarType::BFloat16, device_);
    a_ = empty({mp * mp}, ScalarType::BFloat16, device_);
    b_ = empty({mp * mp}, ScalarType::BFloat16, device_);
    size_t pbytes = 0;
    DEV_CALL(kf_muon_prepare_workspace_bytes(mp, np, &pbytes));
    partial_ = empty({(int64_t)pbytes}, ScalarType::Byte, device_);
    if (gbytes) gemm_scratch_ = empty({(int64_t)gbytes}, ScalarType::Byte, device_);
    lr_ = empty({1}, ScalarType::Float, device_);
    fill_(lr_, any_t(lr));
}

void Muon::step() {
    void *st = dev::stream(device_);
    void *const xp[2] = {x_[0].data_ptr(), x_[1].data_ptr()};
    void *scratch = gemm_scratch_.defined() ? gemm_scratch_.data_ptr() : nullptr;
    const size_t scratch_bytes = gemm_scratch_.defined() ? (size_t)gemm_scratch_.numel() : 0;
    for (size_t i = 0; i < params_.size(); ++i) {
        Tensor &p = params_[i];
        Tensor *g = p.grad();
        if (!g || !g->defined()) continue; // no gradient this step: skipped, its state untouched
        CHECK_FAIL(g->numel() == p.numel() && g->is_dense(), "Muon: the grad of param ", i, " must be a contiguous tensor of its size");
        CHECK_FAIL(muon_dtype_ok(g->dtype()), "Muon: the grad of param ", i, " must be float, half or bfloat16");
        CHECK_FAIL(g->device() == device_, "Muon: the grad of param ", i, " is on another device");
        const int64_t rows = p.shape(0), cols = p.shape(1);
        const NsShape s(rows, cols);
        DEV_CALL(kf_muon_prepare(code(g->dtype()), rows, cols, g->data_ptr(), static_cast<float *>(momentum_[i].data_ptr()), mu_, nesterov_ ? 1 : 0, grad_scale_,
                                 xp[0], s.mp, s.np, s.np, partial_.data_ptr(), (size_t)partial_.numel(), st));
        const int r = ns_iterate(s, ns_steps_, kNsA, kNsB, kNsC, xp, a_.data_ptr(), b_.data_ptr(), scratch, scratch_bytes, device_);
        const double scale = adjust_ == Adjust::Spectral ? std::sqrt(std::max(1.0, (double)rows / (double)cols)) : 0.2 * std::sqrt((double)std::max(rows, cols));
        DEV_CALL(kf_muon_apply(code(p.dtype()), rows, cols, p.data_ptr(), master_[i].defined() ? static_cast<float *>(master_[i].data_ptr()) : nullptr, xp[r],
                               s.np, static_cast<const float *>(lr_.data_ptr()), weight_decay_, (float)scale, st));
    }
}

void Muon::zero_grad() {
    for (Tensor &p : params_) p.impl()->grad_.reset();
}

void Muon::set_lr(double lr) {
    CHECK_FAIL(lr >= 0.0 && std::isfinite(lr), "Muon: invalid learning rate ", lr);
    CHECK_FAIL(!utils::memory::DeviceAllocator::GetInstance()->capture_open(device_),
               "Muon.set_lr: a graph capture is open; set the rate between replays, outside the capture");
    fill_(lr_, any_t(lr));
    lr_value_ = lr;
}

std::tuple<Tensor, Tensor> Muon::state(const Tensor &param) const {
    auto it = index_.find(param.impl());
    CHECK_FAIL(it != index_.end(), "Muon.state: this tensor is not one of the optimizer's params");
    return {momentum_[it->second], master_[it->second]};
}

} // namespace gpu
