// namespace gpu: the chunked linear + cross-entropy loss (linear_ce.h, ops.h).
#include "linear_ce.h"

#include <algorithm>
#include <string>

#include "device_api.h"
#include "ops.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool is_16bit(ScalarType t) { return t == ScalarType::Half || t == ScalarType::BFloat16; }

// C[M, N] (float behind 16-bit operands when c_f32) = op(A) op(B) + beta C, straight through kf_gemm_ex
void product(ScalarType dt, bool ta, bool tb, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda, const void *B, int64_t ldb, float beta,
             void *C, int64_t ldc, bool c_f32, void *stream) {
    kf_gemm_epilogue e{};
    e.c_f32 = c_f32 ? 1 : 0;
    DEV_CALL(kf_gemm_ex(code(dt), ta ? 1 : 0, tb ? 1 : 0, M, N, K, 1.f, A, lda, B, ldb, beta, C, ldc, &e, stream));
}

// Holds the gradients the forward already computed, unscaled: backward(g) applies g (and the mean's 1 / count) with two kf_scale_cast calls.
class LinearCrossEntropyGradFunction : public GradFunction {
public:
    LinearCrossEntropyGradFunction(const Tensor &x, const Tensor &weight, const Tensor &dx, const Tensor &dwacc, const Tensor &count)
        : dx_(dx), dwacc_(dwacc), count_(count) {
        inputs = {x, weight};
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &x = inputs[0], &w = inputs[1];
        Tensor gc = g.dense();
        CHECK_FAIL(gc.dtype() == ScalarType::Float && gc.numel() == 1, "linear_cross_entropy backward: the upstream gradient must be one float");
        CHECK_FAIL(gc.device() == x.device(), "linear_cross_entropy backward: the upstream gradient is on device ", gc.device(), ", x on ", x.device());
        // the held gradients are scaled IN PLACE: a second pass over the same forward would scale them twice
        CHECK_FAIL(!consumed_, "linear_cross_entropy backward ran already for this forward: its gradients were scaled in place");
        consumed_ = true;
        void *st = dev::stream(x.device());
        const float *gp = static_cast<const float *>(gc.data_ptr());
        const float *cp = count_.defined() ? static_cast<const float *>(count_.data_ptr()) : nullptr;
        std::vector<Tensor> out(2);
        if (dx_.defined()) { // in place: dX already has x's dtype
            DEV_CALL(kf_scale_cast(code(x.dtype()), code(x.dtype()), dx_.numel(), dx_.data_ptr(), dx_.data_ptr(), gp, cp, st));
            out[0] = dx_;
        }
        if (dwacc_.defined()) { // the f32 accumulator -> the weight's dtype (f32: in place)
            Tensor dw = w.dtype() == ScalarType::Float ? dwacc_ : empty(w.sizes(), w.dtype(), w.device());
            DEV_CALL(kf_scale_cast(KF_F32, code(w.dtype()), dwacc_.numel(), dwacc_.data_ptr(), dw.data_ptr(), gp, cp, st));
            out[1] = dw;
        }
        return out;
    }

private:
    Tensor dx_, dwacc_, count_;
    bool consumed_ = false;
};
} // namespace

int64_t linear_ce_chunk_rows(int64_t chunk_rows) {
    if (chunk_rows == 0) return kLinearCeDefaultChunkRows;
    CHECK_FAIL(chunk_rows > 0 && chunk_rows % kLinearCeChunkQuantum == 0, "linear_cross_entropy: chunk_rows must be 0 (the default) or a positive multiple of ",
               kLinearCeChunkQuantum, ", got ", chunk_rows);
    return chunk_rows;
}

Tensor linear_cross_entropy(const Tensor &x, const Tensor &weight, const Tensor &target, int64_t ignore_index, int reduction, double label_smoothing,
                            double z_loss, int64_t chunk_rows) {
    CHECK_FAIL(reduction != KF_CE_NONE, "linear_cross_entropy: reduction 'none' is not supported - the gradient is computed in the forward, and only a "
                                        "scalar upstream gradient can scale it afterwards; use 'sum' or 'mean' (or cross_entropy on materialised logits)");
    CHECK_FAIL(reduction == KF_CE_SUM || reduction == KF_CE_MEAN, "linear_cross_entropy: unknown reduction ", reduction);
    CHECK_FAIL(x.defined() && x.dim() >= 1 && x.is_dense(), "linear_cross_entropy expects a contiguous x [..., d]");
    CHECK_FAIL(weight.defined() && weight.dim() == 2 && weight.is_dense(), "linear_cross_entropy expects a contiguous weight [V, d]");
    const ScalarType dt = x.dtype();
    CHECK_FAIL(dt == ScalarType::Float || is_16bit(dt), "linear_cross_entropy supports float, half and bfloat16");
    CHECK_FAIL(weight.dtype() == dt, "linear_cross_entropy: x and weight must share a dtype, got ", dt, " and ", weight.dtype());
    const int64_t d = x.shape(-1), V = weight.shape(0);
    CHECK_FAIL(d > 0 && V > 0 && weight.shape(1) == d, "linear_cross_entropy: weight must be [V, d] with d = x's last dim ", d, ", got [", weight.shape(0), ", ",
               weight.shape(1), "]");
    CHECK_FAIL(target.defined() && target.dtype() == ScalarType::Long, "linear_cross_entropy: target must be of type Long");
    auto lead = x.sizes();
    lead.pop_back();
    CHECK_FAIL(target.sizes() == lead, "linear_cross_entropy: target must have the shape of x without its last dim");
    const int device = x.device();
    CHECK_FAIL(weight.device() == device && target.device() == device, "linear_cross_entropy: x, weight and target must be on one device");
    CHECK_FAIL(label_smoothing >= 0.0 && label_smoothing <= 1.0, "linear_cross_entropy: label_smoothing must lie in [0, 1], got ", label_smoothing);
    CHECK_FAIL(z_loss >= 0.0 && z_loss < 1e30, "linear_cross_entropy: z_loss must be finite and not negative, got ", z_loss);
    const int64_t T = x.numel() / d;
    const int64_t C = std::min(linear_ce_chunk_rows(chunk_rows), (T + kLinearCeChunkQuantum - 1) / kLinearCeChunkQuantum * kLinearCeChunkQuantum);

    const bool h16 = is_16bit(dt), need_dx = x.requires_grad(), need_dw = weight.requires_grad(), need_grad = need_dx || need_dw;
    const int64_t es = x.element_size_in_bytes();
    const int64_t tile = h16 ? 128 : 64; // rows of a matrix-kernel tile: a ragged tail of T runs as its own small product
    void *st = dev::stream(device);
    Tensor t = target.dense();
    const int64_t *tp = static_cast<const int64_t *>(t.data_ptr());

    Tensor loss = empty({1}, ScalarType::Float, device);
    Tensor rowloss = empty({std::max<int64_t>(T, 1)}, ScalarType::Float, device);
    Tensor count = reduction == KF_CE_MEAN && need_grad ? empty({1}, ScalarType::Float, device) : Tensor();
    Tensor dx = need_dx ? empty(x.sizes(), dt, device) : Tensor();
    Tensor dwacc = need_dw ? (T > 0 ? empty({V, d}, ScalarType::Float, device) : zeros({V, d}, ScalarType::Float, device)) : Tensor();

    if (T > 0) {
        // the two chunk buffers, reused by every chunk: f32 logits, and the gradient in the operands' dtype (f32 operands: in place)
        Tensor logits = empty({C, V}, ScalarType::Float, device);
        Tensor dl = need_grad ? (h16 ? empty({C, V}, dt, device) : logits) : Tensor();
        size_t need = 0;
        for (int64_t n : {std::min(C, T), T % C}) {
            size_t b = 0;
            if (n > 0) DEV_CALL(kf_ce_fused_rows_workspace_bytes(n, V, &b));
            need = std::max(need, b);
        }
        utils::memory::DataPtr scratch;
        if (need) scratch = utils::memory::DeviceAllocator::GetInstance()->allocate(need, device);
        const char *xp = static_cast<const char *>(x.data_ptr());
        float *rl = static_cast<float *>(rowloss.data_ptr());
        bool first = true;
        for (int64_t r0 = 0; r0 < T; r0 += C) {
            const int64_t n = std::min(C, T - r0), whole = n / tile * tile;
            const int64_t parts[2][2] = {{0, whole}, {whole, n - whole}}; // (first row, rows): the whole-tile part and the ragged remainder
            for (const auto &p : parts)
                if (p[1] > 0)
                    product(dt, false, true, p[1], V, d, xp + (r0 + p[0]) * d * es, d, weight.data_ptr(), d, 0.f,
                            static_cast<float *>(logits.data_ptr()) + p[0] * V, V, h16, st);
            DEV_CALL(kf_ce_fused_rows(KF_F32, code(dt), n, V, V, logits.data_ptr(), tp + r0, ignore_index, (float)label_smoothing, (float)z_loss, rl + r0,
                                      nullptr, dl.defined() ? dl.data_ptr() : nullptr, V, scratch.get(), need, st));
            for (const auto &p : parts) {
                if (p[1] == 0 || !need_grad) continue;
                const char *dlp = static_cast<const char *>(dl.data_ptr()) + p[0] * V * es;
                if (need_dx) // dX_c = dlogits_c weight
                    product(dt, false, false, p[1], d, V, dlp, V, weight.data_ptr(), d, 0.f, static_cast<char *>(dx.data_ptr()) + (r0 + p[0]) * d * es, d,
                            false, st);
                if (need_dw) { // dWacc += dlogits_c^T x_c, unrounded
                    product(dt, true, false, V, d, p[1], dlp, V, xp + (r0 + p[0]) * d * es, d, first ? 0.f : 1.f, dwacc.data_ptr(), d, h16, st);
                    first = false;
                }
            }
        }
    }
    DEV_CALL(kf_ce_fused_reduce(static_cast<const float *>(rowloss.data_ptr()), tp, T, ignore_index, reduction == KF_CE_MEAN ? 1 : 0,
                                static_cast<float *>(loss.data_ptr()), count.defined() ? static_cast<float *>(count.data_ptr()) : nullptr, st));
    if (need_grad) {
        loss.set_requires_grad(true);
        loss.set_grad_fn(new LinearCrossEntropyGradFunction(x, weight, dx, dwacc, count));
    }
    return loss;
}

} // namespace gpu
