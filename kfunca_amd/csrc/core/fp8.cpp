// namespace gpu: fp8_quantize, gemm_fp8 and linear_fp8 over kf_fp8_amax / kf_fp8_quantize / kf_gemm_fp8 (fp8.h).
#include "fp8.h"

#include "device_api.h"
#include "ops.h"
#include "row_view.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool float_dtype(ScalarType t) { return t == ScalarType::Float || t == ScalarType::Half || t == ScalarType::BFloat16; }
int64_t ceil16(int64_t n) { return (n + 15) / 16 * 16; }
const float *scale_ptr(const Tensor &s) { return static_cast<const float *>(s.data_ptr()); }

// Keeps x_t [K, ceil16(T)], w_t [K, N] (e4m3 bytes) and the two scales: dX = dy_q w_t^T contracts N, dW = dy_t x_t^T contracts ceil16(T)
// over the zero pads of both copies.
class LinearFp8GradFunction : public GradFunction {
public:
    LinearFp8GradFunction(const Tensor &x, const Tensor &w, const Tensor &x_t, const Tensor &w_t, const Tensor &sx, const Tensor &sw)
        : x_t_(x_t), w_t_(w_t), sx_(sx), sw_(sw) {
        inputs = {x, w};
    }
    std::vector<Tensor> backward(Tensor g) override {
        const Tensor &x = inputs[0], &w = inputs[1];
        CHECK_FAIL(g.dtype() == x.dtype() && g.device() == x.device(), "linear_fp8 backward: the upstream gradient must have the output's dtype and device");
        const Fp8Quantized dy = fp8_quantize(g, KF_FP8_E5M2, w.requires_grad());
        std::vector<Tensor> out(2);
        if (x.requires_grad()) out[0] = gemm_fp8(dy.q, w_t_, dy.scale_inv, sw_, KF_FP8_E5M2, KF_FP8_E4M3, x.dtype()).view(x.sizes());
        if (w.requires_grad()) out[1] = gemm_fp8(dy.qt, x_t_, dy.scale_inv, sx_, KF_FP8_E5M2, KF_FP8_E4M3, w.dtype());
        return out;
    }

private:
    Tensor x_t_, w_t_, sx_, sw_;
};
} // namespace

Fp8Quantized fp8_quantize(const Tensor &x, int fmt, bool transpose) {
    CHECK_FAIL(x.defined() && x.dim() >= 1, "fp8_quantize expects x [..., cols]");
    CHECK_FAIL(float_dtype(x.dtype()), "fp8_quantize supports float, half and bfloat16");
    CHECK_FAIL(fmt == KF_FP8_E4M3 || fmt == KF_FP8_E5M2, "fp8_quantize: unknown format ", fmt);
    const RowView v = rows_of(x);
    const int64_t rows = v.rows, cols = x.shape(-1), rows16 = ceil16(rows);
    const int device = x.device();
    void *st = dev::stream(device);
    Fp8Quantized r;
    r.q = empty({rows, cols}, ScalarType::Byte, device);
    if (transpose) r.qt = empty({cols, rows16}, ScalarType::Byte, device);
    r.scale_inv = empty({1}, ScalarType::Float, device);
    Tensor amax = empty({1}, ScalarType::Float, device);
    DEV_CALL(kf_fp8_amax(code(x.dtype()), rows, cols, v.ld, v.t.data_ptr(), static_cast<float *>(amax.data_ptr()), st));
    DEV_CALL(kf_fp8_quantize(code(x.dtype()), fmt, rows, cols, v.ld, v.t.data_ptr(), static_cast<const float *>(amax.data_ptr()), r.q.data_ptr(), cols,
                             transpose ? r.qt.data_ptr() : nullptr, rows16, static_cast<float *>(r.scale_inv.data_ptr()), st));
    return r;
}

Tensor gemm_fp8(const Tensor &a_q, const Tensor &b_q, const Tensor &scale_inv_a, const Tensor &scale_inv_b, int fmt_a, int fmt_b, ScalarType out_dtype) {
    CHECK_FAIL(a_q.defined() && b_q.defined() && a_q.dim() == 2 && b_q.dim() == 2, "gemm_fp8 expects a_q [M, K] and b_q [N, K]");
    CHECK_FAIL(a_q.dtype() == ScalarType::Byte && b_q.dtype() == ScalarType::Byte, "gemm_fp8: the operands are Byte tensors of FP8 codes");
    CHECK_FAIL(float_dtype(out_dtype), "gemm_fp8: out_dtype must be float, half or bfloat16");
    const int64_t M = a_q.shape(0), N = b_q.shape(0), K = a_q.shape(1);
    CHECK_FAIL(b_q.shape(1) == K, "gemm_fp8: a_q is [", M, ", ", K, "], b_q [", N, ", ", b_q.shape(1), "]: the contraction extents differ");
    CHECK_FAIL(K > 0 && K % 16 == 0, "gemm_fp8: K = ", K, " must be a positive multiple of 16");
    CHECK_FAIL(a_q.stride(1) == 1 && b_q.stride(1) == 1, "gemm_fp8: both operands must have unit stride along K");
    const int device = a_q.device();
    CHECK_FAIL(b_q.device() == device, "gemm_fp8: the operands must be on one device");
    for (const Tensor *s : {&scale_inv_a, &scale_inv_b})
        CHECK_FAIL(s->defined() && s->dtype() == ScalarType::Float && s->numel() == 1 && s->device() == device,
                   "gemm_fp8: a scale_inv must be one Float on the operands' device");
    Tensor out = empty({M, N}, out_dtype, device);
    const int64_t lda = M > 1 ? a_q.stride(0) : K, ldb = N > 1 ? b_q.stride(0) : K;
    DEV_CALL(kf_gemm_fp8(fmt_a, fmt_b, code(out_dtype), M, N, K, a_q.data_ptr(), lda, b_q.data_ptr(), ldb, scale_ptr(scale_inv_a), scale_ptr(scale_inv_b),
                         out.data_ptr(), N, dev::stream(device)));
    return out;
}

void linear_fp8_check_dims(int64_t K, int64_t N) {
    CHECK_FAIL(K > 0 && K % 16 == 0, "linear_fp8: K = ", K, " (x's last dim) must be a positive multiple of 16");
    CHECK_FAIL(N > 0 && N % 16 == 0, "linear_fp8: N = ", N, " (weight's rows) must be a positive multiple of 16");
}

Tensor linear_fp8(const Tensor &x, const Tensor &weight) {
    CHECK_FAIL(x.defined() && x.dim() >= 1, "linear_fp8 expects x [..., K]");
    CHECK_FAIL(weight.defined() && weight.dim() == 2, "linear_fp8 expects weight [N, K]");
    CHECK_FAIL(float_dtype(x.dtype()), "linear_fp8 supports float, half and bfloat16");
    CHECK_FAIL(weight.dtype() == x.dtype() && weight.device() == x.device(), "linear_fp8: x and weight must have one dtype and device");
    const int64_t K = x.shape(-1), N = weight.shape(0);
    CHECK_FAIL(weight.shape(1) == K, "linear_fp8: weight must be [N, K] with K = x's last dim ", K, ", got [", N, ", ", weight.shape(1), "]");
    linear_fp8_check_dims(K, N);
    CHECK_FAIL(x.numel() >= K, "linear_fp8: x has no rows");
    const bool need_grad = x.requires_grad() || weight.requires_grad();
    // the transposed copies exist only for the backward: w_t for dX, x_t for dW
    const Fp8Quantized xq = fp8_quantize(x, KF_FP8_E4M3, weight.requires_grad());
    const Fp8Quantized wq = fp8_quantize(weight, KF_FP8_E4M3, x.requires_grad());
    auto shape = x.sizes();
    shape.back() = N;
    Tensor out = gemm_fp8(xq.q, wq.q, xq.scale_inv, wq.scale_inv, KF_FP8_E4M3, KF_FP8_E4M3, x.dtype()).view(shape);
    if (need_grad) {
        out.set_requires_grad(true);
        out.set_grad_fn(new LinearFp8GradFunction(x, weight, xq.qt, wq.qt, xq.scale_inv, wq.scale_inv));
    }
    return out;
}

} // namespace gpu
