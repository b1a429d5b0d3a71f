// namespace gpu: rotary position embeddings over kf_rope (rope.h).
#include "rope.h"

#include "device_api.h"

namespace gpu {

namespace {
int code(ScalarType t) { return static_cast<int>(t); }
bool rope_dtype_ok(ScalarType t) { return t == ScalarType::Float || t == ScalarType::Half || t == ScalarType::BFloat16; }

// what one kf_rope call over [B, H, S, D] needs besides the operands
struct RopeCall {
    int64_t B, H, S, D, h_rot, R;
    bool interleaved;
    Tensor cos, sin, positions;
    void run(const Tensor &x, const kf_attn_layout &lx, Tensor &y, const kf_attn_layout &ly, bool inverse) const {
        DEV_CALL(kf_rope(code(x.dtype()), B, H, S, D, h_rot, R, interleaved ? 1 : 0, inverse ? 1 : 0, static_cast<const float *>(cos.data_ptr()),
                         static_cast<const float *>(sin.data_ptr()), cos.shape(0),
                         positions.defined() ? static_cast<const int64_t *>(positions.data_ptr()) : nullptr, x.data_ptr(), &lx, y.data_ptr(), &ly,
                         dev::stream(x.device())));
    }
};

// the backward of y = rope(x) is one inverse call over the gradient, laid out as y is (dense); dx is laid out the same way
class RopeGradFunction : public GradFunction {
public:
    RopeGradFunction(const Tensor &x, const RopeCall &call, const kf_attn_layout &lay) : call_(call), lay_(lay) { inputs = {x}; }
    std::vector<Tensor> backward(Tensor g) override {
        Tensor gc = g.dense();
        Tensor dx = empty(gc.sizes(), gc.dtype(), gc.device());
        call_.run(gc, lay_, dx, lay_, true);
        return {dx};
    }

private:
    RopeCall call_;
    kf_attn_layout lay_;
};

void check_tables(const Tensor &cos, const Tensor &sin, const Tensor &positions, int64_t tokens, int64_t D, int device, const char *who) {
    CHECK_FAIL(cos.defined() && sin.defined() && cos.dim() == 2 && cos.sizes() == sin.sizes() && cos.is_dense() && sin.is_dense(), who,
               ": cos and sin must be contiguous 2-D tables of one shape [positions, rotary_dim / 2]");
    CHECK_FAIL(cos.dtype() == ScalarType::Float && sin.dtype() == ScalarType::Float, who, ": cos and sin must be float tables");
    CHECK_FAIL(cos.shape(0) >= 1 && cos.shape(1) >= 1 && 2 * cos.shape(1) <= D, who, ": the tables' rotary_dim ", 2 * cos.shape(1),
               " must lie in [2, D = ", D, "]");
    CHECK_FAIL(cos.device() == device && sin.device() == device, who, ": the tables must be on the operand's device");
    if (positions.defined()) {
        CHECK_FAIL(positions.dtype() == ScalarType::Long, who, ": positions must be of type Long");
        CHECK_FAIL(positions.numel() == tokens && positions.device() == device, who, ": positions must hold B*S = ", tokens,
                   " elements on the operand's device");
    }
}
// the kernel reads positions as a dense int64 array in token order: a strided view (pos[:, 1:], pos[::2]) is made dense first
Tensor dense_positions(const Tensor &positions) { return positions.defined() ? positions.dense() : Tensor(); }
} // namespace

std::pair<Tensor, Tensor> rope_table(int64_t max_positions, int64_t rotary_dim, double base, int device) {
    CHECK_FAIL(max_positions >= 1, "rope_table: max_positions must be >= 1, got ", max_positions);
    CHECK_FAIL(rotary_dim >= 2 && rotary_dim % 2 == 0, "rope_table: rotary_dim must be even and >= 2, got ", rotary_dim);
    CHECK_FAIL(base > 0.0, "rope_table: base must be positive, got ", base);
    Tensor c = empty({max_positions, rotary_dim / 2}, ScalarType::Float, device), s = empty({max_positions, rotary_dim / 2}, ScalarType::Float, device);
    DEV_CALL(kf_rope_table(base, rotary_dim, max_positions, static_cast<float *>(c.data_ptr()), static_cast<float *>(s.data_ptr()), dev::stream(device)));
    return {c, s};
}

Tensor rope_qkv(const Tensor &qkv, const Tensor &cos, const Tensor &sin, int64_t B, int64_t S, int64_t H, int64_t kv_heads,
                const Tensor &positions, bool interleaved) {
    const int64_t kv = kv_heads < 0 ? H : kv_heads;
    CHECK_FAIL(qkv.defined() && qkv.dim() == 2 && qkv.is_dense(), "rope_qkv expects a contiguous [B*S, (H + 2*kv_heads)*D] tensor");
    CHECK_FAIL(rope_dtype_ok(qkv.dtype()), "rope_qkv supports float, half and bfloat16");
    CHECK_FAIL(B > 0 && S > 0 && H > 0 && kv > 0 && qkv.shape(0) == B * S && qkv.shape(1) % (H + 2 * kv) == 0,
               "rope_qkv: shape does not match B, S, H, kv_heads");
    const int64_t Ht = H + 2 * kv, W = qkv.shape(1), D = W / Ht;
    check_tables(cos, sin, positions, B * S, D, qkv.device(), "rope_qkv");
    const RopeCall call{B, Ht, S, D, H + kv, 2 * cos.shape(1), interleaved, cos, sin, dense_positions(positions)};
    const kf_attn_layout lay{S * W, D, W};
    Tensor out = empty(qkv.sizes(), qkv.dtype(), qkv.device());
    call.run(qkv, lay, out, lay, false);
    if (qkv.requires_grad()) {
        out.set_requires_grad(true);
        out.set_grad_fn(new RopeGradFunction(qkv, call, lay));
    }
    return out;
}

Tensor rope(const Tensor &x, const Tensor &cos, const Tensor &sin, const Tensor &positions, bool interleaved) {
    CHECK_FAIL(x.defined() && x.dim() == 4 && x.stride(3) == 1, "rope expects x [B, H, S, D] with a unit stride along D");
    CHECK_FAIL(rope_dtype_ok(x.dtype()), "rope supports float, half and bfloat16");
    const int64_t B = x.shape(0), H = x.shape(1), S = x.shape(2), D = x.shape(3);
    check_tables(cos, sin, positions, B * S, D, x.device(), "rope");
    const RopeCall call{B, H, S, D, H, 2 * cos.shape(1), interleaved, cos, sin, dense_positions(positions)};
    const kf_attn_layout lx{x.stride(0), x.stride(1), x.stride(2)}, ly{H * S * D, S * D, D};
    Tensor out = empty({B, H, S, D}, x.dtype(), x.device());
    if (out.numel() > 0) call.run(x, lx, out, ly, false);
    if (x.requires_grad()) {
        out.set_requires_grad(true);
        out.set_grad_fn(new RopeGradFunction(x, call, ly));
    }
    return out;
}

} // namespace gpu
