// Gated activations for gfx950, forward and backward: h = act(g) * u (SwiGLU, GeGLU) and the ungated act(g) (SiLU, GELU), on [rows, F]
// operands addressed by a leading dimension - in particular the two halves gate | up of the packed [rows, 2F] projection in place.
//
//   forward    h = act(g) u                       backward    dup = dh act(g)     dgate = dh u act'(g)     (recomputed from g and u)
//   SiLU       act = g s,  s = sigma(g)                       act' = s (1 + g (1 - s))
//   GELU-tanh  act = g s,  s = sigma(w),  w = 2 sqrt(2/pi) (g + 0.044715 g^3)   (0.5 (1 + tanh z) = sigma(2z))
//                                                             act' = s + g s (1 - s) w'(g)
//   GELU-erf   act = g P,  P = 0.5 erfc(-g / sqrt 2)          act' = P + g exp(-g^2 / 2) / sqrt(2 pi)
//
// The sigmoid is formed from e = exp2(-|x| log2 e) <= 1 and r = 1 / (1 + e): sigma = r (x >= 0) or e r (x < 0), 1 - sigma the other one
// of the two, and sigma (1 - sigma) = e r r. Nothing overflows, so every finite g gives a finite result (the limit 0 or g u where e
// underflows), and both tails keep their relative accuracy. A NaN goes through exp2 and comes out; g = +inf gives inf * u, g = -inf
// gives NaN (-inf * 0, as torch's x * sigmoid(x) does).
//
// An HBM stream: every element is read once and written once. Grid-stride over 16-byte packs (V = 16 / sizeof(T) elements) of the
// [rows, F / V] pack grid; a thread carries (row, pack column) and advances both by the host's split of the grid stride, so the loop
// holds no division. Bases or extents that are not whole aligned packs run the same kernel with V = 1: the same f32 expression per
// element (contraction off, FMAs written out), so both paths give the same bits. Reads of a pack come before its writes and no thread
// touches another's pack, which is what makes the aliases h == gate / up and dgate == gate, dup == up exact.
// All row offsets are 64-bit. No atomics, no LDS, no scratch, no host synchronisation: a call can be captured in a graph.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// the packed and the element path must round alike, bit for bit
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr int kGluBlock = 256;
constexpr int64_t kGluMaxGrid = 2048;   // 8 blocks per CU on 256 CUs; the rest is the grid-stride loop

constexpr float kLog2e = 1.44269504088896340736f;
// 1 / sqrt 2 in two parts: erfc's tail turns a relative error d of its argument into g^2 d, so the constant's own rounding is kept out
constexpr double kRsqrt2d = 0.70710678118654752440;
constexpr float kRsqrt2 = (float)kRsqrt2d, kRsqrt2Lo = (float)(kRsqrt2d - (double)kRsqrt2);
constexpr float kRsqrt2Pi = 0.39894228040143267794f;
// GELU-tanh: w = g (kW1 + kW3 g^2) = 2 sqrt(2/pi) (g + 0.044715 g^3); kT1, kT3 the same in units of log 2 (the exp2 argument)
constexpr double kW1d = 1.59576912160573071176, kW3d = kW1d * 0.044715, kLog2ed = 1.44269504088896340736;
constexpr float kW1 = (float)kW1d, kW3x3 = (float)(3.0 * kW3d);
constexpr float kT1 = (float)(kW1d * kLog2ed), kT3 = (float)(kW3d * kLog2ed);
// g^2 is capped where sigma (1 - sigma) is long zero, so that w'(g) stays finite for every finite g (inf * 0 otherwise)
constexpr float kG2Cap = 1.0e30f;

// V elements at p: one 16-byte pack, or one element (V = 1)
template <typename T, int V>
__device__ __forceinline__ void glu_load(const T *p, float (&f)[V]) {
    if constexpr (V == 1) f[0] = load_f32(p);
    else unpack16<T>(*(const uint4 *)p, f);
}
// one rounding per element, to nearest even in both paths; the hardware bf16 converter (pack16, store_hw) keeps a NaN a NaN.
// f32 -> f16 of values the compiler cannot see through: left to itself it folds the last multiply into the conversion
// (v_fma_mixlo_f16: the exact product rounded once to f16) in the element path only, and the two paths then differ in the last bit
template <typename T, int V>
__device__ __forceinline__ void glu_store(T *p, const float (&f)[V]) {
    float r[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        r[i] = f[i];
        if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(r[i]));
    }
    if constexpr (V == 1) store_hw(p, r[0]);
    else *(uint4 *)p = pack16<T>(r);
}

// sigma(x) and the pieces of its derivative from t = |x| log2 e >= 0: s = sigma(x), q = 1 - sigma(x), sq = sigma (1 - sigma).
// exp2f is the hardware exp2 with the denormal range kept (e below 2^-126 is not flushed); 1 + e lies in [1, 2] for the hardware rcp.
struct GluSigmoid { float s, q, sq; };
__device__ __forceinline__ GluSigmoid glu_sigmoid(float t, bool nonneg) {
    const float e = __builtin_exp2f(-t);
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    const float er = e * r;
    return {nonneg ? r : er, nonneg ? er : r, er * r};
}

// a = act(g) and, with GRAD, d = act'(g)
template <int ACT, bool GRAD>
__device__ __forceinline__ void glu_act(float g, float &a, float &d) {
    if constexpr (ACT == KF_ACT_SILU) {
        const GluSigmoid z = glu_sigmoid(fabsf(g) * kLog2e, g >= 0.f);
        a = g * z.s;
        if constexpr (GRAD) d = z.s * fmaf(g, z.q, 1.f);
    } else if constexpr (ACT == KF_ACT_GELU_TANH) {
        const float g2 = g * g;
        const GluSigmoid z = glu_sigmoid(fabsf(g) * fmaf(kT3, g2, kT1), g >= 0.f);
        a = g * z.s;
        if constexpr (GRAD) d = fmaf(g, z.sq * fmaf(kW3x3, fminf(g2, kG2Cap), kW1), z.s);
    } else {
        const float p = 0.5f * erfcf(fmaf(-g, kRsqrt2, -g * kRsqrt2Lo));
        a = g * p;
        if constexpr (GRAD) d = fmaf(g, __builtin_exp2f(g * g * (-0.5f * kLog2e)) * kRsqrt2Pi, p);
    }
}

struct GluArgs {
    const void *gate, *up, *dh;
    void *o0, *o1;                        // forward: h, -; backward: dgate, dup
    int64_t rows, P;                      // P = packs per row (F / V)
    int64_t ldg, ldu, lddh, ld0, ld1;     // leading dimensions in elements
    int64_t step_rows, step_cols;         // the grid stride in packs, split as step_rows * P + step_cols
};

// thread k of the grid starts at pack k of the [rows, P] pack grid and advances by the grid stride. The increment's comma matters:
// row takes its carry from the OLD col (step_cols < P, so one carry at most) before col itself is advanced and wrapped
#define KF_GLU_WALK(a, row, col)                                                              \
    const int64_t k0_ = (int64_t)blockIdx.x * kGluBlock + threadIdx.x;                        \
    int64_t row = k0_ / (a).P, col = k0_ - row * (a).P;                                       \
    for (; row < (a).rows; row += (a).step_rows + (col + (a).step_cols >= (a).P ? 1 : 0),     \
                           col = col + (a).step_cols >= (a).P ? col + (a).step_cols - (a).P : col + (a).step_cols)

template <typename T, int V, int ACT, bool GATED>
__global__ __launch_bounds__(kGluBlock) void glu_fwd_kernel(const GluArgs a) {
    const T *gate = (const T *)a.gate, *up = (const T *)a.up;
    T *h = (T *)a.o0;
    KF_GLU_WALK(a, row, col) {
        const int64_t c = col * V;
        float g[V], u[V], y[V];
        glu_load<T, V>(gate + row * a.ldg + c, g);
        if constexpr (GATED) glu_load<T, V>(up + row * a.ldu + c, u);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float act, unused;
            glu_act<ACT, false>(g[i], act, unused);
            y[i] = GATED ? act * u[i] : act;
        }
        glu_store<T, V>(h + row * a.ld0 + c, y);
    }
}

template <typename T, int V, int ACT, bool GATED>
__global__ __launch_bounds__(kGluBlock) void glu_bwd_kernel(const GluArgs a) {
    const T *gate = (const T *)a.gate, *up = (const T *)a.up, *dh = (const T *)a.dh;
    T *dgate = (T *)a.o0, *dup = (T *)a.o1;
    KF_GLU_WALK(a, row, col) {
        const int64_t c = col * V;
        float g[V], u[V], dy[V], dg[V], du[V];
        glu_load<T, V>(gate + row * a.ldg + c, g);
        if constexpr (GATED) glu_load<T, V>(up + row * a.ldu + c, u);
        glu_load<T, V>(dh + row * a.lddh + c, dy);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float act, der;
            glu_act<ACT, true>(g[i], act, der);
            if constexpr (GATED) {
                du[i] = dy[i] * act;
                dg[i] = dy[i] * u[i] * der;
            } else {
                dg[i] = dy[i] * der;
            }
        }
        glu_store<T, V>(dgate + row * a.ld0 + c, dg);
        if constexpr (GATED) glu_store<T, V>(dup + row * a.ld1 + c, du);
    }
}
#undef KF_GLU_WALK

// the checks both entries share; ptrs / lds: every operand that is present, outputs included
int glu_check(const char *who, int act, int dtype, int64_t rows, int64_t F, const void *const *ptrs, const int64_t *lds, const char *const *names, int n) {
    KF_REQUIRE(act == KF_ACT_SILU || act == KF_ACT_GELU_TANH || act == KF_ACT_GELU_ERF, KF_ERR_INVALID,
               "%s: act %d is not KF_ACT_SILU, KF_ACT_GELU_TANH or KF_ACT_GELU_ERF", who, act);
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(rows >= 0 && F >= 0, KF_ERR_INVALID, "%s: bad extents rows %lld F %lld", who, (long long)rows, (long long)F);
    const int es = dtype_size(dtype);
    for (int i = 0; i < n; ++i) {
        KF_REQUIRE(lds[i] >= F, KF_ERR_INVALID, "%s: leading dimension of %s %lld < F = %lld", who, names[i], (long long)lds[i], (long long)F);
        KF_REQUIRE((uintptr_t)ptrs[i] % es == 0, KF_ERR_INVALID, "%s: %s not aligned to its element size", who, names[i]);
    }
    return KF_OK;
}

// the 16-byte path: every base aligned, F and every leading dimension whole packs
bool glu_vector_ok(int es, int64_t F, const void *const *ptrs, const int64_t *lds, int n) {
    const int64_t V = 16 / es;
    bool ok = F % V == 0;
    for (int i = 0; i < n; ++i) ok = ok && ((uintptr_t)ptrs[i] & 15u) == 0 && lds[i] % V == 0;
    return ok;
}

// prof: the profile labels of the 16-byte path and of the element path
template <bool BWD>
int glu_run(const char *const *prof, int act, int dtype, int64_t rows, int64_t F, GluArgs a, const void *const *ptrs, const int64_t *lds, int n, void *stream) {
    const int es = dtype_size(dtype);
    const bool vec = glu_vector_ok(es, F, ptrs, lds, n);
    a.rows = rows;
    a.P = vec ? F / (16 / es) : F;
    const int64_t blocks = (rows * a.P + kGluBlock - 1) / kGluBlock;   // rows * P < 2^63: the operands exist
    const unsigned grid = (unsigned)std::min<int64_t>(blocks, kGluMaxGrid);
    const int64_t stride = (int64_t)grid * kGluBlock;
    a.step_rows = stride / a.P;
    a.step_cols = stride % a.P;
    hipStream_t st = as_stream(stream);
    KF_PROF(prof[vec ? 0 : 1], st);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_flags([&](auto VEC, auto GATED) {
            constexpr int V = VEC ? kPack16<T> : 1;
            auto go = [&](auto ACT) {
                if constexpr (BWD) return launch(glu_bwd_kernel<T, V, ACT, GATED>, grid, kGluBlock, 0, st, a);
                else return launch(glu_fwd_kernel<T, V, ACT, GATED>, grid, kGluBlock, 0, st, a);
            };
            return act == KF_ACT_SILU        ? go(std::integral_constant<int, KF_ACT_SILU>{})
                   : act == KF_ACT_GELU_TANH ? go(std::integral_constant<int, KF_ACT_GELU_TANH>{})
                                             : go(std::integral_constant<int, KF_ACT_GELU_ERF>{});
        }, vec, a.up != nullptr);
    });
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_glu_fwd(int act, int dtype, int64_t rows, int64_t F, const void *gate, int64_t ldg, const void *up, int64_t ldu, void *h, int64_t ldh,
                          void *stream) {
    KF_REQUIRE(gate && h, KF_ERR_INVALID, "kf_glu_fwd: null gate or h");
    const void *ptrs[3] = {gate, h, up};
    const int64_t lds[3] = {ldg, ldh, ldu};
    const char *names[3] = {"gate", "h", "up"};
    const int n = up ? 3 : 2;
    const int rc = glu_check("kf_glu_fwd", act, dtype, rows, F, ptrs, lds, names, n);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(h != gate || ldh == ldg, KF_ERR_INVALID, "kf_glu_fwd: alias h == gate needs ldh == ldg");
    KF_REQUIRE(!up || h != up || ldh == ldu, KF_ERR_INVALID, "kf_glu_fwd: alias h == up needs ldh == ldu");
    if (rows == 0 || F == 0) return KF_OK;
    GluArgs a{};
    a.gate = gate; a.up = up; a.o0 = h;
    a.ldg = ldg; a.ldu = up ? ldu : 0; a.ld0 = ldh;
    static const char *const gated[2] = {"glu_fwd_vec", "glu_fwd_elem"}, *const plain[2] = {"act_fwd_vec", "act_fwd_elem"};
    return glu_run<false>(up ? gated : plain, act, dtype, rows, F, a, ptrs, lds, n, stream);
}

extern "C" int kf_glu_bwd(int act, int dtype, int64_t rows, int64_t F, const void *gate, int64_t ldg, const void *up, int64_t ldu, const void *dh,
                          int64_t lddh, void *dgate, int64_t lddg, void *dup, int64_t lddu, void *stream) {
    KF_REQUIRE(gate && dh && dgate, KF_ERR_INVALID, "kf_glu_bwd: null gate, dh or dgate");
    KF_REQUIRE((up != nullptr) == (dup != nullptr), KF_ERR_INVALID, "kf_glu_bwd: dup goes with up (both or neither)");
    const void *ptrs[5] = {gate, dh, dgate, up, dup};
    const int64_t lds[5] = {ldg, lddh, lddg, ldu, lddu};
    const char *names[5] = {"gate", "dh", "dgate", "up", "dup"};
    const int n = up ? 5 : 3;
    const int rc = glu_check("kf_glu_bwd", act, dtype, rows, F, ptrs, lds, names, n);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(dgate != gate || lddg == ldg, KF_ERR_INVALID, "kf_glu_bwd: alias dgate == gate needs lddg == ldg");
    KF_REQUIRE(!up || dup != up || lddu == ldu, KF_ERR_INVALID, "kf_glu_bwd: alias dup == up needs lddu == ldu");
    if (rows == 0 || F == 0) return KF_OK;
    GluArgs a{};
    a.gate = gate; a.up = up; a.dh = dh; a.o0 = dgate; a.o1 = dup;
    a.ldg = ldg; a.ldu = up ? ldu : 0; a.lddh = lddh; a.ld0 = lddg; a.ld1 = up ? lddu : 0;
    static const char *const gated[2] = {"glu_bwd_vec", "glu_bwd_elem"}, *const plain[2] = {"act_bwd_vec", "act_bwd_elem"};
    return glu_run<true>(up ? gated : plain, act, dtype, rows, F, a, ptrs, lds, n, stream);
}
