// The gated delta rule for gfx950, forward with a carried state and the decode step:
//
//   S' = exp(g_t) S_{t-1},   u_t = beta_t (v_t - k_t S'),   S_t = S' + k_t^T u_t,   o_t = scale q_t S_t
//
// Every step reads the state before it writes it, so a 64-step chunk solves a unit-lower-triangular system. With S0 the state at the
// chunk's start and G the in-chunk inclusive prefix sum of g:
//
//   L[t, s] = beta_t exp(G_t - G_s) (k_t . k_s) for s < t,   T = (I + L)^-1
//   W = T diag(beta e^G) K,   Ubar = T diag(beta) V,   U = Ubar - W S0
//   O = diag(scale e^G) Q S0 + P U  (P[t, s] = scale exp(G_t - G_s) (q_t . k_s), s <= t),   S1 = e^{G_end} S0 + K^T diag(e^{G_end - G_s}) U
//
//   delta_prep_kernel   one workgroup per (b, h, chunk): T, W and Ubar depend on one chunk's k, v, beta, g only, so they are taken off
//                       the serial walk. K K^T by MFMA, I + L inverted in f32 by forward substitution (one lane a column), W and Ubar by
//                       MFMA into the workspace
//   delta_fwd_kernel    linear_attn.hip's forward split: one workgroup per (b, h, 64 columns of Dv) walks the chunks in order with the
//                       [Dk, 64] state in f32 accumulators; V is not read, W and the Ubar slice are
//   delta_step_kernel   the recurrence token by token on a state in memory, a bandwidth kernel without matrix instructions
//
// Every exponent is a non-positive difference of in-chunk prefix sums and nothing is divided, not even by beta: beta = 0 is exact. Rows
// past the sequence take beta = 0 and g = 0, which makes their rows of W and Ubar zero without a branch. No atomics, nothing read back:
// results are reproducible to the bit and the calls can be captured.
#include "linear_mix.h"

namespace kf {
namespace {

struct DeltaArgs {
    const char *q, *k, *v;
    const float *g, *beta; // g may be null and then counts as 0
    char *o, *w, *ub;      // the workspace: W and Ubar, [B H, nc 64, D] each
    const float *h0;       // [B, H, Dk, Dv] f32 or null
    float *hT;             // or null; the step kernel's state
    int64_t S;             // the step kernel's T
    int nc;
    float scale;
};

// l_scan, or its result for g = 0 when there is no g
__device__ __forceinline__ void d_scan(const float *g, int valid, float scale, float *out) {
    if (g) {
        l_scan(g, valid, scale, out);
    } else if (threadIdx.x < 64) {
        out[threadIdx.x] = 0.f;
        out[64 + threadIdx.x] = 1.f;
        out[128 + threadIdx.x] = scale;
    }
}

// ---- per chunk: T, W and Ubar ------------------------------------------------------------------------------------------------------------
// LDS: K | V | L [64][64] f32 | Tw | Tu | G, kd, e^G, beta. Wave w: the L block (32 (w >> 1), 32 (w & 1)), then the W and Ubar blocks of
// rows 32 (w >> 1) and columns 32 ((w & 1) D / 64 + i). Wave 0 inverts: lane j solves (I + L) x = e_j down the rows, x in 64 registers,
// the row of L broadcast from LDS 16 bytes at a time - 2016 fused multiply-adds a lane, all in f32. T leaves f32 once, as two 16-bit
// images with its columns scaled in f32 before the rounding: Tw = T diag(beta e^G) and Tu = T diag(beta), so K and V enter the second
// pair of products as they were loaded. W and Ubar are rounded once, into the dead K and V tiles, and leave as 16-byte rows.
template <int D> constexpr int d_prep_lds() { return 2 * L_C * D * 2 + L_C * L_C * 4 + 2 * L_PT + 4 * L_C * 4; }

template <bool BF, int D>
__global__ __launch_bounds__(256) void delta_prep_kernel(const DeltaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = D * 2, QT = L_C * RB, NQ = D / 64;
    constexpr int oK = 0, oV = QT, oL = 2 * QT, oTw = oL + L_C * L_C * 4, oTu = oTw + L_PT, oG = oTu + L_PT;
    const unsigned sm = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), xl = lane & 31, hl = lane >> 5;
    const int tb = wid >> 1, cbk = wid & 1;
    const int64_t bh = blockIdx.x / (unsigned)a.nc, S = a.S;
    const int c = (int)(blockIdx.x % (unsigned)a.nc);
    const int valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C);
    const int64_t row0 = bh * S + (int64_t)c * L_C;
    float *G = (float *)(smem + oG), *bt = G + 192, *L = (float *)(smem + oL);
    l_stage<RB>(a.k + row0 * RB, valid, RB, 0, smem + oK);
    l_stage<RB>(a.v + row0 * RB, valid, RB, 0, smem + oV);
    d_scan(a.g ? a.g + row0 : nullptr, valid, 1.f, G); // G[128 + t] = exp(G_t)
    if (threadIdx.x < 64) bt[threadIdx.x] = (int)threadIdx.x < valid ? a.beta[row0 + threadIdx.x] : 0.f;
    l_landed();
    const unsigned tK = sm + oK, tV = sm + oV, tTw = sm + oTw, tTu = sm + oTu;
    {
        l_f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) acc = l_mma<BF>(l_frag_row<RB>(tK, 32 * tb, 16 * ks), l_frag_row<RB>(tK, 32 * cbk, 16 * ks), acc);
        float gt[16], btt[16];
        l_rows(G, tb, gt);
        l_rows(bt, tb, btt);
        const int s = 32 * cbk + xl;
        const float gs = G[s];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int t = 32 * tb + l_row(e, hl);
            L[t * L_C + s] = s < t ? btt[e] * expf(gt[e] - gs) * acc[e] : 0.f;
        }
    }
    __syncthreads();
    if (wid == 0) { // x[t] = [t == j] - sum_{s < t} L[t, s] x[s]; a lane's x is zero above its own row without a branch
        float x[L_C];
#pragma unroll
        for (int t = 0; t < L_C; ++t) {
            float sum = 0.f;
#pragma unroll
            for (int s4 = 0; s4 < t; s4 += 4) {
                const float4 l = *(const float4 *)(L + t * L_C + s4);
                sum = fmaf(l.x, x[s4], sum);
                if (s4 + 1 < t) sum = fmaf(l.y, x[s4 + 1], sum);
                if (s4 + 2 < t) sum = fmaf(l.z, x[s4 + 2], sum);
                if (s4 + 3 < t) sum = fmaf(l.w, x[s4 + 3], sum);
            }
            x[t] = (t == lane ? 1.f : 0.f) - sum;
        }
        const float cu = bt[lane], cw = cu * G[128 + lane];
#pragma unroll
        for (int t = 0; t < L_C; ++t) {
            const int off = l_off<128>(t, lane >> 3) + (lane & 7) * 2;
            *(uint16_t *)(smem + oTw + off) = (uint16_t)l_cvt16<BF>(x[t] * cw);
            *(uint16_t *)(smem + oTu + off) = (uint16_t)l_cvt16<BF>(x[t] * cu);
        }
    }
    __syncthreads();
    l_f32x16 ow[NQ], ou[NQ];
    int cb[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        cb[i] = cbk * NQ + i;
#pragma unroll
        for (int e = 0; e < 16; ++e) ow[i][e] = ou[i][e] = 0.f;
    }
    for (int ks = 0; ks < 2 * (tb + 1); ++ks) { // T is lower triangular: rows 0 .. 31 end at column 31
        const l_u32x4 fw = l_frag_row<128>(tTw, 32 * tb, 16 * ks), fu = l_frag_row<128>(tTu, 32 * tb, 16 * ks);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            ow[i] = l_mma<BF>(fw, l_frag_col<RB>(tK, 32 * cb[i], 16 * ks), ow[i]);
            ou[i] = l_mma<BF>(fu, l_frag_col<RB>(tV, 32 * cb[i], 16 * ks), ou[i]);
        }
    }
    __syncthreads(); // K and V are read; W and Ubar take their places
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int t = 32 * tb + l_row(e, hl), col = 32 * cb[i] + xl, off = l_off<RB>(t, col >> 3) + (col & 7) * 2;
            *(uint16_t *)(smem + oK + off) = (uint16_t)l_cvt16<BF>(ow[i][e]);
            *(uint16_t *)(smem + oV + off) = (uint16_t)l_cvt16<BF>(ou[i][e]);
        }
    __syncthreads();
    char *wd = a.w + (bh * a.nc + c) * QT, *ud = a.ub + (bh * a.nc + c) * QT; // all 64 rows: the walk reads whole chunks
    for (int at = threadIdx.x; at < L_C * (RB / 16); at += 256) {
        const int r = at / (RB / 16), ch = at % (RB / 16);
        *(uint4 *)(wd + r * RB + ch * 16) = *(const uint4 *)(smem + oK + l_off<RB>(r, ch));
        *(uint4 *)(ud + r * RB + ch * 16) = *(const uint4 *)(smem + oV + l_off<RB>(r, ch));
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------------
// Wave w: the U, P and O blocks of rows 32 (w >> 1) (Dv / key columns 32 (w & 1)) and the state blocks of Dv columns 32 (w & 1), Dk rows
// 32 ((w >> 1) + 2 i). LDS: Q[2] K[2] W[2] | Ubar slice[2] | U | P | state copy [64 dv][Dk] | G. Per chunk: Q K^T, Q S0 and W S0 in one
// pass over Dk (S0 through its 16-bit copy), U = Ubar - W S0 rounded into LDS once, a barrier, O = diag(qd) Q S0 + P U, then the state
// update with the decay on the U fragment.
template <int D> constexpr int d_fwd_lds() { return 6 * L_C * D * 2 + 4 * L_PT + 64 * D * 2 + L_G; }

template <bool BF, int D>
__global__ __launch_bounds__(256) void delta_fwd_kernel(const DeltaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = D * 2, QT = L_C * RB, NS = D / 64, NST = D / 64;
    constexpr int oQ = 0, oK = 2 * QT, oW = 4 * QT, oB = 6 * QT, oU = oB + 2 * L_PT, oP = oU + L_PT, oS = oP + L_PT, oG = oS + 64 * RB;
    const unsigned sm = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), xl = lane & 31, hl = lane >> 5;
    const int tb = wid >> 1, cbk = wid & 1;
    const int64_t bh = blockIdx.x / NS, S = a.S;
    const int slice = blockIdx.x % NS, nc = a.nc;
    const char *q = a.q + bh * S * RB, *k = a.k + bh * S * RB, *w = a.w + bh * nc * QT, *ub = a.ub + bh * nc * QT;
    char *o = a.o + bh * S * RB;
    const float *g = a.g ? a.g + bh * S : nullptr;
    float *gbuf = (float *)(smem + oG);
    auto stage = [&](int c) __attribute__((always_inline)) {
        const int valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C), p = c & 1;
        l_stage<RB>(q + (int64_t)c * QT, valid, RB, 0, smem + oQ + p * QT);
        l_stage<RB>(k + (int64_t)c * QT, valid, RB, 0, smem + oK + p * QT);
        l_stage<RB>(w + (int64_t)c * QT, L_C, RB, 0, smem + oW + p * QT);
        l_stage<128>(ub + (int64_t)c * QT, L_C, RB, slice * 128, smem + oB + p * L_PT);
    };
    l_f32x16 st[NST];
    int db[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) db[i] = tb + 2 * i;
    // this slice of h0 (null: zeros) and its 16-bit copy for the first chunk's products; the chunk's first barrier publishes it
    l_state_in<NST>(st, db, cbk, a.h0 ? a.h0 + bh * D * D + slice * 64 : nullptr, D);
#pragma unroll
    for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], cbk);
    stage(0);
    for (int c = 0; c < nc; ++c) {
        const int p = c & 1, valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C);
        float *G = gbuf + p * 192;
        d_scan(g ? g + (int64_t)c * L_C : nullptr, valid, a.scale, G);
        l_landed(); // chunk c and its G are there for everyone; nobody reads chunk c - 1, its U or its P any more
        float gt[16], qdt[16], kdv[4][8];
        l_rows(G, tb, gt);
        l_rows(G + 128, tb, qdt);
        l_kvec(G + 64, kdv);
        const float gs = G[32 * cbk + xl], dec = expf(G[63]);
        if (c + 1 < nc) stage(c + 1);
        const unsigned tQ = sm + oQ + p * QT, tK = sm + oK + p * QT, tW = sm + oW + p * QT, tU = sm + oU, tP = sm + oP, tS = sm + oS;
        l_f32x16 acc, out, ws;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = out[e] = ws[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) {
            const l_u32x4 fq = l_frag_row<RB>(tQ, 32 * tb, 16 * ks), fs = l_frag_row<RB>(tS, 32 * cbk, 16 * ks);
            acc = l_mma<BF>(fq, l_frag_row<RB>(tK, 32 * cbk, 16 * ks), acc);
            out = l_mma<BF>(fq, fs, out);
            ws = l_mma<BF>(l_frag_row<RB>(tW, 32 * tb, 16 * ks), fs, ws);
        }
        l_mask_store<BF>(acc, smem + oP, tb, cbk, gt, gs, a.scale);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int dv = 32 * cbk + xl, off = l_off<128>(32 * tb + l_row(e, hl), dv >> 3) + (dv & 7) * 2;
            out[e] *= qdt[e];
            *(uint16_t *)(smem + oU + off) = (uint16_t)l_cvt16<BF>(l_f32<BF>(*(const uint16_t *)(smem + oB + p * L_PT + off)) - ws[e]);
        }
        __syncthreads(); // P and U are whole; nobody reads the state copy any more
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) out = l_mma<BF>(l_frag_row<128>(tP, 32 * tb, 16 * ks), l_frag_col<128>(tU, 32 * cbk, 16 * ks), out);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int t = 32 * tb + l_row(e, hl);
            if (t < valid) *(uint16_t *)(o + ((int64_t)c * L_C + t) * RB + (slice * 64 + 32 * cbk + xl) * 2) = (uint16_t)l_cvt16<BF>(out[e]);
        }
        if (c + 1 < nc || a.hT) {
            l_state_update<BF, RB, 128, NST>(st, tK, tU, db, cbk, dec, kdv);
            if (c + 1 < nc) {
#pragma unroll
                for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], cbk);
            }
        }
    }
    // hT: the image [Dk][64] f32 is exactly the two Q tiles, last read before the last chunk's barrier, with no DMA under way
    if (a.hT) l_state_out<NST, 64>(st, db, cbk, (float *)(smem + oQ), D, a.hT + bh * D * D + slice * 64, D);
}

// ---- the recurrence, token by token ------------------------------------------------------------------------------------------------------
// lin_step_kernel's design: one workgroup per (b, h, 64 state columns), lane (rg = tid >> 4, cp = tid & 15) keeps rows rg Dk / 16 .. of
// the columns 4 cp .. in Dk / 16 float4 registers over all T steps; the state is read once and written once. The delta rule needs
// k_t S' before the update; to keep one barrier a step the lane forms its partial sums of k_t S' and q_t S' in the same pass over its
// slice, both are summed over the 16 row groups through LDS in the order 0 .. 15 (every lane sums k S' for its own columns, row group
// 0 also q S'), then u = beta (v - k S'), S = S' + k u element-wise and o = scale (q S' + (q . k) u), q . k summed in index order by
// one lane a step when the operands are widened.
constexpr int D_TB = 16;
template <int D> constexpr int d_step_lds() { return (D_TB * (2 * D + 64) + 3 * D_TB + 2 * 16 * 128) * 4; }

template <bool BF, int D>
__global__ __launch_bounds__(256) void delta_step_kernel(const DeltaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = D / 16, NS = D / 64;
    float *sq = (float *)smem, *sk = sq + D_TB * D, *sv = sk + D_TB * D, *se = sv + D_TB * 64, *sb = se + D_TB, *sqk = sb + D_TB, *red = sqk + D_TB;
    const int tid = threadIdx.x, cp = tid & 15, rg = tid >> 4;
    const int64_t bh = blockIdx.x / NS, T = a.S;
    const int slice = blockIdx.x % NS;
    float *sp = a.hT + bh * D * D + rg * R * D + slice * 64 + 4 * cp;
    float4 s[R];
#pragma unroll
    for (int j = 0; j < R; ++j) s[j] = *(const float4 *)(sp + j * D);
    const uint16_t *q = (const uint16_t *)a.q + bh * T * D, *k = (const uint16_t *)a.k + bh * T * D, *v = (const uint16_t *)a.v + bh * T * D + slice * 64;
    uint16_t *o = (uint16_t *)a.o + bh * T * D + slice * 64;
    const float *g = a.g ? a.g + bh * T : nullptr, *beta = a.beta + bh * T;
    for (int64_t t0 = 0; t0 < T; t0 += D_TB) {
        const int nb = (int)(T - t0 < D_TB ? T - t0 : D_TB);
        __syncthreads(); // the steps before have read their operands
        for (int i = tid; i < nb * D; i += 256) {
            sq[i] = l_f32<BF>(q[t0 * D + i]);
            sk[i] = l_f32<BF>(k[t0 * D + i]);
        }
        for (int i = tid; i < nb * 64; i += 256) sv[i] = l_f32<BF>(v[(t0 + (i >> 6)) * D + (i & 63)]);
        if (tid < nb) {
            se[tid] = g ? expf(g[t0 + tid]) : 1.f;
            sb[tid] = beta[t0 + tid];
        }
        __syncthreads();
        if (tid < nb) { // read after the first step's barrier
            float d = 0.f;
            for (int j = 0; j < D; ++j) d = fmaf(sq[tid * D + j], sk[tid * D + j], d);
            sqk[tid] = d;
        }
        for (int t = 0; t < nb; ++t) {
            const float e = se[t];
            const float4 vv = *(const float4 *)(sv + t * 64 + 4 * cp);
            float kk[R], qq[R];
#pragma unroll
            for (int j = 0; j < R; j += 4) {
                *(float4 *)(kk + j) = *(const float4 *)(sk + t * D + rg * R + j);
                *(float4 *)(qq + j) = *(const float4 *)(sq + t * D + rg * R + j);
            }
            float4 pk = {0.f, 0.f, 0.f, 0.f}, pq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < R; ++j) {
                s[j].x *= e;
                s[j].y *= e;
                s[j].z *= e;
                s[j].w *= e;
                pk.x = fmaf(kk[j], s[j].x, pk.x);
                pk.y = fmaf(kk[j], s[j].y, pk.y);
                pk.z = fmaf(kk[j], s[j].z, pk.z);
                pk.w = fmaf(kk[j], s[j].w, pk.w);
                pq.x = fmaf(qq[j], s[j].x, pq.x);
                pq.y = fmaf(qq[j], s[j].y, pq.y);
                pq.z = fmaf(qq[j], s[j].z, pq.z);
                pq.w = fmaf(qq[j], s[j].w, pq.w);
            }
            float *rp = red + (t & 1) * (16 * 128);
            *(float4 *)(rp + rg * 128 + 4 * cp) = pk;
            *(float4 *)(rp + rg * 128 + 64 + 4 * cp) = pq;
            __syncthreads();
            float4 ks = *(const float4 *)(rp + 4 * cp);
#pragma unroll
            for (int r = 1; r < 16; ++r) {
                const float4 y = *(const float4 *)(rp + r * 128 + 4 * cp);
                ks.x += y.x;
                ks.y += y.y;
                ks.z += y.z;
                ks.w += y.w;
            }
            const float b = sb[t];
            const float4 u = {b * (vv.x - ks.x), b * (vv.y - ks.y), b * (vv.z - ks.z), b * (vv.w - ks.w)};
#pragma unroll
            for (int j = 0; j < R; ++j) {
                s[j].x = fmaf(kk[j], u.x, s[j].x);
                s[j].y = fmaf(kk[j], u.y, s[j].y);
                s[j].z = fmaf(kk[j], u.z, s[j].z);
                s[j].w = fmaf(kk[j], u.w, s[j].w);
            }
            if (rg == 0) {
                float4 qs = *(const float4 *)(rp + 64 + 4 * cp);
#pragma unroll
                for (int r = 1; r < 16; ++r) {
                    const float4 y = *(const float4 *)(rp + r * 128 + 64 + 4 * cp);
                    qs.x += y.x;
                    qs.y += y.y;
                    qs.z += y.z;
                    qs.w += y.w;
                }
                const float qk = sqk[t];
                uint2 w;
                w.x = l_cvt16<BF>(a.scale * fmaf(qk, u.x, qs.x)) | (l_cvt16<BF>(a.scale * fmaf(qk, u.y, qs.y)) << 16);
                w.y = l_cvt16<BF>(a.scale * fmaf(qk, u.z, qs.z)) | (l_cvt16<BF>(a.scale * fmaf(qk, u.w, qs.w)) << 16);
                *(uint2 *)(o + (t0 + t) * D + 4 * cp) = w;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) *(float4 *)(sp + j * D) = s[j];
}

int64_t delta_chunks(int64_t S) { return (S + L_C - 1) / L_C; }
// W and Ubar: whole chunks of 16-bit rows
size_t delta_ws_bytes(int64_t B, int64_t H, int64_t S, int64_t D) { return (size_t)(2 * B * H * delta_chunks(S) * L_C * D * 2); }

int delta_check(const char *who, int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale) {
    const int rc = lin_check(who, dtype, B, H, S, Dk, Dv, scale);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(B * H * delta_chunks(S) < (int64_t)1 << 31, KF_ERR_UNSUPPORTED, "%s: B * H * chunks %lld above one grid", who,
               (long long)(B * H * delta_chunks(S)));
    return KF_OK;
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_delta_rule_fwd_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, size_t *bytes) {
    const char *who = "kf_delta_rule_fwd_workspace_bytes";
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null bytes", who);
    const int rc = delta_check(who, dtype, B, H, S, Dk, Dv, 1.f);
    if (rc != KF_OK) return rc;
    *bytes = delta_ws_bytes(B, H, S, Dk);
    return KF_OK;
}

extern "C" int kf_delta_rule_fwd(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                 const void *v, const float *g, const float *beta, const float *h0, void *o, float *hT, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    const char *who = "kf_delta_rule_fwd";
    KF_REQUIRE(q && k && v && beta && o, KF_ERR_INVALID, "%s: null operand", who);
    const int rc = delta_check(who, dtype, B, H, S, Dk, Dv, scale);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(al16(q) && al16(k) && al16(v) && al16_or_null(g) && al16(beta) && al16(o), KF_ERR_INVALID, "%s: an operand is not aligned to 16 bytes", who);
    KF_REQUIRE(al16_or_null(h0) && al16_or_null(hT), KF_ERR_INVALID, "%s: a state is not aligned to 16 bytes", who);
    const size_t need = delta_ws_bytes(B, H, S, Dk);
    KF_REQUIRE(workspace && workspace_bytes >= need && al16(workspace), KF_ERR_WORKSPACE, "%s: workspace of %zu bytes at %p, %zu aligned to 16 needed", who,
               workspace ? workspace_bytes : (size_t)0, workspace, need);
    hipStream_t st = as_stream(stream);
    DeltaArgs a{};
    a.q = (const char *)q; a.k = (const char *)k; a.v = (const char *)v; a.g = g; a.beta = beta; a.o = (char *)o;
    a.w = (char *)workspace; a.ub = a.w + need / 2;
    a.h0 = h0; a.hT = hT;
    a.S = S; a.nc = (int)delta_chunks(S); a.scale = scale;
    const bool bf = dtype == KF_BF16, big = Dk == 128;
    return with_flags([&](auto BF, auto BIG) {
        constexpr int D = decltype(BIG)::value ? 128 : 64;
        constexpr bool bfv = decltype(BF)::value;
        {
            KF_PROF(bfv ? "delta_rule_prep_bf16" : "delta_rule_prep_f16", st);
            const int r = launch(delta_prep_kernel<bfv, D>, dim3((unsigned)(B * H * a.nc)), dim3(256), (size_t)d_prep_lds<D>(), st, a);
            if (r != KF_OK) return r;
        }
        KF_PROF(bfv ? "delta_rule_fwd_bf16" : "delta_rule_fwd_f16", st);
        return launch(delta_fwd_kernel<bfv, D>, dim3((unsigned)(B * H * (Dv / 64))), dim3(256), (size_t)d_fwd_lds<D>(), st, a);
    }, bf, big);
}

extern "C" int kf_delta_rule_step(int dtype, int64_t B, int64_t H, int64_t T, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                  const void *v, const float *g, const float *beta, float *state, void *o, void *stream) {
    const char *who = "kf_delta_rule_step";
    KF_REQUIRE(q && k && v && beta && state && o, KF_ERR_INVALID, "%s: null operand", who);
    const int rc = delta_check(who, dtype, B, H, T, Dk, Dv, scale);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(al16(q) && al16(k) && al16(v) && al16_or_null(g) && al16(beta) && al16(state) && al16(o), KF_ERR_INVALID,
               "%s: an operand is not aligned to 16 bytes", who);
    hipStream_t st = as_stream(stream);
    DeltaArgs a{};
    a.q = (const char *)q; a.k = (const char *)k; a.v = (const char *)v; a.g = g; a.beta = beta; a.o = (char *)o;
    a.hT = state;
    a.S = T; a.scale = scale;
    const bool bf = dtype == KF_BF16, big = Dk == 128;
    const dim3 grid((unsigned)(B * H * (Dv / 64)));
    KF_PROF(bf ? "delta_rule_step_bf16" : "delta_rule_step_f16", st);
    return with_flags([&](auto BF, auto BIG) {
        constexpr int D = decltype(BIG)::value ? 128 : 64;
        return launch(delta_step_kernel<decltype(BF)::value, D>, grid, dim3(256), (size_t)d_step_lds<D>(), st, a);
    }, bf, big);
}
