// Chunked linear attention with a scalar per-step decay for gfx950, forward and backward:
//
//   S_t = exp(g_t) S_{t-1} + k_t v_t^T,   o_t = scale q_t S_t        <=>   O = scale ((Q K^T) . A) V,  A[t, s] = exp(G_t - G_s) for s <= t
//
//   kf_linear_attn_fwd   one workgroup per (b, h, 64 columns of Dv) walks the head's 64-step chunks in order; the [Dk, 64] state stays in
//                        f32 MFMA accumulators for the whole walk
//   kf_linear_attn_bwd   an ascending walk (S recomputed; dQ and a_t = q_t . dq_t), a descending walk (dS carried; dK, dV and
//                        b_t = k_t . dk_t), one workgroup per (b, h) each with the whole [Dk, Dv] state in accumulators, then
//                        dg_r = sum_{t >= r} (a_t - b_t) in a fixed order
//
// Every decay factor is exp of a non-positive difference of in-chunk prefix sums (G_t - G_s for s <= t, G_t - G_start, G_end - G_s), so
// nothing overflows and nothing is divided. The chunk's Q / K / V / dO tiles arrive by LDS-DMA through buffer descriptors that end with
// the sequence: rows past it read as zeros, their g counts as 0, and their stores are dropped. All tiles are 64 rows of 16-bit values
// with an XOR swizzle on the 16-byte chunk; a fragment whose contraction index runs along a tile's columns is one ds_read_b128, one
// whose contraction index runs along the rows is two ds_read_b64_tr_b16 (l_frag_row / l_frag_col). No atomics, no workspace for the
// forward, nothing read back: results are reproducible to the bit and the calls can be captured.
//
// The three walks also exist as state variants (template flag ST; kf_linear_attn_state_fwd / _bwd): the carried state starts from h0
// (the carried dS from d_hT) instead of zero, the walk's last carry step is done too and the accumulators leave as hT (d_h0), and the
// ascending walk forms <d_hT, hT>, the constant every dg_r gains when a gradient arrives through the final state. The state moves in
// and out at the two ends of a walk, through tiles that are free there. kf_linear_attn_step is the token-by-token recurrence, a
// bandwidth kernel without matrix instructions (lin_step_kernel).
// The tiles, their staging, the fragment readers, the scan and the state helpers are linear_mix.h's, shared with delta_rule.hip.
#include "linear_mix.h"

namespace kf {
namespace {

struct LinArgs {
    const char *q, *k, *v, *d_o;
    const float *g;
    char *o, *dq, *dk, *dv;
    float *wa, *wb, *dg;
    const float *h0, *d_hT; // [B, H, Dk, Dv] f32 or null (state variants only)
    float *hT, *d_h0, *wc;  // wc: <d_hT, hT> per (b, h), null without d_hT; the step kernel's state is hT and its T is S
    int64_t S;
    float scale;
};

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// Wave w: the P block and the O block of query rows 32 (w >> 1) (key / Dv columns 32 (w & 1)), and the state blocks of Dv columns
// 32 (w & 1), Dk rows 32 ((w >> 1) + 2 i). LDS: Q[2] K[2] V-slice[2] | P | state copy [64 dv][Dk] | G.
template <int D> constexpr int l_fwd_lds() { return 2 * (2 * L_C * D * 2 + L_PT) + L_PT + 64 * D * 2 + L_G; }

template <bool BF, int D, bool ST>
__global__ __launch_bounds__(256) void lin_fwd_kernel(const LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = D * 2, QT = L_C * RB, NS = D / 64, NST = D / 64;
    constexpr int oQ = 0, oK = 2 * QT, oV = 4 * QT, oP = oV + 2 * L_PT, oS = oP + L_PT, oG = oS + 64 * RB;
    const unsigned sm = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), xl = lane & 31, hl = lane >> 5;
    const int tb = wid >> 1, cbk = wid & 1;
    const int64_t bh = blockIdx.x / NS, S = a.S;
    const int slice = blockIdx.x % NS;
    const char *q = a.q + bh * S * RB, *k = a.k + bh * S * RB, *v = a.v + bh * S * RB;
    char *o = a.o + bh * S * RB;
    const float *g = a.g + bh * S;
    float *gbuf = (float *)(smem + oG);
    const int nc = (int)((S + L_C - 1) / L_C);
    auto stage = [&](int c) __attribute__((always_inline)) {
        const int valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C), p = c & 1;
        l_stage<RB>(q + (int64_t)c * QT, valid, RB, 0, smem + oQ + p * QT);
        l_stage<RB>(k + (int64_t)c * QT, valid, RB, 0, smem + oK + p * QT);
        l_stage<128>(v + (int64_t)c * QT, valid, RB, slice * 128, smem + oV + p * L_PT);
    };
    l_f32x16 st[NST];
    int db[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        db[i] = tb + 2 * i;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[i][e] = 0.f;
    }
    if constexpr (ST) { // this slice of h0 and its 16-bit copy for the first chunk's Q S_prev; the chunk's first barrier publishes it
        l_state_in<NST>(st, db, cbk, a.h0 ? a.h0 + bh * D * D + slice * 64 : nullptr, D);
#pragma unroll
        for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], cbk);
    }
    stage(0);
    for (int c = 0; c < nc; ++c) {
        const int p = c & 1, valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C);
        float *G = gbuf + p * 192;
        l_scan(g + (int64_t)c * L_C, valid, a.scale, G);
        l_landed(); // chunk c and its G are there for everyone; nobody reads chunk c - 1 any more
        float gt[16], qdt[16], kdv[4][8];
        l_rows(G, tb, gt);
        l_rows(G + 128, tb, qdt);
        l_kvec(G + 64, kdv);
        const float gs = G[32 * cbk + xl], dec = expf(G[63]);
        if (c + 1 < nc) stage(c + 1);
        const unsigned tQ = sm + oQ + p * QT, tK = sm + oK + p * QT, tV = sm + oV + p * L_PT, tP = sm + oP, tS = sm + oS;
        l_f32x16 acc, out;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = out[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) acc = l_mma<BF>(l_frag_row<RB>(tQ, 32 * tb, 16 * ks), l_frag_row<RB>(tK, 32 * cbk, 16 * ks), acc);
        l_mask_store<BF>(acc, smem + oP, tb, cbk, gt, gs, a.scale);
        if (ST || c > 0) { // the carried state, through its 16-bit copy; the row scaling stays in f32
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) out = l_mma<BF>(l_frag_row<RB>(tQ, 32 * tb, 16 * ks), l_frag_row<RB>(tS, 32 * cbk, 16 * ks), out);
#pragma unroll
            for (int e = 0; e < 16; ++e) out[e] *= qdt[e];
        }
        __syncthreads(); // P is whole; nobody reads the state copy any more
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) out = l_mma<BF>(l_frag_row<128>(tP, 32 * tb, 16 * ks), l_frag_col<128>(tV, 32 * cbk, 16 * ks), out);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int t = 32 * tb + l_row(e, hl);
            if (t < valid) *(uint16_t *)(o + ((int64_t)c * L_C + t) * RB + (slice * 64 + 32 * cbk + xl) * 2) = (uint16_t)l_cvt16<BF>(out[e]);
        }
        if (c + 1 < nc || (ST && a.hT)) {
            l_state_update<BF, RB, 128, NST>(st, tK, tV, db, cbk, dec, kdv);
            if (c + 1 < nc) {
#pragma unroll
                for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], cbk);
            }
        }
    }
    // hT: the image [Dk][64] f32 is exactly the two Q tiles, last read before the last chunk's barrier, with no DMA under way
    if (ST && a.hT) l_state_out<NST, 64>(st, db, cbk, (float *)(smem + oQ), D, a.hT + bh * D * D + slice * 64, D);
}

// ---- backward, ascending: dQ and a_t ---------------------------------------------------------------------------------------------------
// Wave w: the dP block (32 (w >> 1), 32 (w & 1)), the dQ blocks of rows 32 (w >> 1) and Dk columns 32 ((w & 1) D / 64 + i), the state
// blocks of Dv columns 32 w and every Dk row block at D = 128 (Dv columns 32 (w & 1), Dk rows 32 (w >> 1) at D = 64).
// LDS: K[2] V[2] dO[2] | M | state copy [Dv][Dk] | G | a_t halves.
template <int D> constexpr int l_asc_lds() { return 6 * L_C * D * 2 + L_PT + D * D * 2 + L_G + 2 * L_C * 4; }

template <bool BF, int D, bool ST>
__global__ __launch_bounds__(256) void lin_bwd_asc_kernel(const LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = D * 2, QT = L_C * RB, NQ = D / 64, NST = D == 128 ? 4 : 1;
    constexpr int oK = 0, oV = 2 * QT, oO = 4 * QT, oM = 6 * QT, oS = oM + L_PT, oG = oS + D * RB, oA = oG + L_G;
    const unsigned sm = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), xl = lane & 31, hl = lane >> 5;
    const int tb = wid >> 1, cbk = wid & 1;
    const int64_t bh = blockIdx.x, S = a.S;
    const char *q = a.q + bh * S * RB, *k = a.k + bh * S * RB, *v = a.v + bh * S * RB, *d_o = a.d_o + bh * S * RB;
    char *dq = a.dq + bh * S * RB;
    const float *g = a.g + bh * S;
    float *gbuf = (float *)(smem + oG), *asum = (float *)(smem + oA);
    const int nc = (int)((S + L_C - 1) / L_C);
    auto stage = [&](int c) __attribute__((always_inline)) {
        const int valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C), p = c & 1;
        l_stage<RB>(k + (int64_t)c * QT, valid, RB, 0, smem + oK + p * QT);
        l_stage<RB>(v + (int64_t)c * QT, valid, RB, 0, smem + oV + p * QT);
        l_stage<RB>(d_o + (int64_t)c * QT, valid, RB, 0, smem + oO + p * QT);
    };
    l_f32x16 st[NST];
    int db[NST], qb[NQ];
    const int sdv = D == 128 ? wid : cbk;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        db[i] = D == 128 ? i : tb;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[i][e] = 0.f;
    }
    if constexpr (ST) {
        l_state_in<NST>(st, db, sdv, a.h0 ? a.h0 + bh * D * D : nullptr, D);
#pragma unroll
        for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], sdv);
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) qb[i] = cbk * NQ + i;
    stage(0);
    for (int c = 0; c < nc; ++c) {
        const int p = c & 1, valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C);
        float *G = gbuf + p * 192;
        l_scan(g + (int64_t)c * L_C, valid, a.scale, G);
        l_landed();
        float gt[16], qdt[16], kdv[4][8];
        l_rows(G, tb, gt);
        l_rows(G + 128, tb, qdt);
        l_kvec(G + 64, kdv);
        const float gs = G[32 * cbk + xl], dec = expf(G[63]);
        if (c + 1 < nc) stage(c + 1);
        const unsigned tK = sm + oK + p * QT, tV = sm + oV + p * QT, tO = sm + oO + p * QT, tM = sm + oM, tS = sm + oS;
        l_f32x16 acc, out[NQ];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) out[i][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) acc = l_mma<BF>(l_frag_row<RB>(tO, 32 * tb, 16 * ks), l_frag_row<RB>(tV, 32 * cbk, 16 * ks), acc);
        l_mask_store<BF>(acc, smem + oM, tb, cbk, gt, gs, a.scale);
        if (ST || c > 0) { // dO S_prev^T: k runs over Dv, the rows of the state copy
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) {
                const l_u32x4 fa = l_frag_row<RB>(tO, 32 * tb, 16 * ks);
#pragma unroll
                for (int i = 0; i < NQ; ++i) out[i] = l_mma<BF>(fa, l_frag_col<RB>(tS, 32 * qb[i], 16 * ks), out[i]);
            }
#pragma unroll
            for (int i = 0; i < NQ; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) out[i][e] *= qdt[e];
        }
        __syncthreads(); // M is whole; nobody reads the state copy any more
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const l_u32x4 fa = l_frag_row<128>(tM, 32 * tb, 16 * ks);
#pragma unroll
            for (int i = 0; i < NQ; ++i) out[i] = l_mma<BF>(fa, l_frag_col<RB>(tK, 32 * qb[i], 16 * ks), out[i]);
        }
        float part[16]; // q_t . dq_t over this wave's columns, from the f32 rows
#pragma unroll
        for (int e = 0; e < 16; ++e) part[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int t = 32 * tb + l_row(e, hl);
                if (t < valid) {
                    const int64_t at = ((int64_t)c * L_C + t) * RB + (32 * qb[i] + xl) * 2;
                    *(uint16_t *)(dq + at) = (uint16_t)l_cvt16<BF>(out[i][e]);
                    part[e] += l_f32<BF>(*(const uint16_t *)(q + at)) * out[i][e];
                }
            }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float s = l_half_sum(part[e]);
            if (xl == 0) asum[cbk * L_C + 32 * tb + l_row(e, hl)] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < valid) a.wa[bh * S + (int64_t)c * L_C + threadIdx.x] = asum[threadIdx.x] + asum[L_C + threadIdx.x];
        if (c + 1 < nc || (ST && a.d_hT)) {
            l_state_update<BF, RB, RB, NST>(st, tK, tV, db, sdv, dec, kdv);
            if (c + 1 < nc) {
#pragma unroll
                for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], sdv);
            }
        }
    }
    if (ST && a.d_hT) { // <d_hT, hT>: each lane over its own elements, the wave by shuffles, the four waves in order
        const float *dh = a.d_hT + bh * D * D;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NST; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) s += st[i][e] * dh[(32 * db[i] + l_row(e, hl)) * D + 32 * sdv + xl];
        s = l_half_sum(s);
        s += __shfl_xor(s, 32);
        __syncthreads(); // the a_t halves are read
        if (lane == 0) asum[wid] = s;
        __syncthreads();
        if (threadIdx.x == 0) a.wc[bh] = ((asum[0] + asum[1]) + asum[2]) + asum[3];
    }
}

// ---- backward, descending: dK, dV and b_t ----------------------------------------------------------------------------------------------
// The carried dS[d][dv] = sum over later t of scale exp(G_t - G_end of this chunk) q_t dO_t^T. Wave w: the P and M blocks
// (32 (w >> 1), 32 (w & 1)), the dK and dV blocks of key rows 32 (w >> 1) and columns 32 ((w & 1) D / 64 + i), the dS blocks as the
// ascending walk's state blocks. LDS: NBUF x (Q K V dO) | P | M | dS copy [Dv][Dk] | G | b_t halves; four 16 KiB tiles twice do not
// fit beside the rest at D = 128, so there the next chunk is fetched after this one's last read (NBUF 1).
template <int D> constexpr int l_desc_nbuf() { return D == 64 ? 2 : 1; }
template <int D> constexpr int l_desc_lds() { return l_desc_nbuf<D>() * 4 * L_C * D * 2 + 2 * L_PT + D * D * 2 + L_G + 2 * L_C * 4; }

template <bool BF, int D, bool ST>
__global__ __launch_bounds__(256) void lin_bwd_desc_kernel(const LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RB = D * 2, QT = L_C * RB, NQ = D / 64, NST = D == 128 ? 4 : 1, NBUF = l_desc_nbuf<D>();
    constexpr int oP = NBUF * 4 * QT, oM = oP + L_PT, oS = oM + L_PT, oG = oS + D * RB, oB = oG + L_G;
    const unsigned sm = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), xl = lane & 31, hl = lane >> 5;
    const int tb = wid >> 1, cbk = wid & 1;
    const int64_t bh = blockIdx.x, S = a.S;
    const char *q = a.q + bh * S * RB, *k = a.k + bh * S * RB, *v = a.v + bh * S * RB, *d_o = a.d_o + bh * S * RB;
    char *dk = a.dk + bh * S * RB, *dv = a.dv + bh * S * RB;
    const float *g = a.g + bh * S;
    float *gbuf = (float *)(smem + oG), *bsum = (float *)(smem + oB);
    const int nc = (int)((S + L_C - 1) / L_C);
    auto stage = [&](int c, int buf) __attribute__((always_inline)) {
        const int valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C);
        char *base = smem + buf * 4 * QT;
        l_stage<RB>(q + (int64_t)c * QT, valid, RB, 0, base);
        l_stage<RB>(k + (int64_t)c * QT, valid, RB, 0, base + QT);
        l_stage<RB>(v + (int64_t)c * QT, valid, RB, 0, base + 2 * QT);
        l_stage<RB>(d_o + (int64_t)c * QT, valid, RB, 0, base + 3 * QT);
    };
    l_f32x16 st[NST];
    int db[NST], cb[NQ];
    const int sdv = D == 128 ? wid : cbk;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        db[i] = D == 128 ? i : tb;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[i][e] = 0.f;
    }
    if constexpr (ST) { // the carried dS starts from d_hT
        l_state_in<NST>(st, db, sdv, a.d_hT ? a.d_hT + bh * D * D : nullptr, D);
#pragma unroll
        for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], sdv);
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) cb[i] = cbk * NQ + i;
    stage(nc - 1, 0);
    for (int it = 0; it < nc; ++it) {
        const int c = nc - 1 - it, buf = it % NBUF, valid = (int)(S - (int64_t)c * L_C < L_C ? S - (int64_t)c * L_C : L_C);
        float *G = gbuf + (it & 1) * 192;
        l_scan(g + (int64_t)c * L_C, valid, a.scale, G);
        l_landed();
        float gt[16];
        l_rows(G, tb, gt);
        const float gs = G[32 * cbk + xl], dec = expf(G[63]);
        if (NBUF == 2 && c > 0) stage(c - 1, buf ^ 1);
        const unsigned tQ = sm + buf * 4 * QT, tK = tQ + QT, tV = tQ + 2 * QT, tO = tQ + 3 * QT, tP = sm + oP, tM = sm + oM, tS = sm + oS;
        l_f32x16 accp, accm, ok[NQ], ov[NQ];
#pragma unroll
        for (int e = 0; e < 16; ++e) accp[e] = accm[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) ok[i][e] = ov[i][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) {
            accp = l_mma<BF>(l_frag_row<RB>(tQ, 32 * tb, 16 * ks), l_frag_row<RB>(tK, 32 * cbk, 16 * ks), accp);
            accm = l_mma<BF>(l_frag_row<RB>(tO, 32 * tb, 16 * ks), l_frag_row<RB>(tV, 32 * cbk, 16 * ks), accm);
        }
        l_mask_store<BF>(accp, smem + oP, tb, cbk, gt, gs, a.scale);
        l_mask_store<BF>(accm, smem + oM, tb, cbk, gt, gs, a.scale);
        if (ST || it > 0) { // V dS^T (k over Dv, the copy's rows) and K dS (k over Dk, the copy's columns)
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) {
                const l_u32x4 fv = l_frag_row<RB>(tV, 32 * tb, 16 * ks), fk = l_frag_row<RB>(tK, 32 * tb, 16 * ks);
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    ok[i] = l_mma<BF>(fv, l_frag_col<RB>(tS, 32 * cb[i], 16 * ks), ok[i]);
                    ov[i] = l_mma<BF>(fk, l_frag_row<RB>(tS, 32 * cb[i], 16 * ks), ov[i]);
                }
            }
            float kds[16]; // (read where they are used, like qdv below: the walk at D = 128 has no registers to hold them across the chunk)
            l_rows(G + 64, tb, kds); // this wave's key rows are block w >> 1 too
#pragma unroll
            for (int i = 0; i < NQ; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    ok[i][e] *= kds[e];
                    ov[i][e] *= kds[e];
                }
        }
        __syncthreads(); // P and M are whole; nobody reads the dS copy any more
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { // k runs over the chunk's query rows: M^T Q and P^T dO
            const l_u32x4 fm = l_frag_col<128>(tM, 32 * tb, 16 * ks), fp = l_frag_col<128>(tP, 32 * tb, 16 * ks);
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                ok[i] = l_mma<BF>(fm, l_frag_col<RB>(tQ, 32 * cb[i], 16 * ks), ok[i]);
                ov[i] = l_mma<BF>(fp, l_frag_col<RB>(tO, 32 * cb[i], 16 * ks), ov[i]);
            }
        }
        float part[16]; // k_s . dk_s over this wave's columns, from the f32 rows
#pragma unroll
        for (int e = 0; e < 16; ++e) part[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int s = 32 * tb + l_row(e, hl), col = 32 * cb[i] + xl;
                if (s < valid) {
                    const int64_t at = ((int64_t)c * L_C + s) * RB + col * 2;
                    *(uint16_t *)(dk + at) = (uint16_t)l_cvt16<BF>(ok[i][e]);
                    *(uint16_t *)(dv + at) = (uint16_t)l_cvt16<BF>(ov[i][e]);
                    part[e] += l_f32<BF>(*(const uint16_t *)(smem + buf * 4 * QT + QT + l_off<RB>(s, col >> 3) + (col & 7) * 2)) * ok[i][e];
                }
            }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float s = l_half_sum(part[e]);
            if (xl == 0) bsum[cbk * L_C + 32 * tb + l_row(e, hl)] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < valid) a.wb[bh * S + (int64_t)c * L_C + threadIdx.x] = bsum[threadIdx.x] + bsum[L_C + threadIdx.x];
        if (c > 0 || (ST && a.d_h0)) {
            float qdv[4][8];
            l_kvec(G + 128, qdv);
            l_state_update<BF, RB, RB, NST>(st, tQ, tO, db, sdv, dec, qdv);
            if (c > 0) {
#pragma unroll
                for (int i = 0; i < NST; ++i) l_state_store<BF, RB>(st[i], smem + oS, db[i], sdv);
                if (NBUF == 1) {
                    __syncthreads(); // the last read of this chunk's tiles
                    stage(c - 1, 0);
                }
            }
        }
    }
    // d_h0 = the carry step past chunk 0; its image [Dk][Dv] f32 lies over the chunk tiles (64 KiB at D = 128: all four of them)
    if (ST && a.d_h0) l_state_out<NST, D>(st, db, sdv, (float *)smem, D, a.d_h0 + bh * D * D, D);
}

// dg_r = sum_{t >= r} (a_t - b_t) (+ <d_hT, hT>, the carry's start, when a gradient came through the final state): one wave per (b, h) walks the sequence downwards in blocks of 64, a suffix scan inside the block
__global__ __launch_bounds__(64) void lin_dg_kernel(const LinArgs a) {
    const int64_t S = a.S, base = (int64_t)blockIdx.x * S;
    const int lane = threadIdx.x;
    float carry = a.wc ? a.wc[blockIdx.x] : 0.f;
    for (int64_t blk = (S + 63) / 64 - 1; blk >= 0; --blk) {
        const int64_t t = blk * 64 + lane;
        float x = t < S ? a.wa[base + t] - a.wb[base + t] : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float y = __shfl_down(x, o);
            if (lane + o < 64) x += y;
        }
        if (t < S) a.dg[base + t] = x + carry;
        carry += __shfl(x, 0);
    }
}

// ---- the recurrence, token by token ----------------------------------------------------------------------------------------------------
// S <- exp(g_t) S + k_t v_t^T, o_t = scale q_t S for t = 0 .. T - 1 on a state in memory: at T = 1 the call moves 2 Dk Dv 4 bytes a head
// beside a few hundred bytes of operands, so the design is the state's traffic. One workgroup per (b, h, 64 state columns): columns
// need no reduction across workgroups. Lane (rg = tid >> 4, cp = tid & 15) owns rows rg Dk / 16 .. of the 16-byte pack of columns
// 4 cp ..: Dk / 16 float4 registers (32 floats at D = 128), loaded once, all loads in flight together, kept across the T steps and
// stored once. The operands of up to L_TB steps are widened to f32 in LDS (with exp(g_t)) ahead of the steps; a step is then two
// broadcast LDS reads a row, a multiply and a fused multiply-add a state element, the lane's partial o over its rows, and the sum over
// the 16 row groups through LDS in the order 0 .. 15 (two parities: one barrier a step), scale, one rounding to 16 bits.
constexpr int L_TB = 16;
template <int D> constexpr int l_step_lds() { return (L_TB * (2 * D + 64) + L_TB + 2 * 16 * 64) * 4; }

template <bool BF, int D>
__global__ __launch_bounds__(256) void lin_step_kernel(const LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = D / 16, NS = D / 64;
    float *sq = (float *)smem, *sk = sq + L_TB * D, *sv = sk + L_TB * D, *se = sv + L_TB * 64, *red = se + L_TB;
    const int tid = threadIdx.x, cp = tid & 15, rg = tid >> 4;
    const int64_t bh = blockIdx.x / NS, T = a.S;
    const int slice = blockIdx.x % NS;
    float *sp = a.hT + bh * D * D + rg * R * D + slice * 64 + 4 * cp;
    float4 s[R];
#pragma unroll
    for (int j = 0; j < R; ++j) s[j] = *(const float4 *)(sp + j * D);
    const uint16_t *q = (const uint16_t *)a.q + bh * T * D, *k = (const uint16_t *)a.k + bh * T * D, *v = (const uint16_t *)a.v + bh * T * D + slice * 64;
    uint16_t *o = (uint16_t *)a.o + bh * T * D + slice * 64;
    const float *g = a.g + bh * T;
    for (int64_t t0 = 0; t0 < T; t0 += L_TB) {
        const int nb = (int)(T - t0 < L_TB ? T - t0 : L_TB);
        __syncthreads(); // the steps before have read their operands
        for (int i = tid; i < nb * D; i += 256) {
            sq[i] = l_f32<BF>(q[t0 * D + i]);
            sk[i] = l_f32<BF>(k[t0 * D + i]);
        }
        for (int i = tid; i < nb * 64; i += 256) sv[i] = l_f32<BF>(v[(t0 + (i >> 6)) * D + (i & 63)]);
        if (tid < nb) se[tid] = expf(g[t0 + tid]);
        __syncthreads();
        for (int t = 0; t < nb; ++t) {
            const float e = se[t];
            const float4 vv = *(const float4 *)(sv + t * 64 + 4 * cp);
            float kk[R], qq[R];
#pragma unroll
            for (int j = 0; j < R; j += 4) {
                *(float4 *)(kk + j) = *(const float4 *)(sk + t * D + rg * R + j);
                *(float4 *)(qq + j) = *(const float4 *)(sq + t * D + rg * R + j);
            }
            float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < R; ++j) {
                s[j].x = fmaf(kk[j], vv.x, e * s[j].x);
                s[j].y = fmaf(kk[j], vv.y, e * s[j].y);
                s[j].z = fmaf(kk[j], vv.z, e * s[j].z);
                s[j].w = fmaf(kk[j], vv.w, e * s[j].w);
                acc.x = fmaf(qq[j], s[j].x, acc.x);
                acc.y = fmaf(qq[j], s[j].y, acc.y);
                acc.z = fmaf(qq[j], s[j].z, acc.z);
                acc.w = fmaf(qq[j], s[j].w, acc.w);
            }
            float *rp = red + (t & 1) * (16 * 64);
            *(float4 *)(rp + rg * 64 + 4 * cp) = acc;
            __syncthreads();
            if (tid < 64) {
                float x = rp[tid];
#pragma unroll
                for (int r = 1; r < 16; ++r) x += rp[r * 64 + tid];
                o[(t0 + t) * D + tid] = (uint16_t)l_cvt16<BF>(x * a.scale);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) *(float4 *)(sp + j * D) = s[j];
}

// a_t and b_t; with a state, one more float per (b, h) behind them
size_t lin_ws_bytes(int64_t B, int64_t H, int64_t S, bool state) { return (size_t)(((2 * B * H * S + (state ? B * H : 0)) * 4 + 15) / 16 * 16); }

// the stateless entries are these with null states: the kernels are then the instantiations without the state flag
int lin_fwd(const char *who, const char *label, int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale, const void *q,
            const void *k, const void *v, const float *g, const float *h0, void *o, float *hT, void *stream) {
    KF_REQUIRE(q && k && v && g && o, KF_ERR_INVALID, "%s: null operand", who);
    const int rc = lin_check(who, dtype, B, H, S, Dk, Dv, scale);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(al16(q) && al16(k) && al16(v) && al16(g) && al16(o), KF_ERR_INVALID, "%s: an operand is not aligned to 16 bytes", who);
    KF_REQUIRE(al16_or_null(h0) && al16_or_null(hT), KF_ERR_INVALID, "%s: a state is not aligned to 16 bytes", who);
    hipStream_t st = as_stream(stream);
    LinArgs a{};
    a.q = (const char *)q; a.k = (const char *)k; a.v = (const char *)v; a.g = g; a.o = (char *)o;
    a.h0 = h0; a.hT = hT;
    a.S = S; a.scale = scale;
    const bool bf = dtype == KF_BF16, big = Dk == 128;
    const dim3 grid((unsigned)(B * H * (Dv / 64)));
    KF_PROF(label, st);
    return with_flags([&](auto BF, auto BIG, auto ST) {
        constexpr int D = decltype(BIG)::value ? 128 : 64;
        return launch(lin_fwd_kernel<decltype(BF)::value, D, decltype(ST)::value>, grid, dim3(256), (size_t)l_fwd_lds<D>(), st, a);
    }, bf, big, h0 || hT);
}

int lin_bwd(const char *who, const char *label, bool state_entry, int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale,
            const void *q, const void *k, const void *v, const float *g, const float *h0, const void *d_o, const float *d_hT, void *dq, void *dk,
            void *dv, float *dg, float *d_h0, void *workspace, size_t workspace_bytes, void *stream) {
    KF_REQUIRE(q && k && v && g && d_o && dq && dk && dv && dg, KF_ERR_INVALID, "%s: null operand", who);
    const int rc = lin_check(who, dtype, B, H, S, Dk, Dv, scale);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(al16(q) && al16(k) && al16(v) && al16(g) && al16(d_o) && al16(dq) && al16(dk) && al16(dv) && al16(dg), KF_ERR_INVALID,
               "%s: an operand is not aligned to 16 bytes", who);
    KF_REQUIRE(al16_or_null(h0) && al16_or_null(d_hT) && al16_or_null(d_h0), KF_ERR_INVALID, "%s: a state is not aligned to 16 bytes", who);
    KF_REQUIRE(!d_h0 || h0, KF_ERR_INVALID, "%s: d_h0 without h0", who);
    const size_t need = lin_ws_bytes(B, H, S, state_entry);
    KF_REQUIRE(workspace && workspace_bytes >= need, KF_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               workspace ? workspace_bytes : (size_t)0, need);
    KF_REQUIRE(al16(workspace), KF_ERR_INVALID, "%s: workspace is not aligned to 16 bytes", who);
    hipStream_t st = as_stream(stream);
    LinArgs a{};
    a.q = (const char *)q; a.k = (const char *)k; a.v = (const char *)v; a.g = g; a.d_o = (const char *)d_o;
    a.dq = (char *)dq; a.dk = (char *)dk; a.dv = (char *)dv; a.dg = dg;
    a.wa = (float *)workspace; a.wb = a.wa + B * H * S;
    a.h0 = h0; a.d_hT = d_hT; a.d_h0 = d_h0; a.wc = d_hT ? a.wb + B * H * S : nullptr;
    a.S = S; a.scale = scale;
    const bool bf = dtype == KF_BF16, big = Dk == 128;
    const dim3 grid((unsigned)(B * H));
    KF_PROF(label, st);
    const int r2 = with_flags([&](auto BF, auto BIG, auto ST) {
        constexpr int D = decltype(BIG)::value ? 128 : 64;
        const int r = launch(lin_bwd_asc_kernel<decltype(BF)::value, D, decltype(ST)::value>, grid, dim3(256), (size_t)l_asc_lds<D>(), st, a);
        return r != KF_OK ? r : launch(lin_bwd_desc_kernel<decltype(BF)::value, D, decltype(ST)::value>, grid, dim3(256), (size_t)l_desc_lds<D>(), st, a);
    }, bf, big, h0 || d_hT);
    return r2 != KF_OK ? r2 : launch(lin_dg_kernel, grid, dim3(64), 0, st, a);
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_linear_attn_fwd(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                  const void *v, const float *g, void *o, void *stream) {
    return lin_fwd("kf_linear_attn_fwd", dtype == KF_BF16 ? "linear_attn_fwd_bf16" : "linear_attn_fwd_f16", dtype, B, H, S, Dk, Dv, scale, q, k, v, g,
                   nullptr, o, nullptr, stream);
}

extern "C" int kf_linear_attn_state_fwd(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                        const void *v, const float *g, const float *h0, void *o, float *hT, void *stream) {
    return lin_fwd("kf_linear_attn_state_fwd", dtype == KF_BF16 ? "linear_attn_state_fwd_bf16" : "linear_attn_state_fwd_f16", dtype, B, H, S, Dk, Dv,
                   scale, q, k, v, g, h0, o, hT, stream);
}

extern "C" int kf_linear_attn_step(int dtype, int64_t B, int64_t H, int64_t T, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                   const void *v, const float *g, float *state, void *o, void *stream) {
    const char *who = "kf_linear_attn_step";
    KF_REQUIRE(q && k && v && g && state && o, KF_ERR_INVALID, "%s: null operand", who);
    const int rc = lin_check(who, dtype, B, H, T, Dk, Dv, scale);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(al16(q) && al16(k) && al16(v) && al16(g) && al16(state) && al16(o), KF_ERR_INVALID, "%s: an operand is not aligned to 16 bytes", who);
    hipStream_t st = as_stream(stream);
    LinArgs a{};
    a.q = (const char *)q; a.k = (const char *)k; a.v = (const char *)v; a.g = g; a.o = (char *)o;
    a.hT = state;
    a.S = T; a.scale = scale;
    const bool bf = dtype == KF_BF16, big = Dk == 128;
    const dim3 grid((unsigned)(B * H * (Dv / 64)));
    KF_PROF(bf ? "linear_attn_step_bf16" : "linear_attn_step_f16", st);
    return with_flags([&](auto BF, auto BIG) {
        constexpr int D = decltype(BIG)::value ? 128 : 64;
        return launch(lin_step_kernel<decltype(BF)::value, D>, grid, dim3(256), (size_t)l_step_lds<D>(), st, a);
    }, bf, big);
}

static int lin_ws_entry(const char *who, bool state, int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null bytes", who);
    const int rc = lin_check(who, dtype, B, H, S, Dk, Dv, 1.f);
    if (rc != KF_OK) return rc;
    *bytes = lin_ws_bytes(B, H, S, state);
    return KF_OK;
}

extern "C" int kf_linear_attn_bwd_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, size_t *bytes) {
    return lin_ws_entry("kf_linear_attn_bwd_workspace_bytes", false, dtype, B, H, S, Dk, Dv, bytes);
}

extern "C" int kf_linear_attn_state_bwd_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, size_t *bytes) {
    return lin_ws_entry("kf_linear_attn_state_bwd_workspace_bytes", true, dtype, B, H, S, Dk, Dv, bytes);
}

extern "C" int kf_linear_attn_bwd(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                  const void *v, const float *g, const void *d_o, void *dq, void *dk, void *dv, float *dg, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return lin_bwd("kf_linear_attn_bwd", dtype == KF_BF16 ? "linear_attn_bwd_bf16" : "linear_attn_bwd_f16", false, dtype, B, H, S, Dk, Dv, scale, q, k,
                   v, g, nullptr, d_o, nullptr, dq, dk, dv, dg, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int kf_linear_attn_state_bwd(int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale, const void *q, const void *k,
                                        const void *v, const float *g, const float *h0, const void *d_o, const float *d_hT, void *dq, void *dk,
                                        void *dv, float *dg, float *d_h0, void *workspace, size_t workspace_bytes, void *stream) {
    return lin_bwd("kf_linear_attn_state_bwd", dtype == KF_BF16 ? "linear_attn_state_bwd_bf16" : "linear_attn_state_bwd_f16", true, dtype, B, H, S, Dk,
                   Dv, scale, q, k, v, g, h0, d_o, d_hT, dq, dk, dv, dg, d_h0, workspace, workspace_bytes, stream);
}
