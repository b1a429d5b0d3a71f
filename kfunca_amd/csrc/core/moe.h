// namespace gpu: the token routing of a mixture-of-experts layer on the device (kf_moe_plan, kf_moe_gate_*, kf_moe_dispatch,
// kf_moe_combine, kf_moe_combine_bwd) with autograd. No reference counterpart. Nothing is read back to the host between the router's
// top-k and the layer's result, so the layer can be captured in a graph:
//     p = softmax(x @ router); ids = p.topk(k)[1]; plan = moe_plan(ids, E); gate = moe_gate(p, plan, true); xs = moe_dispatch(x, plan);
//     h = expert_linear(xs, w_gate_up, plan.offsets); a = swiglu(h); ys = expert_linear(a, w_down, plan.offsets); y = moe_combine(ys, plan, gate)
#pragma once

#include <cstdint>
#include <utility>

#include "tensor.h"

namespace gpu {

// The routing of T tokens to k of E experts each, built once per layer and used by that layer's forward and backward. Pair p = t k + j is
// token t's j-th choice. row_pair Int [T k]: the pair in sorted row r (a stable sort by expert; a pair whose id lies outside [0, E) is
// dropped to the tail); pair_row Int [T, k]: its inverse; offsets Long [E + 1]: expert e owns the sorted rows offsets[e] .. offsets[e + 1]
// (what expert_linear takes), offsets[E] = the number of live pairs; ids: the Long [T, k] the plan was built from.
struct MoePlan {
    Tensor offsets, row_pair, pair_row, ids;
    int64_t T = 0, k = 0, E = 0;
};

// ids: Long [T, k] on the device (the indices of p.topk(k, -1, true)). One sort, no read-back; scratch comes from the allocator.
MoePlan moe_plan(const Tensor &ids, int64_t num_experts);

// p [T, E] (contiguous or row-pitched; float, half or bfloat16): gate[t, j] = p[t, ids[t, j]], 0 for a dropped pair; normalize divides by
// their sum over j (f32, in the order j). Differentiable in p: dp is zero off the chosen columns.
Tensor moe_gate(const Tensor &p, const MoePlan &plan, bool normalize = false);

// x [T, d] (contiguous or row-pitched, read in place) -> xs [T k, d]: xs[r] = x[row_pair[r] / k], bit for bit. Differentiable in x:
// dx[t] = sum_j dxs[pair_row[t, j]] in f32 in the order j (kf_moe_combine without a gate: a gather-sum, no sort).
Tensor moe_dispatch(const Tensor &x, const MoePlan &plan);

// ys [T k, d], gate [T, k] or undefined (1): y[t] = sum_j gate[t, j] ys[pair_row[t, j]] in f32 in the order j, rounded once; dropped
// pairs are skipped (neither their row nor their gate is read). Differentiable in ys and gate through one pass of kf_moe_combine_bwd:
// dys[pair_row[t, j]] = gate[t, j] dy[t] (zero for a dropped pair), dgate[t, j] = dy[t] . ys[pair_row[t, j]].
Tensor moe_combine(const Tensor &ys, const MoePlan &plan, const Tensor &gate = Tensor());

// The router in front of the plan, fused (kf_moe_router_*, kf_moe_aux_loss_*; no reference counterpart), so that the layer reads
//     logits = x @ router; ids, gate = moe_route(logits, k); plan = moe_plan(ids, E); aux = moe_aux_loss(logits, plan, ...)
//
// logits [T, E] (contiguous or row-pitched, read in place; float, half or bfloat16; E <= 1024, 1 <= k <= min(E, 64)). ids Long [T, k]:
// the first k positions of the stable descending order of each row in the sort's key order - logits.topk(k)[1] bit for bit. gate [T, k]:
// softmax(logits)[ids] (score 0) or sigmoid(logits[ids]) (score 1), divided by their sum over j when normalize. gate is differentiable
// in logits (one launch, every element of dlogits written, the row recomputed); ids carries no gradient.
std::pair<Tensor, Tensor> moe_route(const Tensor &logits, int64_t k, int score = 0, bool normalize = true);

// Float [1]: balance_coef L_bal + z_coef L_z with p = softmax(logits), L_bal = E / (T k) sum_e c_e mean_t p[t, e] (c_e the plan's live
// pairs of expert e, read on the device, a constant; 1 for uniform routing, HF-Mixtral's value is k times this) and L_z = mean_t lse_t^2.
// parts, when given, receives Float [2] = {L_bal, L_z} (no gradient). Differentiable in logits: the gradient is read from the device.
Tensor moe_aux_loss(const Tensor &logits, const MoePlan &plan, double balance_coef = 1e-2, double z_coef = 0.0, Tensor *parts = nullptr);

} // namespace gpu
