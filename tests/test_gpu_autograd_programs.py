"""-m gpu: the reverse-mode engine against torch's on random operator graphs (tests/autograd_programs.py: shared intermediates, broadcast
operands, views of views, repeated and mixed-dtype cat inputs, conversions inside the graph, double backward, non-contiguous grad_outputs).

Exact tier: by construction every value and every gradient is exactly representable (tests/test_autograd_programs_reference.py proves it in
torch alone), so every leaf's gradient has the leaf's shape and dtype and torch's BITS, and so has the root's value. No tolerance. Two seed
blocks: 200 programs of arithmetic, views, conversions, gemm / gemm_fused / embedding, and behind them 90 that also hold expert_linear,
moe_dispatch, moe_combine and moe_gate (a gather), which are exact on the tier's values too.

Smooth tier: f32 programs around one fused operator each - 99 for the 11 operators of the first block, 63 for the 7 of the second
(softmax, log_softmax, attention and attention_qkv in their four mask families, rope_qkv, qk_norm_rope, moe_gate(normalize=True) behind a
softmax) - the yardstick is torch in f64 on the same f32 inputs, and the bound comes from the reference alone: per compared tensor
|kfunca - torch64| <= C * max|torch32 - torch64| + 2^-23 * max|torch64|. C is the next power of two at or above 4 x the worst ratio the
committed sweep showed on an MI355X, per operator (DESIGN.md section 5 records the ratios): 16 for all but two of the second block's (C_BY_OP
below). The kernels' f32 summation order legitimately differs from torch's, and another seed must not flake."""
import collections
import os

import numpy as np
import pytest
import torch

import kfunca_amd as kfunca
from tests import autograd_programs as AP

pytestmark = pytest.mark.gpu
SEED = int(os.environ.get("KF_FUZZ_SEED", "0"))  # `KF_FUZZ_SEED=n pytest tests/test_gpu_autograd_programs.py`: other programs (0 = the committed sweep)
# Worst needed C per operator over the committed sweep on an MI355X: rms_norm 0.528, layer_norm 0.592, silu 0.548, gelu 0.473, swiglu 0.321, geglu 0.343,
# rope 0.198, cross_entropy 3.447, attn 2.024, attn_gqa 2.687, attn_qkv 3.384. 4 x 3.447 = 13.8; the next power of two:
C = 16.0
# The second block, by the same rule: softmax 1.601, log_softmax 0.273, attention 3.768, attention_qkv 11.195, rope_qkv 0.000 (every tensor
# within the floor), qk_norm_rope 4.578, moe_gate 0.762. Two of them need more than 16 and get their own C; every other operator keeps 16.
#   attention_qkv 11.195 (4 x = 44.8): seed 116, dv of a prefix-LM mask whose q is 4 x a uniform leaf, so scores reach |s| ~ 45. The error is
#       1.35e-6 on max|dv| = 1.97 (5.7 ulp) where torch's f32 is 1.0e-7 off. Supposed cause, not measured: the kernels form P as
#       exp2(s log2(e) - lse), which carries the rounding of the product (2^-24 |s| in the exponent) into P; torch subtracts the row maximum
#       first. The same kernels need 3.4 under the first block's attn_qkv, whose q is not scaled.
#   qk_norm_rope 4.578 (4 x = 18.3): seed 104, a [1, 1] leaf added to the operator's output and to a copy of it: its gradient is the sum of
#       768 grad_output values through the engine's broadcast reduction, 1.03e-6 off 2.58 (3.3 ulp), and ONE element of torch's f32
#       (1.6e-7 off) is a noisy yardstick. No other tensor of the operator's nine programs needs more than 4.
C_BY_OP = {"attention_qkv": 64.0, "qk_norm_rope": 32.0}


def exact_findings(mod, seeds):
    found = []
    for s in seeds:
        prog = AP.make_program(s, "exact")
        bad = AP.compare_exact(prog, AP.run_torch(prog), AP.run_kfunca(mod, prog))
        if bad:
            found.append((s, bad, prog))
    return found


def smooth_needs(mod, seeds):
    """[(seed, operator, what, needed C, err, noise, floor)] over the sweep; a program the module refuses counts as needing infinity."""
    rows = []
    for s in seeds:
        prog = AP.make_program(s, "smooth")
        kind = AP.smooth_case(s)[0]
        got = AP.run_kfunca(mod, prog)
        if got["error"] is not None:
            rows.append((s, kind, f"raised at {got['error'][0]}: {got['error'][1]}", float("inf"), 0.0, 0.0, 0.0))
            continue
        for row in AP.smooth_ratios(prog, AP.run_torch(prog, torch.float32), AP.run_torch(prog, torch.float64), got):
            rows.append((s, kind) + row)
    return rows


def check_exact(block):
    seeds = AP.sweep("exact", SEED, block)
    found = exact_findings(kfunca, seeds)
    print(f"exact tier, block {block}: {len(seeds)} programs, {len(found)} with findings")
    text = "\n".join(f"seed {s}: {bad}\n{AP.describe(prog)}" for s, bad, prog in found[:3])
    assert not found, f"{len(found)} of {len(seeds)} programs differ from torch; seeds {[s for s, _, _ in found][:20]}\n{text}"


def check_smooth(block, ops):
    rows = smooth_needs(kfunca, AP.sweep("smooth", SEED, block))
    worst, where = collections.defaultdict(float), {}
    for s, kind, what, need, err, noise, floor in rows:
        if need > worst[kind]:
            worst[kind], where[kind] = need, f"seed {s}, {what}: err {err:.3e}, noise {noise:.3e}, floor {floor:.3e}"
    for kind in ops:
        print(f"smooth tier: worst needed C for {kind}: {worst[kind]:.3f} ({where.get(kind, 'within the floor everywhere')})")
    over = [(s, kind, what, need, err, noise, floor) for s, kind, what, need, err, noise, floor in rows if not need <= C_BY_OP.get(kind, C)]
    assert not over, f"beyond C = {C} ({C_BY_OP}): {over[:5]}\n" + AP.describe(AP.make_program(over[0][0], "smooth"))


def test_exact_tier_gradients_have_torchs_bits():
    check_exact(1)


def test_exact_tier_moe_gradients_have_torchs_bits():
    check_exact(2)


def test_smooth_tier_gradients_within_the_reference_noise():
    check_smooth(1, AP.SMOOTH_OPS)


def test_smooth_tier_second_block_gradients_within_the_reference_noise():
    check_smooth(2, AP.SMOOTH_OPS2)
