"""-m gpu: the reverse-mode engine against torch's on random operator graphs (tests/autograd_programs.py: shared intermediates, broadcast
operands, views of views, repeated and mixed-dtype cat inputs, conversions inside the graph, double backward, non-contiguous grad_outputs).

Exact tier: by construction every value and every gradient is exactly representable (tests/test_autograd_programs_reference.py proves it in
torch alone), so every leaf's gradient has the leaf's shape and dtype and torch's BITS, and so has the root's value. No tolerance.

Smooth tier: f32 programs around one fused operator each; the yardstick is torch in f64 on the same f32 inputs, and the bound comes from the
reference alone: per compared tensor |kfunca - torch64| <= C * max|torch32 - torch64| + 2^-23 * max|torch64|. C is the next power of two at or
above 4 x the worst ratio the committed sweep showed on an MI355X (DESIGN.md section 5 records the ratios per operator): the kernels' f32
summation order legitimately differs from torch's, and another seed must not flake."""
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


def test_exact_tier_gradients_have_torchs_bits():
    seeds = AP.sweep("exact", SEED)
    found = exact_findings(kfunca, seeds)
    print(f"exact tier: {len(seeds)} programs, {len(found)} with findings")
    text = "\n".join(f"seed {s}: {bad}\n{AP.describe(prog)}" for s, bad, prog in found[:3])
    assert not found, f"{len(found)} of {len(seeds)} programs differ from torch; seeds {[s for s, _, _ in found][:20]}\n{text}"


def test_smooth_tier_gradients_within_the_reference_noise():
    rows = smooth_needs(kfunca, AP.sweep("smooth", SEED))
    worst = collections.defaultdict(float)
    for s, kind, what, need, err, noise, floor in rows:
        worst[kind] = max(worst[kind], need)
    for kind in AP.SMOOTH_OPS:
        print(f"smooth tier: worst needed C for {kind}: {worst[kind]:.3f}")
    over = [(s, kind, what, need, err, noise, floor) for s, kind, what, need, err, noise, floor in rows if not need <= C]
    assert not over, f"beyond C = {C}: {over[:5]}\n" + AP.describe(AP.make_program(over[0][0], "smooth"))
