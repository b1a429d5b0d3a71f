"""CPU: the generator of tests/autograd_programs.py against torch alone - what makes a mismatch in tests/test_gpu_autograd_programs.py this
project's fault and nobody else's. Every exact-tier program of the committed sweep gives the same gradient bits in f32 and in f64, every
value is representable in its tensor's own dtype and lies under the shadow's bound, and the sweep covers what it claims to cover."""
import collections

import numpy as np
import pytest
import torch

from tests import autograd_programs as AP

NP = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def exact_programs():
    return [AP.make_program(s, "exact") for s in AP.sweep("exact")]


@pytest.fixture(scope="module")
def smooth_programs():
    return [AP.make_program(s, "smooth") for s in AP.sweep("smooth")]


def test_no_program_of_the_sweep_is_dropped(exact_programs, smooth_programs):
    assert len(exact_programs) == AP.N_EXACT and len(smooth_programs) == AP.N_SMOOTH   # the share of skipped cases is 0
    again = AP.make_program(AP.sweep("exact")[7], "exact")
    assert AP.describe(again) == AP.describe(exact_programs[7])   # a seed names one program


def test_exact_tier_is_exact_in_torch_alone(exact_programs):
    for prog in exact_programs:
        own, r32, r64 = AP.run_torch(prog), AP.run_torch(prog, torch.float32), AP.run_torch(prog, torch.float64, trace=True)
        what = AP.describe(prog)
        for res in (own, r32):
            assert np.array_equal(res["root"].astype(np.float64), r64["root"]), what
            for i, g in r64["grads"].items():
                assert (g is None) == (res["grads"][i] is None), what
                if g is not None:
                    assert res["grads"][i].shape == g.shape and np.array_equal(res["grads"][i].astype(np.float64), g), (i, what)
        for i, g in own["grads"].items():   # torch hands every leaf a gradient of the leaf's dtype and shape: what the GPU test asks of the engine
            if g is not None:
                leaf = next(a for j, a, _ in prog["leaves"] if j == i)
                assert g.dtype == leaf.dtype and g.shape == leaf.shape, (i, what)
        for i, v in r64["values"].items():
            shape, dt, bound, fbits, req = prog["nodes"][i]
            assert v.shape == tuple(shape), (i, what)
            assert np.array_equal(v.astype(NP[dt]).astype(np.float64), v), (i, what)                       # its own dtype holds it
            assert np.array_equal(v * 2.0 ** fbits, np.round(v * 2.0 ** fbits)), (i, what)                    # an integer over 2^fbits
            assert np.abs(v).max(initial=0.0) <= bound and bound * 2.0 ** fbits < AP.LIMIT, (i, what)
        for i, g in r64["node_grads"].items():
            if i not in prog["reached"]:
                continue
            bound, fbits = prog["gbounds"][i]
            assert np.abs(g).max(initial=0.0) <= bound and np.array_equal(g * 2.0 ** fbits, np.round(g * 2.0 ** fbits)), (i, what)
            assert bound * 2.0 ** fbits < AP.LIMIT, (i, what)


def test_the_sweep_covers_every_instruction_and_every_suspicion(exact_programs, smooth_programs):
    count = collections.Counter()
    for prog in exact_programs:
        count.update(prog["features"])
    kinds = ["add", "sub", "mul", "div", "adds", "subs", "muls", "divs", "contiguous", "to", "bf16", "permute", "getitem", "view", "split", "cat",
             "gemm", "gemm_fused", "embedding", "embedding_negative"]
    wanted = kinds + ["bcast_grad_add", "bcast_grad_sub", "bcast_grad_mul", "view_of_view_offset", "cat_repeat", "cat_mixed_dtype", "fanin3",
                      "leaf_reached_twice", "non_requiring_leaf", "double_backward", "noncontig_grad_permute", "noncontig_grad_step"]
    thin = {k: count[k] for k in wanted if count[k] < 3}
    assert not thin, thin
    fused = {"bias": 0, "mul": 0, "add": 0, "none": 0, "all": 0}   # programs with each tail operand, with none of them and with all three
    for prog in exact_programs:
        for op, outs, ins, par in prog["instrs"]:
            if op == "gemm_fused" and outs[0] in prog["reached"]:
                have = [k for k, i in zip(("bias", "mul", "add"), ins[2:]) if i >= 0]
                for k in have:
                    fused[k] += 1
                if not have:
                    fused["none"] += 1
                if len(have) == 3:
                    fused["all"] += 1
    assert all(v >= 1 for v in fused.values()), fused
    scount = collections.Counter()
    for prog in smooth_programs:
        scount.update(prog["features"])
    for op in AP.SMOOTH_OPS:
        assert scount[op] >= 4 and scount[op + "_from_view"] >= 2 and scount[op + "_from_fanin"] >= 2, (op, scount)
        assert scount[op + "_noncontig_grad"] >= 1, (op, scount)   # its backward is handed a strided gradient (checked on the shadow's strides)
    reds = {prog["instrs"][k][3][1] for prog in smooth_programs for k in range(len(prog["instrs"])) if prog["instrs"][k][0] == "cross_entropy"}
    assert reds == {"none", "sum", "mean"}


def test_smooth_tier_runs_in_torch_and_its_f32_noise_is_small(smooth_programs):
    for prog in smooth_programs:
        a, b = AP.run_torch(prog, torch.float32), AP.run_torch(prog, torch.float64, trace=True)
        assert np.isfinite(b["root"]).all(), AP.describe(prog)
        for op, outs, ins, par in prog["instrs"]:   # the featured operator works on data, not on a tensor that cancelled to a constant
            if op in AP.SMOOTH_OPS:
                assert all(b["values"][i].std() > 0 for i in ins if i >= 0), AP.describe(prog)
        reached = 0
        for i, g in b["grads"].items():
            if g is None:
                continue
            reached += 1
            assert np.isfinite(g).all() and a["grads"][i].shape == g.shape, (i, AP.describe(prog))
        assert reached >= 1, AP.describe(prog)
        assert np.abs(a["root"] - b["root"]).max() <= 1e-4 * max(1.0, np.abs(b["root"]).max()), AP.describe(prog)
