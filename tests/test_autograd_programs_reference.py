"""CPU: the generator of tests/autograd_programs.py against torch alone - what makes a mismatch in tests/test_gpu_autograd_programs.py this
project's fault and nobody else's. Every exact-tier program of the committed sweep (200 of the first block, 90 of the second with the
mixture-of-experts operators) gives the same gradient bits in f32 and in f64, every value is representable in its tensor's own dtype and lies
under the shadow's bound, and the sweep covers what it claims to cover (99 + 63 smooth programs: 11 + 7 featured operators). The first
blocks are pinned by a digest; every branch run_torch has for an operator of the second blocks is held against the project's own f64 numpy
reference of that operator."""
import collections
import hashlib

import numpy as np
import pytest
import torch

from tests import autograd_programs as AP

NP = {"f32": np.float32, "f64": np.float64}
# sha256 over describe(prog) and the bytes of every leaf, const and grad_output array (in that order, per program) of the exact seeds 0..199
# and then the smooth seeds 0..98, computed at the commit before the second blocks were added (b9e8423) by the function below.
FIRST_BLOCKS_DIGEST = "aae2293a879b24abe185c62ef8bdc4294a58ef584b1b7a57072f49252454334d"


@pytest.fixture(scope="module")
def exact_programs():
    return [AP.make_program(s, "exact") for s in AP.sweep("exact")]


@pytest.fixture(scope="module")
def smooth_programs():
    return [AP.make_program(s, "smooth") for s in AP.sweep("smooth")]


def programs_digest(programs):
    h = hashlib.sha256()
    for prog in programs:
        h.update(AP.describe(prog).encode())
        for _, a, _ in prog["leaves"]:
            h.update(a.tobytes())
        for c in prog["consts"]:
            h.update(c.tobytes())
        for g, _, _ in prog["grads"]:
            h.update(g.tobytes())
    return h.hexdigest()


def test_the_first_blocks_are_the_programs_they_were(exact_programs, smooth_programs):
    assert (AP.N_EXACT, AP.N_SMOOTH) == (200, 99) and AP.sweep("exact", 0, 1) == list(range(200)) and AP.sweep("smooth", 0, 1) == list(range(99))
    assert programs_digest(exact_programs[:200] + smooth_programs[:99]) == FIRST_BLOCKS_DIGEST
    for prog in exact_programs[:200]:   # the new instructions are drawn behind the first block only
        assert not any(op in AP.MOE_OPS for op, _, _, _ in prog["instrs"]), AP.describe(prog)


def test_a_shifted_seed_names_the_same_case_in_both_blocks():
    for shift in (1, 2, 5):
        for tier in ("exact", "smooth"):
            for s0, s in zip(AP.sweep(tier), AP.sweep(tier, shift)):
                assert AP.in_second_block(s0, tier) == AP.in_second_block(s, tier)
                assert (s0 % 12, s0 % 4) == (s % 12, s % 4)
                if tier == "smooth":
                    assert AP.smooth_case(s0) == AP.smooth_case(s)
    for shift in (1, 2, 3):   # every shifted seed yields a program too (shift 2 once met a cat of a powers-of-two leaf that had no partner)
        for tier in ("exact", "smooth"):
            for s in AP.sweep(tier, shift):
                assert AP.make_program(s, tier)["seed"] == s
    # the scenario of a second-block exact seed: read off the program (every scenario ends in its own instruction pattern)
    for s0 in AP.sweep("exact", 0, 2)[:9]:
        ops = lambda p: sorted(op for op, _, _, _ in p["instrs"] if op in AP.MOE_OPS)   # noqa: E731
        a, b = AP.make_program(s0, "exact"), AP.make_program(AP.SEED_STRIDE + s0, "exact")
        assert a["scenario"] == b["scenario"] == (s0 - AP.N_EXACT) % AP.N_SCENARIOS, (s0, ops(a), ops(b))


def test_no_program_of_the_sweep_is_dropped(exact_programs, smooth_programs):
    assert len(exact_programs) == AP.N_EXACT + AP.N_EXACT2 and len(smooth_programs) == AP.N_SMOOTH + AP.N_SMOOTH2   # the share of skipped cases is 0
    assert len(AP.sweep("exact", 0, 2)) == AP.N_EXACT2 == 90 and len(AP.sweep("smooth", 0, 2)) == AP.N_SMOOTH2 == 63
    for at in (7, AP.N_EXACT + 7):
        again = AP.make_program(AP.sweep("exact")[at], "exact")
        assert AP.describe(again) == AP.describe(exact_programs[at])   # a seed names one program


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
    for prog in exact_programs[:AP.N_EXACT]:
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
    for prog in smooth_programs[:AP.N_SMOOTH]:
        scount.update(prog["features"])
    for op in AP.SMOOTH_OPS:
        assert scount[op] >= 4 and scount[op + "_from_view"] >= 2 and scount[op + "_from_fanin"] >= 2, (op, scount)
        assert scount[op + "_noncontig_grad"] >= 1, (op, scount)   # its backward is handed a strided gradient (checked on the shadow's strides)
    reds = {prog["instrs"][k][3][1] for prog in smooth_programs for k in range(len(prog["instrs"])) if prog["instrs"][k][0] == "cross_entropy"}
    assert reds == {"none", "sum", "mean"}

    # ---- the second exact block: the mixture-of-experts operators in both dtypes, every scenario ten times, and what each has to reach
    count2 = collections.Counter()
    for prog in exact_programs[AP.N_EXACT:]:
        count2.update(prog["features"])
        count2["scenario_%d" % prog["scenario"]] += 1
        count2["base_" + prog["nodes"][0][1]] += 1
        assert any(op in AP.MOE_OPS and outs[0] in prog["reached"] for op, outs, _, _ in prog["instrs"]), AP.describe(prog)
    wanted2 = (list(AP.MOE_OPS) + ["scenario_%d" % i for i in range(AP.N_SCENARIOS)] + ["base_f32", "base_f64", "expert_linear_behind_a_conversion"] +
               ["expert_linear_offsets_" + k for k in ("offsets", "ids", "plan")] +
               ["expert_linear_empty_expert", "expert_linear_uncovered_rows", "expert_linear_x_column_window", "expert_linear_w_reached_twice",
                "expert_linear_w_also_through_gemm", "moe_dropped_pair", "moe_k1", "moe_k2", "moe_k3", "moe_gate_gather", "moe_gate_p_column_window"] +
               ["moe_combine_" + k for k in ("gate_none", "gate_leaf", "gate_from_moe_gate", "gate_requiring", "gate_not_requiring", "ys_requiring",
                                             "ys_not_requiring")] +
               ["double_backward", "noncontig_grad_permute", "noncontig_grad_step", "leaf_reached_twice", "non_requiring_leaf"])
    thin = {k: count2[k] for k in wanted2 if count2[k] < 3}
    assert not thin, thin

    # ---- the second smooth block: per operator the three modes, and every variant the operators' own edges ask for, at least once
    scount2 = collections.Counter()
    for prog in smooth_programs[AP.N_SMOOTH:]:
        scount2.update(prog["features"])
    for op in AP.SMOOTH_OPS2:
        assert scount2[op] >= 4 and scount2[op + "_from_view"] >= 2 and scount2[op + "_from_fanin"] >= 2, (op, scount2)
        assert scount2[op + "_noncontig_grad"] >= 1, (op, scount2)
    once = []
    for op in ("softmax", "log_softmax"):
        once += [op + k for k in ("_nonlast_dim", "_scale", "_column_window", "_permuted_view", "_dense")]
    for op in ("attention", "attention_qkv"):
        once += [op + k for k in ("_full", "_prefix", "_window", "_doc", "_kv_len_0", "_keyless_query", "_causal_no_prefix", "_prefix_len", "_hkv_h", "_hkv_1",
                                  "_window_causal", "_window_noncausal", "_window_left_none", "_window_left_0", "_window_left_small", "_window_right_none",
                                  "_window_right_0", "_window_right_small", "_doc_full", "_doc_causal", "_zero_length_document",
                                  "_token_in_no_document")]
    once.append("attention_skv_ne_sq")
    for op in ("rope_qkv", "qk_norm_rope"):
        once += [op + k for k in ("_positions", "_no_positions", "_interleaved", "_rotate_half", "_r_lt_d", "_hkv_h", "_hkv_1")]
    once += ["qk_norm_rope" + k for k in ("_both_weights", "_none_weight", "_no_tables", "_tables", "_weight_requiring", "_weight_not_requiring")]
    once += ["moe_gate_normalize", "moe_gate_p_column_window", "moe_dropped_pair", "moe_dispatch", "moe_combine", "moe_combine_gate_from_moe_gate"]
    missing = [k for k in once if scount2[k] < 1]
    assert not missing, missing


def test_smooth_tier_runs_in_torch_and_its_f32_noise_is_small(smooth_programs):
    for prog in smooth_programs:
        a, b = AP.run_torch(prog, torch.float32), AP.run_torch(prog, torch.float64, trace=True)
        assert np.isfinite(b["root"]).all(), AP.describe(prog)
        for op, outs, ins, par in prog["instrs"]:   # the featured operator works on data, not on a tensor that cancelled to a constant
            if op in AP.SMOOTH_OPS + AP.SMOOTH_OPS2:
                assert all(b["values"][i].std() > 0 for i in ins if i >= 0), AP.describe(prog)
            if op in ("attention", "attention_qkv"):   # some query has a key: an attention that sees nothing is all zeros and measures nothing
                assert b["values"][outs[0]].std() > 0, AP.describe(prog)
        reached = 0
        for i, g in b["grads"].items():
            if g is None:
                continue
            reached += 1
            assert np.isfinite(g).all() and a["grads"][i].shape == g.shape, (i, AP.describe(prog))
            # second block: no gradient is the residue of a cancellation (an operand broadcast along a softmax's dim, a per-head factor ahead of a
            # norm): such a tensor is 0 in exact arithmetic, and what f32 leaves of it says nothing about either engine. (The first block, kept
            # as it is, has one: seed 40, the [8, 1] shift under cross_entropy.)
            if AP.in_second_block(prog["seed"], "smooth"):
                assert np.abs(g).max() == 0.0 or np.abs(g).max() > 1e-6, (i, np.abs(g).max(), AP.describe(prog))
        assert reached >= 1, AP.describe(prog)
        assert np.abs(a["root"] - b["root"]).max() <= 1e-4 * max(1.0, np.abs(b["root"]).max()), AP.describe(prog)


# ---- run_torch's branches for the second blocks' operators against the project's f64 numpy references ------------------------------------------
def one_op(op, arrays, par, consts, gy):
    """run_torch in f64 on the one-instruction program op(arrays...) (None: an absent operand) under the gradient gy: (value, [gradients])."""
    leaves = [(i, np.asarray(a, np.float64), True) for i, a in enumerate(arrays) if a is not None]
    o = len(arrays)
    prog = {"leaves": leaves, "instrs": [(op, (o,), tuple(i if a is not None else -1 for i, a in enumerate(arrays)), par)], "consts": consts, "root": o,
            "grads": [(np.asarray(gy, np.float64), "plain", None)], "nodes": [(None, "f64", 0, 0, True)] * (o + 1)}
    res = AP.run_torch(prog, torch.float64)
    return res["root"], [res["grads"].get(i) for i in range(o)]


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want).max(initial=0.0)), (what, np.abs(got - want).max())


def test_run_torch_softmax_is_the_softmax_reference():
    from tests import softmax_ref as SR
    rng = np.random.default_rng(1)
    x, dy = rng.normal(0, 2, (5, 7)), rng.normal(0, 1, (5, 7))
    for op, kind in (("softmax", SR.SOFTMAX), ("log_softmax", SR.LOG_SOFTMAX)):
        for scale in (1.0, 0.5):
            y, (dx,) = one_op(op, [x], (-1, scale), [], dy)
            want, _ = SR.forward(kind, x, scale)
            close(y, want, (op, scale))
            close(dx, SR.backward(kind, want, dy, scale), (op, scale, "dx"))
            y, (dx,) = one_op(op, [x], (0, scale), [], dy)   # over the first dim: the reference on the transposed problem
            want, _ = SR.forward(kind, x.T, scale)
            close(y, want.T, (op, scale, "dim 0"))
            close(dx, SR.backward(kind, want, dy.T, scale).T, (op, scale, "dim 0 dx"))


def test_run_torch_qk_norm_rope_and_rope_qkv_are_the_qk_norm_reference():
    from tests import qk_norm_ref as QR
    rng = np.random.default_rng(2)
    B, S, H, D = 2, 3, 2, 8
    for kv, R, inter, use_pos, has_q, has_k in ((2, 4, True, True, True, True), (1, 8, False, False, False, True), (1, 0, False, False, True, False)):
        T, W = B * S, (H + 2 * kv) * D
        x, dy = rng.uniform(-2, 2, (T, W)), rng.uniform(-1, 1, (T, W))
        wq, wk = (rng.uniform(-2, 2, D) if has_q else None), (rng.uniform(-2, 2, D) if has_k else None)
        pos = rng.integers(0, 16, T).astype(np.int64) if use_pos else None
        cos, sin = AP.rope_tables(16, R) if R else (None, None)
        consts = [pos] if use_pos else []
        y, (dx, dwq, dwk) = one_op("qk_norm_rope", [x, wq, wk], (B, S, H, kv, R, inter, 0 if use_pos else None, 1e-6), consts, dy)
        want = QR.forward(x, wq, wk, cos, sin, pos, B, S, H, kv, kv, D, R, inter, 1e-6)[0]
        back = QR.backward(x, dy, wq, wk, cos, sin, pos, B, S, H, kv, kv, D, R, inter, 1e-6)
        what = (kv, R, inter, use_pos)
        close(y, want, what)
        close(dx, back["dx"], what + ("dx",))
        if has_q:
            close(dwq, back["dwq"], what + ("dwq",))
        if has_k:
            close(dwk, back["dwk"], what + ("dwk",))
        if R:   # rope_qkv: the rotation alone of the q and k heads (the reference's rotate), its backward the inverse rotation of dy
            y, (dx,) = one_op("rope_qkv", [x], (B, S, H, kv, R, inter, 0 if use_pos else None), consts, dy)
            c, s = QR.token_tables(cos, sin, pos, T, S, R)
            for got, src, inverse in ((y, x, False), (dx, dy, True)):
                src3 = src.reshape(T, H + 2 * kv, D)
                rot = QR.rotate(src3[:, :H + kv], c, s, R, inter, inverse=inverse)[0]
                close(got, np.concatenate([rot, src3[:, H + kv:]], 1).reshape(T, W), what + ("rope_qkv", inverse))


def _attention_masks():
    """(mask, consts, Skv) per family, each with its edge: a batch without keys, a padded causal batch, a prefix, a window that leaves queries
    without a key, documents with an empty one and a token in none."""
    K = lambda a: np.asarray(a, np.int64)   # noqa: E731
    return [(("full", 0, None, None, False, None), [K([0, 4])], 5),
            (("prefix", 0, None, None, True, None), [K([0, 5])], 5),
            (("prefix", 0, 1, None, True, None), [K([4, 0]), K([3, 1])], 5),
            (("window", 0, None, (0, 1), False, None), [K([2, 3])], 3),
            (("window", 0, None, (1, None), True, None), [K([1, 3])], 3),
            (("doc", None, None, None, False, 0), [K([[0, 1, 1, 2], [0, 3, 3, 3]])], 3),
            (("doc", None, None, None, True, 0), [K([[0, 1, 1, 2], [0, 3, 3, 3]])], 3)]


def _vis_of(mask, consts, B, Sq, Skv):
    """The visibility straight from the four reference functions (not through AP.attn_vis, which is under test here)."""
    from tests import attn_doc_ref, attn_full_ref, attn_prefix_ref, attn_window_ref
    fam, kv, pre, win, causal, doc = mask
    kvl = None if kv is None else consts[kv]
    if fam == "full":
        return attn_full_ref.key_len_vis(kvl, Sq, Skv, B)
    if fam == "prefix":
        return attn_prefix_ref.prefix_vis(kvl, None if pre is None else consts[pre], Sq, Skv, B)
    if fam == "window":
        return attn_window_ref.window_vis(kvl, win[0], 0 if causal else win[1], Sq, Skv, B)
    return attn_doc_ref.doc_vis(consts[doc], Sq, causal)


def test_run_torch_attention_is_the_attention_reference_under_each_visibility():
    from oracle import oracle as O
    from tests import attn_full_ref
    rng = np.random.default_rng(3)
    B, H, Sq, D = 2, 2, 3, 4
    for mask, consts, Skv in _attention_masks():
        for kv in (H, 1):
            q, go = (rng.uniform(-2, 2, (B, H, Sq, D)).astype(np.float32) for _ in range(2))
            k, v = (rng.uniform(-2, 2, (B, kv, Skv, D)).astype(np.float32) for _ in range(2))
            vis = _vis_of(mask, consts, B, Sq, Skv)
            assert vis.any() and not vis.any(-1).all(), mask   # every case has live rows and a query without a key
            ref = attn_full_ref.attn_ref64_vis(q, k, v, go, vis, O.F32)
            y, (dq, dk, dv) = one_op("attention", [q, k, v], mask, consts, go)
            for name, got in (("o", y), ("dq", dq), ("dk", dk), ("dv", dv)):
                close(got, ref[name], (mask, kv, name))
            if Skv != Sq:
                continue
            # the packed form: [B*S, (H + 2 kv) D], columns q | k | v, heads inside
            pack = lambda t: t.transpose(0, 2, 1, 3).reshape(B * Sq, -1)   # noqa: E731
            y, (dqkv,) = one_op("attention_qkv", [np.concatenate([pack(q), pack(k), pack(v)], 1)], (B, Sq, H, kv, mask), consts, pack(go))
            close(y, pack(ref["o"]), (mask, kv, "packed o"))
            close(dqkv, np.concatenate([pack(ref["dq"]), pack(ref["dk"]), pack(ref["dv"])], 1), (mask, kv, "packed gradient"))


def test_run_torch_expert_linear_is_the_segmented_gemm_reference():
    from tests import gemm_seg_ref as GS
    rng = np.random.default_rng(4)
    T, Din, Dout, E = 7, 3, 4, 3
    x, w, dy = rng.normal(0, 1, (T, Din)), rng.normal(0, 1, (E, Din, Dout)), rng.normal(0, 1, (T, Dout))
    ids = np.array([-1, 0, 0, 2, 2, 2, 3], np.int64)   # a row before every segment, expert 1 empty, a row behind
    for par, consts in ((("offsets", 0, E), [GS.segment_offsets(ids, E)]), (("ids", 0, E), [ids]), (("offsets", 0, E), [np.array([5, 2, 9, -3], np.int64)])):
        off = AP.host_offsets(par, consts, T)
        y, (dx, dw) = one_op("expert_linear", [x, w], par, consts, dy)
        close(y, GS.forward(x, w, off), par)
        close(dx, GS.forward(dy, w, off, trans_b=True), par + ("dx",))
        close(dw, GS.wgrad(x, dy, off), par + ("dw",))
    # the plan's offsets: E + 1 entries, the dropped pairs behind the last segment
    from tests import moe_ref as MR
    tk = np.array([[0, 2], [3, 1], [2, 2], [-1, 0]], np.int64)   # T k = 8 rows, two dropped pairs
    x8, dy8 = rng.normal(0, 1, (8, Din)), rng.normal(0, 1, (8, Dout))
    off = MR.plan(tk, E)[0]
    y, (dx, dw) = one_op("expert_linear", [x8, w], ("plan", 0, E), [tk], dy8)
    assert off[E] == 6
    close(y, GS.forward(x8, w, off), "plan")
    close(dx, GS.forward(dy8, w, off, trans_b=True), "plan dx")
    close(dw, GS.wgrad(x8, dy8, off), "plan dw")


def test_run_torch_routing_is_the_moe_reference():
    from tests import moe_ref as MR
    rng = np.random.default_rng(5)
    T, E, d = 5, 4, 3
    for k in (1, 2, 3):
        ids = np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int64)
        if k > 1:   # (normalize with every pair of a token dropped is 0 / 0)
            ids[1, 0], ids[3, k - 1] = E, -1
        offsets, row_pair, pair_row = MR.plan(ids, E)
        n = T * k
        p, dgate = rng.uniform(0.1, 1, (T, E)), rng.normal(0, 1, (T, k))
        for normalize in (False, True):
            gate, (dp,) = one_op("moe_gate", [p], (0, E, normalize), [ids], dgate)
            want = MR.gate_fwd(p, ids, E, normalize, "f32", exact=True)
            close(gate, want, ("gate", k, normalize))
            close(dp, MR.gate_bwd(p, ids, E, normalize, want, dgate, "f32", exact=True), ("dp", k, normalize))
        x, dxs = rng.normal(0, 1, (T, d)), rng.normal(0, 1, (n, d))
        xs, (dx,) = one_op("moe_dispatch", [x], (0, E), [ids], dxs)
        close(xs, MR.dispatch(x, row_pair, k), ("dispatch", k))
        close(dx, MR.combine(dxs, pair_row, None, None, T, k, "f32", exact=True)[0], ("dispatch dx", k))   # every pair's row, the dropped ones' too
        ys, dy, g = rng.normal(0, 1, (n, d)), rng.normal(0, 1, (T, d)), rng.normal(0, 1, (T, k))
        for gate in (None, g):
            y, (dys, dg) = one_op("moe_combine", [ys, gate], (0, E), [ids], dy)
            close(y, MR.combine(ys, pair_row, offsets[E], gate, T, k, "f32", exact=True)[0], ("combine", k, gate is None))
            wdys, wdg, _ = MR.combine_bwd(ys, pair_row, offsets[E], gate, dy, T, k, "f32", want_dgate=gate is not None, fill=0.0, exact=True)
            close(dys, wdys, ("dys", k, gate is None))
            if gate is not None:
                close(dg, wdg, ("dgate", k))
