"""not gpu: the generated attention forward (tools/gen_attn_fwd.py -> kfunca_amd/csrc/device/attn_fwd_w4.inc).

The tile body is one hand-placed instruction stream; what hipcc would otherwise do for it the generator does itself, and this test
holds it to that: (1) the address maps of the LDS image - what the DMA pieces write, what the K row reads and the transposed V reads
deliver as MFMA operands - agree in a pure-Python model (`selftest`); (2) every variant of the emitted stream keeps the distances the
hardware does not interlock (`check`: MFMA result -> VALU, VALU -> MFMA operand, LDS read -> use behind a wait); (3) the committed .inc is
what the generator writes today (nobody edited one without the other)."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


def test_address_maps_and_hazard_distances():
    import gen_attn_fwd as G
    assert G.selftest()
    for f16 in (False, True):
        for mut in (False, True):
            for scaled in (False, True):   # exact f32 scores (default) | the query scaled and rounded once per pass (KF_ATTN_SCALED_OPERANDS)
                g = G.Gen(f16, mut, scaled=scaled).build()
                assert G.check(g.out) == []
                variants = {i.text[2:-4] for i in g.out if i.kind == "label" and i.text.endswith("_%=:")}
                assert {"steady", "first", "masked", "firstmasked", "drain", "idle"} <= variants and ("steadydrop" in variants) == mut
                assert sum(1 for i in g.out if i.kind == "mfma") == (64 + 48 + 56 + 40 + 16 + (64 if mut else 0))  # MFMAs per variant: steady, first, masked, firstmasked, drain
                steady = [i for i in G.gap_table(g.out, "steady")]
                assert sum(r["n"] for r in steady) > 0


def test_committed_inc_is_the_generators_output(tmp_path):
    out = tmp_path / "w4.inc"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_attn_fwd.py"), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_text() == (ROOT / "kfunca_amd" / "csrc" / "device" / "attn_fwd_w4.inc").read_text(), "run tools/gen_attn_fwd.py"


def test_dkv_generator_address_maps_hazards_and_freshness(tmp_path):
    """The same three guarantees for the generated dK / dV pass (tools/gen_attn_dkv.py -> attn_dkv_w4.inc): tile-image model, hazard
    distances in every variant of the slice body (both dtypes, mutation build, with and without the dS stores), committed stream ==
    generator output."""
    import gen_attn_dkv as G
    assert G.selftest()
    for f16 in (False, True):
        for mut in (False, True):
            for ds in (True, False):
                for scaled in (False, True):   # exact f32 scores (default) | K scaled and rounded once per block
                    g = G.Gen(f16, mut, ds, scaled=scaled).build()
                    assert G.check(g.out) == []
                    assert sum(1 for i in g.out if i.kind == "mfma") == 16 + 64 + 64 + 32 + (64 if mut else 0)   # accumulator clearing, steady, diag1, diag0 (one sub-block), drop
                    stores = sum(1 for i in g.out if "global_store_dwordx4" in i.text)
                    assert stores == ((4 + 4 + 2 + (4 if mut else 0)) if ds else 0)
    out = tmp_path / "dkv.inc"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_attn_dkv.py"), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_text() == (ROOT / "kfunca_amd" / "csrc" / "device" / "attn_dkv_w4.inc").read_text(), "run tools/gen_attn_dkv.py"


def test_checkers_reject_a_transcendental_read_one_wait_state_later():
    """gfx950 does not interlock a transcendental's result against the very next instruction (measured round 4, tools/scratch/trans_hazard.hip:
    `v_exp; v_add` as neighbours leave the old value in the lanes with (lane & 4) == 0; one wait state is what the hardware needs). The
    generators keep one in reserve: both checkers must flag an adjacent consumer and the `s_nop 0` form, and accept two wait states or a
    real instruction in between; the forward's stream, built WITHOUT its repair pass,
    must trip the rule (the drain iteration has gaps without MFMAs)."""
    import gen_attn_dkv as D
    import gen_attn_fwd as G
    Ins, V = G.Ins, G.V
    exp = lambda: Ins("v_exp_f32 v1, v1", "trans", V(1), V(1))       # noqa: E731
    use = lambda: Ins("v_add_f32 v2, v2, v1", "valu", V(2) + V(1), V(2))  # noqa: E731
    other = lambda: Ins("v_mov_b32 v3, v4", "valu", V(4), V(3))      # noqa: E731
    nop = lambda n: Ins(f"s_nop {n}", "salu")                        # noqa: E731
    for mod, label in ((G, "L_steady_%=:"), (D, "L_steady_%=:")):
        body = lambda mid: [Ins(label, "label"), exp()] + mid + [use(), Ins("L_epilogue_%=:", "label")]  # noqa: E731
        assert any("transcendental" in p for p in mod.check(body([])))
        assert any("transcendental" in p for p in mod.check(body([nop(0)])))
        assert not any("transcendental" in p for p in mod.check(body([nop(1)])))
        assert not any("transcendental" in p for p in mod.check(body([other()])))
    g = G.Gen()
    g.fix_trans_use = lambda: None
    assert any("transcendental" in p for p in G.check(g.build().out))


def test_head_size_64_streams_hazards_counts_and_wait_fields():
    """Round 5: both generators at D = 64 (the reference's second fast head size). Hazard distances in every variant, the MFMA counts of
    the half-size tile / slice (32 per steady body), and - the regression of the round - no s_waitcnt field beyond what the hardware has:
    lgkmcnt is 4 bits wide (the first D = 64 dK/dV stream asked for lgkmcnt(23): the assembler refused it, the old library stayed in
    place, and nothing said so)."""
    import gen_attn_dkv as D
    import gen_attn_fwd as G
    for f16 in (False, True):
        for mut in (False, True):
            g = G.Gen(f16, mut, D=64).build()
            assert G.check(g.out) == []
            assert sum(1 for i in g.out if i.kind == "mfma") == (32 + 24 + 28 + 20 + 8 + (32 if mut else 0))   # steady, first, masked, firstmasked, drain (+ steadydrop)
            for ds in (True, False):
                d = D.Gen(f16, mut, ds, D=64).build()
                assert D.check(d.out) == []
                assert sum(1 for i in d.out if i.kind == "mfma") == 8 + 32 + 32 + 16 + (32 if mut else 0)        # accumulator clearing, steady, diag1, diag0, drop
    # (the width of the wait fields is a rule of the checker, for every stream: whole stream, not only the loop bodies)
    for d in (D.Gen(False, D=64).build(), D.Gen(False, D=128).build(), D.Gen(True, scaled=True).build()):
        assert D.check(d.out) == []
    for text, ok in (("s_waitcnt lgkmcnt(16)", False), ("s_waitcnt vmcnt(64)", False), ("s_waitcnt vmcnt(63) lgkmcnt(15)", True)):
        for mod in (G, D):
            probs = mod.check([mod.Ins(text, "wait", tag="auto"), mod.Ins("L_steady_%=:", "label"), mod.Ins("L_epilogue_%=:", "label")])
            assert (probs == []) == ok and all(re.search(r"lgkmcnt|vmcnt", p) for p in probs), (text, probs)
    inc = (ROOT / "kfunca_amd" / "csrc" / "device" / "attn_dkv_w4.inc").read_text() + (ROOT / "kfunca_amd" / "csrc" / "device" / "attn_fwd_w4.inc").read_text()
    for name in ("KF_DKV_W4_D64_ASM_BF16_DS", "KF_DKV_W4_D64_ASM_F16_NODS", "KF_FWD_W4_D64_ASM_BF16", "KF_FWD_W4_D64_ASM_F16"):
        assert f"#define {name} " in inc, name


def _flags(mod, body):
    """The checker's problems for `body` as the one loop body of a stream (so it is walked behind itself)."""
    return mod.check([mod.Ins("L_steady_%=:", "label")] + body + [mod.Ins("L_epilogue_%=:", "label")])


def test_checker_mfma_and_valu_distances_on_synthetic_streams():
    """Rules 1 and 2 of asm_stream.check, each on a stream that must be flagged and on the minimally repaired one."""
    import gen_attn_dkv as D
    import gen_attn_fwd as G
    for mod in (G, D):
        Ins, V, A = mod.Ins, mod.V, mod.A
        mfma = lambda d, a=120, c=None: Ins(f"v_mfma v[{d}:{d + 15}]", "mfma", V(a, 4) + V(a + 4, 4) + V(d if c is None else c, 16), V(d, 16), tag=f"m{d}")  # noqa: E731
        use = lambda: Ins("v_add_f32 v100, v100, v0", "valu", V(100) + V(0), V(100))     # noqa: E731
        other = lambda: Ins("v_mov_b32 v103, v104", "valu", V(104), V(103))              # noqa: E731
        nop = lambda n: Ins(f"s_nop {n}", "salu")                                         # noqa: E731
        # rule 1: an MFMA result is read by a VALU 0 / 1 MFMAs later (flagged), 2 MFMAs or 22 wait states later (passes); its own chain passes
        assert any("MFMA(s)" in p for p in _flags(mod, [mfma(0), use()]))
        assert any("MFMA(s)" in p for p in _flags(mod, [mfma(0), mfma(16), use()]))
        assert _flags(mod, [mfma(0), mfma(16), mfma(32), use()]) == []
        assert any("MFMA(s)" in p for p in _flags(mod, [mfma(0), nop(15), nop(3), use()]))
        assert _flags(mod, [mfma(0), nop(15), nop(4), use()]) == []
        assert _flags(mod, [mfma(0), mfma(0), mfma(0)]) == []
        assert any("MFMA(s)" in p for p in _flags(mod, [mfma(0), mfma(16, c=0), mfma(32), mfma(48)]))     # another chain's C operand is no chain
        assert any("overwrites" in p for p in _flags(mod, [mfma(0), Ins("v_mov_b32 v1, v104", "valu", V(104), V(1)), mfma(16), mfma(32)]))
        assert _flags(mod, [mfma(0), mfma(16), mfma(32), Ins("v_mov_b32 v1, v104", "valu", V(104), V(1)), other(), other(), other()]) == []
        # rule 2: a VALU result is an MFMA operand 1 .. 3 instructions later (flagged), 4 later (passes)
        wr = lambda: Ins("v_mov_b32 v121, v104", "valu", V(104), V(121))                  # noqa: E731
        tail = [mfma(16), mfma(32)]                                                       # (so that no VALU stands right behind an MFMA that wrote v0..)
        assert any("after a VALU wrote it" in p for p in _flags(mod, [wr(), mfma(0)] + tail))
        assert any("after a VALU wrote it" in p for p in _flags(mod, [wr(), other(), other(), mfma(0)] + tail))
        assert _flags(mod, [wr(), other(), other(), other(), mfma(0)] + tail) == []
        assert _flags(mod, [wr(), nop(2), mfma(0)] + tail) == []
        assert A(3, 2) == [("a", 3), ("a", 4)]


def test_checker_lds_reads_need_a_wait_that_covers_them():
    """Rule 4: the destination of an LDS read is read or rewritten only behind a wait that has retired the read; lgkmcnt(N) retires all but
    the youngest N, and a counted wait (N > 0) means that only while at most 15 reads are in flight."""
    import gen_attn_dkv as D
    import gen_attn_fwd as G
    for mod in (G, D):
        Ins, V = mod.Ins, mod.V
        rd = lambda i: Ins(f"ds_read_b128 v[{110 + 4 * i}:{113 + 4 * i}], v105", "lds", V(105), V(110 + 4 * i, 4))       # noqa: E731
        use = lambda i: Ins(f"v_add_f32 v100, v100, v{110 + 4 * i}", "valu", V(100) + V(110 + 4 * i), V(100))             # noqa: E731
        wait = lambda n: Ins(f"s_waitcnt lgkmcnt({n})", "wait", tag="auto")                                                # noqa: E731
        lds = lambda body: [p for p in _flags(mod, body) if "LDS read" in p]                                               # noqa: E731
        assert lds([rd(0), use(0), wait(0)])                                   # no wait in front of the use
        assert _flags(mod, [rd(0), wait(0), use(0)]) == []
        assert _flags(mod, [rd(0), rd(1), wait(1), use(0), wait(0), use(1)]) == []          # the older of two behind lgkmcnt(1)
        assert lds([rd(0), rd(1), wait(1), use(1), wait(0)])                   # the younger of two behind lgkmcnt(1)
        assert lds([rd(0), rd(0), wait(0)])                                    # rewritten by the next read
        assert lds([rd(0), rd(1), wait(1), use(0)])                            # behind itself: the younger read is still in flight when the body rewrites its register
        many = lambda n: [rd(i) for i in range(n)] + [wait(1), use(0), wait(0)]                                            # noqa: E731
        assert _flags(mod, many(15)) == []
        assert any("in flight" in p for p in _flags(mod, many(16)))            # a counted wait with 16 reads in flight: the 4-bit counter says nothing
        assert _flags(mod, [rd(i) for i in range(16)] + [wait(0), use(0)]) == []   # (lgkmcnt(0) always holds)


def test_checker_walks_every_ordered_pair_of_bodies():
    """The dispatch can follow any body with any other: what one body leaves in flight is judged at the head of every other one."""
    import gen_attn_dkv as D
    Ins, V = D.Ins, D.V
    rd = lambda: Ins("ds_read_b128 v[110:113], v105", "lds", V(105), V(110, 4))                   # noqa: E731
    use = lambda: Ins("v_add_f32 v100, v100, v110", "valu", V(100) + V(110), V(100))              # noqa: E731
    wait = lambda: Ins("s_waitcnt lgkmcnt(0)", "wait", tag="lgkm")                                 # noqa: E731
    steady = [Ins("L_steady_%=:", "label"), use(), rd(), wait()]          # fine behind itself and behind nothing
    diag1 = [Ins("L_diag1_%=:", "label"), wait(), use(), rd()]            # fine behind itself, and behind steady
    end = [Ins("L_epilogue_%=:", "label")]
    assert D.check(steady + end) == [] and D.check(diag1 + end) == []
    probs = D.check(steady + diag1 + end)
    assert probs and all(p.startswith("diag1 -> steady: ") and "LDS read" in p for p in probs), probs


def test_lds_rule_bites_on_the_real_dkv_stream():
    """finish_waits CONSTRUCTS the counted waits of the dK / dV stream; the checker must be able to tell when one is missing. The default
    stream's steady slice holds ten lgkmcnt waits: each is deleted in turn and steady -> steady is checked.
    Eight of them stand in front of the first use of a fragment or a row constant: without one, that use reads a register whose LDS read has
    not been retired. The other two are the `lgkmcnt(14)` that finish_waits puts in front of a sixteenth read: they guard no register -
    every use still has its own counted wait behind them - but the counter's 4-bit field: without them sixteen or more reads are in flight
    and the next counted wait says nothing (the second half of rule 4)."""
    import gen_attn_dkv as D
    g = D.Gen().build()
    at = [i for i, x in enumerate(g.out) if x.kind == "label" and re.match(D.VARIANTS, x.text)]
    body = g.out[at[0]:at[1]]
    assert body[0].text == "L_steady_%=:"
    end = [D.Ins("L_epilogue_%=:", "label")]
    assert D.check(body + end) == []
    waits = [i for i, x in enumerate(body) if "lgkmcnt" in x.text]
    assert len(waits) == 10
    found = {i: D.check(body[:i] + body[i + 1:] + end) for i in waits}
    assert sum(1 for p in found.values() if any("LDS read not yet waited for" in m for m in p)) >= 8
    for i in waits:
        if body[i].text == "s_waitcnt lgkmcnt(14)" and body[i + 1].kind == "lds":
            assert any("in flight" in m for m in found[i]), body[i + 1].text
