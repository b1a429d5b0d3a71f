#!/usr/bin/env python3
"""Generator of the 16-bit causal-attention dK / dV kernel for gfx950 as ONE hand-placed instruction stream
(kfunca_amd/csrc/device/attn_dkv_w4.inc, included by attention.hip). The reference has no backward at all
(src/core/binary_ops.cpp:16-33 is its only GradFunction); this is the kernel VERDICT round 3 #2 asks for:

  * a workgroup = 4 waves = 256 keys of one (batch, head); a wave = 64 keys (two 32-key sub-blocks) and the whole register file:
      a[0:127]   dV^T accumulators [ksb][db]     a[128:255] dK^T accumulators [ksb][db]          (never leave; no atomics: bitwise reproducible)
      v[128:191] K fragments [ksb][kk] (pre-scaled by scale log2 e)      v[192:255] V fragments [ksb][kk]        (B operands, loaded once)
      v[0:31]    S accumulators [ksb] -> p = exp2(S'') in place          v[32:63]   dP accumulators -> dS = p dP' in place -> packed in place
      v[64:79]   P packed [ksb][s]                                        v[80:111]  ONE ring of 8 A-operand fragments
      v[112:127] addresses and temporaries
  * "key on the lane": S = Q K^T and dP = dO V^T come out with the key on the lane and the query in the register, which makes the
    accumulators - packed - the B operands of dV^T += dO^T P and dK^T += Q^T dS with no lane movement (cdna_hip_programming.md, section 3).
    A query slice (32 queries) is 64 MFMAs in four slots of 16:  S | dP | dV | dK, each slot ksb-major, so the 8 fragments of its A
    operand (Q rows | dO rows | dO^T | Q^T of the slice) serve BOTH key sub-blocks: 512 B of LDS reads per MFMA, half of the 32-key
    kernel's. The 8 fragments live in one ring: slot j of the ring is free after its second MFMA and takes fragment j of the NEXT set.
  * row constants as initial accumulators: -lse log2(e) and -delta of the slice's queries are read straight into the S and dP
    accumulator registers, the chains start from them (C = D), p = exp2(S'') needs no subtraction.
  * Q / dO slices (+ their 64 row constants) arrive by LDS-DMA into a two-slot ring, one slice ahead, 4 + 1 pieces per wave; ONE barrier
    per slice (in front of slot 4, whose MFMAs read no LDS); dS = P o (dP - delta), already packed as the dK product's operands, leaves
    with 4 write-through stores per slice for the dQ kernel (the layout of DS_TILE in attention.hip).
  * causal: a wave's first two computed slices are its diagonal ones (variants diag0 / diag1, the fully masked sub-block's MFMAs are
    not issued); earlier slices it only keeps the DMA and the barrier going (idle).
LDS waits are COUNTED and inserted by the generator (`finish_waits`): before an instruction that reads the destination of a pending LDS
read, s_waitcnt lgkmcnt(N) with N = the reads issued after that one."""
import argparse
import functools
import os
import re
import sys
from pathlib import Path

import asm_stream
from asm_stream import A, Ins, V, ar, m0_write, render, sr, vr  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "kfunca_amd" / "csrc" / "device" / "attn_dkv_w4.inc"

# ------------------------------------------------------------------ register map
def S(ksb, e=0): return 16 * ksb + e
def DP(ksb, e=0): return 32 + 16 * ksb + e
def DSP(ksb, s): return 32 + 16 * ksb + 4 * s      # packed dS of k-step s: the first 8 registers of the sub-block's dP tuple
def P(ksb, s): return 64 + 8 * ksb + 4 * s
def RING(j): return 80 + 4 * j
RB, TB, LR = (112, 113), (114, 115), 116
DMAQ, DMAD, DMAC, DSOFF, RM = 117, 118, 119, 120, 121
T = [64, 65, 66, 67, 68, 69]   # prologue / epilogue temporaries: the P registers, idle then
# (K / V fragments and the dV / dK accumulators depend on the head size: Gen.KFR / VFR / DV / DK)

Q_SRD, DO_SRD, C_SRD, O_SRD = 36, 40, 44, 48
S_QOFF, S_DOOFF, S_COFF, S_QSTEP, S_DOSTEP, S_QMAX, S_DOMAX, S_CMAX = 52, 53, 54, 55, 56, 57, 58, 59
S_M0, S_IT, S_NS, S_D0, S_TMP, S_TMP2 = 60, 61, 62, 63, 64, 65
S_DS0, S_DS1 = 66, 68   # pairs
S_SL, S_STAGE = 70, 71
S_WID, S_LDS, S_SCALE, S_MUT, S_OSR = "%[wid]", "%[lds]", "%[scale]", "%[mut]", "%[osr]"   # read-only inputs: used in place
S_X0, S_X1 = 72, 73
S_DSSTEP = 74           # bytes from the last slice of the current query block to the first of the next one in the dS workspace (ds_next)
S_SPAN = 75             # 32-key sub-blocks between this wave's two (its second diagonal slice comes S_SPAN slices behind the first): 7 - 2 w balanced, 1 adjacent
V_SRD = 76             # 4-aligned quad: the V fragments' descriptor (prologue only)
S_PSH = 76             # f16 streams, from the end of the prologue on: 2^P_SHIFT as a float (the multiplier of the P pack, below)
S_M0C, S_MKT, S_MKC = 77, 78, 79   # from the end of the prologue on: DMA destination of the row constants; the ring's XOR masks (tiles | constants)
P_SHIFT = 14           # f16: P is carried as P 2^14 (<= 16384: cannot overflow; subnormal only below 3.7e-9 instead of 6.1e-5), dV scaled back in the epilogue
N_SGPR_HI = 80
N_VGPR = 250            # v250 .. v255 stay the compiler's (it needs somewhere to keep scalars it cannot hold in SGPRs)

# S and dP slots: sub-block 1's FIRST k-step goes first (its C operand is sub-block 0's registers, which still hold the row constants),
# then sub-block 0's chain, then the rest of sub-block 1's: the 16 constants of a slice are read once, not once per sub-block.
CHAIN_ORDER = [(1, 0)] + [(0, i) for i in range(8)] + [(1, i) for i in range(1, 8)]
# ring slot j's last use in those slots: slot 0 at gap 1, slot j >= 1 at gap 8 + j; in the dV / dK slots (ksb-major) slot j at gap 8 + j
RING_FREE_S = [1] + [8 + j for j in range(1, 8)]
NEXTQ_G = [56 + j for j in range(8)]

# Round 5: a FOUR-slot slice ring in the 64 KiB the two-slot ring had (round 4: two slots of 32 KiB, half of each unused). A slot = the Q tile
# (8 KiB) + the dO tile (8 KiB); the 64 row constants of a slice live in their own 4 x 256 B area behind the ring. The DMA of slice it + 2 then
# overwrites the slot slice it - 2 was read from - a whole slice behind every wave's last read of it - so the slice barrier no longer has to
# prove "all my LDS reads of this slot have returned" (s_waitcnt lgkmcnt(0) in front of it: the transposed Q reads issued in the eight gaps
# before stalled there every slice: tools/attn_dkv_w4_timeline.py, "barrier wait + barrier + slot dK" 993 cycles for 512 of matrix pipe); it only
# publishes the next slice's arrival. Slot b -> b + 1 (mod 4) is an XOR with 0x4000 (b even) or 0xC000 (b odd): one SGPR mask that flips bit
# 15 every slice; the constants' area steps by 256 the same way (0x100 / 0x300). (All of it relies on the dynamic LDS starting at a
# multiple of 64 KiB - offset 0 - as the two-slot XOR did.)
BUF = 16384             # one ring slot: Q tile | dO tile
NBUF = 4
SLICE_DO = 8192         # dO tile behind the Q tile
CBASE = NBUF * BUF      # 4 x (32 x -lse / scale | 32 x -delta)
CSLOT = 256
STAGE0 = CBASE + NBUF * CSLOT
STAGE_ROW = 272
LDS_BYTES = STAGE0 + 4 * 64 * STAGE_ROW
DS_TILE = 2048


class Gen(asm_stream.Emitter):
    # non-temporal: measured same-box against write-through (sc0 sc1), sc1 and plain stores (tools/scratch/ab_dkv.sh): this kernel's time is the same
    # under all four (1.99 - 2.04 ms on that box), the dQ kernel that streams the dS back runs 3 - 4 % faster behind nt stores (0.95 - 0.97 vs 1.00 ms)
    store_policy = "nt"
    skip_tail_dma = False   # (A/B: --skip-tail-dma; measured same-box: no gain, 1.98 - 2.07 ms with it against 1.97 - 2.00 without)

    def __init__(self, f16=False, mutant=False, ds=True, ablate=(), stamps=False, scaled=False, D=128):
        # D = 64 (round 5, VERDICT round 4 #4: the reference's second fast head size, causal_attention_kernel.cu:40-52): the same stream with half
        # the k-steps and half the column blocks - 32 MFMAs per slice in four slots of 8 (slice64), the same per-score VALU work, so the
        # slice is VALU-issue bound where D = 128 is matrix bound. The LDS images keep their 256-byte rows with only the first 128 used: every
        # address formula, swizzle and read instruction is the D = 128 one, a tile's 8-row group is ONE 1-KiB DMA piece instead of two.
        super().__init__(f16, mutant, ablate, stamps, scaled, D)
        self.ds = ds
        # early (D = 128): the scalar bookkeeping of a slice - ring step + source offsets of the next request (10 s_*), dS tile addresses (11 s_*) - runs in
        # slot S of the slice that USES it (gaps 10, 12) instead of slot dK of the slice before (gaps 50, 62): slot dK is the full one (DMA pieces, dS stores,
        # ring toggles, the next slice's head reads). The prologue then leaves both one step behind.
        self.early = D == 128 and os.environ.get("KF_GEN_DKV_EARLY", "0") == "1"
        # balanced (round 6, VERDICT round 5 next #1 lever i): wave w owns the block's 32-key sub-blocks w and 7 - w instead of 2 w and 2 w + 1. A wave
        # then has ONE sub-block at work from slice w on and both from slice 7 - w on: the pass's first four slices cost a one-sub-block slice (1.9 k
        # cycles) instead of a full one for the sake of wave 0 alone while waves 1..3 idled. One more variant of the slice body ("half": sub-block 0
        # only, unmasked). Results are bit-identical (a key's sums run over the same slices in the same order; the whole attention suite + the mutants
        # pass on it). MEASURED same-box, five interleaved pairs (profiles/r06_ab_ds_layout.txt): 1.942 ms against 1.932 for the adjacent form - the
        # 2.1 k cycles per pass the timeline promised (1.1 %) do not show: OFF (KF_GEN_DKV_BALANCED=1 builds it; the mutation build's defect 2 in
        # attention.hip then wants wave 3 at slice 5).
        self.balanced = D == 128 and bool(os.environ.get("KF_GEN_DKV_BALANCED"))
        kf0 = 122
        self.KFR = lambda ksb, kk: kf0 + 4 * self.NKK * ksb + 4 * kk
        self.VFR = lambda ksb, kk: kf0 + 8 * self.NKK + 4 * self.NKK * ksb + 4 * kk
        self.DV = lambda ksb, db: 16 * self.NDB * ksb + 16 * db
        self.DK = lambda ksb, db: 32 * self.NDB + 16 * self.NDB * ksb + 16 * db
        # scaled: K is multiplied by scale log2(e) and ROUNDED to the element type once per block, the row constant is -lse log2(e), and the S
        # accumulator is the exponent (no multiply per score: -32 VALU per slice, no scaling pass in the prologue... and a score error of
        # eps scale sum|q k| that grows with the logits; KF_ATTN_SCALED_OPERANDS). Default: exact f32 scores - K as it is, the row
        # constant is -lse / scale, one multiply by %[scale] (= scale log2(e) then) per score in front of its exp2.
        # stamps (tools/attn_dkv_w4_timeline.py, -DKF_DKV_W4_STAMPS): s_memtime sums per wave and block pass. A whole stamp() stands where nothing is
        # in flight (prologue, epilogue); in the loop stamp_take() requests the clock and stamp_add() uses it BEHIND a wait the stream has anyway (the slice
        # barrier's lgkmcnt(0)), so the stamps do not drain the LDS reads in flight - the schedule measured is the product's. Buckets: 0 block start -> head
        # reads, 1 steady / 2 diag1 / 3 diag0 / 4 idle slices (barrier to barrier, booked one slice late), 5 last booked barrier -> epilogue, 6 epilogue,
        # 7 the number of steady slices.

    def mm(self, d, dn, a, b, c=None, tag="", acc="v"):
        """D = A B + C on registers: d first of 16 (VGPR or AGPR by `acc`), a / b first of 4 VGPRs, C = D unless `c` names another tuple."""
        if os.environ.get("KF_GEN_DKV_PROBE_16X16"):
            # TIMING PROBE ONLY (wrong results): the same FLOPs as two v_mfma_f32_16x16x32 on the same operand registers - what would the cheaper
            # matrix shape buy under the power cap? (tools/scratch: never in the product)
            m16 = self.mfma.replace("32x32x16", "16x16x32")
            r = (lambda i, n: vr(i, n)) if acc == "v" else (lambda i, n: ar(i, n))
            W = V(d, 16) if acc == "v" else A(d, 16)
            cc = d if c is None else c
            cr = (lambda i: r(i, 4)) if c is None else (lambda i: vr(i, 4))
            self.out.append(Ins(f"{m16} {r(d, 4)}, {vr(a, 4)}, {vr(b, 4)}, {cr(cc)}", "mfma", V(a, 4) + V(b, 4) + (W if c is None else V(c, 16)), W, tag=tag))
            self.out.append(Ins(f"{m16} {r(d + 8, 4)}, {vr(a, 4)}, {vr(b, 4)}, {cr(cc + 8)}", "raw"))
            return
        dst = vr(d, 16) if acc == "v" else ar(d, 16)
        W = V(d, 16) if acc == "v" else A(d, 16)
        if c is None:
            self.out.append(Ins(f"{self.mfma} {dst}, {vr(a, 4)}, {vr(b, 4)}, {dst}", "mfma", V(a, 4) + V(b, 4) + W, W, tag=tag))
        else:
            self.out.append(Ins(f"{self.mfma} {dst}, {vr(a, 4)}, {vr(b, 4)}, {vr(c, 16)}", "mfma", V(a, 4) + V(b, 4) + V(c, 16), W, tag=tag))

    def lds_row(self, dst, kk, tile_off):      # A fragment of k-step kk of a 32-row tile: row = lane & 31, chunk 2 kk + (lane >> 5)
        if "lds" in self.ablate: return
        self.out.append(Ins(f"ds_read_b128 {vr(dst, 4)}, {vr(RB[kk & 1])} offset:{tile_off + 512 * (kk >> 1)}", "lds", V(RB[kk & 1]), V(dst, 4)))

    def lds_tr(self, dst, s, db, sec, tile_off):  # half of the transposed fragment (k-step s = queries 16 s .., column block db)
        if "lds" in self.ablate: return
        self.out.append(Ins(f"ds_read_b64_tr_b16 {vr(dst + 2 * sec, 2)}, {vr(TB[sec])} offset:{tile_off + 2048 * (2 * s + sec) + 512 * db}", "lds",
                            V(TB[sec]), V(dst + 2 * sec, 2)))

    def lds_const(self, dst, g, off):           # 4 of the 16 row constants of this lane: rows 8 g + 4 h + {0..3}
        if "lds" in self.ablate: return
        self.out.append(Ins(f"ds_read_b128 {vr(dst + 4 * g, 4)}, {vr(LR)} offset:{off + 32 * g}", "lds", V(LR), V(dst + 4 * g, 4)))

    def dma_slice(self, seps=()):
        """This wave's pieces of one slice: rows 8 w .. 8 w + 7 of the Q tile and of the dO tile (two 1-KiB pieces each), and the 64 row
        constants (every wave fetches them: identical bytes, uniform counts). seps: up to five one-instruction emitters that stand between an
        M0 write and its request instead of an s_nop (any left over are emitted behind the last request)."""
        seps = list(seps)
        nxt = lambda: seps.pop(0) if seps else None  # noqa: E731
        self.dma(Q_SRD, DMAQ, S_QOFF, S_M0, 0, 0, sep=nxt())
        if self.D == 128: self.dma(Q_SRD, DMAQ, S_QOFF, S_M0, 896, 128, sep=nxt())
        self.dma(DO_SRD, DMAD, S_DOOFF, S_M0, SLICE_DO, 0, sep=nxt())
        if self.D == 128: self.dma(DO_SRD, DMAD, S_DOOFF, S_M0, SLICE_DO + 896, 128, sep=nxt())
        self.dma(C_SRD, DMAC, S_COFF, S_M0C, dword=True, sep=nxt())
        for f in seps:
            f()

    def ring_step(self):
        """DMA destinations one ring slot on (slot b -> b + 1 mod 4: XOR 0x4000 from an even slot, 0xC000 from an odd one; the read bases
        made the same step behind the barrier, with the same masks), then the masks for the next slice."""
        self.salu(f"s_xor_b32 {sr(S_M0)}, {sr(S_M0)}, {sr(S_MKT)}")
        self.salu(f"s_xor_b32 {sr(S_M0C)}, {sr(S_M0C)}, {sr(S_MKC)}")
        self.salu(f"s_xor_b32 {sr(S_MKT)}, {sr(S_MKT)}, {2 * BUF}")
        self.salu(f"s_xor_b32 {sr(S_MKC)}, {sr(S_MKC)}, {2 * CSLOT}")

    def advance_dma(self):
        """Source offsets one slice further, saturating at the block's last slice (a clamped slice is fetched again and never used)."""
        for off, step, mx in ((S_QOFF, S_QSTEP, S_QMAX), (S_DOOFF, S_DOSTEP, S_DOMAX)):
            self.salu(f"s_add_u32 {sr(off)}, {sr(off)}, {sr(step)}")
            self.salu(f"s_min_u32 {sr(off)}, {sr(off)}, {sr(mx)}")
        self.salu(f"s_add_u32 {sr(S_COFF)}, {sr(S_COFF)}, 128")
        self.salu(f"s_min_u32 {sr(S_COFF)}, {sr(S_COFF)}, {sr(S_CMAX)}")

    # -------------------------------------------------------------- one slice of one variant
    def slice(self, name, kind, prev_stores):
        """kind: 'steady' | 'diag0' (sub-block 0 on the diagonal, sub-block 1 wholly above it: not computed) | 'diag1' (sub-block 0 visible,
        sub-block 1 on the diagonal) | 'idle' | 'drop' (mutation build: the slice's probabilities are zero)."""
        compute = kind != "idle"
        ksbs = [0] if kind in ("diag0", "half") else [0, 1]
        G = [[] for _ in range(64)]
        def put(g, key, fn): G[g].append((key, fn))
        self.in_loop = True
        nvalu = "valu" in self.ablate

        # ---- the ring: fragment j of the next set goes into slot j behind the slot's second use (gap 8 + j of the MFMA slot in front)
        if compute:
            for j in range(8):
                put(max(RING_FREE_S[j], 6 + j), (2, j), lambda j=j: self.lds_row(RING(j), j, SLICE_DO))    # dO rows, for slot 2
                for sec in (0, 1):
                    put(16 + max(RING_FREE_S[j], 6 + j), (2, 2 * j + sec), lambda j=j, sec=sec: self.lds_tr(RING(j), j >> 2, j & 3, sec, SLICE_DO))  # dO^T, slot 3
                    put(40 + j, (2, 2 * j + sec), lambda j=j, sec=sec: self.lds_tr(RING(j), j >> 2, j & 3, sec, 0))         # Q^T, slot 4
            # -delta of this slice's queries into sub-block 0's dP accumulator (sub-block 1's chain takes it as its C operand before
            # sub-block 0's chain overwrites it: SECOND_FIRST below): behind the previous slice's dK MFMAs, ahead of slot 2
            for g in range(4):
                put(2 + g, (1, g), lambda g=g: self.lds_const(DP(0), g, 128))
        # ---- what the NEXT slice's head expects, read from the other buffer behind the barrier (every variant, idle ones too):
        #      -lse log2 e into the S accumulators, its Q rows into the ring
        for g in range(4):
            put(52 + g, (1, g), lambda g=g: self.lds_const(S(0), g, 0))
        for j in range(8):
            put(NEXTQ_G[j], (2, j), lambda j=j: self.lds_row(RING(j), j, 0))

        # ---- arithmetic
        if compute and not nvalu:
            for ksb in ksbs:
                e0, m0 = (10, 27) if ksb == 0 else (25, 34)
                if not self.scaled and ksb == 0:
                    e0 = 11    # exact scores: sub-block 0's multiplies take gaps 10 .. 25, its exps follow one gap behind (two exps share gaps 25, 26)
                diag = (kind == "diag0" and ksb == 0) or (kind == "diag1" and ksb == 1)
                for n in range(16):
                    x, d = S(ksb, n), DP(ksb, n)
                    if not self.scaled:   # exponent = (score - lse / scale) * scale log2(e): the accumulator holds the bracket
                        put(e0 + n - 1, (0, -1), lambda x=x: self.valu(f"v_mul_f32 {vr(x)}, {sr(S_SCALE)}, {vr(x)}", V(x), V(x)))
                    if kind == "drop":
                        put(e0 + n, (0, 0), lambda x=x: self.valu(f"v_mov_b32 {vr(x)}, 0", (), V(x)))
                    else:
                        put(e0 + n, (0, 0), lambda x=x: self.valu(f"v_exp_f32 {vr(x)}, {vr(x)}", V(x), V(x), trans=True))
                    if diag:  # key r > query (n & 3) + 8 (n >> 2) + 4 h  <=>  r - 4 h > kc
                        kc = (n & 3) + 8 * (n >> 2)
                        def m(x=x, kc=kc):
                            self.valu(f"v_cmp_lt_i32 vcc, {kc}, {vr(RM)}", V(RM), [("vcc", 0)])
                            self.valu(f"v_cndmask_b32_e64 {vr(x)}, {vr(x)}, 0, vcc", V(x) + [("vcc", 0)], V(x))
                        put(e0 + n + 1, (0, 1), m)
                    if self.f16:
                        # f16 (round 5): both packs are mixed-precision FMAs that multiply in f32 and round ONCE to f16 - the same number of VALU
                        # instructions as multiply + multiply + convert. P leaves as P 2^14 (the f16 format holds nothing below 6e-8 and nothing
                        # exactly below 6.1e-5: at large logits whole key columns of P sat there and dV lost them - VERDICT round 4 #1; dV is
                        # scaled back in the epilogue); dS = p dP' is rounded once instead of twice and stays at its natural scale (no shift is safe:
                        # |dS| has no bound the kernel knows).
                        if n % 2 == 1:
                            pd = P(ksb, n // 8) + (n % 8) // 2
                            def pk(x=x, pd=pd):
                                self.valu(f"v_fma_mixlo_f16 {vr(pd)}, {vr(x - 1)}, {sr(S_PSH)}, 0", V(x - 1), V(pd))
                                self.valu(f"v_fma_mixhi_f16 {vr(pd)}, {vr(x)}, {sr(S_PSH)}, 0", V(x) + V(pd), V(pd))
                            put(e0 + n + 2, (0, 2), pk)
                            dd = DP(ksb, n // 2)
                            put(m0 + n - 1, (0, 3), lambda x=x, d=d, dd=dd: self.valu(f"v_fma_mixlo_f16 {vr(dd)}, {vr(x - 1)}, {vr(d - 1)}, 0", V(x - 1) + V(d - 1), V(dd)))
                            put(m0 + n, (0, 3), lambda x=x, d=d, dd=dd: self.valu(f"v_fma_mixhi_f16 {vr(dd)}, {vr(x)}, {vr(d)}, 0", V(x) + V(d) + V(dd), V(dd)))
                        continue
                    if n % 2 == 1:
                        pd = P(ksb, n // 8) + (n % 8) // 2
                        put(e0 + n + 2, (0, 2), lambda x=x, pd=pd: self.valu(f"{self.cvt} {vr(pd)}, {vr(x - 1)}, {vr(x)}", V(x - 1) + V(x), V(pd)))
                    put(m0 + n, (0, 3), lambda x=x, d=d: self.valu(f"v_mul_f32 {vr(d)}, {vr(x)}, {vr(d)}", V(x) + V(d), V(d)))
                    if n % 2 == 1:
                        dd = DP(ksb, n // 2)
                        put(m0 + n + 2, (0, 4), lambda d=d, dd=dd: self.valu(f"{self.cvt} {vr(dd)}, {vr(d - 1)}, {vr(d)}", V(d - 1) + V(d), V(dd)))
        # (round 6) the five requests of slice it + 2 in gaps 0..4 - slot S, whose gaps hold next to nothing - instead of all five in gap 49 behind the barrier:
        # same-box 1.844 / 1.849 ms against 1.873 / 1.868 (two runs of 4-5 interleaved pairs; gaps 2..6 the same, 6..10 and 12..16 half of it, all five in gap 0
        # +1.7 %; profiles/r06_ab_ds_layout.txt). KF_GEN_DKV_DMA_GAPS="49": the old form; "g0,..,g4": one request per listed gap.
        env_gaps = os.environ.get("KF_GEN_DKV_DMA_GAPS", "0,1,2,3,4" if self.D == 128 else "49")
        dma_gaps = [] if env_gaps.strip() == "49" else [int(x) for x in env_gaps.split(",") if x]
        # ---- behind the barrier: ring toggle, DMA of slice it + 2 into the buffer this slice has finished with, then this slice's dS
        # the five read-base toggles of the ring step (behind the barrier, ahead of the next slice's head reads at gap 52) - round 6: each between an M0
        # write and the request that reads it, where an s_nop stood (KF_GEN_DKV_NOP_SEP=1: the old form, toggles at gap 48 and five s_nop)
        toggles = [lambda r=r: self.valu(f"v_xor_b32 {vr(r)}, {sr(S_MKT)}, {vr(r)}", V(r), V(r)) for r in (RB[0], RB[1], TB[0], TB[1])]
        toggles.append(lambda: self.valu(f"v_xor_b32 {vr(LR)}, {sr(S_MKC)}, {vr(LR)}", V(LR), V(LR)))
        nop_sep = bool(os.environ.get("KF_GEN_DKV_NOP_SEP")) or self.skip_tail_dma
        def after_barrier():
            for f in toggles: f()
        if nop_sep: put(48, (-3, 0), after_barrier)
        def dma_guarded():
            # slice it + 2 of this pass - if there is one: round 4 re-fetched the clamped last slice twice per pass (never used), and the
            # epilogue waited ~2.5 k cycles for those ten pieces (tools/attn_dkv_w4_timeline.py: "last barrier -> epilogue")
            self.salu(f"s_add_u32 {sr(S_TMP)}, {sr(S_IT)}, 2")
            self.salu(f"s_cmp_lt_u32 {sr(S_TMP)}, {sr(S_NS)}")
            self.salu(f"s_cbranch_scc0 L_nodma_{name}_%=")
            self.dma_slice()
            self.label(f"L_nodma_{name}_%=")
        # Where the five requests of slice it + 2 stand. They write the ring slot of slice it - 2, which every wave finished reading before the barrier of
        # slice it - 1: ANY gap of this slice is safe. Default: all behind the barrier in gap 49 (with the toggles as separators). KF_GEN_DKV_DMA_GAPS="g0,..,g4":
        # one piece per listed gap (round 6 experiment: a piece costs ~60 cycles of issue, a gap hides at most 24 of them - five pieces in gap 49 leave the
        # matrix pipe idle for ~320 cycles, spread over five slack gaps for ~220 by the issue model).
        if dma_gaps and not self.skip_tail_dma:
            assert len(dma_gaps) == 5 and all(0 <= g < 62 for g in dma_gaps) and dma_gaps == sorted(dma_gaps), dma_gaps
            if not nop_sep: put(48, (-3, 0), after_barrier)
            pieces = [(Q_SRD, DMAQ, S_QOFF, 0, 0), (Q_SRD, DMAQ, S_QOFF, 896, 128), (DO_SRD, DMAD, S_DOOFF, SLICE_DO, 0), (DO_SRD, DMAD, S_DOOFF, SLICE_DO + 896, 128)]
            for pc, g in zip(pieces, dma_gaps[:4]):
                put(g, (-9, 0), lambda pc=pc: self.salu(m0_write(S_M0, pc[3])))      # (M0 at the head of the gap - in a "dma" ablation too -, the request at its end)
                put(g, (9, 0), lambda pc=pc: self.dma_load(pc[0], pc[1], pc[2], pc[4]))
            put(dma_gaps[4], (-9, 0), lambda: self.salu(m0_write(S_M0C)))
            put(dma_gaps[4], (9, 0), lambda: self.dma_load(C_SRD, DMAC, S_COFF, dword=True))
        else:
            put(49, (3, 0), dma_guarded if self.skip_tail_dma else (self.dma_slice if nop_sep else (lambda: self.dma_slice(toggles))))
        def book():
            self.ring_step()
            self.advance_dma()
        put(10 if self.early else max([50] + [g + 1 for g in dma_gaps]), (4, 0), book)   # (the ring step and the next source offsets: behind the slice's last request)
        nst = 0
        if self.ds and compute and "stores" not in self.ablate:
            order = [(0, 0, 54), (0, 1, 56), (1, 0, 58), (1, 1, 60)]
            for ksb, s, g in order:
                if ksb not in ksbs:
                    continue
                nst += 1
                base = S_DS0 if ksb == 0 else S_DS1
                put(g, (5, 0), lambda ksb=ksb, s=s, base=base: self.out.append(
                    Ins(f"global_store_dwordx4 {vr(DSOFF)}, {vr(DSP(ksb, s), 4)}, {sr(base, 2)} offset:{1024 * s} {self.store_policy}", "vmem", V(DSOFF) + V(DSP(ksb, s), 4))))
        put(62, (6, 0), self.ds_next)

        self.label(f"L_{name}_%=")
        for g in range(64):
            slot, j = g // 16, g % 16
            if self.stamps and kind == "steady" and g in (0, 16, 32):
                self.salu(f"s_memtime s[{92 + 2 * (g // 16)}:{93 + 2 * (g // 16)}]")     # slot boundaries of a steady slice (consumed behind the barrier's wait)
            if g == 48:
                if self.stamps and kind == "steady":
                    self.salu("s_memtime s[98:99]")                                          # in front of the barrier's wait
                # this wave's pieces of the NEXT slice have landed (the stores issued behind them may still be on their way), every LDS
                # read of the current buffer has returned; then everyone's
                # (no lgkmcnt here: the slot this slice reads is not rewritten before slice it + 2's request, two barriers on; the stamps build
                #  keeps the full wait - it consumes its clock requests behind it)
                # (what may still be in flight: the previous slice's stores - and, when this slice's own requests stand in front of the barrier, those five)
                n_vm = prev_stores + (5 if dma_gaps and not self.skip_tail_dma and max(dma_gaps) < 48 and "dma" not in self.ablate else 0)
                if self.stamps:
                    self.wait(vm=n_vm, lgkm=0)
                else:
                    self.wait(vm=n_vm)
                self.barrier()
                # diagnostic build: the clock requested behind the PREVIOUS barrier has long returned (the wait above covers it): the period
                # that ended there is booked now - one slice late, so a kind's bucket holds its predecessor's period at every change of
                # kind (4 per pass) - and the next request goes out; nothing waits for it and no LDS read is drained for it (a counted
                # wait behind it can only be stricter by one).
                self.stamp_add({"steady": 1, "drop": 1, "diag1": 2, "diag0": 3, "half": 3, "idle": 4}[kind])
                self.stamp_take()
                if self.stamps and kind == "steady":
                    self.salu("s_add_u32 s90, s90, 1")        # bucket 6 is written at the very end: until then s90 counts the steady slices
                    # slots S | dP | dV of this slice (gap 0 -> 16 -> 32 -> the barrier's wait); what is left of the slice is wait + barrier + slot dK
                    for acc, hi, lo in ((91, 94, 92), (100, 96, 94), (101, 98, 96)):
                        self.salu(f"s_sub_u32 s83, s{hi}, s{lo}")
                        self.salu(f"s_add_u32 s{acc}, s{acc}, s83")
            ksb, i = j >> 3, j & 7
            if slot < 2:
                ksb, i = CHAIN_ORDER[j]
            if compute and ksb in ksbs:
                c_from = None
                if slot < 2 and ksb == 1 and i == 0:
                    c_from = S(0) if slot == 0 else DP(0)      # the row constants, still untouched in sub-block 0's registers
                if slot == 0: self.mm(S(ksb), 16, RING(i), self.KFR(ksb, i), tag=f"S ksb{ksb} kk{i}", c=c_from)
                elif slot == 1: self.mm(DP(ksb), 16, RING(i), self.VFR(ksb, i), tag=f"dP ksb{ksb} kk{i}", c=c_from)
                elif slot == 2: self.mm(self.DV(ksb, i & 3), 16, RING(i), P(ksb, i >> 2), tag=f"dV ksb{ksb} s{i >> 2} db{i & 3}", acc="a")
                else: self.mm(self.DK(ksb, i & 3), 16, RING(i), DSP(ksb, i >> 2), tag=f"dK ksb{ksb} s{i >> 2} db{i & 3}", acc="a")
            else:
                self.out.append(Ins("", "nomfma"))
                if compute and j == 9 and slot < 2:
                    self.salu("s_nop 15")   # diag0: the chain that has just ended gets its time before its first reader
                    self.salu("s_nop 7")
            for _, fn in sorted(G[g], key=lambda t: t[0]):
                fn()
        self.in_loop = False
        self.stores_of = getattr(self, "stores_of", {})
        self.stores_of[kind] = nst

    # -------------------------------------------------------------- one slice, head size 64: 32 MFMAs in four slots of 8
    def slice64(self, name, kind, vm_ok):
        """Same products, same accumulators, same LDS images as slice(); what changes is the count (4 k-steps, 2 column blocks) and with it
        the whole placement: gap g of 32, slots S 0..7 | dP 8..15 | dV 16..23 | dK 24..31. A gap is 32 cycles of matrix pipe at D = 128 and at
        D = 64, but the per-score VALU work is the same: this slice is VALU-issue bound, its gaps are short, and an LDS read eight gaps ahead of
        its consumer (the D = 128 distance) is only ~300 cycles ahead - it came back late at every slot head (first form of this stream: 2170
        cycles per slice). Head size 64 leaves 64 vector registers free (K / V fragments are half as many), so here every fragment set has its OWN
        registers and is read a whole slice (24 gaps) ahead:
            RA Q rows   v[80:95]   consumer slot S  of slice it + 1, read at gaps  8..11 of slice it
            RB dO rows  v[96:111]  consumer slot dP of slice it + 1, read at gaps 16..19
            RC dO^T     v[186:201] consumer slot dV of slice it + 1, read at gaps 24..27
            RD Q^T      v[202:217] consumer slot dK of slice it,     read at gaps  0.. 3 (compute variants only; in front of everything else)
            -lse / scale of slice it + 1 -> S accumulators at gaps 24, 25; -delta -> dP accumulators at 28, 29
        All of slice it + 1's reads sit behind the slice barrier, which moves to gap 8 (in front of slot dP), and the DMA requests run THREE
        slices ahead (the four-slot ring allows it: slice it + 3 overwrites the slot of slice it - 1, whose last read was consumed before
        this barrier): slice it + 1, published by this barrier, was requested two slices ago. vm_ok = what may still be in flight at the
        barrier's wait (the requests of slice it + 2 and the dS stores of the two slices before: build() derives it per variant)."""
        compute = kind != "idle"
        ksbs = [0] if kind == "diag0" else [0, 1]
        NG, BAR = 32, 8
        G = [[] for _ in range(NG)]
        def put(g, key, fn):
            assert 0 <= g < NG, g
            G[g].append((key, fn))
        self.in_loop = True
        nvalu = "valu" in self.ablate
        ORDER = [(1, 0)] + [(0, i) for i in range(4)] + [(1, i) for i in range(1, 4)]
        RA, RB_, RC, RD = (lambda i: 80 + 4 * i), (lambda i: 96 + 4 * i), (lambda i: 186 + 4 * i), (lambda i: 202 + 4 * i)
        if compute:
            for i in range(4):        # Q^T of THIS slice (slot dK); fragment (s, db) = (i >> 1, i & 1); RD(i)'s last use was gap 28 + i of the previous slice
                for sec in (0, 1):
                    put(i, (-5, 2 * i + sec), lambda i=i, sec=sec: self.lds_tr(RD(i), i >> 1, i & 1, sec, 0))
        # everything the NEXT slice reads, behind the barrier, in EVERY variant and in one fixed order (finish_waits counts on it)
        for kk in range(4):           # RA(kk)'s last use is gap [1, 5, 6, 7][kk]
            put(BAR + kk, (2, kk), lambda kk=kk: self.lds_row(RA(kk), kk, 0))
        for kk in range(4):           # RB(kk)'s last use is gap [9, 13, 14, 15][kk]
            put(16 + kk, (2, kk), lambda kk=kk: self.lds_row(RB_(kk), kk, SLICE_DO))
        for g in range(4):            # the S accumulators are free once sub-block 0's dS multiplies have read p (gap 22)
            put(24 + g // 2, (1, g), lambda g=g: self.lds_const(S(0), g, 0))
        for i in range(4):            # RC(i)'s last use is gap 20 + i
            for sec in (0, 1):
                put(24 + i, (2, 2 * i + sec), lambda i=i, sec=sec: self.lds_tr(RC(i), i >> 1, i & 1, sec, SLICE_DO))
        for g in range(4):            # sub-block 0's dP tuple is free behind its dK MFMAs (24 .. 27) and dS stores (26, 27)
            put(28 + g // 2, (1, g), lambda g=g: self.lds_const(DP(0), g, 128))

        if compute and not nvalu:
            for ksb in ksbs:
                e0, m0 = (6, 15) if ksb == 0 else (11, 19)   # score n: multiply at e0 + n // 2, exp2 one gap on; dS multiply at m0 + n // 2
                diag = (kind == "diag0" and ksb == 0) or (kind == "diag1" and ksb == 1)
                for n in range(16):
                    x, d = S(ksb, n), DP(ksb, n)
                    ge, gm = e0 + n // 2, m0 + n // 2
                    put(ge, (0, -1), lambda x=x: self.valu(f"v_mul_f32 {vr(x)}, {sr(S_SCALE)}, {vr(x)}", V(x), V(x)))
                    if kind == "drop":
                        put(ge + 1, (0, 0), lambda x=x: self.valu(f"v_mov_b32 {vr(x)}, 0", (), V(x)))
                    else:
                        put(ge + 1, (0, 0), lambda x=x: self.valu(f"v_exp_f32 {vr(x)}, {vr(x)}", V(x), V(x), trans=True))
                    if diag:
                        kc = (n & 3) + 8 * (n >> 2)
                        def m(x=x, kc=kc):
                            self.valu(f"v_cmp_lt_i32 vcc, {kc}, {vr(RM)}", V(RM), [("vcc", 0)])
                            self.valu(f"v_cndmask_b32_e64 {vr(x)}, {vr(x)}, 0, vcc", V(x) + [("vcc", 0)], V(x))
                        put(ge + 2, (0, 1), m)
                    if n % 2 == 1:
                        pd, dd = P(ksb, n // 8) + (n % 8) // 2, DP(ksb, n // 2)
                        if self.f16:   # (see slice(): P leaves as P 2^14, dS is rounded once)
                            def pk(x=x, pd=pd):
                                self.valu(f"v_fma_mixlo_f16 {vr(pd)}, {vr(x - 1)}, {sr(S_PSH)}, 0", V(x - 1), V(pd))
                                self.valu(f"v_fma_mixhi_f16 {vr(pd)}, {vr(x)}, {sr(S_PSH)}, 0", V(x) + V(pd), V(pd))
                            put(ge + 3, (0, 2), pk)
                            def dsk(x=x, d=d, dd=dd):
                                self.valu(f"v_fma_mixlo_f16 {vr(dd)}, {vr(x - 1)}, {vr(d - 1)}, 0", V(x - 1) + V(d - 1), V(dd))
                                self.valu(f"v_fma_mixhi_f16 {vr(dd)}, {vr(x)}, {vr(d)}, 0", V(x) + V(d) + V(dd), V(dd))
                            put(gm, (0, 3), dsk)
                        else:
                            put(ge + 3, (0, 2), lambda x=x, pd=pd: self.valu(f"{self.cvt} {vr(pd)}, {vr(x - 1)}, {vr(x)}", V(x - 1) + V(x), V(pd)))
                    if not self.f16:
                        put(gm, (0, 3), lambda x=x, d=d: self.valu(f"v_mul_f32 {vr(d)}, {vr(x)}, {vr(d)}", V(x) + V(d), V(d)))
                        if n % 2 == 1:
                            dd = DP(ksb, n // 2)
                            put(gm + 1, (0, 4), lambda d=d, dd=dd: self.valu(f"{self.cvt} {vr(dd)}, {vr(d - 1)}, {vr(d)}", V(d - 1) + V(d), V(dd)))
        def after_barrier():
            for r in (RB[0], RB[1], TB[0], TB[1]):
                self.valu(f"v_xor_b32 {vr(r)}, {sr(S_MKT)}, {vr(r)}", V(r), V(r))
            self.valu(f"v_xor_b32 {vr(LR)}, {sr(S_MKC)}, {vr(LR)}", V(LR), V(LR))
        put(BAR, (-3, 0), after_barrier)
        put(BAR + 1, (3, 0), self.dma_slice)
        def book():
            # the DMA side runs three slots ahead of the read side: the other parity, so the other step mask
            self.salu(f"s_xor_b32 {sr(S_TMP)}, {sr(S_MKT)}, {2 * BUF}")
            self.salu(f"s_xor_b32 {sr(S_M0)}, {sr(S_M0)}, {sr(S_TMP)}")
            self.salu(f"s_xor_b32 {sr(S_TMP)}, {sr(S_MKC)}, {2 * CSLOT}")
            self.salu(f"s_xor_b32 {sr(S_M0C)}, {sr(S_M0C)}, {sr(S_TMP)}")
            self.salu(f"s_xor_b32 {sr(S_MKT)}, {sr(S_MKT)}, {2 * BUF}")
            self.salu(f"s_xor_b32 {sr(S_MKC)}, {sr(S_MKC)}, {2 * CSLOT}")
            self.advance_dma()
        put(BAR + 2, (4, 0), book)
        nst = 0
        if self.ds and compute and "stores" not in self.ablate:
            for ksb, s_, g in [(0, 0, 26), (0, 1, 27), (1, 0, 29), (1, 1, 30)]:
                if ksb not in ksbs:
                    continue
                nst += 1
                base = S_DS0 if ksb == 0 else S_DS1
                put(g, (5, 0), lambda ksb=ksb, s_=s_, base=base: self.out.append(
                    Ins(f"global_store_dwordx4 {vr(DSOFF)}, {vr(DSP(ksb, s_), 4)}, {sr(base, 2)} offset:{1024 * s_} {self.store_policy}", "vmem", V(DSOFF) + V(DSP(ksb, s_), 4))))
        put(31, (6, 0), self.ds_next)

        self.label(f"L_{name}_%=")
        for g in range(NG):
            slot, j = g // 8, g % 8
            if g == BAR:
                self.wait(vm=vm_ok)
                self.barrier()
            ksb, i = j >> 2, j & 3
            if slot < 2:
                ksb, i = ORDER[j]
            if compute and ksb in ksbs:
                c_from = None
                if slot < 2 and ksb == 1 and i == 0:
                    c_from = S(0) if slot == 0 else DP(0)
                if slot == 0: self.mm(S(ksb), 16, RA(i), self.KFR(ksb, i), tag=f"S ksb{ksb} kk{i}", c=c_from)
                elif slot == 1: self.mm(DP(ksb), 16, RB_(i), self.VFR(ksb, i), tag=f"dP ksb{ksb} kk{i}", c=c_from)
                elif slot == 2: self.mm(self.DV(ksb, i & 1), 16, RC(i), P(ksb, i >> 1), tag=f"dV ksb{ksb} s{i >> 1} db{i & 1}", acc="a")
                else: self.mm(self.DK(ksb, i & 1), 16, RD(i), DSP(ksb, i >> 1), tag=f"dK ksb{ksb} s{i >> 1} db{i & 1}", acc="a")
            else:
                self.out.append(Ins("", "nomfma"))
                if compute and j == 5 and slot < 2:
                    self.salu("s_nop 15")   # diag0: the chain that has just ended gets its time before its first reader
                    self.salu("s_nop 7")
            for _, fn in sorted(G[g], key=lambda t: t[0]):
                fn()
        self.in_loop = False
        self.stores_of = getattr(self, "stores_of", {})
        self.stores_of[kind] = nst

    def ds_next(self):
        """The dS tiles of the next slice (attention.hip, ds_tile_index: [256-query block][256-key block][32-key block][slice of the query
        block], 2 KiB each): one tile on inside a query block; into the next query block, its row's length less seven tiles on - a row grows by
        one square of 64 tiles per query block until it holds all the key blocks. This wave's two tiles (its two 32-key blocks) lie 8 S_SPAN apart."""
        self.salu(f"s_add_u32 {sr(S_SL)}, {sr(S_SL)}, 1")
        self.salu(f"s_and_b32 {sr(S_TMP2)}, {sr(S_SL)}, 7")
        self.salu(f"s_cmp_eq_u32 {sr(S_TMP2)}, 0")
        self.salu(f"s_cselect_b32 {sr(S_TMP)}, {sr(S_DSSTEP)}, {DS_TILE}")
        self.salu(f"s_cselect_b32 {sr(S_TMP2)}, {64 * DS_TILE}, 0")
        self.salu(f"s_add_u32 {sr(S_DS0)}, {sr(S_DS0)}, {sr(S_TMP)}")
        self.salu(f"s_addc_u32 {sr(S_DS0 + 1)}, {sr(S_DS0 + 1)}, 0")
        self.salu(f"s_add_u32 {sr(S_DSSTEP)}, {sr(S_DSSTEP)}, {sr(S_TMP2)}")
        self.salu(f"s_min_u32 {sr(S_DSSTEP)}, {sr(S_DSSTEP)}, %[dsrm]")
        self.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_SPAN)}, 14")
        self.salu(f"s_add_u32 {sr(S_DS1)}, {sr(S_DS0)}, {sr(S_TMP)}")
        self.salu(f"s_addc_u32 {sr(S_DS1 + 1)}, {sr(S_DS0 + 1)}, 0")

    # -------------------------------------------------------------- block pass
    def prologue(self):
        e = self
        self.stamp_init(list(range(84, 92)) + [100, 101])
        # num_records (round 6: ragged sequence lengths): gfx950 range-checks voffset + soffset + the instruction offset against it
        # (tools/scratch/buffer_bounds.hip): a Q / dO row beyond the last query and a K / V row beyond the last key arrive in LDS as ZEROS, a
        # dK / dV row beyond the last key is not stored - no instruction in the loop. Zero rows contribute nothing: P of a zero query row is
        # finite (its row constants are zero: the pre-pass pads them), times dO = 0 and Q = 0; a zero key lies above every real query's diagonal.
        ins = [("qp", Q_SRD, "qn"), ("dop", DO_SRD, "don"), ("cp", C_SRD, None)]
        for nm, srd, n in ins:
            e.salu(f"s_mov_b64 {sr(srd, 2)}, %[{nm}]")
            e.salu(f"s_mov_b32 {sr(srd + 2)}, " + (f"%[{n}]" if n else "0xffffffff"))
            e.salu(f"s_mov_b32 {sr(srd + 3)}, 0x00020000")
        e.salu(f"s_mov_b32 {sr(O_SRD + 2)}, %[kn]")                              # (the K tiles' descriptor here; the epilogue's stores set their own)
        e.salu(f"s_mov_b32 {sr(O_SRD + 3)}, 0x00020000")
        for dst, src in ((S_NS, "ns"), (S_SL, "s0")):
            e.salu(f"s_mov_b32 {sr(dst)}, %[{src}]")
        e.salu(f"s_mov_b32 {sr(S_DSSTEP)}, %[dsrs]")
        e.salu(f"s_mov_b64 {sr(S_DS0, 2)}, %[dsp]")                             # the block's diagonal square of the dS workspace: slice s0 = 8 kb
        # this wave's two 32-key sub-blocks of the block: A = S_D0 (its first diagonal slice too) and A + S_SPAN
        if self.balanced:
            e.salu(f"s_mov_b32 {sr(S_D0)}, {sr(S_WID)}")                       # w and 7 - w
            e.salu(f"s_lshl_b32 {sr(S_SPAN)}, {sr(S_WID)}, 1")
            e.salu(f"s_sub_u32 {sr(S_SPAN)}, 7, {sr(S_SPAN)}")
        else:
            e.salu(f"s_lshl_b32 {sr(S_D0)}, {sr(S_WID)}, 1")                   # 2 w and 2 w + 1
            e.salu(f"s_mov_b32 {sr(S_SPAN)}, 1")
        e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_D0)}, 14")                       # a 32-key block's tiles of a query block: 8 x 2 KiB, one per slice
        e.salu(f"s_add_u32 {sr(S_DS0)}, {sr(S_DS0)}, {sr(S_TMP)}")
        e.salu(f"s_addc_u32 {sr(S_DS0 + 1)}, {sr(S_DS0 + 1)}, 0")
        e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_SPAN)}, 14")
        e.salu(f"s_add_u32 {sr(S_DS1)}, {sr(S_DS0)}, {sr(S_TMP)}")
        e.salu(f"s_addc_u32 {sr(S_DS1 + 1)}, {sr(S_DS0 + 1)}, 0")
        # DMA: slice s0's offsets, steps, saturation values
        e.salu(f"s_lshl_b32 {sr(S_QSTEP)}, %[qsr], 5")
        e.salu(f"s_lshl_b32 {sr(S_DOSTEP)}, %[dosr], 5")
        e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_WID)}, 3")
        e.salu(f"s_mul_i32 {sr(S_X0)}, {sr(S_TMP)}, %[qsr]")                    # rows 8 w .. of a slice
        e.salu(f"s_mul_i32 {sr(S_X1)}, {sr(S_TMP)}, %[dosr]")
        e.salu(f"s_mul_i32 {sr(S_QOFF)}, {sr(S_SL)}, {sr(S_QSTEP)}")
        e.salu(f"s_add_u32 {sr(S_QOFF)}, {sr(S_QOFF)}, {sr(S_X0)}")
        e.salu(f"s_mul_i32 {sr(S_DOOFF)}, {sr(S_SL)}, {sr(S_DOSTEP)}")
        e.salu(f"s_add_u32 {sr(S_DOOFF)}, {sr(S_DOOFF)}, {sr(S_X1)}")
        e.salu(f"s_lshl_b32 {sr(S_COFF)}, {sr(S_SL)}, 7")
        e.salu(f"s_sub_u32 {sr(S_TMP)}, {sr(S_NS)}, 1")                         # last slice (absolute index)
        e.salu(f"s_mul_i32 {sr(S_QMAX)}, {sr(S_TMP)}, {sr(S_QSTEP)}")
        e.salu(f"s_add_u32 {sr(S_QMAX)}, {sr(S_QMAX)}, {sr(S_X0)}")
        e.salu(f"s_mul_i32 {sr(S_DOMAX)}, {sr(S_TMP)}, {sr(S_DOSTEP)}")
        e.salu(f"s_add_u32 {sr(S_DOMAX)}, {sr(S_DOMAX)}, {sr(S_X1)}")
        e.salu(f"s_lshl_b32 {sr(S_CMAX)}, {sr(S_TMP)}, 7")
        # a key block beyond the last query (Skv > Sq) has no slice (%[ns] is the number of slices the QUERIES have): the two slices the
        # prologue requests anyway must not lie behind the tensors' last row (they are fetched, never used) - the same saturation
        # advance_dma applies from the second request on
        for off, mx in ((S_QOFF, S_QMAX), (S_DOOFF, S_DOMAX), (S_COFF, S_CMAX)):
            e.salu(f"s_min_u32 {sr(off)}, {sr(off)}, {sr(mx)}")
        e.salu(f"s_mul_i32 {sr(S_TMP)}, {sr(S_WID)}, {64 * STAGE_ROW}")
        e.salu(f"s_add_u32 {sr(S_STAGE)}, {sr(S_LDS)}, {STAGE0}")
        e.salu(f"s_add_u32 {sr(S_STAGE)}, {sr(S_STAGE)}, {sr(S_TMP)}")
        e.salu(f"s_sub_i32 {sr(S_NS)}, {sr(S_NS)}, {sr(S_SL)}")                 # slices of this block from here on; none for a key block beyond the last query (Skv > Sq)
        e.salu(f"s_max_i32 {sr(S_NS)}, {sr(S_NS)}, 0")
        # ---- lane constants
        lane, r, h, t0, t1, t2 = T[0], T[1], T[2], T[3], T[4], T[5]
        e.valu(f"v_mbcnt_lo_u32_b32 {vr(lane)}, -1, 0")
        e.valu(f"v_mbcnt_hi_u32_b32 {vr(lane)}, -1, {vr(lane)}")
        e.valu(f"v_and_b32 {vr(r)}, 31, {vr(lane)}")
        e.valu(f"v_lshrrev_b32 {vr(h)}, 5, {vr(lane)}")
        # ---- first of all this wave's K and V tiles (64 keys = two 32-row tiles each) by LDS-DMA: K into the wave's quarter of the slice
        #      ring (free until the first slices are requested), V into its quarter of the staging slab (free until the epilogue). The
        #      fragments are then row reads of those tiles. (Round 4, first form: 32 buffer_load_dwordx4 per wave straight into the fragment
        #      registers - a lane's 16 bytes of a 256-byte row each, 64 separate requests per instruction: 8192 requests per workgroup kept
        #      the CU's address unit busy for most of the 12 k cycles tools/attn_dkv_w4_timeline.py showed before the first slice; a DMA piece
        #      is 1 KiB of consecutive lanes.)
        kve, kvo = S(0, 0), S(0, 1)     # source offsets of a piece, even / odd row group (the score registers are idle until the head reads)
        e.valu(f"v_bfe_u32 {vr(t0)}, {vr(lane)}, 2, 3")                        # row7
        e.valu(f"v_mul_lo_u32 {vr(t0)}, {vr(t0)}, %[kvsr]")
        e.valu(f"v_lshl_add_u32 {vr(t0)}, {vr(h)}, 6, {vr(t0)}")               # + 64 sub32
        e.valu(f"v_and_b32 {vr(t1)}, 3, {vr(lane)}")
        e.valu(f"v_bfe_u32 {vr(t2)}, {vr(lane)}, 4, 1")
        e.valu(f"v_xor_b32 {vr(t1)}, {vr(t1)}, {vr(t2)}")                       # slot ^ b4
        e.valu(f"v_lshl_add_u32 {vr(kve)}, {vr(t1)}, 4, {vr(t0)}")
        e.valu(f"v_xor_b32 {vr(t1)}, 2, {vr(t1)}")
        e.valu(f"v_lshl_add_u32 {vr(kvo)}, {vr(t1)}, 4, {vr(t0)}")
        e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_D0)}, 5")
        e.salu(f"s_mul_i32 {sr(S_X0)}, {sr(S_TMP)}, %[kvsr]")                   # this wave's first key row (sub-block A), bytes
        e.salu(f"s_lshl_b32 {sr(S_X1)}, %[kvsr], 3")                            # 8 rows further
        e.salu(f"s_sub_u32 {sr(S_IT)}, {sr(S_SPAN)}, 1")                        # (S_IT is a temporary here) sub-block B lies S_SPAN sub-blocks behind A:
        e.salu(f"s_lshl_b32 {sr(S_IT)}, {sr(S_IT)}, 5")                         # ... 32 (S_SPAN - 1) rows behind A's last row group
        e.salu(f"s_mul_i32 {sr(S_IT)}, {sr(S_IT)}, %[kvsr]")
        e.salu(f"s_mov_b64 {sr(O_SRD, 2)}, %[kp]")
        e.salu(f"s_mov_b64 {sr(V_SRD, 2)}, %[vp]")
        e.salu(f"s_mov_b32 {sr(V_SRD + 2)}, %[kn]")
        e.salu(f"s_mov_b32 {sr(V_SRD + 3)}, 0x00020000")
        e.salu(f"s_lshl_b32 {sr(S_TMP2)}, {sr(S_WID)}, 14")                     # 16 KiB per wave
        e.salu(f"s_add_u32 {sr(S_M0)}, {sr(S_LDS)}, {sr(S_TMP2)}")
        for srd, base in ((O_SRD, 0), (V_SRD, STAGE0)):
            e.salu(f"s_mov_b32 {sr(S_TMP)}, {sr(S_X0)}")
            for g in range(8):                                                     # row groups 0..7 of the wave's 64 keys
                for half in range(2 if self.D == 128 else 1):           # (D = 64: a row group's 8 x 128 B are ONE piece, the first half of the image)
                    e.salu(f"s_add_u32 m0, {sr(S_M0)}, {base + 2048 * g + 1024 * half - 128 * half}")
                    e.dma_load(srd, kvo if g & 1 else kve, S_TMP, 128 * half)
                e.salu(f"s_add_u32 {sr(S_TMP)}, {sr(S_TMP)}, {sr(S_X1)}")
                if g == 3:
                    e.salu(f"s_add_u32 {sr(S_TMP)}, {sr(S_TMP)}, {sr(S_IT)}")   # on to sub-block B's rows
        for i in range(8):
            e.valu(f"v_mov_b32 {vr(S(0, 8) + i)}, 0")                            # (operands of the accumulator-clearing MFMAs below)
        e.valu(f"v_lshlrev_b32 {vr(t0)}, 2, {vr(h)}")
        e.valu(f"v_sub_u32 {vr(RM)}, {vr(r)}, {vr(t0)}")                        # r - 4 h
        # row-read bases of a 32-row tile: 2048 (r >> 3) + 64 (r & 7) + 16 (h ^ ((r >> 2) & 3))
        e.valu(f"v_lshrrev_b32 {vr(t0)}, 3, {vr(r)}")
        e.valu(f"v_lshlrev_b32 {vr(t0)}, 11, {vr(t0)}")
        e.valu(f"v_and_b32 {vr(t1)}, 7, {vr(r)}")
        e.valu(f"v_lshl_add_u32 {vr(t0)}, {vr(t1)}, 6, {vr(t0)}")
        e.valu(f"v_bfe_u32 {vr(t2)}, {vr(r)}, 2, 2")
        e.valu(f"v_xor_b32 {vr(t2)}, {vr(t2)}, {vr(h)}")
        e.valu(f"v_lshl_add_u32 {vr(RB[0])}, {vr(t2)}, 4, {vr(t0)}")
        e.valu(f"v_add_u32 {vr(RB[0])}, {sr(S_LDS)}, {vr(RB[0])}")
        e.valu(f"v_xor_b32 {vr(RB[1])}, 32, {vr(RB[0])}")
        # transposed-read bases: i = lane & 15, q = i >> 2, p = i & 3, g = lane >> 4: 64 (4 h + q) + 16 ((2 (g & 1) + (p >> 1)) ^ h) + 8 (p & 1)
        e.valu(f"v_bfe_u32 {vr(t0)}, {vr(lane)}, 2, 2")
        e.valu(f"v_lshl_add_u32 {vr(t0)}, {vr(h)}, 2, {vr(t0)}")
        e.valu(f"v_lshlrev_b32 {vr(t0)}, 6, {vr(t0)}")
        e.valu(f"v_bfe_u32 {vr(t1)}, {vr(lane)}, 4, 1")
        e.valu(f"v_bfe_u32 {vr(t2)}, {vr(lane)}, 1, 1")
        e.valu(f"v_lshl_add_u32 {vr(t1)}, {vr(t1)}, 1, {vr(t2)}")
        e.valu(f"v_xor_b32 {vr(t1)}, {vr(t1)}, {vr(h)}")
        e.valu(f"v_lshl_add_u32 {vr(t0)}, {vr(t1)}, 4, {vr(t0)}")
        e.valu(f"v_and_b32 {vr(t2)}, 1, {vr(lane)}")
        e.valu(f"v_lshl_add_u32 {vr(TB[0])}, {vr(t2)}, 3, {vr(t0)}")
        e.valu(f"v_add_u32 {vr(TB[0])}, {sr(S_LDS)}, {vr(TB[0])}")
        e.valu(f"v_xor_b32 {vr(TB[1])}, 32, {vr(TB[0])}")
        e.valu(f"v_lshl_add_u32 {vr(LR)}, {vr(h)}, 4, {sr(S_LDS)}")            # row constants: 16 h (+ 32 g + 128 for -delta as immediates), slot 0 of their area
        e.valu(f"v_add_u32 {vr(LR)}, {CBASE}, {vr(LR)}")
        # DMA source offsets: row 8 w + row7 (row7 = (lane >> 2) & 7), chunk 4 sub32 + (slot ^ x), x = ((w & 1) << 1) | ((lane >> 4) & 1)
        e.valu(f"v_bfe_u32 {vr(t0)}, {vr(lane)}, 2, 3")
        e.valu(f"v_and_b32 {vr(t1)}, 3, {vr(lane)}")
        e.valu(f"v_bfe_u32 {vr(t2)}, {vr(lane)}, 4, 1")
        e.salu(f"s_and_b32 {sr(S_TMP)}, {sr(S_WID)}, 1")
        e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_TMP)}, 1")
        e.valu(f"v_or_b32 {vr(t2)}, {sr(S_TMP)}, {vr(t2)}")
        e.valu(f"v_xor_b32 {vr(t1)}, {vr(t1)}, {vr(t2)}")
        e.valu(f"v_lshlrev_b32 {vr(t1)}, 4, {vr(t1)}")
        e.valu(f"v_lshl_add_u32 {vr(t1)}, {vr(h)}, 6, {vr(t1)}")                # + 64 sub32
        e.valu(f"v_mul_lo_u32 {vr(DMAQ)}, {vr(t0)}, %[qsr]")
        e.valu(f"v_add_u32 {vr(DMAQ)}, {vr(DMAQ)}, {vr(t1)}")
        e.valu(f"v_mul_lo_u32 {vr(DMAD)}, {vr(t0)}, %[dosr]")
        e.valu(f"v_add_u32 {vr(DMAD)}, {vr(DMAD)}, {vr(t1)}")
        # the 64 row constants: lanes 0..31 the slice's -lse log2 e, lanes 32..63 its -delta (%[cdelta] bytes further)
        e.valu(f"v_lshlrev_b32 {vr(DMAC)}, 2, {vr(r)}")
        e.valu(f"v_mul_lo_u32 {vr(t0)}, {vr(h)}, %[cdelta]")
        e.valu(f"v_add_u32 {vr(DMAC)}, {vr(DMAC)}, {vr(t0)}")
        # dS store: lane (key r, half h) writes its 16 bytes at 32 r + 16 h of a 1-KiB operand
        e.valu(f"v_lshlrev_b32 {vr(DSOFF)}, 5, {vr(r)}")
        e.valu(f"v_lshl_add_u32 {vr(DSOFF)}, {vr(h)}, 4, {vr(DSOFF)}")
        # dV = dK = 0: sixteen MFMAs of zero operands (0 * 0 + 0 into 16 accumulator registers each) instead of 256 v_accvgpr_write - 16 issue
        # slots, the matrix pipe does the rest while this wave computes on
        for i in range(4 * self.NDB):
            e.out.append(Ins(f"{self.mfma} {ar(16 * i, 16)}, {vr(S(0, 8), 4)}, {vr(S(0, 12), 4)}, 0", "mfma", V(S(0, 8), 4) + V(S(0, 12), 4), A(16 * i, 16), tag="zero"))
        # ---- the fragments: K (k = 16 kk + 8 h .. of key 32 ksb + r) as soon as this wave's 16 K pieces have landed, then V. In-order counter:
        #      the pieces are this wave's own, nobody else reads or writes its quarters: no barrier in front of the reads
        rbk = (S(0, 2), S(0, 3))
        e.salu(f"s_lshl_b32 {sr(S_TMP2)}, {sr(S_WID)}, 14")
        for i in range(2):
            e.valu(f"v_add_u32 {vr(rbk[i])}, {sr(S_TMP2)}, {vr(RB[i])}")
        e.wait(vm=2 * self.NKK)       # the V pieces may still be in flight
        for ksb in range(2):
            for kk in range(self.NKK):
                e.out.append(Ins(f"ds_read_b128 {vr(self.KFR(ksb, kk), 4)}, {vr(rbk[kk & 1])} offset:{8192 * ksb + 512 * (kk >> 1)}", "lds", V(rbk[kk & 1]), V(self.KFR(ksb, kk), 4)))
        e.salu(f"s_add_u32 {sr(S_TMP2)}, {sr(S_TMP2)}, {STAGE0}")
        rbv = (S(0, 4), S(0, 5))
        for i in range(2):
            e.valu(f"v_add_u32 {vr(rbv[i])}, {sr(S_TMP2)}, {vr(RB[i])}")
        e.wait(vm=0)
        for ksb in range(2):
            for kk in range(self.NKK):
                e.out.append(Ins(f"ds_read_b128 {vr(self.VFR(ksb, kk), 4)}, {vr(rbv[kk & 1])} offset:{8192 * ksb + 512 * (kk >> 1)}", "lds", V(rbv[kk & 1]), V(self.VFR(ksb, kk), 4)))
        e.wait(lgkm=0)
        e.barrier()     # every wave has its K fragments out of the ring
        if self.f16:
            e.salu(f"s_mov_b32 {sr(S_PSH)}, 0x{(127 + P_SHIFT) << 23:08x}")          # 2^14 (the V descriptor's registers are free from here on)
        # ---- the first two slices on their way (their flight runs under the scaling of K below)
        e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_WID)}, 11")
        e.salu(f"s_add_u32 {sr(S_M0)}, {sr(S_LDS)}, {sr(S_TMP)}")               # DMA destination of this wave's row group in ring slot 0
        e.salu(f"s_add_u32 {sr(S_M0C)}, {sr(S_LDS)}, {CBASE}")                  # ... and of the row constants (every wave fetches all 64: identical bytes)
        e.salu(f"s_mov_b32 {sr(S_MKT)}, {BUF}")                                 # slot 0 -> 1
        e.salu(f"s_mov_b32 {sr(S_MKC)}, {CSLOT}")
        e.dma_slice()
        e.ring_step()
        e.advance_dma()
        e.dma_slice()
        if not self.early:                                                      # (early: the first slice's own gap 10 takes this step)
            e.ring_step()                                                       # the DMA side now points at slot 2, the masks are slot 0 -> 1 again: the loop's first step
            e.advance_dma()
        if self.D == 64:                                                        # three slices ahead (slice64): slot 2 as well, the DMA side moves on to slot 3
            e.dma_slice()
            e.salu(f"s_xor_b32 {sr(S_M0)}, {sr(S_M0)}, {BUF}")
            e.salu(f"s_xor_b32 {sr(S_M0C)}, {sr(S_M0C)}, {CSLOT}")
            e.advance_dma()
        if self.scaled:
            # K *= scale log2(e): unpack the pair, two multiplies, pack (64 registers, once per block)
            e.valu(f"v_mov_b32 {vr(t2)}, 0x3fb8aa3b")
            e.valu(f"v_mul_f32 {vr(t2)}, {sr(S_SCALE)}, {vr(t2)}")
            for i in range(64):
                x = self.KFR(0, 0) + i
                if self.f16:
                    e.valu(f"v_cvt_f32_f16 {vr(t0)}, {vr(x)}")
                    e.valu(f"v_cvt_f32_f16_sdwa {vr(t1)}, {vr(x)} dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1")
                else:
                    e.valu(f"v_lshlrev_b32 {vr(t0)}, 16, {vr(x)}")
                    e.valu(f"v_and_b32 {vr(t1)}, 0xffff0000, {vr(x)}")
                e.valu(f"v_mul_f32 {vr(t0)}, {vr(t0)}, {vr(t2)}")
                e.valu(f"v_mul_f32 {vr(t1)}, {vr(t1)}, {vr(t2)}")
                e.valu(f"{self.cvt} {vr(x)}, {vr(t0)}, {vr(t1)}")
        # ---- slice s0 has landed for everyone (slice s0 + 1's 5 pieces may still be in flight); the first slice's head state
        e.wait(vm=5 if self.D == 128 else 6)    # (D = 128: slice s0 + 1's 5 pieces may be in flight; D = 64: two slices of 3)
        e.barrier()
        self.stamp(0)
        # (in the ORDER every slice's tail issues them: the loop's counted waits assume it)
        if self.D == 128:
            for g in range(4):
                e.lds_const(S(0), g, 0)
            for j in range(8):
                e.lds_row(RING(j), j, 0)
        else:               # what slice64 reads for its successor, in its order: Q rows, dO rows, [-lse / scale, dO^T], -delta
            for kk in range(4): e.lds_row(80 + 4 * kk, kk, 0)
            for kk in range(4): e.lds_row(96 + 4 * kk, kk, SLICE_DO)
            for i in range(4):
                if i < 2:
                    e.lds_const(S(0), 2 * i, 0); e.lds_const(S(0), 2 * i + 1, 0)
                for sec in (0, 1): e.lds_tr(186 + 4 * i, i >> 1, i & 1, sec, SLICE_DO)
            for g in range(4): e.lds_const(DP(0), g, 128)
        e.salu(f"s_mov_b32 {sr(S_IT)}, 0")

    def dispatch(self):
        e = self
        e.label("L_loop_%=")
        e.salu(f"s_cmp_ge_u32 {sr(S_IT)}, {sr(S_NS)}")
        e.salu("s_cbranch_scc1 L_epilogue_%=")
        e.salu(f"s_sub_u32 {sr(S_TMP)}, {sr(S_IT)}, {sr(S_D0)}")               # slices since this wave's first diagonal one (wraps below it)
        e.salu(f"s_cmp_lt_i32 {sr(S_TMP)}, 0")
        e.salu("s_cbranch_scc1 L_idle_%=")
        e.salu(f"s_cmp_eq_u32 {sr(S_TMP)}, 0")
        e.salu("s_cbranch_scc1 L_diag0_%=")
        e.salu(f"s_cmp_eq_u32 {sr(S_TMP)}, {sr(S_SPAN)}")                      # its second sub-block's diagonal slice
        e.salu("s_cbranch_scc1 L_diag1_%=")
        if self.balanced:
            e.salu(f"s_cmp_lt_u32 {sr(S_TMP)}, {sr(S_SPAN)}")                  # between the two: only sub-block A is at work
            e.salu("s_cbranch_scc1 L_half_%=")
        if self.mutant:
            e.salu(f"s_cmp_eq_u32 {sr(S_IT)}, {sr(S_MUT)}")
            e.salu("s_cbranch_scc1 L_drop_%=")

    def next_iter(self, steady=False):
        self.salu(f"s_add_u32 {sr(S_IT)}, {sr(S_IT)}, 1")
        if steady and not self.mutant and not os.environ.get("KF_GEN_NO_STEADY_LOOP"):
            # round 6: a wave runs idle* diag0 diag1 steady*: behind a steady slice comes a steady slice or the epilogue - three scalar instructions
            # instead of the eleven of the general dispatch (an instruction of a lone wave's stream costs its issue slot whatever it does)
            self.salu(f"s_cmp_lt_u32 {sr(S_IT)}, {sr(S_NS)}")
            self.salu("s_cbranch_scc1 L_steady_%=")
            self.salu("s_branch L_epilogue_%=")
            return
        self.salu("s_branch L_loop_%=")

    def epilogue(self):
        e = self
        lane, r, h = T[0], T[1], T[2]
        e.label("L_epilogue_%=")
        # nothing this wave has in flight writes LDS any more (no DMA beyond the pass's last slice), and its dS stores read their registers
        # at issue: only the LDS reads of the last slice's tail have to be back before their registers are reused
        # (round 6: without skip_tail_dma the requests of the slices fetched past the pass's end and the last slice's dS stores - which retire ~1 us
        #  after issue - are still in flight here: nothing the epilogue touches depends on them (registers, the wave's slab). What must hold is that
        #  they have LANDED before the barrier at the epilogue's end lets the next pass's K tiles into the ring: a counted wait in front of that
        #  barrier - everything but the epilogue's own stores - instead of vmcnt(0) here. KF_GEN_EPI_VMWAIT=1 restores the old form: same-box A/B.)
        self.epi_late_wait = not self.skip_tail_dma and not os.environ.get("KF_GEN_EPI_VMWAIT") and not self.stamps
        e.wait(vm=None if (self.skip_tail_dma or self.epi_late_wait) else 0, lgkm=0)
        if self.skip_tail_dma:
            # (a pass WITHOUT slices - a key block beyond the last query - comes here straight from the prologue, whose second request is
            #  still in flight: it must have landed before the barrier below lets the next pass's K tiles into the ring)
            e.salu(f"s_cmp_lg_u32 {sr(S_NS)}, 0")
            e.salu("s_cbranch_scc1 L_epi_go_%=")
            e.wait(vm=0)
            e.label("L_epi_go_%=")
        self.stamp(5)
        e.salu("s_nop 15")
        e.valu(f"v_mbcnt_lo_u32_b32 {vr(lane)}, -1, 0")
        e.valu(f"v_mbcnt_hi_u32_b32 {vr(lane)}, -1, {vr(lane)}")
        e.valu(f"v_and_b32 {vr(r)}, 31, {vr(lane)}")
        e.valu(f"v_lshrrev_b32 {vr(h)}, 5, {vr(lane)}")
        st, rd, oo = T[3], T[4], T[5]
        e.valu(f"v_mul_u32_u24 {vr(st)}, {STAGE_ROW}, {vr(r)}")
        e.valu(f"v_lshl_add_u32 {vr(st)}, {vr(h)}, 3, {vr(st)}")
        e.valu(f"v_add_u32 {vr(st)}, {sr(S_STAGE)}, {vr(st)}")
        e.valu(f"v_lshrrev_b32 {vr(rd)}, {4 if self.D == 128 else 3}, {vr(lane)}")     # row of a store instruction: 16 lanes per 256-byte row | 8 lanes per 128-byte row
        e.valu(f"v_and_b32 {vr(oo)}, {15 if self.D == 128 else 7}, {vr(lane)}")
        e.valu(f"v_lshlrev_b32 {vr(oo)}, 4, {vr(oo)}")
        e.valu(f"v_mul_lo_u32 {vr(RM)}, {vr(rd)}, {sr(S_OSR)}")
        e.valu(f"v_mul_u32_u24 {vr(rd)}, {STAGE_ROW}, {vr(rd)}")
        e.valu(f"v_add3_u32 {vr(rd)}, {vr(rd)}, {vr(oo)}, {sr(S_STAGE)}")
        e.valu(f"v_add_u32 {vr(oo)}, {vr(oo)}, {vr(RM)}")
        for which, accf, ptr in ((0, self.DV, "dvp"), (1, self.DK, "dkp")):
            # accumulators -> 16-bit rows of this wave's slab: lane (key r, half h) writes 4 consecutive d of key 32 ksb + r
            for ksb in range(2):
                for db in range(self.NDB):
                    for gq in range(4):
                        a0 = accf(ksb, db) + 4 * gq
                        x = [RING(0) + i for i in range(4)]
                        for jj in range(4):
                            e.valu(f"v_accvgpr_read_b32 {vr(x[jj])}, {ar(a0 + jj)}")
                        if which == 1:
                            for jj in range(4):
                                e.valu(f"v_mul_f32 {vr(x[jj])}, %[scl], {vr(x[jj])}")   # dK = scale dS^T Q (%[scale] is scale log2 e in the exact form)
                        elif self.f16:
                            for jj in range(4):
                                e.valu(f"v_ldexp_f32 {vr(x[jj])}, {vr(x[jj])}, {-P_SHIFT}")  # dV was accumulated from P 2^14
                        e.valu(f"{self.cvt} {vr(x[0])}, {vr(x[0])}, {vr(x[1])}")
                        e.valu(f"{self.cvt} {vr(x[1])}, {vr(x[2])}, {vr(x[3])}")
                        e.out.append(Ins(f"ds_write_b64 {vr(st)}, {vr(x[0], 2)} offset:{32 * ksb * STAGE_ROW + 64 * db + 16 * gq}", "ldsw"))
            e.wait(lgkm=0)
            e.salu(f"s_mov_b64 {sr(O_SRD, 2)}, %[{ptr}]")
            e.salu(f"s_mov_b32 {sr(O_SRD + 2)}, %[on]")                        # rows beyond the last key are not stored
            e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_D0)}, 5")
            e.salu(f"s_mul_i32 {sr(S_X0)}, {sr(S_TMP)}, {sr(S_OSR)}")              # sub-block A's first row
            rows_per = 4 if self.D == 128 else 8                                    # rows one store instruction covers
            e.salu(f"s_lshl_b32 {sr(S_X1)}, {sr(S_OSR)}, {2 if self.D == 128 else 3}")
            e.salu(f"s_sub_u32 {sr(S_TMP2)}, {sr(S_SPAN)}, 1")                      # sub-block B's rows: 32 (S_SPAN - 1) behind A's last
            e.salu(f"s_lshl_b32 {sr(S_TMP2)}, {sr(S_TMP2)}, 5")
            e.salu(f"s_mul_i32 {sr(S_TMP2)}, {sr(S_TMP2)}, {sr(S_OSR)}")
            for j in range(64 // rows_per):
                d = 32 + 4 * (j % 8)    # v[32..63]: the dP registers are free now
                e.out.append(Ins(f"ds_read_b128 {vr(d, 4)}, {vr(rd)} offset:{rows_per * j * STAGE_ROW}", "ldsw"))
                if j % 8 == 7:
                    e.wait(lgkm=0)
                    for i in range(8):
                        e.out.append(Ins(f"buffer_store_dwordx4 {vr(32 + 4 * i, 4)}, {vr(oo)}, {sr(O_SRD, 4)}, {sr(S_X0)} offen", "vmem"))
                        e.salu(f"s_add_u32 {sr(S_X0)}, {sr(S_X0)}, {sr(S_X1)}")
                    if rows_per * (j + 1) == 32:
                        e.salu(f"s_add_u32 {sr(S_X0)}, {sr(S_X0)}, {sr(S_TMP2)}")
            # (no wait for the stores: their registers and the descriptor were read at issue, the slab is rewritten behind the lgkmcnt(0)
            #  above; they drain under the second tensor's conversion and the next pass's prologue, whose counted waits they only make stricter)
        if self.stamps:
            e.valu(f"v_mov_b32 {vr(32 + 7)}, s90")                            # [7] = the number of steady slices
            e.salu("s_mov_b32 s90, 0")
            self.stamp(6)
            e.salu(f"s_lshl_b32 {sr(S_TMP)}, {sr(S_WID)}, 6")                  # 16 dwords per wave (%[dbg] already points at this pass)
            e.valu(f"v_mov_b32 {vr(T[0])}, {sr(S_TMP)}")
            for i in range(7):
                e.valu(f"v_mov_b32 {vr(32 + i)}, s{84 + i}")
            for i, r in enumerate((91, 100, 101)):
                e.valu(f"v_mov_b32 {vr(40 + i)}, s{r}")                        # [8..10] = steady slices: slot S, slot dP, slot dV
            e.valu(f"v_mov_b32 {vr(43)}, 0")
            e.salu("s_mov_b64 exec, 1")
            e.out.append(Ins(f"global_store_dwordx4 {vr(T[0])}, {vr(32, 4)}, %[dbg]", "vmem"))
            e.out.append(Ins(f"global_store_dwordx4 {vr(T[0])}, {vr(36, 4)}, %[dbg] offset:16", "vmem"))
            e.out.append(Ins(f"global_store_dwordx4 {vr(T[0])}, {vr(40, 4)}, %[dbg] offset:32", "vmem"))
            e.salu("s_mov_b64 exec, -1")
            e.wait(vm=0)
        if self.epi_late_wait:
            n_st = 2 * (64 // (4 if self.D == 128 else 8))     # this epilogue's own dV + dK row stores: the only memory operations that may still be in flight
            e.wait(vm=n_st)
        e.barrier()   # the next block's DMA reuses the slice buffers: every wave is past its last reads (they are, since the last slice's barrier) and every wave's requests of this pass have landed

    def build(self):
        self.prologue()
        self.dispatch()
        sl = self.slice if self.D == 128 else self.slice64
        # D = 128 - prev_stores: the stores a wave issued behind its last DMA pieces in the PREVIOUS slice, by what that slice was.
        # D = 64 - what may be in flight at the barrier of slice it: the 3 pieces of slice it + 2 (requested one slice ago) and the dS stores of
        # slices it - 2 and it - 1, which were issued behind the pieces of slice it + 1 that the wait is for; a wave runs idle* diag0 diag1
        # steady*, so the two slices before a steady one stored 2 + 4 (its first) or 4 + 4: the smaller count is the safe one
        st = (lambda a, b: 3 + ((a + b) if self.ds else 0))
        vm = {"steady": 4, "diag1": 2, "diag0": 0, "idle": 0, "drop": 4, "half": 2} if self.D == 128 else \
             {"steady": st(2, 4), "diag1": st(0, 2), "diag0": st(0, 0), "idle": st(0, 0), "drop": st(2, 4)}
        if self.D == 128 and not self.ds:
            vm = {k: 0 for k in vm}
        sl("steady", "steady", vm["steady"])
        self.next_iter(steady=True)
        sl("diag1", "diag1", vm["diag1"])
        self.next_iter()
        sl("diag0", "diag0", vm["diag0"])
        self.next_iter()
        sl("idle", "idle", vm["idle"])
        self.next_iter()
        if self.balanced:
            sl("half", "half", vm["half"])
            self.next_iter()
        if self.mutant:
            sl("drop", "drop", vm["drop"])
            self.next_iter()
        self.epilogue()
        asm_stream.finish_waits(self.out, VARIANTS, WAIT_BATCH_AGE)
        return self


# ------------------------------------------------------------------ counted LDS waits
VARIANTS = r"L_(steady|diag1|diag0|idle|half|drop)_%=:"


# 0: one counted wait per first use (rounds 4-5: 35 s_waitcnt per steady slice); N > 0: a wait also covers every later read that is N MFMA gaps old
# (5: 11 per slice; same-box 1.952 vs 1.975 ms over five interleaved pairs, profiles/r06_ab_ds_layout.txt)
WAIT_BATCH_AGE = int(os.environ.get("KF_GEN_DKV_WAIT_AGE", "5"))


check = functools.partial(asm_stream.check, variants=VARIANTS)   # (the rules: asm_stream.check)


def selftest():
    """The 32-row tile image: what this wave's DMA pieces write, what the row reads deliver as the A operand of S / dP (lane (r, h):
    A[row r][k = 16 kk + 8 h + j]) and what the transposed reads deliver as the A operand of dV / dK in the k order of a score
    accumulator used as the B operand (element j of half h <-> query 16 s + 8 (j >> 2) + 4 h + (j & 3))."""
    pieces = [(2048 * w + 1024 * hp, w, hp) for w in range(4) for hp in range(2)]   # wave w: row group w of the slice's tile
    lds = asm_stream.tile_image(pieces, 256 + 96)   # (a row stride that is not the tile's own)
    asm_stream.row_reads_agree(lds, 1)
    asm_stream.transposed_reads_agree(lds, 2)
    return True


CLOBBERS = (["memory", "vcc", "scc", "m0"] + [f"s{i}" for i in range(36, N_SGPR_HI)] + [f"v{i}" for i in range(N_VGPR)] + [f"a{i}" for i in range(256)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    ap.add_argument("--out", default=str(OUT))
    ap.add_argument("--ablate", default="")
    ap.add_argument("--dump", default="", help="print one variant's stream")
    ap.add_argument("--store-policy", default=Gen.store_policy, help="cache bits of the dS stores (experiment)")
    ap.add_argument("--scaled", action="store_true", help="--dump / --check-only look at the scaled-K stream (the file always holds both forms)")
    ap.add_argument("--skip-tail-dma", action="store_true", help="A/B: no DMA request beyond a pass's last slice (measured: no gain)")
    ap.add_argument("--stamps", action="store_true", help="diagnostic build: s_memtime sums per slice kind, prologue, epilogue (needs -DKF_DKV_W4_STAMPS)")
    args = ap.parse_args()
    abl = tuple(x for x in args.ablate.split(",") if x)
    Gen.store_policy = args.store_policy
    Gen.skip_tail_dma = args.skip_tail_dma
    assert selftest()
    g = Gen(False, ablate=abl, stamps=args.stamps, scaled=args.scaled).build()
    probs = check(g.out) + ([] if args.scaled else check(Gen(False, ablate=abl, stamps=args.stamps, scaled=True).build().out))
    for p in probs[:40]:
        print("HAZARD:", p, file=sys.stderr)
    if args.dump:
        on = False
        for i in g.out:
            if i.kind == "label" and re.match(VARIANTS, i.text):
                on = i.text == f"L_{args.dump}_%=:"
            if on:
                print(f"{i.kind:7s} {i.text}  {i.tag}")
    if probs and not abl:
        return 1
    if args.check_only:
        return 0
    def stream(name, *a, **kw):
        gg = Gen(*a, ablate=abl, **kw).build()
        assert abl or not check(gg.out), check(gg.out)[:5]
        return name, gg.out
    def streams(mut):
        kinds = [(f16, ds, f"{'F16' if f16 else 'BF16'}_{'DS' if ds else 'NODS'}") for f16 in (False, True) for ds in (True, False)]
        return [stream(f"KF_DKV_W4_ASM_{nm}{'_SQ' if sq else ''}", f16, mut, ds, stamps=args.stamps, scaled=sq) for f16, ds, nm in kinds for sq in (False, True)] + \
               [stream(f"KF_DKV_W4_D64_ASM_{nm}", f16, mut, ds, D=64) for f16, ds, nm in kinds]
    n_ins = sum(1 for i in g.out if i.kind not in ("raw", "label", "nomfma"))
    asm_stream.write_inc(args.out, f"""// GENERATED by tools/gen_attn_dkv.py - do not edit; edit the generator and run it again.
// The 16-bit causal-attention dK / dV pass of one 256-key block as ONE instruction stream ({n_ins} instructions): 4 waves x 64 keys,
// one wave per SIMD, all 512 registers asm-owned; see the generator's header for the structure.
// Two forms: exact f32 scores (default: %[scale] = scale log2 e, row constant -lse / scale), and _SQ = K scaled and rounded once per block
// (KF_ATTN_SCALED_OPERANDS: %[scale] = the softmax scale, row constant -lse log2 e). _D64_ = head size 64 (exact form only): 32 MFMAs per slice.""",
                        ("KF_DKV_W4_LDS_BYTES", LDS_BYTES), ("KF_DKV_W4_CLOBBERS", CLOBBERS + ([f"s{i}" for i in range(80, 102)] if args.stamps else [])), streams)
    print(f"wrote {args.out} ({n_ins} instructions)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
