"""What the generators of hand-placed gfx950 instruction streams share (gen_attn_fwd.py, gen_attn_dkv.py): registers and instructions,
the base emitter, the passes over a finished stream (`fix_trans_use`, `finish_waits`), the hazard checker (`check`), the model of the
swizzled 32-row LDS tile image and the writer of the .inc file. Nothing here describes one schedule: register maps, placement tables and
the bodies of the streams stay with their generators."""
import re
from pathlib import Path


def vr(i, n=1): return f"v{i}" if n == 1 else f"v[{i}:{i + n - 1}]"
def ar(i, n=1): return f"a{i}" if n == 1 else f"a[{i}:{i + n - 1}]"


def sr(i, n=1):
    """s-register text; a read-only input operand ("%[name]") passes through."""
    if isinstance(i, str):
        return i
    return f"s{i}" if n == 1 else f"s[{i}:{i + n - 1}]"


class Ins:
    """One instruction with what the checker needs to know about it."""
    def __init__(self, text, kind, reads=(), writes=(), tag=""):
        self.text, self.kind, self.reads, self.writes, self.tag = text, kind, tuple(reads), tuple(writes), tag


def V(i, n=1): return [("v", j) for j in range(i, i + n)]
def A(i, n=1): return [("a", j) for j in range(i, i + n)]


def is_nop(x): return x.kind == "salu" and x.text.startswith("s_nop")
def m0_write(src, add=0): return f"s_add_u32 m0, {sr(src)}, {add}" if add else f"s_mov_b32 m0, {sr(src)}"


class Emitter:
    """The emit layer of a stream: `out` is the list of Ins (labels and comments as kinds "label" / "raw", a gap without an MFMA as "nomfma")."""
    def __init__(self, f16=False, mutant=False, ablate=(), stamps=False, scaled=False, D=128):
        assert D in (64, 128) and not (scaled and D == 64)
        self.D, self.NKK, self.NDB = D, D // 16, D // 32        # head size, its k-steps of 16 and its column blocks of 32
        self.f16, self.mutant, self.scaled = f16, mutant, scaled
        self.stamps = stamps        # diagnostic build (the timeline tools): s_memtime sums per wave
        self.ablate = set(ablate)   # timing experiments only: parts of the loop body left out - WRONG results
        self.in_loop = False        # the ablations apply inside the loop body only
        self.mfma = "v_mfma_f32_32x32x16_f16" if f16 else "v_mfma_f32_32x32x16_bf16"
        self.cvt = "v_cvt_pk_f16_f32" if f16 else "v_cvt_pk_bf16_f32"
        self.out = []

    def raw(self, text): self.out.append(Ins(text, "raw"))
    def label(self, name): self.out.append(Ins(f"{name}:", "label"))
    def salu(self, text): self.out.append(Ins(text, "salu"))
    def valu(self, text, reads=(), writes=(), trans=False): self.out.append(Ins(text, "trans" if trans else "valu", reads, writes))

    def wait(self, vm=None, lgkm=None):
        parts = ([f"vmcnt({vm})"] if vm is not None else []) + ([f"lgkmcnt({lgkm})"] if lgkm is not None else [])
        self.out.append(Ins("s_waitcnt " + " ".join(parts), "wait", tag=f"{'vm' if vm is not None else ''}{'lgkm' if lgkm is not None else ''}"))

    def barrier(self):
        if "barrier" in self.ablate and self.in_loop: return
        self.out.append(Ins("s_barrier", "barrier"))

    # ---- one LDS-DMA request: M0 = the LDS destination, then buffer_load ... lds (1 KiB, or 256 B as dword)
    def dma_m0(self, m0_from, m0_add=0):
        if "dma" in self.ablate and self.in_loop: return
        self.salu(m0_write(m0_from, m0_add))

    def dma_load(self, srd, voff, soff, inst_off=0, dword=False, sep=None):
        """The request alone. A scalar write of M0 needs one wait state before the request that reads it: an s_nop 0 only if the write is
        the previous instruction. `sep` (an emitter of ONE instruction that had to be issued anyway) stands there instead."""
        if sep: sep()
        if "dma" in self.ablate and self.in_loop: return
        if self.out[-1].text.startswith(("s_add_u32 m0", "s_mov_b32 m0")):
            self.salu("s_nop 0")
        o = f" offset:{inst_off}" if inst_off else ""
        self.out.append(Ins(f"buffer_load_{'dword' if dword else 'dwordx4'} {vr(voff)}, {sr(srd, 4)}, {sr(soff)} offen{o} lds", "dma", V(voff)))

    def dma(self, srd, voff, soff, m0_from, m0_add=0, inst_off=0, dword=False, sep=None):
        self.dma_m0(m0_from, m0_add)
        self.dma_load(srd, voff, soff, inst_off, dword, sep)

    # ---- clock stamps (diagnostic build): the cycles since the previous stamp go to the sum s[84 + bucket]
    def stamp_init(self, sums):
        if not self.stamps: return
        for i in sums:
            self.salu(f"s_mov_b32 s{i}, 0")
        self.stamp_take()
        self.wait(lgkm=0)
        self.salu("s_mov_b32 s82, s80")

    def stamp_take(self):
        """Requests the clock; stamp_add() uses it behind a wait - its own in stamp(), or one the stream has anyway."""
        if self.stamps: self.salu("s_memtime s[80:81]")

    def stamp_add(self, bucket):
        if not self.stamps: return
        self.salu("s_sub_u32 s83, s80, s82")
        self.salu(f"s_add_u32 s{84 + bucket}, s{84 + bucket}, s83")
        self.salu("s_mov_b32 s82, s80")

    def stamp(self, bucket):
        """A whole stamp. Its SMEM round trip (~100 cycles) lands in the bucket that FOLLOWS it."""
        if not self.stamps: return
        self.stamp_take()
        self.wait(lgkm=0)
        self.stamp_add(bucket)


# ------------------------------------------------------------------ passes over a finished stream
def fix_trans_use(ins):
    """gfx950 does not interlock a transcendental result against the VERY NEXT instruction reading it: the lanes with
    (lane & 4) == 0 get the old register value (tools/scratch/trans_hazard.hip, profiles/r04_trans_hazard.txt). One wait state
    is what the hardware needs (LLVM's hasTransForwardingHazard; hipcc inserts it for compiled code, never inside inline asm).
    Behind an MFMA the stream never has the two as neighbours; where gaps hold no MFMA (drain, a first tile's empty slot,
    prologue, epilogue, the rare rescale) they can be: `s_nop 1` (one more than needed) goes between them, and an `s_nop 0`
    that is all that separates them is widened."""
    out, prev, sep = [], None, 0
    for x in ins:
        if x.kind in ("raw", "label", "nomfma"):
            out.append(x)
            if x.kind == "label": prev = None
            continue
        if prev is not None and is_nop(x) and sep == 0:
            if int(x.text.split()[1]) < 1:
                x = Ins("s_nop 1", "salu")
            out.append(x)
            sep = 2
            continue
        if prev is not None and sep == 0 and x.kind in ("valu", "trans") and set(prev.writes) & set(x.reads):
            out.append(Ins("s_nop 1", "salu"))
        out.append(x)
        prev, sep = (x, 0) if x.kind == "trans" else (None, 0)
    ins[:] = out


def finish_waits(ins, variants, batch_age):
    """Inserts `s_waitcnt lgkmcnt(N)` in front of every instruction that reads (or rewrites) the destination of an LDS read still in
    flight, N = the LDS reads issued after it. `variants` is the pattern of the loop bodies' labels. Each body is walked with the reads
    its predecessor's tail left pending (every body ends with the same reads for the next one; the steady body's are taken), the prologue
    and the epilogue linearly.
    batch_age: an s_waitcnt is an instruction of the wave's stream like any other (4 issue cycles in a gap that is already full); with
    batch_age > 0 a wait that has to be there anyway is widened over the younger reads that are at least that many MFMA gaps old - they
    have landed - so their own first uses need none. A wider wait is only ever stricter: correctness does not depend on it."""
    # the tail every variant leaves behind (with how many MFMA gaps lie between each read and the variant's end)
    tail, gaps_after = [], []
    on = False
    for x in ins:
        if x.kind == "label" and re.match(variants, x.text):
            on = x.text.startswith("L_steady")
            if on: tail, gaps_after = [], []
        elif on and x.kind == "lds":
            tail.append(x)
            gaps_after.append(0)
        elif on and x.kind == "wait" and "lgkm" in x.tag:
            tail, gaps_after = [], []
        elif on and x.kind in ("mfma", "nomfma"):
            gaps_after = [g + 1 for g in gaps_after]
        elif on and x.kind == "label" and x.text.startswith("L_loop"):
            on = False
    # (never more than 15 in flight: the walk below retires the oldest before a 16th is issued, in every variant and in the prologue - so only
    #  the LAST 15 reads of the tail can still be pending where a variant starts; the counter's field is 4 bits wide)
    out, pending, born = [], [], []     # pending: destination registers of the reads in flight; born: the gap counter when each was issued
    gap = 0
    for x in ins:
        if x.kind == "label" and (re.match(variants, x.text) or x.text.startswith("L_epilogue")):
            pending = [t.writes for t in tail][-15:]
            gap = 0
            born = [-g for g in gaps_after][-15:]
        if x.kind in ("mfma", "nomfma"):
            gap += 1
        if x.kind == "wait" and "lgkm" in x.tag:
            pending, born = [], []
        touched = set(x.reads) | set(x.writes)
        need = -1
        for i, w in enumerate(pending):
            if touched & set(w):
                need = i
        if need >= 0:
            if batch_age > 0:
                while need + 1 < len(pending) and gap - born[need + 1] >= batch_age:
                    need += 1
            n = len(pending) - 1 - need
            out.append(Ins(f"s_waitcnt lgkmcnt({n})", "wait", tag="auto"))
            pending, born = pending[need + 1:], born[need + 1:]
        if x.kind == "lds":
            if len(pending) >= 15:   # the counter saturates at 15: retire the oldest first (it is 15 reads old)
                out.append(Ins("s_waitcnt lgkmcnt(14)", "wait", tag="auto"))
                pending, born = pending[len(pending) - 14:], born[len(born) - 14:]
            pending.append(x.writes)
            born.append(gap)
        out.append(x)
    ins[:] = out


# ------------------------------------------------------------------ static checks on the emitted stream
class _Walk:
    """The checker's state behind the instructions walked so far."""
    def __init__(self):
        self.mfma_w, self.valu_w, self.lds_w = {}, {}, {}   # register -> its last writer: (MFMA count, tag, position) | position | number of the LDS read
        self.n_mfma = self.n_ins = self.lds_issued = self.lds_done = 0
        self.trans, self.tws = None, 0                      # the transcendental just issued, the wait states behind it

    def fork(self):
        w = _Walk()
        w.__dict__.update({k: dict(v) if isinstance(v, dict) else v for k, v in self.__dict__.items()})
        return w

    def step(self, x, say):
        if is_nop(x):
            if self.trans is not None: self.tws += int(x.text.split()[1]) + 1
        else:
            if self.trans is not None and x.kind in ("valu", "trans") and set(self.trans.writes) & set(x.reads) and self.tws < 2:
                say(f"'{x.text}' reads the result of the transcendental '{self.trans.text}' {self.tws} wait state(s) behind it (needs 2)")
            self.trans, self.tws = (x, 0) if x.kind == "trans" else (None, 0)
        self.n_ins += 1 + (int(x.text.split()[1]) if is_nop(x) else 0)
        self.n_mfma += x.kind == "mfma"
        for n in re.findall(r"lgkmcnt\((\d+)\)", x.text):   # retires all but the youngest n reads
            if int(n) and self.lds_issued - self.lds_done > 15:
                say(f"'{x.text}' counts on lgkmcnt with {self.lds_issued - self.lds_done} LDS reads in flight (the counter holds 15)")
            self.lds_done = max(self.lds_done, self.lds_issued - int(n))
        for reg in dict.fromkeys(x.reads + x.writes):
            if self.lds_w.get(reg, 0) > self.lds_done:
                say(f"'{x.text}' uses {reg} of an LDS read not yet waited for")
        for reg in x.reads:
            if reg in self.mfma_w:
                m, tag, at = self.mfma_w[reg]
                chain = x.kind == "mfma" and reg in x.writes
                if not chain and self.n_mfma - m < 2 and self.n_ins - at < 22:
                    say(f"'{x.text}' reads {reg} {self.n_mfma - m} MFMA(s) / {self.n_ins - at} wait states after '{tag}' wrote it")
            if x.kind == "mfma" and reg in self.valu_w and self.n_ins - self.valu_w[reg] < 4:
                say(f"'{x.text}' reads {reg} {self.n_ins - self.valu_w[reg]} instruction(s) after a VALU wrote it")
        if x.kind == "lds":
            self.lds_issued += 1
        for reg in x.writes:
            if x.kind != "mfma" and reg in self.mfma_w and self.n_mfma - self.mfma_w[reg][0] < 2 and self.n_ins - self.mfma_w[reg][2] < 22:
                say(f"'{x.text}' overwrites {reg} right behind '{self.mfma_w[reg][1]}'")
            self.mfma_w.pop(reg, None)
            self.valu_w.pop(reg, None)
            if x.kind == "mfma":
                self.mfma_w[reg] = (self.n_mfma, x.tag, self.n_ins)
            elif x.kind == "lds":
                self.lds_w[reg] = self.lds_issued
            else:
                self.valu_w[reg] = self.n_ins


def check(ins, variants):
    """The distances and waits the hardware does not interlock. `variants` is the pattern of the loop bodies' labels; the dispatch can
    follow any body with any other, so every ORDERED PAIR of bodies is walked, a first and then a second:
      1. an MFMA result is read or overwritten by anything but its own accumulate chain only >= 2 MFMAs or >= 22 wait states later;
      2. a VALU result feeds an MFMA operand only with >= 4 instructions in between;
      3. a transcendental's result is read by the next VALU only behind >= 2 wait states or a real instruction;
      4. the destination of an LDS read is read or rewritten only after a wait has retired the read: lgkmcnt(N) retires all but the
         youngest N, and N > 0 counts only while at most 15 reads are in flight (the counter's field is 4 bits wide);
      5. no lgkmcnt field above 15 and no vmcnt field above 63 anywhere in the stream.
    A body's own problems are reported as "name: ...", what only shows behind another body as "first -> name: ..."."""
    problems = []
    for x in ins:
        for field, width in (("lgkmcnt", 15), ("vmcnt", 63)):
            problems += [f"'{x.text}': the {field} field holds at most {width}" for n in re.findall(field + r"\((\d+)\)", x.text) if int(n) > width]
    cur, bodies = None, {}
    for x in ins:
        if x.kind == "label" and re.match(variants, x.text):
            cur = bodies[x.text[2:-4]] = []
        elif x.kind == "label" and x.text.startswith("L_epilogue"):
            cur = None
        elif cur is not None and x.kind not in ("raw", "label", "nomfma"):
            cur.append(x)
    behind, own = {}, {}
    for name, body in bodies.items():
        behind[name] = _Walk()
        for x in body:
            behind[name].step(x, lambda msg: None)
    for first, second in [(n, n) for n in bodies] + [(a, b) for a in bodies for b in bodies if a != b]:
        found, walk = [], behind[first].fork()
        for x in bodies[second]:
            walk.step(x, found.append)
        if first == second:
            own[second] = set(found)
            problems += [f"{second}: {msg}" for msg in found]
        else:
            problems += [f"{first} -> {second}: {msg}" for msg in found if msg not in own[second]]
    return problems


# ------------------------------------------------------------------ pure-Python model of the swizzled LDS image of 32-row tiles
def tile_image(pieces, stride):
    """What the DMA pieces write: {LDS byte address: (source row, column)} per 16-bit element. A piece (LDS base, row group, half) is 1 KiB:
    lane L fetches 16 bytes of row 8 group + ((L >> 2) & 7) - the soffset / voffset / instruction-offset sum the streams form - to base + 16 L."""
    lds = {}
    for base, rg, hp in pieces:
        for L in range(64):
            row7, sub32, slot, b4 = (L >> 2) & 7, L >> 5, L & 3, (L >> 4) & 1
            src = (8 * rg + row7) * stride + 64 * sub32 + 16 * (slot ^ (2 * (rg & 1) | b4)) + 128 * hp
            for byte in range(0, 16, 2):
                lds[base + 16 * L + byte] = (src // stride, (src % stride + byte) // 2)
    assert len(lds) == 512 * len(pieces)
    return lds


def row_reads_agree(lds, tiles):
    """ds_read_b128 of k-step kk delivers the A operand of v_mfma_32x32x16: lane (r, h) gets A[row r][k = 16 kk + 8 h + j] of its tile."""
    for sub in range(tiles):
        for kk in range(8):
            for lane in range(64):
                r, h = lane & 31, lane >> 5
                b0 = 2048 * (r >> 3) + 64 * (r & 7) + 16 * (h ^ ((r >> 2) & 3))
                addr = (b0 ^ (32 if kk & 1 else 0)) + 8192 * sub + 512 * (kk >> 1)
                for j in range(8):
                    assert lds[addr + 2 * j] == (32 * sub + r, 16 * kk + 8 * h + j), ("row", sub, kk, lane, j, lds[addr + 2 * j])


def transposed_reads_agree(lds, ksteps):
    """The two ds_read_b64_tr_b16 of fragment (ks, db) deliver the transposed operand in the k order of a score accumulator used as the
    B operand: element j of half h <-> row 16 ks + 8 (j >> 2) + 4 h + (j & 3), column 32 db + r."""
    for ks in range(ksteps):
        for db in range(4):
            for sec in range(2):
                imm = 2048 * (2 * ks + sec) + 512 * db
                got = {}
                for grp in range(4):
                    blk = {}
                    for i in range(16):
                        lane = 16 * grp + i
                        h, q, p, g1 = lane >> 5, i >> 2, i & 3, grp & 1
                        t0 = 64 * (4 * h + q) + 16 * ((2 * g1 + (p >> 1)) ^ h) + 8 * (p & 1)
                        addr = (t0 ^ (32 if sec else 0)) + imm
                        for c in range(4):
                            blk[(q, 4 * p + c)] = lds[addr + 2 * c]
                    for i in range(16):
                        got[16 * grp + i] = [blk[(qq, i)] for qq in range(4)]
                for lane in range(64):
                    r, h = lane & 31, lane >> 5
                    for e in range(4):
                        j = 4 * sec + e
                        row = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)
                        assert got[lane][e] == (row, 32 * db + r), ("tr", ks, db, sec, lane, e, got[lane][e], (row, 32 * db + r))


# ------------------------------------------------------------------ writing the file
def render(ins):
    lines = []
    for i in ins:
        if i.kind == "nomfma":
            continue
        if i.kind == "raw" and i.text.startswith("#"):
            lines.append(i.text)
        elif i.kind in ("raw", "label"):
            lines.append(f'    "{i.text}\\n"')
        else:
            lines.append(f'    "\\t{i.text}\\n"')
    return "\n".join(lines)


def write_inc(path, header, lds_bytes, clobbers, streams, mutant_note=""):
    """The C++ header both generators write: `header` (comment lines), the LDS-bytes and clobber-list macros as (name, value), then one
    string-literal macro per (name, Ins list) of streams(mutant) - the mutation build's set under #ifdef KF_MUTANT, the product's behind it."""
    def defines(mutant):
        return "\n".join(f"#define {name} \\\n" + render(ins).replace("\n", " \\\n") for name, ins in streams(mutant))
    Path(path).write_text(f"""{header}
#pragma once
#define {lds_bytes[0]} {lds_bytes[1]}
#define {clobbers[0]} {", ".join('"' + c + '"' for c in clobbers[1])}
#ifdef KF_MUTANT{mutant_note}
{defines(True)}
#else
{defines(False)}
#endif
""")
