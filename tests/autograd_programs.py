"""Random operator graphs for the differential test of the reverse-mode engine (Tensor::backward, update_grad, ViewGradFunction,
CatGradFunction and the arithmetic GradFunctions): a generator and two interpreters. No test functions here; the users are
tests/test_autograd_programs_reference.py (CPU: the generator against torch alone) and tests/test_gpu_autograd_programs.py (-m gpu).

make_program(seed, tier) decides from a SHADOW only - per node: shape and strides (a numpy int8 array that goes through the same view
operations), dtype, an upper bound of |value|, the number of fractional bits, whether it requires a gradient - never from computed values.

Tier "exact": all leaf data and grad_outputs are integers over a power of two, scalars are +-{0.5, 1, 2, 3, 4}, divisors are powers of two. The
shadow carries (bound, fbits) for every tensor AND for the gradient flowing back to it: every element is m / 2^fbits with an integer
|m| <= bound * 2^fbits. An instruction is kept only if bound * 2^fbits < 2^22 holds for every value and every gradient of the program (a
conversion through bfloat16, 8 significant bits: <= 2^8). That is stricter than "bound < 2^22" and it is what makes an f32 significand (24
bits) hold every sum, product, column reduction, GEMM accumulation and scatter-add exactly in any order; f64 programs keep the same limit, so
that one program can be run in either type with the same bits. Two correct engines must then agree bit for bit.

Tier "smooth": f32 leaves with uniform data, the exact tier's instructions (without dtype conversions) around ONE featured fused operator
(norms, activations, GLUs, rope, cross-entropy, the three attentions) whose input is a view, or whose output fans out into
several consumers whose gradients the engine sums, or whose only consumer hands its backward a strided gradient - the root is a cat along
the last dim, or the operator is the root under a stepped or permuted grad_output (smooth_case).

Seed blocks. The first blocks - exact seeds 0..199, smooth seeds 0..98 (the 11 operators above) - are frozen: a digest in
tests/test_autograd_programs_reference.py pins their instructions, leaf data and grad_outputs. Behind them, exact seeds 200..289 put one of
nine mixture-of-experts graphs (_moe_scenario: expert_linear, moe_dispatch, moe_combine, moe_gate as a gather - all exact on the tier's values,
with shadow bounds like gemm's) on a 2-D node of an otherwise random program, and draw them as random instructions too; smooth seeds 99..161
feature 7 more operators in 9 cases each (_featured2: softmax, log_softmax, attention and attention_qkv in their four mask families, rope_qkv,
qk_norm_rope, moe_gate(normalize=True) behind a softmax). KF_FUZZ_SEED shifts all blocks by SEED_STRIDE; a seed's block and case are read off
seed % SEED_STRIDE."""
import numpy as np

LIMIT = 2.0 ** 22
BF16_LIMIT = 2.0 ** 8
SCALARS = (0.5, 1.0, 2.0, 3.0, 4.0)
POW2 = (0.5, 1.0, 2.0, 4.0)
SMOOTH_OPS = ("rms_norm", "layer_norm", "silu", "gelu", "swiglu", "geglu", "rope", "cross_entropy", "attn", "attn_gqa", "attn_qkv")
SMOOTH_OPS2 = ("softmax", "log_softmax", "attention", "attention_qkv", "rope_qkv", "qk_norm_rope", "moe_gate")   # the second smooth block's
MOE_OPS = ("expert_linear", "moe_dispatch", "moe_combine", "moe_gate")   # exact on the exact tier's values: drawn in the second exact block only
N_SCENARIOS = 9
VIEW_OPS = ("permute", "getitem", "view", "split")


def _f2(c):  # fractional bits a multiplication by c adds; |c| in SCALARS
    return 1 if abs(c) == 0.5 else 0


class Node:
    def __init__(self, arr, dt, bound, fbits, req, view=False, src=None, pow2=False):
        self.arr, self.dt, self.bound, self.fbits, self.req = arr, dt, bound, fbits, req
        self.view, self.src, self.pow2 = view, src, pow2   # src: the node this one is a view of

    shape = property(lambda s: tuple(s.arr.shape))
    dense = property(lambda s: bool(s.arr.flags.c_contiguous))

    def offset(self):
        base = self.arr
        while base.base is not None:
            base = base.base
        return self.arr.__array_interface__["data"][0] - base.__array_interface__["data"][0]


class Builder:
    def __init__(self, rng, tier, base_dt, new_block=False):
        self.rng, self.tier, self.base_dt, self.new_block = rng, tier, base_dt, new_block
        self.nodes, self.leaves, self.instrs, self.consts, self.feat = [], [], [], [], set()
        self.must, self.fan_extra = set(), []   # nodes the root has to reach; further inputs of the fan-in cat (second blocks only)
        # Second smooth block, ahead of the featured operator: no broadcast operands. softmax and log_softmax do not see a shift that is constant
        # along their dim, qk_norm_rope and the normalised gate no such factor: the gradient of an operand broadcast that way is 0 in exact
        # arithmetic and rounding residue in f32, which torch's f32 - the noise the bound is made of - may or may not show.
        self.no_bcast = False

    # ---- nodes ---------------------------------------------------------------------------------------------------------------
    def new(self, shape_or_arr, dt, bound, fbits, req, **kw):
        arr = shape_or_arr if isinstance(shape_or_arr, np.ndarray) else np.zeros(shape_or_arr, np.int8)
        self.nodes.append(Node(arr, dt, bound, fbits, req, **kw))
        return len(self.nodes) - 1

    def leaf(self, shape, dt=None, req=None, pow2=False):
        rng = self.rng
        dt = dt or (self.base_dt if self.tier == "smooth" or rng.random() < 0.75 else ("f64" if self.base_dt == "f32" else "f32"))
        req = bool(rng.random() < 0.65) if req is None else req
        npdt = np.float32 if dt == "f32" else np.float64
        if pow2:
            data = rng.choice(POW2, size=shape) * rng.choice((-1.0, 1.0), size=shape)
            bound, fbits = 4.0, 1
        elif self.tier == "exact":
            fbits = int(rng.integers(0, 3))
            data = rng.integers(-3, 4, size=shape) / 2.0 ** fbits
            bound = 3.0
        else:
            data, bound, fbits = rng.uniform(-2, 2, size=shape), 2.0, 0
        i = self.new(tuple(shape), dt, bound, fbits, req, pow2=pow2)
        self.leaves.append((i, np.ascontiguousarray(data.astype(npdt)), req))
        return i

    def const(self, a):
        self.consts.append(a)
        return len(self.consts) - 1

    def emit(self, op, outs, ins, par=None):
        self.instrs.append((op, tuple(outs), tuple(ins), par))

    def uses(self):
        u = [0] * len(self.nodes)
        for _, _, ins, _ in self.instrs:
            for i in ins:
                if i >= 0:
                    u[i] += 1
        return u

    def pick(self, ok=lambda n: True):
        """A node satisfying ok: unused ones first (the graph stays connected), recent ones next."""
        ids = [i for i, n in enumerate(self.nodes) if ok(n)]
        if not ids:
            return None
        u = self.uses()
        fresh = [i for i in ids if u[i] == 0]
        if fresh and self.rng.random() < 0.7:
            return int(fresh[-1 - int(self.rng.integers(0, min(2, len(fresh))))])
        return int(ids[int(self.rng.integers(0, len(ids)))])

    # ---- helpers that emit the small instructions an operator's preconditions need ---------------------------------------------
    def unary(self, op, a, par=None, arr=None, bound=None, fbits=None, dt=None, view=False):
        n = self.nodes[a]
        o = self.new(np.zeros(n.shape, np.int8) if arr is None else arr, dt or n.dt, n.bound if bound is None else bound,
                     n.fbits if fbits is None else fbits, n.req, view=view, src=a if view else None)
        self.emit(op, [o], [a], par)
        return o

    def densify(self, a):
        return a if self.nodes[a].dense else self.unary("contiguous", a)

    def as_dt(self, a, dt):
        return a if self.nodes[a].dt == dt else self.unary("to", a, dt, dt=dt)

    def view_op(self, op, a, arr, par):
        n = self.nodes[a]
        if n.view and Node(arr, n.dt, 0, 0, False).offset() != 0:
            self.feat.add("view_of_view_offset")
        return self.unary(op, a, par, arr=arr, view=True)

    # ---- the exact tier's instruction set ------------------------------------------------------------------------------------------
    def binary(self):
        rng = self.rng
        op = ("add", "sub", "mul", "div")[int(rng.integers(0, 4))]
        a = self.pick()
        na = self.nodes[a]
        if op == "div":   # the divisor: a leaf of powers of two (|b| in [0.5, 4]), same shape or broadcast
            b = self.leaf(self.sub_shape(na.shape), pow2=True)
        else:
            cands = [i for i, n in enumerate(self.nodes) if n.arr.ndim == na.arr.ndim and self.bcast(na.shape, n.shape) and not n.pow2]
            # (no_bcast: a fresh operand always - (x + 3) - x would hand the featured operator a constant)
            b = int(cands[int(rng.integers(0, len(cands)))]) if cands and rng.random() < 0.5 and not self.no_bcast else self.operand(na.shape)
        if self.tier == "smooth" and a == b:   # x - x would hand the featured operator an all-zero input: nothing to measure
            b = self.operand(na.shape)
        if op != "div" and rng.random() < 0.5:
            a, b = b, a
        na, nb = self.nodes[a], self.nodes[b]
        shape = np.broadcast_shapes(na.shape, nb.shape)
        dt = "f64" if "f64" in (na.dt, nb.dt) else "f32"
        if op in ("add", "sub"):
            bound, fbits = na.bound + nb.bound, max(na.fbits, nb.fbits)
        elif op == "mul":
            bound, fbits = na.bound * nb.bound, na.fbits + nb.fbits
        else:
            bound, fbits = na.bound * 2.0, na.fbits + 2
        o = self.new(tuple(shape), dt, bound, fbits, na.req or nb.req)
        self.emit(op, [o], [a, b])
        return o

    @staticmethod
    def bcast(s, t):
        try:
            np.broadcast_shapes(s, t)
            return True
        except ValueError:
            return False

    def sub_shape(self, shape):
        """A shape of the SAME rank that broadcasts against `shape`: the same, or with extent-1 dims. (Both hosts - this one and the one it was
        modelled on - refuse operands of different rank, so the generator does not draw them: a lower-rank operand is a `view` instruction to
        [1, .., N] first, which operand() emits.)"""
        rng = self.rng
        if self.no_bcast or rng.random() < 0.4 or len(shape) == 0:
            return tuple(shape)
        return tuple(1 if rng.random() < 0.5 else v for v in shape)

    def operand(self, shape):
        """A fresh leaf that broadcasts against `shape`: of its rank, or - one time in three - of lower rank and viewed up to it."""
        rng = self.rng
        full = self.sub_shape(shape)
        lead = int(rng.integers(1, len(full))) if not self.no_bcast and len(full) >= 2 and rng.random() < 0.33 else 0
        if not lead:
            return self.leaf(full)
        leaf = self.leaf(full[lead:])
        padded = (1,) * lead + tuple(full[lead:])
        return self.view_op("view", leaf, self.nodes[leaf].arr.reshape(padded), padded)

    def scalar(self):
        rng = self.rng
        op = ("adds", "subs", "muls", "divs")[int(rng.integers(0, 4))]
        c = float(rng.choice(POW2 if op == "divs" else SCALARS) * rng.choice((-1.0, 1.0)))
        a = self.pick()
        n = self.nodes[a]
        if op in ("adds", "subs"):
            bound, fbits = n.bound + abs(c), max(n.fbits, _f2(c))
        elif op == "muls":
            bound, fbits = n.bound * abs(c), n.fbits + _f2(c)
        else:
            bound, fbits = n.bound / abs(c), n.fbits + max(0, int(np.log2(abs(c))))
        return self.unary(op, a, c, bound=bound, fbits=fbits)

    def convert(self):
        a = self.pick()
        n = self.nodes[a]
        k = int(self.rng.integers(0, 3))
        if k == 0:
            return self.unary("contiguous", a)
        if k == 1:
            return self.unary("to", a, "f64" if n.dt == "f32" else "f32", dt="f64" if n.dt == "f32" else "f32")
        return self.unary("bf16", a)   # x.bfloat16() and back to x's dtype; the caller's bound check knows the 2^8 limit

    def permute(self):
        a = self.pick(lambda n: n.arr.ndim >= 2)
        if a is None:
            return None
        perm = [int(p) for p in self.rng.permutation(self.nodes[a].arr.ndim)]
        return self.view_op("permute", a, self.nodes[a].arr.transpose(perm), perm)

    def getitem(self, a=None):
        rng = self.rng
        a = self.pick(lambda n: n.arr.ndim >= 1 and max(n.shape) >= 2) if a is None else a
        if a is None:
            return None
        n = self.nodes[a]
        key, kept = [], 0
        for d, ext in enumerate(n.shape[:int(rng.integers(1, n.arr.ndim + 1))]):
            k = int(rng.integers(0, 4))
            if k == 0 or ext < 2:
                key.append((None, None, None))
                kept += 1
            elif k == 1 and (kept or d < n.arr.ndim - 1):
                key.append(int(rng.integers(-ext, ext)))
            else:
                lo = int(rng.integers(0, ext - 1))
                hi = int(rng.integers(lo + 1, ext + 1))
                key.append((lo, hi, int(rng.integers(1, 3))))
                kept += 1
        pykey = tuple(k if isinstance(k, int) else slice(*k) for k in key)
        arr = n.arr[pykey]
        if arr.ndim == 0 or arr.size == 0:
            return None
        return self.view_op("getitem", a, arr, tuple(key))

    def view(self):
        a = self.pick(lambda n: n.dense and n.arr.size >= 2)
        if a is None:
            return None
        n = self.nodes[a]
        size = n.arr.size
        divs = [d for d in range(2, size) if size % d == 0]
        k = int(self.rng.integers(0, 3))
        if k == 0 or not divs:
            shape = (size,)
        else:
            d = int(divs[int(self.rng.integers(0, len(divs)))])
            shape = (d, size // d) if k == 1 else (d, -1)
        arr = n.arr.reshape(shape)
        return self.view_op("view", a, arr, tuple(int(v) for v in shape))

    def split(self):
        a = self.pick(lambda n: n.arr.ndim >= 1 and max(n.shape) >= 2)
        if a is None:
            return None
        n = self.nodes[a]
        dim = int(self.rng.choice([d for d, e in enumerate(n.shape) if e >= 2]))
        ext = n.shape[dim]
        cut = sorted(set(int(c) for c in self.rng.integers(1, ext, size=int(self.rng.integers(1, 3)))))
        sizes = [b - a_ for a_, b in zip([0] + cut, cut + [ext])]
        outs, at = [], 0
        for s in sizes:
            sl = [slice(None)] * n.arr.ndim
            sl[dim] = slice(at, at + s)
            arr = n.arr[tuple(sl)]
            if n.view and Node(arr, n.dt, 0, 0, False).offset() != 0:
                self.feat.add("view_of_view_offset")
            outs.append(self.new(arr, n.dt, n.bound, n.fbits, n.req, view=True, src=a))
            at += s
        self.emit("split", outs, [a], (sizes, dim))
        return outs[int(self.rng.integers(0, len(outs)))]

    def cat(self, first=None, dim=None, force_repeat=False):
        rng = self.rng
        a = self.pick(lambda n: n.arr.ndim >= 1) if first is None else first
        n = self.nodes[a]
        dim = int(rng.integers(0, n.arr.ndim)) if dim is None else dim
        same = [i for i, m in enumerate(self.nodes) if m.arr.ndim == n.arr.ndim and not m.pow2 and
                all(d == dim or x == y for d, (x, y) in enumerate(zip(m.shape, n.shape)))]
        ins = [a]
        for _ in range(int(rng.integers(1, 3))):
            # (`not same`: a is a leaf of powers of two, which `same` leaves out - it is repeated. Shifted seeds met this; the committed ones never did.)
            ins.append(a if force_repeat or rng.random() < 0.35 or not same else int(same[int(rng.integers(0, len(same)))]))
        shape = list(n.shape)
        shape[dim] = sum(self.nodes[i].shape[dim] for i in ins)
        o = self.new(tuple(shape), n.dt, max(self.nodes[i].bound for i in ins), max(self.nodes[i].fbits for i in ins),
                     any(self.nodes[i].req for i in ins))
        self.emit("cat", [o], ins, dim)
        return o

    def gemm(self):
        rng = self.rng
        a = self.pick(lambda n: n.arr.ndim >= 1 and not n.pow2)
        a = self.densify(a)
        na = self.nodes[a]
        if na.dt != self.base_dt and rng.random() < 0.5:
            a = self.as_dt(a, self.base_dt)
            na = self.nodes[a]
        K = na.shape[-1]
        cands = [i for i, n in enumerate(self.nodes) if n.arr.ndim == 2 and n.shape[0] == K and not n.pow2]
        if cands and rng.random() < 0.5:
            b = self.as_dt(self.densify(int(cands[int(rng.integers(0, len(cands)))])), na.dt)
        else:
            b = self.leaf((K, int(rng.choice((1, 2, 3, 5, 8)))), dt=na.dt)
        nb = self.nodes[b]
        N, M = nb.shape[1], na.arr.size // K
        alpha = float(rng.choice((1.0, 1.0, 0.5, 2.0, -1.0)))
        out_shape = na.shape[:-1] + (N,)
        bound, fbits = abs(alpha) * na.bound * nb.bound * K, na.fbits + nb.fbits + _f2(alpha)
        if rng.random() < 0.5:
            o = self.new(out_shape, na.dt, bound, fbits, na.req or nb.req)
            self.emit("gemm", [o], [a, b], alpha)
            return o
        extra, req = [], na.req or nb.req
        for which, shape in (("bias", (N,)), ("mul", out_shape), ("add", out_shape)):
            if rng.random() < 0.5:
                extra.append(-1)
                continue
            cands = [i for i, n in enumerate(self.nodes) if n.shape == tuple(shape) and not n.pow2 and i != a]
            e = self.as_dt(self.densify(int(cands[int(rng.integers(0, len(cands)))])), na.dt) if cands and rng.random() < 0.5 else self.leaf(shape, dt=na.dt)
            ne = self.nodes[e]
            req = req or ne.req
            if which == "mul":
                bound, fbits = bound * ne.bound, fbits + ne.fbits
            else:
                bound, fbits = bound + ne.bound, max(fbits, ne.fbits)
            extra.append(e)
        o = self.new(out_shape, na.dt, bound, fbits, req)
        self.emit("gemm_fused", [o], [a, b] + extra, alpha)
        return o

    def embedding(self):
        rng = self.rng
        t = self.pick(lambda n: n.arr.ndim == 2 and not n.pow2)
        if t is None:
            return None
        t = self.as_dt(self.densify(t), "f32")   # the scatter-add of the backward takes float, half and bfloat16 tables
        n = self.nodes[t]
        shape = (int(rng.integers(2, 7)),) if rng.random() < 0.6 else (2, 3)
        idx = rng.integers(-n.shape[0], n.shape[0], size=shape).astype(np.int64)
        idx.reshape(-1)[-1] = idx.reshape(-1)[0]   # a duplicate for certain
        o = self.new(shape + (n.shape[1],), "f32", n.bound, n.fbits, n.req)
        self.emit("embedding", [o], [t], self.const(idx))
        return o

    def random_instr(self):
        w = {"binary": 5, "scalar": 3, "convert": 2 if self.tier == "exact" else 0, "permute": 2, "getitem": 3, "view": 2, "split": 1, "cat": 2,
             "gemm": 2, "embedding": 1}
        if self.new_block and self.tier == "exact":   # (a key of its own: the first block's draws stay what they were)
            w["moe"] = 2
        names = list(w)
        p = np.array([w[k] for k in names], float)
        return getattr(self, names[int(self.rng.choice(len(names), p=p / p.sum()))])()

    def moe(self):
        return _moe_scenario(self, int(self.rng.integers(0, N_SCENARIOS)))

    # ---- gradient bounds: the reverse pass over the shadow ---------------------------------------------------------------------
    def grad_bounds(self, root, gb, gf):
        """{node: (bound, fbits)} of the gradient reaching every requiring node from `root`, or None where a limit is exceeded."""
        N = self.nodes
        g = {root: (gb, gf)}

        def give(i, b, f):
            if i >= 0 and N[i].req:
                ob, of = g.get(i, (0.0, 0))
                g[i] = (ob + b, max(of, f))

        for op, outs, ins, par in reversed(self.instrs):
            for oi, o in enumerate(outs):
                if o not in g:
                    continue
                b, f = g[o]
                lim = LIMIT
                if b * 2.0 ** f >= lim:
                    return None
                osize = max(1, N[o].arr.size)
                red = lambda i: osize / max(1, N[i].arr.size)   # noqa: E731  (a broadcast operand sums this many terms)
                if op in ("add", "sub"):
                    for i in ins:
                        give(i, b * red(i), f)
                elif op == "mul":
                    give(ins[0], b * N[ins[1]].bound * red(ins[0]), f + N[ins[1]].fbits)
                    give(ins[1], b * N[ins[0]].bound * red(ins[1]), f + N[ins[0]].fbits)
                elif op == "div":
                    give(ins[0], b * 2.0 * red(ins[0]), f + 2)
                    give(ins[1], b * N[ins[0]].bound * 4.0 * red(ins[1]), f + N[ins[0]].fbits + 4)
                elif op in ("adds", "subs", "contiguous", "to", "permute", "getitem", "view", "split"):
                    give(ins[0], b, f)
                elif op == "bf16":
                    if b * 2.0 ** f > BF16_LIMIT:
                        return None
                    give(ins[0], b, f)
                elif op == "muls":
                    give(ins[0], b * abs(par), f + _f2(par))
                elif op == "divs":
                    give(ins[0], b / abs(par), f + max(0, int(np.log2(abs(par)))))
                elif op == "cat":
                    for i in ins:
                        give(i, b, f)
                elif op in ("gemm", "gemm_fused"):
                    a_, b_ = ins[0], ins[1]
                    K = N[a_].shape[-1]
                    M, Nn = N[a_].arr.size // K, N[b_].shape[1]
                    al, fa = abs(par), _f2(par)
                    tb_, tf_ = b, f   # the gradient of the bracket (alpha a b + bias)
                    if op == "gemm_fused":
                        bias, mul, add = ins[2:]
                        give(add, b, f)
                        if mul >= 0:
                            raw_b = al * N[a_].bound * N[b_].bound * K + (N[bias].bound if bias >= 0 else 0.0)
                            raw_f = max(N[a_].fbits + N[b_].fbits + fa, N[bias].fbits if bias >= 0 else 0)
                            give(mul, b * raw_b, f + raw_f)
                            tb_, tf_ = b * N[mul].bound, f + N[mul].fbits
                        give(bias, tb_ * M, tf_)
                    give(a_, al * tb_ * N[b_].bound * Nn, tf_ + N[b_].fbits + fa)
                    give(b_, al * tb_ * N[a_].bound * M, tf_ + N[a_].fbits + fa)
                elif op == "embedding":
                    give(ins[0], b * self.consts[par].size, f)
                elif op == "expert_linear":   # dx = dy w[e]^T: Dout terms; dw[e] = x[seg]^T dy[seg]: at most T terms
                    x_, w_ = ins
                    give(x_, b * N[w_].bound * N[w_].shape[2], f + N[w_].fbits)
                    give(w_, b * N[x_].bound * N[x_].shape[0], f + N[x_].fbits)
                elif op in ("moe_dispatch", "moe_gate"):   # a gather: the gradient sums the k pairs of a token (moe_gate: normalize=False)
                    give(ins[0], b * self.consts[par[0]].shape[1], f)
                elif op == "moe_combine":
                    ys, gt = ins
                    give(ys, b * (N[gt].bound if gt >= 0 else 1.0), f + (N[gt].fbits if gt >= 0 else 0))
                    give(gt, b * N[ys].bound * N[ys].shape[1], f + N[ys].fbits)
                else:   # a smooth operator: no exactness to keep
                    for i in ins:
                        give(i, b, f)
        for b, f in g.values():
            if b * 2.0 ** f >= LIMIT:
                return None
        return g

    def values_ok(self, since):
        for n in self.nodes[since:]:
            if n.bound * 2.0 ** n.fbits >= LIMIT:
                return False
        for op, outs, ins, _ in self.instrs:
            if op == "bf16" and outs[0] >= since:
                n = self.nodes[ins[0]]
                if n.bound * 2.0 ** n.fbits > BF16_LIMIT:
                    return False
        return True

    def checkpoint(self):
        return len(self.nodes), len(self.leaves), len(self.instrs), len(self.consts), set(self.feat)

    def rollback(self, cp):
        del self.nodes[cp[0]:], self.leaves[cp[1]:], self.instrs[cp[2]:], self.consts[cp[3]:]
        self.feat = cp[4]

    def step(self, make, gb, gf, need_req=False):
        """Draw one instruction (and the small ones it needs); keep it only if every value and gradient bound stays under the limit."""
        for _ in range(40):
            cp = self.checkpoint()
            o = make()
            if o is not None and (self.tier == "smooth" or self.values_ok(cp[0])) and (self.nodes[o].req or not need_req):
                if not self.nodes[o].req or self.tier == "smooth" or self.grad_bounds(o, gb, gf) is not None:
                    return o
            self.rollback(cp)
        return None


# ---- the second exact block's mixture-of-experts scenarios ---------------------------------------------------------------------------
def _sorted_ids(rng, T, E):
    """Ascending expert ids of T rows with (T permitting) a row below 0, a row at E - both outside every segment - and an expert without rows."""
    ids = rng.integers(0, E, size=T)
    empty = int(rng.integers(0, E))
    ids[ids == empty] = (empty + 1) % E
    if T >= 3:
        ids[0], ids[-1] = -1, E
    return np.sort(ids).astype(np.int64)


def _topk_ids(rng, T, E, k, drops=1):
    """[T, k] expert ids, distinct in a row while k <= E, with `drops` pairs outside [0, E) - never two in one row."""
    ids = np.stack([rng.permutation(max(E, k))[:k] % E for _ in range(T)]).astype(np.int64)
    for t in rng.permutation(T)[:drops]:
        ids[t, int(rng.integers(0, k))] = (-1, E)[int(rng.integers(0, 2))]
    return ids


def _moe_scenario(b, sc):
    """One of the N_SCENARIOS small graphs of expert_linear / moe_dispatch / moe_combine / moe_gate on a 2-D node of the program; returns
    its output node, or None where no node fits. Bounds (bound, fbits) as gemm and embedding keep them."""
    rng, N = b.rng, b.nodes

    def pick2d(min_cols=2):
        a = b.pick(lambda n: n.arr.ndim == 2 and not n.pow2 and n.shape[0] <= 8 and min_cols <= n.shape[1] <= 8)
        return None if a is None else b.as_dt(a, "f32")   # (expert_linear and the routing have no f64)

    def window(a, width=None):   # a column window of a: row-pitched, read in place through a leading dimension
        cols = N[a].shape[1]
        width = cols - 1 if width is None else width
        lo = int(rng.integers(0, cols - width + 1))
        return b.view_op("getitem", a, N[a].arr[:, lo:lo + width], ((None, None, None), (lo, lo + width, 1)))

    def weight(E, Din):
        return b.leaf((E, Din, int(rng.integers(3, 9))), dt="f32", req=True)

    def el(x, w, par):
        nx, nw = N[x], N[w]
        o = b.new((nx.shape[0], nw.shape[2]), "f32", nx.shape[1] * nx.bound * nw.bound, nx.fbits + nw.fbits, nx.req or nw.req)
        b.emit("expert_linear", [o], [x, w], par)
        return o

    def offsets(T, E):   # built on the host, or by segment_offsets on the device from the sorted ids
        ids = _sorted_ids(rng, T, E)
        if rng.random() < 0.5:
            return ("ids", b.const(ids), E)
        return ("offsets", b.const(np.searchsorted(ids, np.arange(E + 1), side="left").astype(np.int64)), E)

    def plan(T, E=None):
        E = int(rng.integers(2, 5)) if E is None else E
        k = int(rng.integers(1, 4))
        return b.const(_topk_ids(rng, T, E, k, drops=int(rng.integers(1, 3)))), E, k

    def dispatch(x, cidx, E, k):
        n = N[x]
        o = b.new((n.shape[0] * k, n.shape[1]), "f32", n.bound, n.fbits, n.req)
        b.emit("moe_dispatch", [o], [x], (cidx, E))
        return o

    def combine(ys, gate, cidx, E, k):
        n, g = N[ys], (N[gate] if gate >= 0 else None)
        o = b.new((n.shape[0] // k, n.shape[1]), "f32", k * n.bound * (g.bound if g else 1.0), n.fbits + (g.fbits if g else 0),
                  n.req or bool(g and g.req))
        b.emit("moe_combine", [o], [ys, gate], (cidx, E))
        return o

    def gate_of(p, cidx, E, k):
        n = N[p]
        o = b.new((n.shape[0], k), "f32", n.bound, n.fbits, n.req)
        b.emit("moe_gate", [o], [p], (cidx, E, False))
        return o

    def add(a, c):
        o = b.new(N[a].shape, "f32", N[a].bound + N[c].bound, max(N[a].fbits, N[c].fbits), N[a].req or N[c].req)
        b.emit("add", [o], [a, c])
        return o

    x = pick2d(3 if sc in (1, 7, 8) else 2)
    if x is None:
        return None
    T, cols = N[x].shape
    E = int(rng.integers(2, 5))
    if sc == 0:
        return el(x, weight(E, cols), offsets(T, E))
    if sc == 1:   # x is a column window of a wider tensor
        xw = window(x)
        return el(xw, weight(E, cols - 1), offsets(T, E))
    if sc == 2:   # the same weight reached by two expert_linear calls
        w = weight(E, cols)
        return add(el(x, w, offsets(T, E)), el(b.unary("muls", x, 2.0, bound=N[x].bound * 2.0), w, offsets(T, E)))
    if sc == 3:   # the same weight reached by expert_linear and, through w[e], by gemm
        xd, w = b.densify(x), weight(E, cols)
        e = int(rng.integers(0, E))
        we = b.view_op("getitem", w, N[w].arr[e], (e,))
        y2 = b.new((T, N[w].shape[2]), "f32", cols * N[xd].bound * N[w].bound, N[xd].fbits + N[w].fbits, True)
        b.emit("gemm", [y2], [xd, we], 1.0)
        return add(el(x, w, offsets(T, E)), y2)
    if sc == 4:   # dispatch and combine without a gate
        cidx, E, k = plan(T)
        return combine(dispatch(x, cidx, E, k), -1, cidx, E, k)
    if sc == 5:   # dispatch, the expert product on the plan's offsets, combine under a leaf gate of powers of two
        cidx, E, k = plan(T)
        h = el(dispatch(x, cidx, E, k), weight(E, cols), ("plan", cidx, E))
        return combine(h, b.leaf((T, k), dt="f32", req=True, pow2=True), cidx, E, k)
    if sc == 6:   # a gate that needs no gradient, or rows that need none under a gate that does
        cidx, E, k = plan(T)
        if rng.random() < 0.5:
            return combine(dispatch(x, cidx, E, k), b.leaf((T, k), dt="f32", req=False, pow2=True), cidx, E, k)
        return combine(b.leaf((T * k, int(rng.integers(3, 9))), dt="f32", req=False), b.leaf((T, k), dt="f32", req=True, pow2=True), cidx, E, k)
    # the gate gathered from p, a column window of the node (or all of it), over the node's own rows dispatched
    E = int(rng.integers(2, min(4, cols - 1) + 1))
    p = x if cols <= 4 and sc == 8 and rng.random() < 0.5 else window(x, E)
    cidx, E, k = plan(T, N[p].shape[1])
    gate = gate_of(p, cidx, E, k)
    xs = dispatch(x, cidx, E, k)
    if sc == 7:
        return combine(xs, gate, cidx, E, k)
    return combine(el(xs, weight(E, cols), ("plan", cidx, E)), gate, cidx, E, k)   # sc 8: the whole layer


def host_offsets(par, consts, T):
    """The offsets of an expert_linear instruction as int64 [E + 1]: (how they are made, const, E)."""
    how, cidx, E = par
    if how == "offsets":
        return consts[cidx]
    if how == "ids":
        from tests import gemm_seg_ref
        return gemm_seg_ref.segment_offsets(consts[cidx], E)
    from tests import moe_ref
    return moe_ref.plan(consts[cidx], E)[0]


def _sanitized(offsets, T):
    from tests import gemm_seg_ref
    return gemm_seg_ref.sanitize(offsets, T)


def attn_vis(mask, consts, B, Sq, Skv):
    """bool [B, Sq, Skv] of an attention instruction's mask (family, kv_len const, prefix_len const, window, causal, cu_doclens const): built
    by the visibility functions of the kernels' own references."""
    from tests import attn_doc_ref, attn_full_ref, attn_prefix_ref, attn_window_ref
    fam, kv, pre, win, causal, doc = mask
    kv = None if kv is None else consts[kv]
    if fam == "full":
        return attn_full_ref.key_len_vis(kv, Sq, Skv, B)
    if fam == "prefix":
        return attn_prefix_ref.prefix_vis(kv, None if pre is None else consts[pre], Sq, Skv, B)
    if fam == "window":
        return attn_window_ref.window_vis(kv, win[0], 0 if causal else win[1], Sq, Skv, B)
    assert fam == "doc" and Sq == Skv
    return attn_doc_ref.doc_vis(consts[doc], Sq, causal)


def _case_mask(b, kind, case):
    """The mask of the attention operators' case 0..8: every family, with the edges each family has."""
    K = lambda a: b.const(np.asarray(a, np.int64))   # noqa: E731
    if case == 8:   # attention: keys of another length than the queries (Skv = 6); attention_qkv: a causal window with an open right side
        return ("full", K([5, 2]), None, None, False, None) if kind == "attention" else ("window", None, None, (2, None), True, None)
    return (lambda: ("full", K([0, 3]), None, None, False, None),            # a batch without keys
            lambda: ("prefix", K([2, 4]), None, None, True, None),           # causal over a padded batch
            lambda: ("prefix", None, K([3, 1]), None, True, None),           # prefix-LM
            lambda: ("window", None, None, (1, None), False, None),
            lambda: ("window", None, None, (None, 0), True, None),
            lambda: ("window", K([2, 4]), None, (0, 1), False, None),        # queries 2 and 3 of batch 0 see no key
            lambda: ("doc", None, None, None, False, K([[0, 2, 2, 3], [0, 1, 4, 4]])),   # a zero-length document; token 3 of row 0 in none
            lambda: ("doc", None, None, None, True, K([[0, 2, 2, 3], [0, 1, 4, 4]])))[case]()


def _featured2(b, kind, case, view_fed, fanin):
    """The second smooth block's operators on the pool's main [T, d] tensor; case = 3 * variant + (view, fan-in, noncontig)."""
    rng, N = b.rng, b.nodes
    B_, S_, H_, D_ = 2, 4, 2, 8
    T, d = B_ * S_, H_ * D_
    variant = case // 3
    x = b.densify(b.pick(lambda n: n.shape == (T, d) and n.req))

    def smooth(op, ins, shape, par=None):
        o = b.new(shape if isinstance(shape, np.ndarray) else tuple(shape), "f32", 1.0, 0, True)
        b.emit(op, [o], ins, par)
        for i in ins:
            if i >= 0 and N[i].view:
                b.feat.add(kind + "_from_view")
        return o

    if kind in ("softmax", "log_softmax"):
        dim = (-1, -1, 0)[variant] if view_fed else (-1, 0, -1)[variant]
        if view_fed and variant == 1:   # a permuted view: densified
            x = b.view_op("permute", x, N[x].arr.transpose(1, 0), [1, 0])
        elif view_fed:   # a column window: row-pitched, read in place
            x = b.view_op("getitem", x, N[x].arr[:, 2:14], ((None, None, None), (2, 14, 1)))
        shape = N[x].shape
        if dim == 0:   # dim and the last dimension change places and back: the result is a permuted view of a dense tensor, not a dense one
            shape = np.zeros(shape[::-1], np.int8).transpose(1, 0)
        return smooth(kind, [x], shape, (dim, (1.0, 0.5, 2.0)[variant]))

    def heads(t, h, S):   # [B*S, h*D] -> [B, h, S, D]: a dense view as it stands (view_fed), or split heads the usual way
        if view_fed:
            return b.view_op("view", t, N[t].arr.reshape(B_, h, S, D_), (B_, h, S, D_))
        t4 = b.view_op("view", t, N[t].arr.reshape(B_, S, h, D_), (B_, S, h, D_))
        return b.densify(b.view_op("permute", t4, N[t4].arr.transpose(0, 2, 1, 3), [0, 2, 1, 3]))

    def packed(kv, v_req):   # cat([x, k, v]) along the columns; view-fed: a dense view of a view of it
        k, v = b.leaf((T, kv * D_), req=True), b.leaf((T, kv * D_), req=v_req)
        q = b.new((T, d + 2 * kv * D_), "f32", 2.0, 0, True)
        b.emit("cat", [q], [x, k, v], 1)
        if view_fed:
            q = b.view_op("view", q, N[q].arr.reshape(-1), (-1,))
            q = b.view_op("view", q, N[q].arr.reshape(T, -1), (T, -1))
        return q

    kv = H_ if case % 2 == 0 else 1
    if kind == "attention":
        Skv = 6 if case == 8 else S_
        k, v = b.leaf((B_ * Skv, kv * D_), req=True), b.leaf((B_ * Skv, kv * D_), req=case % 3 != 1)
        return smooth(kind, [heads(x, H_, S_), heads(k, kv, Skv), heads(v, kv, Skv)], (B_, H_, S_, D_), _case_mask(b, kind, case))
    if kind == "attention_qkv":
        return smooth(kind, [packed(kv, bool(case % 3))], (T, d), (B_, S_, H_, kv, _case_mask(b, kind, case)))
    if kind in ("rope_qkv", "qk_norm_rope"):
        R, inter = (8, 4, 4)[variant], bool(case % 2)
        pos = b.const(rng.integers(0, 16, size=(T,)).astype(np.int64)) if case in (1, 3, 8) else None
        q = packed(kv, bool(case % 3))
        if kind == "rope_qkv":
            return smooth(kind, [q], N[q].shape, (B_, S_, H_, kv, R, inter, pos))
        wq = -1 if case in (1, 5) else b.leaf((D_,), req=case % 2 == 0)
        wk = -1 if case in (2, 5) else b.leaf((D_,), req=case % 4 != 0)
        return smooth(kind, [q, wq, wk], N[q].shape, (B_, S_, H_, kv, 0 if case in (3, 7) else R, inter, pos, 1e-6))   # R = 0: no tables
    assert kind == "moe_gate"   # the router: softmax -> moe_gate(normalize=True) (-> moe_combine, once, where the gate fans out)
    p = b.new((T, d), "f32", 1.0, 0, True)
    b.emit("softmax", [p], [x], (-1, 1.0))
    E = d
    if view_fed:
        p, E = b.view_op("getitem", p, N[p].arr[:, 2:14], ((None, None, None), (2, 14, 1))), 12
    k = (2, 3, 2)[variant]
    cidx = b.const(_topk_ids(rng, T, E, k, drops=2))
    o = smooth(kind, [p], (T, k), (cidx, E, True))
    if fanin:
        xs = b.new((T * k, d), "f32", 2.0, 0, True)
        b.emit("moe_dispatch", [xs], [x], (cidx, E))
        y = b.new((T, d), "f32", 2.0, 0, True)
        b.emit("moe_combine", [y], [xs, o], (cidx, E))
        b.fan_extra = [y]
    return o


# ---- the smooth tier's featured operator -----------------------------------------------------------------------------------------
def _featured(b, kind, variant, view_fed, noncontig=False):
    """Emit `kind` on the pool's main [T, d] tensor; returns the operator's output node. B, S, H, D = 2, 4, 2, 8: T = 8, d = 16."""
    rng, N = b.rng, b.nodes
    B_, S_, H_, D_ = 2, 4, 2, 8
    T, d = B_ * S_, H_ * D_
    main = lambda: b.densify(b.pick(lambda n: n.shape == (T, d) and n.req))   # noqa: E731
    x = main()

    def smooth(op, ins, shape, par=None):
        o = b.new(tuple(shape), "f32", 1.0, 0, True)
        b.emit(op, [o], ins, par)
        for i in ins:
            if i >= 0 and N[i].view:
                b.feat.add(kind + "_from_view")
        return o

    if kind in ("rms_norm", "layer_norm", "cross_entropy"):
        if view_fed:   # a dense view with a storage offset: rows 1.. of the tensor
            x = b.view_op("getitem", x, N[x].arr[1:], ((1, None, 1),))
        rows, cols = N[x].shape
        w = b.leaf((cols,), req=True) if variant % 2 == 0 or kind == "layer_norm" else -1
        if kind == "rms_norm":
            return smooth(kind, [x, w], (rows, cols), 1e-5)
        if kind == "layer_norm":
            return smooth(kind, [x, w, b.leaf((cols,), req=bool(variant % 2))], (rows, cols), 1e-5)
        tgt = rng.integers(0, cols, size=(rows,)).astype(np.int64)
        tgt[1] = -100
        red = "none" if noncontig else ("none", "sum", "mean")[variant % 3]   # (a one-element loss has no strided gradient)
        return smooth(kind, [x], (rows,) if red == "none" else (1,), (b.const(tgt), red, -100))
    if kind in ("silu", "gelu", "swiglu", "geglu"):
        approx = ("none", "tanh")[variant % 2]
        if kind in ("silu", "gelu"):
            if view_fed:   # a column window: rows with a leading dimension wider than the row
                x = b.view_op("getitem", x, N[x].arr[:, 2:14], ((None, None, None), (2, 14, 1)))
            return smooth(kind, [x], N[x].shape, approx)
        if variant % 2 == 0:   # packed gate | up
            if view_fed:
                x = b.view_op("getitem", x, N[x].arr[1:7], ((1, 7, 1),))
            return smooth(kind, [x, -1], (N[x].shape[0], d // 2), approx)
        parts = [b.new(N[x].arr[:, i * 8:(i + 1) * 8], "f32", 2.0, 0, True, view=True, src=x) for i in range(2)]
        b.emit("split", parts, [x], ([8, 8], 1))
        if not view_fed:
            parts = [b.densify(p) for p in parts]
        return smooth(kind, parts, (T, 8), approx)
    if kind == "rope":
        x4 = b.view_op("view", x, N[x].arr.reshape(B_, S_, H_, D_), (B_, S_, H_, D_))
        xp = b.view_op("permute", x4, N[x4].arr.transpose(0, 2, 1, 3), [0, 2, 1, 3])
        if not view_fed:
            xp = b.densify(xp)
        R = (8, 4)[variant % 2]
        pos = None if variant % 3 else b.const(rng.integers(0, 16, size=(B_ * S_,)).astype(np.int64))
        return smooth(kind, [xp], (B_, H_, S_, D_), (R, bool(variant % 2), pos))

    def heads(t, h):   # [T, h*D] -> [B, h, S, D]: a dense view as it stands (view_fed), or split heads the usual way
        if view_fed:
            return b.view_op("view", t, N[t].arr.reshape(B_, h, S_, D_), (B_, h, S_, D_))
        t4 = b.view_op("view", t, N[t].arr.reshape(B_, S_, h, D_), (B_, S_, h, D_))
        return b.densify(b.view_op("permute", t4, N[t4].arr.transpose(0, 2, 1, 3), [0, 2, 1, 3]))

    if kind == "attn":
        k = x if variant % 2 else b.leaf((T, d), req=True)
        v = b.leaf((T, d), req=bool(variant % 3))
        return smooth(kind, [heads(x, H_), heads(k, H_), heads(v, H_)], (B_, H_, S_, D_))
    if kind == "attn_gqa":
        k, v = b.leaf((T, D_), req=True), b.leaf((T, D_), req=bool(variant % 2))
        return smooth(kind, [heads(x, H_), heads(k, 1), heads(v, 1)], (B_, H_, S_, D_))
    assert kind == "attn_qkv"
    kv = 1 if variant % 2 else H_
    k, v = b.leaf((T, kv * D_), req=True), b.leaf((T, kv * D_), req=bool(variant % 3))
    q = b.new((T, d + 2 * kv * D_), "f32", 2.0, 0, True)
    b.emit("cat", [q], [x, k, v], 1)
    if view_fed:
        q = b.view_op("view", q, N[q].arr.reshape(-1), (-1,))
        q = b.view_op("view", q, N[q].arr.reshape(T, -1), (T, -1))
    return smooth(kind, [q], (T, d), (B_, S_, H_, kv))


def make_program(seed, tier="exact"):
    """A program: {"seed", "tier", "leaves": [(node, array, requires)], "instrs": [(op, outs, ins, par)], "consts", "root", "grads":
    [(base array, how, par)], "nodes": [(shape, dtype, bound, fbits, requires)], "gbounds": {node: (bound, fbits)}, "features": set}."""
    assert tier in ("exact", "smooth")
    for attempt in range(200):
        rng = np.random.default_rng([seed, attempt, 0 if tier == "exact" else 1])
        new = in_second_block(seed, tier)
        b = Builder(rng, tier, "f32" if tier == "smooth" or rng.random() < 0.6 else "f64", new)
        twice = seed % 4 == 3
        gb, gf = (4.0 if twice else 2.0), 1
        if tier == "exact" and new:   # a 2-D leaf, a few instructions, the seed's mixture-of-experts scenario on one of their nodes, a few more
            b.leaf((int(rng.integers(5, 9)), int(rng.integers(3, 9))), req=True)
            for _ in range(int(rng.integers(1, 4))):
                b.step(b.random_instr, gb, gf)
            o = b.step(lambda: _moe_scenario(b, (seed % SEED_STRIDE - N_EXACT) % N_SCENARIOS), gb, gf, need_req=True)
            if o is None:
                continue
            b.must.add(o)
            for _ in range(int(rng.integers(0, 3))):
                b.step(b.random_instr, gb, gf)
            root = b.step(b.random_instr, gb, gf, need_req=True)
        elif tier == "exact":
            shape = tuple(int(v) for v in rng.choice((1, 2, 3, 4, 5, 6), size=int(rng.integers(1, 4))))
            b.leaf(shape, req=True)
            for _ in range(int(rng.integers(5, 12))):
                b.step(b.random_instr, gb, gf)
            root = b.step(b.random_instr, gb, gf, need_req=True)
        else:
            kind, mode, variant = smooth_case(seed)
            view_fed = mode == "view"
            b.leaf((8, 16), req=True)
            b.no_bcast = new
            for _ in range(int(rng.integers(1, 4))):
                b.step(lambda: (b.binary, b.scalar)[int(rng.integers(0, 2))](), gb, gf)
            b.no_bcast = False
            if new:
                o = _featured2(b, kind, 3 * variant + ("view", "fanin", "noncontig").index(mode), view_fed, mode == "fanin")
            else:
                o = _featured(b, kind, variant, view_fed, mode == "noncontig")
            if mode == "noncontig":
                # the operator's ONLY consumer hands its backward a strided gradient: the root is cat([o, other], last dim), whose backward narrows
                # the root's gradient to o's columns - or o is the root itself and the grad_output is a stepped or permuted view
                no = b.nodes[o]
                if no.arr.ndim >= 2 and variant % 2 == 0:
                    other = b.leaf(no.shape, req=bool(seed % 2))
                    root = b.new(no.shape[:-1] + (2 * no.shape[-1],), "f32", 2.0, 0, True)
                    b.emit("cat", [root], [o, other], no.arr.ndim - 1)
                    how = None
                else:
                    root, how = o, ("step" if no.arr.ndim == 1 or variant % 4 == 1 else "permute")
                prog = _finish(b, root, seed, tier, twice, how, (kind, o))
                if prog is not None:
                    return prog
                continue
            if mode == "fanin":   # the operator's gradient: the sum of two or three consumers (the engine adds the cat's windows to the rest)
                o2 = b.unary("muls", o, 2.0)
                wide = (3 if seed % 2 else 2) * b.nodes[o].shape[-1] + sum(b.nodes[i].shape[-1] for i in b.fan_extra)
                c = b.new(b.nodes[o].shape[:-1] + (wide,), "f32", 2.0, 0, True)
                b.emit("cat", [c], ([o, o, o2] if seed % 2 else [o, o2]) + b.fan_extra, b.nodes[o].arr.ndim - 1)
            for _ in range(int(rng.integers(1, 4))):
                b.step(b.random_instr, gb, gf)
            root = b.step(b.random_instr, gb, gf, need_req=True)
        if root is None:
            continue
        prog = _finish(b, root, seed, tier, twice)
        if prog is not None:
            return prog
    raise AssertionError(f"no program for seed {seed}, tier {tier}")


def smooth_case(seed):
    """(operator, how it is fed, variant) of a smooth-tier seed: 99 seeds = 11 operators x (view, fan-in) x 3 variants, then x (noncontig) x 3;
    the second block's 63 = 7 operators x 3 variants x (view, fan-in, noncontig)."""
    if in_second_block(seed, "smooth"):   # 63 seeds = 7 operators x case 0..8; case = 3 * variant + (view, fan-in, noncontig)
        s = (seed % SEED_STRIDE - N_SMOOTH) % N_SMOOTH2
        case = s // len(SMOOTH_OPS2)
        return SMOOTH_OPS2[s % len(SMOOTH_OPS2)], ("view", "fanin", "noncontig")[case % 3], case // 3
    s = seed % N_SMOOTH
    kind = SMOOTH_OPS[s % len(SMOOTH_OPS)]
    if s < 66:
        return kind, ("view", "fanin")[(s // 11) % 2], s // 22
    return kind, "noncontig", (s - 66) // 11


def _col_window(n):
    a = n.arr
    return a.ndim == 2 and a.shape[1] > 1 and a.strides[1] == 1 and a.strides[0] > a.shape[1]   # (int8 shadow: strides in elements)


def _cover_second_blocks(b, instrs, uses, feat):
    """What the reached instructions of the second blocks' operators cover, read off their parameters, constants and the shadow."""
    N, consts = b.nodes, b.consts
    w_el, w_gemm = {}, {}
    producer = {o: op for op, outs, _, _ in instrs for o in outs}

    def routing(cidx, E):
        ids = consts[cidx]
        feat.add(f"moe_k{ids.shape[1]}")
        if ((ids < 0) | (ids >= E)).any():
            feat.add("moe_dropped_pair")

    for op, outs, ins, par in instrs:
        if op == "expert_linear":
            x, w = ins
            T, E = N[x].shape[0], par[2]
            off = _sanitized(host_offsets(par, consts, T), T)
            feat.add("expert_linear_offsets_" + par[0])
            if (off[1:] == off[:-1]).any():
                feat.add("expert_linear_empty_expert")
            if off[0] > 0 or off[E] < T:
                feat.add("expert_linear_uncovered_rows")
            if _col_window(N[x]):
                feat.add("expert_linear_x_column_window")
            if producer.get(x) == "to":
                feat.add("expert_linear_behind_a_conversion")
            w_el[w] = w_el.get(w, 0) + 1
        elif op == "gemm" and N[ins[1]].view and N[ins[1]].src is not None:
            w_gemm[N[ins[1]].src] = 1
        elif op == "moe_dispatch":
            routing(par[0], par[1])
            if _col_window(N[ins[0]]):
                feat.add("moe_dispatch_x_column_window")
        elif op == "moe_combine":
            ys, gate = ins
            routing(par[0], par[1])
            feat.add("moe_combine_ys_" + ("requiring" if N[ys].req else "not_requiring"))
            if gate < 0:
                feat.add("moe_combine_gate_none")
            else:
                feat.add("moe_combine_gate_" + ("requiring" if N[gate].req else "not_requiring"))
                feat.add("moe_combine_gate_" + ("from_moe_gate" if producer.get(gate) == "moe_gate" else "leaf"))
        elif op == "moe_gate":
            routing(par[0], par[1])
            feat.add("moe_gate_normalize" if par[2] else "moe_gate_gather")
            if _col_window(N[ins[0]]):
                feat.add("moe_gate_p_column_window")
        elif op in ("softmax", "log_softmax"):
            nd = N[ins[0]].arr.ndim
            if par[0] % nd != nd - 1:
                feat.add(op + "_nonlast_dim")
            if par[1] != 1.0:
                feat.add(op + "_scale")
            feat.add(op + ("_column_window" if _col_window(N[ins[0]]) else "_dense" if N[ins[0]].dense else "_permuted_view"))
        elif op in ("attention", "attention_qkv"):
            mask = par if op == "attention" else par[4]
            fam, kv, pre, win, causal, doc = mask
            if op == "attention":
                Bq, Hq, Sq, _ = N[ins[0]].shape
                Hkv, Skv = N[ins[1]].shape[1], N[ins[1]].shape[2]
            else:
                Bq, Sq, Hq, Hkv = par[:4]
                Skv = Sq
            feat.add(f"{op}_{fam}")
            feat.add(f"{op}_hkv_" + ("h" if Hkv == Hq else "1"))
            if Skv != Sq:
                feat.add(op + "_skv_ne_sq")
            if fam == "prefix":
                feat.add(op + ("_causal_no_prefix" if pre is None else "_prefix_len"))
            if fam == "window":
                feat.add(op + "_window_" + ("causal" if causal else "noncausal"))
                for side, v in zip(("left", "right"), win):
                    feat.add(f"{op}_window_{side}_" + ("none" if v is None else "0" if v == 0 else "small"))
            vis = attn_vis(mask, consts, Bq, Sq, Skv)
            keyless = ~vis.any(-1)
            if keyless.any() and not keyless.all():
                feat.add(op + "_keyless_query")
            if kv is not None and (consts[kv] == 0).any():
                feat.add(op + "_kv_len_0")
            if fam == "doc":
                cu = consts[doc]
                feat.add(op + ("_doc_causal" if causal else "_doc_full"))
                if (np.diff(cu, axis=1) == 0).any():
                    feat.add(op + "_zero_length_document")
                if (cu[:, -1] < Sq).any():
                    feat.add(op + "_token_in_no_document")
        elif op in ("rope_qkv", "qk_norm_rope"):
            Bq, Sq, Hq, kvh, R, inter, pos = par[:7]
            D = N[ins[0]].shape[1] // (Hq + 2 * kvh)
            feat.add(op + ("_positions" if pos is not None else "_no_positions"))
            feat.add(op + ("_interleaved" if inter else "_rotate_half"))
            feat.add(f"{op}_hkv_" + ("h" if kvh == Hq else "1"))
            if 0 < R < D:
                feat.add(op + "_r_lt_d")
            if op == "qk_norm_rope":
                feat.add(op + ("_no_tables" if R == 0 else "_tables"))
                feat.add(op + ("_none_weight" if min(ins[1:]) < 0 else "_both_weights"))
                for w in ins[1:]:
                    if w >= 0:
                        feat.add(op + "_weight_" + ("requiring" if N[w].req else "not_requiring"))
    for w, n in w_el.items():
        if N[w].req and n >= 2:
            feat.add("expert_linear_w_reached_twice")
        if N[w].req and w in w_gemm:
            feat.add("expert_linear_w_also_through_gemm")


def _finish(b, root, seed, tier, twice, force_how=None, noncontig=None):
    rng, N = b.rng, b.nodes
    reach, order = {root}, []
    for ins_i in range(len(b.instrs) - 1, -1, -1):
        op, outs, ins, par = b.instrs[ins_i]
        if any(o in reach for o in outs):
            order.append(ins_i)
            reach.update(i for i in ins if i >= 0)
    if any(m not in reach for m in b.must):
        return None
    # the featured operators: any of the first block's, the seed's own in the second (whose router case holds a softmax besides its moe_gate)
    featured = () if tier == "exact" else ((smooth_case(seed)[0],) if b.new_block else SMOOTH_OPS)
    if tier == "smooth" and not any(b.instrs[i][0] in featured for i in order):
        return None
    mode = smooth_case(seed)[1] if tier == "smooth" else None
    gbounds = b.grad_bounds(root, 4.0 if twice else 2.0, 1)
    if gbounds is None and tier == "exact":
        return None
    # ---- grad_outputs: one or two, a third of the programs hand theirs over as a non-contiguous view
    shape = N[root].shape
    npdt = np.float32 if N[root].dt == "f32" else np.float64
    grads = []
    for gi in range(2 if twice else 1):
        how = (force_how or ("plain", "permute", "step")[seed % 3]) if gi == 0 else "plain"
        if how == "permute" and len(shape) < 2:
            how = "step"
        perm = [int(p) for p in rng.permutation(len(shape))] if how == "permute" else None
        if how == "permute" and perm == sorted(perm):
            perm = perm[::-1]
        base_shape = tuple(shape[perm.index(i)] for i in range(len(shape))) if how == "permute" else (shape[:-1] + (2 * shape[-1],) if how == "step" else shape)
        data = rng.integers(-2, 3, size=base_shape) / 2.0 if tier == "exact" else rng.uniform(-1, 1, size=base_shape)
        grads.append((np.ascontiguousarray(data.astype(npdt)), how, perm))
    # ---- what the program covers (over the part the root reaches)
    feat = set(b.feat)
    uses = [0] * len(N)
    for i in order:
        op, outs, ins, par = b.instrs[i]
        feat.add(op)
        for j in ins:
            if j >= 0:
                uses[j] += 1
        if op in ("add", "sub", "mul"):
            for j in ins:
                if N[j].req and N[j].shape != N[outs[0]].shape:
                    feat.add("bcast_grad_" + op)
        if op == "cat" and len(set(ins)) < len(ins) and N[ins[0]].req:
            feat.add("cat_repeat")
        if op == "cat" and len({N[j].dt for j in ins}) > 1:
            feat.add("cat_mixed_dtype")
        if op == "embedding":
            feat.add("embedding_negative" if (b.consts[par] < 0).any() else "embedding")
    for i in order:
        op, outs, ins, par = b.instrs[i]
        if op in featured:
            if uses[outs[0]] >= 2:
                feat.add(op + "_from_fanin")
            elif mode == "fanin":
                return None
    _cover_second_blocks(b, [b.instrs[i] for i in order], uses, feat)
    if noncontig is not None:   # the gradient the featured operator's backward receives is strided: checked on the shadow, not assumed
        kind, o = noncontig
        if root == o:
            base, how, perm = grads[0]
            g = np.zeros(base.shape, np.int8)
            g = g.transpose(perm) if how == "permute" else g[..., ::2]
        else:
            g = np.zeros(N[root].shape, np.int8)[..., :N[o].shape[-1]]
        if uses[o] != (0 if root == o else 1) or g.flags.c_contiguous or g.shape != N[o].shape:
            return None
        feat.add(kind + "_noncontig_grad")
    leaf_ids = {i for i, _, _ in b.leaves}
    if any(u >= 3 and N[i].req and i not in leaf_ids for i, u in enumerate(uses)):
        feat.add("fanin3")
    if any(u >= 2 and N[i].req and i in leaf_ids for i, u in enumerate(uses)):
        feat.add("leaf_reached_twice")
    if any(not r and i in reach for i, _, r in b.leaves):
        feat.add("non_requiring_leaf")
    if twice:
        feat.add("double_backward")
    if grads[0][1] != "plain":
        feat.add("noncontig_grad_" + grads[0][1])
    return {"seed": seed, "tier": tier, "leaves": list(b.leaves), "instrs": list(b.instrs), "consts": list(b.consts), "root": root, "grads": grads,
            "nodes": [(n.shape, n.dt, n.bound, n.fbits, n.req) for n in N], "gbounds": gbounds or {}, "features": feat,
            "reached": reach, "scenario": (seed % SEED_STRIDE - N_EXACT) % N_SCENARIOS if tier == "exact" and b.new_block else None}


# ---- interpreters ---------------------------------------------------------------------------------------------------------------------
def rope_tables(P, R, base=10000.0):
    """f32 tables rounded from f64, [P, R / 2] each: both interpreters read these same values."""
    i = np.arange(R // 2, dtype=np.float64)
    th = np.arange(P, dtype=np.float64)[:, None] * base ** (-2 * i / R)[None, :]
    return np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)


def _pykey(key):
    return tuple(k if isinstance(k, int) else slice(*k) for k in key)


def _grad_view(t, how, perm):
    if how == "permute":
        return t.permute(*perm)
    if how == "step":
        return t[(slice(None),) * (t.dim() - 1) + (slice(None, None, 2),)]
    return t


def _torch_attention(q, k, v, vis):
    """where(any key visible, softmax(masked scores), 0) @ v of q [B, Hq, Sq, D] over k, v [B, Hkv, Skv, D] under vis [B, Sq, Skv]: a query without
    a key gives a zero row and no gradient (scaled_dot_product_attention gives NaN there)."""
    import torch
    g = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    m = torch.from_numpy(np.ascontiguousarray(vis))[:, None]
    some = m.any(-1, keepdim=True)
    s = torch.matmul(q, k.transpose(-1, -2)) / float(np.sqrt(q.shape[-1]))
    s = torch.where(some, s.masked_fill(~m, float("-inf")), torch.zeros((), dtype=s.dtype))
    p = torch.where(some & m, torch.softmax(s, -1), torch.zeros((), dtype=s.dtype))
    return torch.matmul(p, v)


def run_torch(prog, dtype=None, trace=False):
    """The program in torch on the CPU. dtype None: every tensor in the program's own dtype; torch.float32 / torch.float64: everything in that
    one type (a conversion keeps the type; the bfloat16 round trip stays). Returns {"root": array, "grads": {leaf node: array or None}} and, with
    trace, "values" and "node_grads" of every node."""
    import torch
    import torch.nn.functional as F

    tdt = {"f32": torch.float32, "f64": torch.float64}
    own = lambda i: dtype or tdt[prog["nodes"][i][1]]   # noqa: E731
    T, consts = {}, prog["consts"]
    for i, arr, req in prog["leaves"]:
        T[i] = torch.tensor(arr, dtype=own(i), requires_grad=req)
    for op, outs, ins, par in prog["instrs"]:
        x = [T[i] if i >= 0 else None for i in ins]
        o = outs[0]
        if op in ("add", "sub", "mul", "div"):
            r = {"add": torch.add, "sub": torch.sub, "mul": torch.mul, "div": torch.div}[op](x[0], x[1])
        elif op in ("adds", "subs", "muls", "divs"):
            r = {"adds": x[0] + par, "subs": x[0] - par, "muls": x[0] * par, "divs": x[0] / par}[op]
        elif op == "contiguous":
            r = x[0].contiguous()
        elif op == "to":
            r = x[0].to(own(o))
        elif op == "bf16":
            r = x[0].to(torch.bfloat16).to(own(o))
        elif op == "permute":
            r = x[0].permute(*par)
        elif op == "getitem":
            r = x[0][_pykey(par)]
        elif op == "view":
            r = x[0].reshape(*par)
        elif op == "split":
            for oi, part in zip(outs, torch.split(x[0], par[0], par[1])):
                T[oi] = part
            continue
        elif op == "cat":
            r = torch.cat([t.to(x[0].dtype) for t in x], par)   # concat converts to the FIRST input's dtype
        elif op == "gemm":
            r = par * torch.matmul(x[0], x[1])
        elif op == "gemm_fused":
            r = par * torch.matmul(x[0], x[1])
            if x[2] is not None:
                r = r + x[2]
            if x[3] is not None:
                r = r * x[3]
            if x[4] is not None:
                r = r + x[4]
        elif op == "embedding":
            r = x[0][torch.from_numpy(consts[par])]
        elif op == "rms_norm":
            r = x[0] * torch.rsqrt((x[0] * x[0]).mean(-1, keepdim=True) + par)
            r = r * x[1] if x[1] is not None else r
        elif op == "layer_norm":
            r = F.layer_norm(x[0], x[0].shape[-1:], x[1], x[2], par)
        elif op == "silu":
            r = F.silu(x[0])
        elif op == "gelu":
            r = F.gelu(x[0], approximate=par)
        elif op in ("swiglu", "geglu"):
            gate, up = (x[0], x[1]) if x[1] is not None else x[0].chunk(2, -1)
            r = (F.silu(gate) if op == "swiglu" else F.gelu(gate, approximate=par)) * up
        elif op == "rope":
            R, inter, pos = par
            Bq, Hq, Sq, Dq = x[0].shape
            c, s = (torch.from_numpy(t).to(x[0].dtype) for t in rope_tables(16, R))
            p = torch.arange(Sq).repeat(Bq) if pos is None else torch.from_numpy(consts[pos])
            cc, ss = c[p].reshape(Bq, 1, Sq, R // 2), s[p].reshape(Bq, 1, Sq, R // 2)
            ia = torch.arange(0, R, 2) if inter else torch.arange(R // 2)
            ib = ia + 1 if inter else ia + R // 2
            xa, xb = x[0][..., ia], x[0][..., ib]
            r = x[0].clone()
            r[..., ia] = xa * cc - xb * ss
            r[..., ib] = xb * cc + xa * ss
        elif op == "cross_entropy":
            tgt, red, ign = par
            r = F.cross_entropy(x[0], torch.from_numpy(consts[tgt]), ignore_index=ign, reduction=red)
            r = r.reshape(1) if red != "none" else r
        elif op in ("attn", "attn_gqa"):
            g = x[0].shape[1] // x[1].shape[1]
            r = F.scaled_dot_product_attention(x[0], x[1].repeat_interleave(g, 1), x[2].repeat_interleave(g, 1), is_causal=True)
        elif op == "attn_qkv":
            Bq, Sq, Hq, kv = par
            Dq = x[0].shape[1] // (Hq + 2 * kv)
            q, k, v = torch.split(x[0], [Hq * Dq, kv * Dq, kv * Dq], 1)
            hd = lambda t, h: t.reshape(Bq, Sq, h, Dq).permute(0, 2, 1, 3)   # noqa: E731
            a = F.scaled_dot_product_attention(hd(q, Hq), hd(k, kv).repeat_interleave(Hq // kv, 1), hd(v, kv).repeat_interleave(Hq // kv, 1), is_causal=True)
            r = a.permute(0, 2, 1, 3).reshape(Bq * Sq, Hq * Dq)
        elif op in ("softmax", "log_softmax"):
            r = (torch.softmax if op == "softmax" else torch.log_softmax)(x[0] * par[1], par[0])
        elif op == "attention":
            r = _torch_attention(x[0], x[1], x[2], attn_vis(par, consts, x[0].shape[0], x[0].shape[2], x[1].shape[2]))
        elif op == "attention_qkv":
            Bq, Sq, Hq, kv, mask = par
            Dq = x[0].shape[1] // (Hq + 2 * kv)
            q, k, v = torch.split(x[0], [Hq * Dq, kv * Dq, kv * Dq], 1)
            hd = lambda t, h: t.reshape(Bq, Sq, h, Dq).permute(0, 2, 1, 3)   # noqa: E731
            a = _torch_attention(hd(q, Hq), hd(k, kv), hd(v, kv), attn_vis(mask, consts, Bq, Sq, Sq))
            r = a.permute(0, 2, 1, 3).reshape(Bq * Sq, Hq * Dq)
        elif op in ("rope_qkv", "qk_norm_rope"):
            Bq, Sq, Hq, kv, R, inter, pos = par[:7]
            Tq, Ht = Bq * Sq, Hq + 2 * kv
            x3 = x[0].reshape(Tq, Ht, -1)
            n = x3[:, :Hq + kv]
            if op == "qk_norm_rope":   # rstd = 1 / sqrt(mean x^2 + eps), n = x rstd w per q and k head; a missing weight is 1
                one = torch.ones(x3.shape[2], dtype=x3.dtype)
                w = torch.cat([(one if x[1] is None else x[1]).expand(Hq, -1), (one if x[2] is None else x[2]).expand(kv, -1)], 0)
                n = n * torch.rsqrt((n * n).mean(-1, keepdim=True) + par[7]) * w[None]
            if R:
                c, s = (torch.from_numpy(t).to(x3.dtype) for t in rope_tables(16, R))
                p = torch.arange(Tq) % Sq if pos is None else torch.from_numpy(consts[pos])
                cc, ss = c[p][:, None, :], s[p][:, None, :]
                ia = torch.arange(0, R, 2) if inter else torch.arange(R // 2)
                ib = ia + 1 if inter else ia + R // 2
                na, nb = n[..., ia], n[..., ib]
                n = n.clone()
                n[..., ia] = na * cc - nb * ss
                n[..., ib] = nb * cc + na * ss
            r = torch.cat([n, x3[:, Hq + kv:]], 1).reshape(Tq, -1)
        elif op == "expert_linear":
            Tq, E = x[0].shape[0], x[1].shape[0]
            so = _sanitized(host_offsets(par, consts, Tq), Tq)
            zero = lambda rows: torch.zeros(int(rows), x[1].shape[2], dtype=x[0].dtype)   # noqa: E731
            r = torch.cat([zero(so[0])] + [x[0][int(so[e]):int(so[e + 1])] @ x[1][e] for e in range(E)] + [zero(Tq - so[E])], 0)
        elif op in ("moe_dispatch", "moe_combine", "moe_gate"):
            from tests import moe_ref
            ids, E = consts[par[0]], par[1]
            k = ids.shape[1]
            offsets, row_pair, pair_row = moe_ref.plan(ids, E)
            if op == "moe_dispatch":
                r = x[0][torch.from_numpy(row_pair.astype(np.int64) // k)]
            elif op == "moe_combine":   # dropped pairs sort behind the live ones: rows offsets[E].. are never read
                pr = torch.from_numpy(pair_row.astype(np.int64).reshape(-1, k))
                terms = x[0][pr] if x[1] is None else x[1][..., None] * x[0][pr]
                r = torch.where((pr < int(offsets[E]))[..., None], terms, torch.zeros((), dtype=terms.dtype)).sum(1)
            else:
                ok = torch.from_numpy((ids >= 0) & (ids < E))
                r = torch.where(ok, x[0].gather(1, torch.from_numpy(np.where((ids >= 0) & (ids < E), ids, 0))), torch.zeros((), dtype=x[0].dtype))
                if par[2]:
                    r = r / r.sum(1, keepdim=True)
        else:
            raise AssertionError(op)
        if trace and r is x[0]:   # torch's contiguous() / to() of a tensor that needs neither: a node of its own for the trace
            r = r.clone()
        T[o] = r
    if trace:
        for i, t in T.items():
            if t.requires_grad and not t.is_leaf:
                t.retain_grad()
    root = T[prog["root"]]
    for gi, (base, how, perm) in enumerate(prog["grads"]):
        root.backward(_grad_view(torch.tensor(base, dtype=root.dtype), how, perm), retain_graph=gi + 1 < len(prog["grads"]))
    out = {"root": root.detach().contiguous().numpy(),
           "grads": {i: (None if T[i].grad is None else T[i].grad.numpy()) for i, _, req in prog["leaves"] if req}}
    if trace:
        out["values"] = {i: t.detach().numpy() for i, t in T.items()}
        out["node_grads"] = {i: t.grad.numpy() for i, t in T.items() if t.requires_grad and t.grad is not None}
    return out


def run_kfunca(mod, prog):
    """The program on the module under test. Returns what run_torch returns, plus "meta": {leaf node: (shape, dtype name)} of each gradient and
    "error": (instruction index or "backward", message) if the module raised."""
    T, consts = {}, prog["consts"]
    conv = {"f32": lambda t: t.float(), "f64": lambda t: t.double()}
    out = {"root": None, "grads": {}, "meta": {}, "error": None}
    up = lambda a: mod.from_numpy(np.ascontiguousarray(a), 0)   # noqa: E731
    plans = {}

    def plan_of(cidx, E):   # one plan per routing, shared by its gate, dispatch, expert product and combine as a layer shares it
        if (cidx, E) not in plans:
            plans[cidx, E] = mod.moe_plan(up(consts[cidx]), E)
        return plans[cidx, E]

    for i, arr, req in prog["leaves"]:
        T[i] = up(arr)
        if req:
            T[i].set_requires_grad(True)
    step = 0
    try:
        for step, (op, outs, ins, par) in enumerate(prog["instrs"]):
            x = [T[i] if i >= 0 else None for i in ins]
            o = outs[0]
            own = prog["nodes"][o][1]
            if op in ("add", "adds"):
                r = x[0] + (x[1] if op == "add" else par)
            elif op in ("sub", "subs"):
                r = x[0] - (x[1] if op == "sub" else par)
            elif op in ("mul", "muls"):
                r = x[0] * (x[1] if op == "mul" else par)
            elif op in ("div", "divs"):
                r = x[0] / (x[1] if op == "div" else par)
            elif op == "contiguous":
                r = x[0].contiguous()
            elif op == "to":
                r = conv[own](x[0])
            elif op == "bf16":
                r = conv[own](x[0].bfloat16())
            elif op == "permute":
                r = x[0].permute(*par)
            elif op == "getitem":
                r = x[0][_pykey(par)]
            elif op == "view":
                r = x[0].view(*par)
            elif op == "split":
                for oi, part in zip(outs, x[0].split(list(par[0]), par[1])):
                    T[oi] = part
                continue
            elif op == "cat":
                r = mod.cat(x, par)
            elif op == "gemm":
                r = mod.gemm(x[0], x[1], par, 0.0)
            elif op == "gemm_fused":
                r = mod.gemm_fused(x[0], x[1], par, bias=x[2], mul=x[3], add=x[4])
            elif op == "embedding":
                r = mod.embedding(x[0], up(consts[par]))
            elif op == "rms_norm":
                r = mod.rms_norm(x[0], x[1], par)
            elif op == "layer_norm":
                r = mod.layer_norm(x[0], x[1], x[2], par)
            elif op == "silu":
                r = mod.silu(x[0])
            elif op == "gelu":
                r = mod.gelu(x[0], approximate=par)
            elif op == "swiglu":
                r = mod.swiglu(x[0], x[1])
            elif op == "geglu":
                r = mod.geglu(x[0], x[1], approximate=par)
            elif op == "rope":
                R, inter, pos = par
                c, s = rope_tables(16, R)
                r = mod.rope(x[0], up(c), up(s), positions=None if pos is None else up(consts[pos]), interleaved=inter)
            elif op == "cross_entropy":
                tgt, red, ign = par
                r = mod.cross_entropy(x[0], up(consts[tgt]), ignore_index=ign, reduction=red)
            elif op == "attn":
                r = mod.causal_attention(x[0], x[1], x[2])
            elif op == "attn_gqa":
                r = mod.causal_attention_gqa(x[0], x[1], x[2])
            elif op == "attn_qkv":
                r = mod.causal_attention_qkv(x[0], par[0], par[1], par[2], kv_heads=par[3])
            elif op in ("softmax", "log_softmax"):
                r = getattr(mod, op)(x[0], dim=par[0], scale=par[1])
            elif op in ("attention", "attention_qkv"):
                fam, kv, pre, win, causal, doc = par if op == "attention" else par[4]
                S_ = x[0].sizes()[2] if op == "attention" else par[1]
                kw = dict(kv_len=None if kv is None else up(consts[kv]), causal=causal, prefix_len=None if pre is None else up(consts[pre]),
                          window=win, doc_mask=None if doc is None else mod.doc_mask(up(consts[doc]), S_))
                r = mod.attention(x[0], x[1], x[2], **kw) if op == "attention" else mod.attention_qkv(x[0], par[0], par[1], par[2], kv_heads=par[3], **kw)
            elif op in ("rope_qkv", "qk_norm_rope"):
                Bq, Sq, Hq, kv, R, inter, pos = par[:7]
                c, s = (up(t) for t in rope_tables(16, R)) if R else (None, None)
                posd = None if pos is None else up(consts[pos])
                if op == "rope_qkv":
                    r = mod.rope_qkv(x[0], c, s, Bq, Sq, Hq, kv_heads=kv, positions=posd, interleaved=inter)
                else:
                    r = mod.qk_norm_rope(x[0], x[1], x[2], c, s, Bq, Sq, Hq, kv_heads=kv, positions=posd, interleaved=inter, eps=par[7])
            elif op == "expert_linear":
                how, cidx, E = par
                off = plan_of(cidx, E).offsets if how == "plan" else (mod.segment_offsets(up(consts[cidx]), E) if how == "ids" else up(consts[cidx]))
                r = mod.expert_linear(x[0], x[1], off)
            elif op == "moe_dispatch":
                r = mod.moe_dispatch(x[0], plan_of(par[0], par[1]))
            elif op == "moe_combine":
                r = mod.moe_combine(x[0], plan_of(par[0], par[1]), gate=x[1])
            elif op == "moe_gate":
                r = mod.moe_gate(x[0], plan_of(par[0], par[1]), normalize=par[2])
            else:
                raise AssertionError(op)
            T[o] = r
        root = T[prog["root"]]
        step = "backward"
        for base, how, perm in prog["grads"]:
            root.backward(_grad_view(up(base), how, perm))
        out["root"] = root.contiguous().numpy()
        for i, _, req in prog["leaves"]:
            if not req:
                continue
            g = T[i].grad()
            if not g.defined():
                out["grads"][i] = None
                continue
            out["meta"][i] = (tuple(g.sizes()), str(g.dtype()).split(".")[-1])
            out["grads"][i] = g.contiguous().numpy()
    except (RuntimeError, ValueError, TypeError) as e:   # (the newer bindings raise the latter two: a refusal names its program all the same)
        out["error"] = (step, f"{type(e).__name__}: {e}" if not isinstance(e, RuntimeError) else str(e))
    return out


def describe(prog):
    """The program as text, for a failing assertion's message."""
    lines = [f"seed {prog['seed']} tier {prog['tier']} root {prog['root']} grads {[(g[0].shape, g[1], g[2]) for g in prog['grads']]}"]
    lines += [f"  leaf {i}: {a.shape} {a.dtype} requires={r}" for i, a, r in prog["leaves"]]
    lines += [f"  {outs} = {op}{ins} {par if not isinstance(par, np.ndarray) else ''}" for op, outs, ins, par in prog["instrs"]]
    return "\n".join(lines)


# ---- the committed sweep -----------------------------------------------------------------------------------------------------------
N_EXACT, N_SMOOTH = 200, 99          # 99 = 3 variants x (fed by a view | fan-in | a strided gradient) x the 11 smooth operators (smooth_case)
SEED_STRIDE = 1188000                # KF_FUZZ_SEED shifts both sweeps by this: a multiple of 99 and of 12, so seed % k keeps its meaning


N_EXACT2, N_SMOOTH2 = 90, 63         # the second blocks, behind the first ones: 10 x the 9 mixture-of-experts scenarios; 7 operators x 9 cases


def in_second_block(seed, tier):
    return seed % SEED_STRIDE >= (N_EXACT if tier == "exact" else N_SMOOTH)


def sweep(tier, shift=0, block=None):
    """The seeds of the sweep (block 1 or 2: of that block alone); every one of them yields a program (make_program raises otherwise):
    nothing is skipped."""
    n1, n2 = (N_EXACT, N_EXACT2) if tier == "exact" else (N_SMOOTH, N_SMOOTH2)
    lo, hi = {None: (0, n1 + n2), 1: (0, n1), 2: (n1, n1 + n2)}[block]
    return [shift * SEED_STRIDE + s for s in range(lo, hi)]


def compare_exact(prog, want, got):
    """The exact tier's verdict on one program: a list of findings (empty = the two engines agree bit for bit). The one normalisation: x + 0.0 on
    both sides, which turns -0 into +0 and changes nothing else - the sign of an exact zero SUM is the accumulator's start and the order of the
    terms (-0 + -0 = -0, +0 + -0 = +0), which two correct engines are free to choose."""
    bad = []
    if got["error"] is not None:
        return [f"raised at {got['error'][0]}: {got['error'][1]}"]
    names = {"f32": ("float", np.float32), "f64": ("double", np.float64)}
    if got["root"].shape != want["root"].shape or got["root"].dtype != want["root"].dtype:
        bad.append(f"root is {got['root'].shape} {got['root'].dtype}, torch's is {want['root'].shape} {want['root'].dtype}")
    elif not np.array_equal((got["root"] + 0.0).view(np.uint8), (want["root"] + 0.0).view(np.uint8)):
        bad.append("root value differs")
    for i, arr, req in prog["leaves"]:
        if not req:
            continue
        w, g = want["grads"][i], got["grads"][i]
        if w is None or g is None:
            if (w is None) != (g is None):
                bad.append(f"leaf {i}: gradient {'missing' if g is None else 'present'}, torch's is {'missing' if w is None else 'present'}")
            continue
        shape, dt = got["meta"][i]
        if shape != arr.shape or dt != names[prog["nodes"][i][1]][0]:
            bad.append(f"leaf {i} {arr.shape} {arr.dtype}: gradient is {shape} {dt}")
        elif not np.array_equal((g + 0.0).view(np.uint8), (w + 0.0).view(np.uint8)):
            bad.append(f"leaf {i}: gradient bits differ (max |diff| {np.abs(g.astype(np.float64) - w).max()})")
    return bad


def smooth_ratios(prog, t32, t64, got):
    """[(what, needed C, err, noise, floor)] for the root and every leaf gradient of a smooth program: the bound is
    |kfunca - torch64| <= C * max|torch32 - torch64| + 2^-23 * max|torch64| per tensor; needed C = (err - floor) / noise (0 when err <= floor)."""
    rows = []
    pairs = [("root", got["root"], t32["root"], t64["root"])]
    for i, arr, req in prog["leaves"]:
        if req:
            pairs.append((f"leaf {i}", got["grads"][i], t32["grads"][i], t64["grads"][i]))
    for what, g, a, b in pairs:
        if b is None or g is None:
            rows.append((what, 0.0 if (b is None) == (g is None) else float("inf"), 0.0, 0.0, 0.0))
            continue
        if g.shape != b.shape or g.dtype != np.float32:
            rows.append((what + f" shape {g.shape} {g.dtype}", float("inf"), 0.0, 0.0, 0.0))
            continue
        err = float(np.abs(g.astype(np.float64) - b).max()) if np.isfinite(g).all() else float("inf")
        noise, floor = float(np.abs(a.astype(np.float64) - b).max()), 2.0 ** -23 * float(np.abs(b).max())
        need = 0.0 if err <= floor else (float("inf") if noise == 0.0 else (err - floor) / noise)
        rows.append((what, need, err, noise, floor))
    return rows
