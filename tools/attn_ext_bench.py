#!/usr/bin/env python3
"""Attention with score modifiers (kf_attn_ext_fwd / kf_attn_ext_bwd) through the C ABI, bf16: median HIP-event times of forward and
backward beside THE SAME MASK WITHOUT MODIFIERS ON THE SAME TENSORS, and the time of the dsink kernel.

Cases (S 4096):
  gemma2 window   window (4095, 0), softcap 50, D 128, GQA 32/8      Gemma-2's sliding-window layers
  gemma2 causal   full causal,      softcap 50, D 128, GQA 32/8      its global layers
  gpt-oss window  window (127, 0),  sinks,      D 64,  GQA 64/8      gpt-oss's sliding-window layers
For each case the four calls - modified forward, plain forward, modified backward, plain backward - run interleaved in one loop of
--iters after --warmup, in an order that rotates by one every iteration (no call always follows the same neighbour); each backward
reads the o and lse of its own forward. Reported: the medians, the ratio modified / plain per direction (time_ratio), and the mean time
of attn_sink_grad from the library's own per-kernel profile in a separate pass (a sink case only).
--check compares sampled K/V heads of the modified call with the float64 reference (tests/attn_ext_ref.py) under the project's bounds,
dsink among them (recomputed for the sample's batch alone is not possible - dsink sums over the batch - so dsink is checked on a
smaller call of the same kind). Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

# (name, B, Hq, Hkv, S, D, (left, right) with None = unbounded, softcap, sinks)
CASES = [
    ("gemma2 window 4095 cap 50 D128", 2, 32, 8, 4096, 128, (4095, 0), 50.0, False),
    ("gemma2 causal cap 50 D128", 2, 32, 8, 4096, 128, (None, 0), 50.0, False),
    ("gpt-oss window 127 sinks D64", 2, 64, 8, 4096, 64, (127, 0), 0.0, True),
]


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def draw(rng, B, Hq, Hkv, S, D):
    base = O.f32_to_bf16(rng.uniform(-1, 1, (B * Hq * S * D + 4096,)).astype(np.float32))
    take = lambda off, shp: np.ascontiguousarray(base[off:off + int(np.prod(shp))].reshape(shp))  # noqa: E731  (four windows of one draw)
    return take(0, (B, Hq, S, D)), take(2048, (B, Hkv, S, D)), take(3072, (B, Hkv, S, D)), take(1024, (B, Hq, S, D))


class Call:
    """the device buffers of one problem and its modified / plain calls"""

    def __init__(self, q, k, v, go, window, softcap, sink):
        self.code, (self.B, self.Hq, self.S, self.D), self.Hkv = H.BF16, q.shape, k.shape[1]
        B, Hq, S, D, Hkv = self.B, self.Hq, self.S, self.D, self.Hkv
        scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
        self.keep = [H.DevBuf.from_numpy(x) for x in (q, k, v, go)]
        bq, bk, bv, bgo = self.keep
        self.bsink = None if sink is None else H.DevBuf.from_numpy(sink)
        self.o, self.lse, self.o2, self.lse2 = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S)
        self.dq, self.dk, self.dv, self.ds = H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes), H.DevBuf(4 * Hq)
        need = H.attn_ext_bwd_workspace_bytes(self.code, B, Hq, Hkv, S, S, D)
        self.ws = H.DevBuf(need)
        wl, wr = (-1 if x is None else x for x in window)
        mask = H.attn_mask(H.ATTN_MASK_WINDOW, window_left=wl, window_right=wr)
        dims = (self.code, B, Hq, Hkv, S, S, D, scale, bq.ptr, bk.ptr, bv.ptr)
        sp = None if self.bsink is None else self.bsink.ptr
        grads = (bgo.ptr, self.dq.ptr, self.dk.ptr, self.dv.ptr, self.ws.ptr, need)
        self.ext_fwd = lambda: H.attn_ext_fwd(*dims, self.o.ptr, self.lse.ptr, mask=mask, softcap=softcap, sink=sp)
        self.ext_bwd = lambda: H.attn_ext_bwd(*dims, self.o.ptr, self.lse.ptr, *grads, mask=mask, softcap=softcap, sink=sp, dsink=None if sp is None else self.ds.ptr)
        self.plain_fwd = lambda: H.attn_ext_fwd(*dims, self.o2.ptr, self.lse2.ptr, mask=mask)
        self.plain_bwd = lambda: H.attn_ext_bwd(*dims, self.o2.ptr, self.lse2.ptr, *grads, mask=mask)

    def results(self, q, k):
        H.device_sync()
        B, Hq, S = self.B, self.Hq, self.S
        return (self.o.to_numpy(q.shape, q.dtype), self.lse.to_numpy((B, Hq, S), np.float32), self.dq.to_numpy(q.shape, q.dtype),
                self.dk.to_numpy(k.shape, k.dtype), self.dv.to_numpy(k.shape, k.dtype), self.ds.to_numpy((Hq,), np.float32))


def check(name, window, softcap, sink, q, k, v, go, got):
    """sampled groups of the timed call (o, lse, dq, dk, dv), then dsink on a smaller call of the same kind"""
    from oracle import checks as K
    from tests.attn_ext_ref import attn_ref64_ext, check_lse_ext
    from tests.attn_full_ref import format_floor_vis
    from tests.attn_window_ref import window_vis
    code = H.BF16
    B, Hq, S, _ = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    o, lse, dq, dk, dv, _ = got
    for b, j in ((1 % B, 0), (B - 1, Hkv - 1)):
        hs, js = slice(j * G, (j + 1) * G), slice(j, j + 1)
        sl = lambda x, s: x[b:b + 1, s]  # noqa: E731
        vis = window_vis(None, window[0], window[1], S, S, 1)
        ops = (sl(q, hs), sl(k, js), sl(v, js), sl(go, hs))
        sk = None if sink is None else sink[hs]
        ref, fl = attn_ref64_ext(*ops, vis, code, softcap=softcap, sink=sk), format_floor_vis(*ops, vis, code)
        for nm, g in (("o", sl(o, hs)), ("dq", sl(dq, hs)), ("dk", sl(dk, js)), ("dv", sl(dv, js))):
            K.check_one(nm, g, ref, code, f"{name} b{b} kv-head {j}", floor=fl.get(nm))
        check_lse_ext(sl(lse, hs), ref, softcap, sk, name)
    if sink is not None:
        Bs, Ss = 2, 512
        qs, ks, vs, gs = (np.ascontiguousarray(x[:Bs, :, :Ss]) for x in (q, k, v, go))
        small = Call(qs, ks, vs, gs, window, softcap, sink)
        small.ext_fwd()
        small.ext_bwd()
        ref = attn_ref64_ext(qs, ks, vs, gs, window_vis(None, window[0], window[1], Ss, Ss, Bs), code, softcap=softcap, sink=sink)
        d = np.abs(small.results(qs, ks)[5].astype(np.float64) - ref["dsink"])
        assert (d <= ref["dsink_bound"]).all(), f"{name} dsink: worst error / bound {np.max(d / ref['dsink_bound']):.3f}"
        return float(np.max(d / ref["dsink_bound"]))
    return None


def run_case(case, args):
    name, B, Hq, Hkv, S, D, window, softcap, with_sink = case
    rng = np.random.default_rng(len(name))
    q, k, v, go = draw(rng, B, Hq, Hkv, S, D)
    sink = rng.uniform(-1.0, 3.0, Hq).astype(np.float32) if with_sink else None
    c = Call(q, k, v, go, window, softcap, sink)
    timed = [("ext_fwd", c.ext_fwd), ("ext_bwd", c.ext_bwd), ("plain_fwd", c.plain_fwd), ("plain_bwd", c.plain_bwd)]
    t = {n: [] for n, _ in timed}
    for n, fn in timed:     # each backward needs its forward's o and lse once before the rotation starts
        fn()
    for it in range(args.warmup + args.iters):
        r = it % len(timed)
        for n, fn in timed[r:] + timed[:r]:
            ms = event_ms(fn)
            if it >= args.warmup:
                t[n].append(ms)
    med = {n: statistics.median(x) for n, x in t.items()}
    out = {"case": name, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "D": D, "window": [-1 if x is None else x for x in window], "softcap": softcap,
           "sinks": with_sink}
    out.update({f"{n}_ms": round(m, 4) for n, m in med.items()})
    out["fwd_time_ratio"] = round(med["ext_fwd"] / med["plain_fwd"], 3)
    out["bwd_time_ratio"] = round(med["ext_bwd"] / med["plain_bwd"], 3)
    if with_sink:
        H.profile_reset()
        H.profile_enable(True)
        try:
            for _ in range(args.iters):
                c.ext_bwd()
        finally:
            H.profile_enable(False)
        ms, cnt = H.profile_results()["attn_sink_grad"]
        out["sink_grad_ms"] = round(ms / cnt, 4)
    if args.check:
        c.ext_fwd()
        c.ext_bwd()
        worst = check(name, window, softcap, sink, q, k, v, go, c.results(q, k))
        out["check"] = "ok"
        if worst is not None:
            out["dsink_error_over_bound"] = round(worst, 4)
    print(f"[attn_ext_bench] {name}: fwd {out['fwd_time_ratio']}x, bwd {out['bwd_time_ratio']}x of the same mask without modifiers", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--json")
    args = ap.parse_args()
    H.set_device(0)
    cases = [c for c in CASES if not args.cases or c[0] in args.cases.split(",")]
    props = H.device_props(0)
    import bench
    res = {"tool": "attn_ext_bench", "device": props.name.decode(), "dtype": "bf16", "iters": args.iters, "results": [run_case(c, args) for c in cases]}
    res.update(bench.stamp(("attn_ext.hip", "attn_full.hip", "attn_full_kernels.h", "common.h", "runtime.hip")))   # the sources every column comes from
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
