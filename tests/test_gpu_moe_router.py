"""-m gpu: the fused mixture-of-experts router (kf_moe_router_fwd / kf_moe_router_bwd) and the auxiliary losses (kf_moe_aux_loss_fwd /
kf_moe_aux_loss_bwd) against tests/moe_router_ref.py, on the shapes, draws and bounds that file holds (tests/test_moe_router_ref.py
shows on the CPU that an f32 evaluation meets those bounds there and that wrong formulas do not).

Selection is exact: ids equal the numpy key reference and this library's own logits.topk(k)[1] on every draw, non-finite rows included.
Gates and dlogits are held to the bounds on the rows without non-finite values; on the other rows the NaN pattern must be the
reference's. Outputs live in buffers filled with a poison byte (tests/poison.py's patterns): every element inside the extents is
written, nothing outside them is. Every call is made twice into fresh buffers: the same bits."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import moe_router_ref as R
from tests import poison as P

pytestmark = pytest.mark.gpu

CODE_IDS = [R.CODE_NAME[c] for c in R.CODES]
NAN_BITS = {R.BF16: 0x7FC1, R.F16: 0x7E01, R.F32: 0x7FC00001}


class Rows:
    """[T, cols] of an unsigned type at leading dimension ld, `off` elements into a device buffer with 64 elements behind it. Everything
    outside the window holds `fill` before the call and must hold it afterwards."""

    def __init__(self, T, cols, utype, ld=None, off=0, fill=0):
        self.T, self.cols, self.ld, self.off, self.utype = T, cols, cols if ld is None else ld, off, np.dtype(utype)
        self.img = np.full(off + T * self.ld + 64, fill, dtype=self.utype)
        self.idx = off + np.arange(T)[:, None] * self.ld + np.arange(cols)[None, :]
        self.buf = None

    def put(self, b=None):
        if b is not None:
            self.img[self.idx] = b
        self.buf = H.DevBuf.from_numpy(self.img)
        return self

    @property
    def ptr(self):
        return self.buf.ptr + self.off * self.utype.itemsize

    def get(self):
        after = self.buf.to_numpy(self.img.shape, self.utype)
        mask = np.ones(after.shape, bool)
        mask[self.idx] = False
        assert np.array_equal(after[mask], self.img[mask]), "elements outside the window were written"
        return after[self.idx]


def poison_of(utype, byte):
    return np.frombuffer(bytes([byte]) * np.dtype(utype).itemsize, dtype=utype)[0]


def run_router(code, b, k, score, normalize, dgb, pad=0, off=0, byte=0xFF):
    """(ids, gate bits, dlogits bits) of one forward and one backward. pad: extra elements of every leading dimension (the logits' padding
    holds NaNs, the outputs' the poison byte); off: elements in front of the logits and of dlogits (an odd base takes the element path)."""
    T, E = b.shape
    ut = R.UINT[code]
    lg = Rows(T, E, ut, E + pad, off, NAN_BITS[code]).put(b)
    ids = Rows(T, k, np.int64, fill=poison_of(np.int64, byte)).put()
    gate = Rows(T, k, ut, k + pad, 0, poison_of(ut, byte)).put()
    H.moe_router_fwd(code, T, E, k, score, normalize, lg.ptr, lg.ld, ids.ptr, gate.ptr, gate.ld)
    dg = Rows(T, k, ut, k + pad, 0, NAN_BITS[code]).put(dgb)
    dl = Rows(T, E, ut, E + pad, off, poison_of(ut, byte)).put()
    H.moe_router_bwd(code, T, E, k, score, normalize, lg.ptr, lg.ld, ids.ptr, dg.ptr, dg.ld, dl.ptr, dl.ld)
    H.device_sync()
    return ids.get(), gate.get(), dl.get()


def device_topk(code, b, k):
    """logits.topk(k)[1] of this library: the stable segmented sort of every row."""
    if code == R.BF16:
        t = kfunca.from_numpy_bf16(np.ascontiguousarray(b), 0)
    else:
        t = kfunca.from_numpy(np.ascontiguousarray(b).view(np.float16 if code == R.F16 else np.float32), 0)
    return t.topk(k, -1, True)[1].numpy().astype(np.int64)


def case(code, T, E, k, draw):
    rng = np.random.default_rng(R.seed_of(T, E, k, code, draw))
    return R.draw_logits(rng, draw, code, T, E), R.draw_dgate(rng, code, T, k)


def check_router(code, b, dgb, k, ids, gate_bits, dl_bits, score, normalize, what):
    T, E = b.shape
    x, dg = R.floats(b, code), R.floats(dgb, code)
    fin = R.finite_rows(b, code)
    ref = R.gate(x, ids, score, normalize)
    got = R.floats(gate_bits, code)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "gate NaN pattern")
    err, bound = np.abs(got - ref)[fin], R.gate_bound(code, ref)[fin]
    print(f"{what}: gate worst err / bound {float((err / bound).max()) if err.size else 0.0:.3f}")
    assert (err <= bound).all(), (what, "gate", float((err / bound).max()))
    ref = R.router_backward(x, ids, dg, score, normalize)
    got = R.floats(dl_bits, code)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "dlogits NaN pattern")
    err, bound = np.abs(got - ref)[fin], R.router_backward_bound(code, E, k, dg, ref)[fin]
    print(f"{what}: dlogits worst err / bound {float((err / bound).max()) if err.size else 0.0:.3f}")
    assert (err <= bound).all(), (what, "dlogits", float((err / bound).max()))


@pytest.mark.parametrize("code", R.CODES, ids=CODE_IDS)
@pytest.mark.parametrize("T,E,k", R.ROUTER_SHAPES)
def test_router_selection_is_exact_and_gates_and_gradients_meet_the_bounds(code, T, E, k):
    for draw in R.DRAWS:
        b, dgb = case(code, T, E, k, draw)
        want = R.select(b, code, k)
        assert np.array_equal(device_topk(code, b, k), want), (draw, "topk")
        if draw == "equal":
            assert np.array_equal(want, np.tile(np.arange(k), (T, 1)))
        for score in R.SCORES:
            for normalize in (False, True):
                what = f"{R.CODE_NAME[code]} T{T} E{E} k{k} {draw} {R.SCORE_NAME[score]} normalize={normalize}"
                ids, gate, dl = run_router(code, b, k, score, normalize, dgb)
                assert np.array_equal(ids, want), (what, "ids")
                check_router(code, b, dgb, k, ids, gate, dl, score, normalize, what)
                again = run_router(code, b, k, score, normalize, dgb, byte=0x7F)
                assert all(np.array_equal(u, v) for u, v in zip((ids, gate, dl), again)), (what, "second run")


@pytest.mark.parametrize("code", R.CODES, ids=CODE_IDS)
@pytest.mark.parametrize("T,E,k", [(5, 8, 2), (5, 64, 64), (257, 128, 8), (4, 65, 6), (5, 1000, 6), (3, 1024, 64)])
def test_pitched_rows_and_the_element_path_give_the_packed_path_s_bits(code, T, E, k):
    """ldl > E with NaN in the padding, pitched outputs with poisoned padding, and a base one element off (so no row is 16-byte aligned)."""
    for draw in ("normal", "ties"):
        b, dgb = case(code, T, E, k, draw)
        for score in R.SCORES:
            for normalize in (False, True):
                packed = run_router(code, b, k, score, normalize, dgb)
                pad = 16 // R.ES[code]                                  # whole packs: still the 16-byte path where E allows it
                for kw in (dict(pad=pad), dict(pad=3), dict(off=1), dict(pad=pad, off=1, byte=0x7F)):
                    got = run_router(code, b, k, score, normalize, dgb, **kw)
                    assert all(np.array_equal(u, v) for u, v in zip(packed, got)), (draw, score, normalize, kw)


def test_an_id_outside_the_experts_contributes_nothing_and_reads_nothing():
    code, T, E, k = R.BF16, 5, 128, 8
    b, dgb = case(code, T, E, k, "normal")
    ids = R.select(b, code, k)
    ids[1, 2], ids[3, 0], ids[4, 7] = E, -1, 1 << 40
    ut = R.UINT[code]
    for score in R.SCORES:
        for normalize in (False, True):
            lg = Rows(T, E, ut).put(b)
            d_ids = H.DevBuf.from_numpy(ids)
            dg = Rows(T, k, ut).put(dgb)
            dl = Rows(T, E, ut, fill=poison_of(ut, 0xFF)).put()
            H.moe_router_bwd(code, T, E, k, score, normalize, lg.ptr, E, d_ids.ptr, dg.ptr, k, dl.ptr, E)
            H.device_sync()
            x, g = R.floats(b, code), R.floats(dgb, code)
            ref = R.router_backward(x, ids, g, score, normalize)
            err = np.abs(R.floats(dl.get(), code) - ref)
            assert (err <= R.router_backward_bound(code, E, k, g, ref)).all(), (score, normalize)


# ---- the auxiliary losses -----------------------------------------------------------------------------------------------------------
def device_offsets(ids, E):
    """offsets [E + 1] of a real kf_moe_plan, left on the device."""
    T, k = ids.shape
    d_ids = H.DevBuf.from_numpy(ids)
    off, rp, pr = H.DevBuf(8 * (E + 1)), H.DevBuf(4 * T * k), H.DevBuf(4 * T * k)
    need = H.moe_plan_workspace_bytes(T, k, E)
    ws = H.DevBuf(need)
    H.moe_plan(d_ids.ptr, T, k, E, off.ptr, rp.ptr, pr.ptr, ws.ptr if need else None, need)
    H.device_sync()
    return off


def run_aux(code, b, off, k, bc, zc, dloss, byte, pad=0, base=0, parts=True):
    T, E = b.shape
    ut = R.UINT[code]
    lg = Rows(T, E, ut, E + pad, base, NAN_BITS[code]).put(b)
    need = H.moe_aux_loss_workspace_bytes(T, E)
    ws = H.DevBuf(need)
    P.fill(ws.ptr, need, byte)                                          # the workspace needs no initialisation
    out = Rows(1, 3, np.uint32, fill=poison_of(np.uint32, byte)).put()  # loss, then the two parts
    H.moe_aux_loss_fwd(code, T, E, k, lg.ptr, lg.ld, off.ptr, bc, zc, out.ptr, out.ptr + 4 if parts else None, ws.ptr, need)
    d_dloss = H.DevBuf.from_numpy(np.array([dloss], np.float32))
    dl = Rows(T, E, ut, E + pad, base, poison_of(ut, byte)).put()
    H.moe_aux_loss_bwd(code, T, E, k, lg.ptr, lg.ld, off.ptr, bc, zc, d_dloss.ptr, dl.ptr, dl.ld)
    H.device_sync()
    return out.get().view(np.float32)[0], dl.get()


@pytest.mark.parametrize("code", R.CODES, ids=CODE_IDS)
@pytest.mark.parametrize("T,E,k,plan", R.AUX_SHAPES)
def test_aux_loss_and_its_gradient_meet_the_bounds(code, T, E, k, plan):
    for draw in ("normal", "ties"):
        rng = np.random.default_rng(R.seed_of(T, E, k, code, plan, draw))
        b = R.draw_logits(rng, draw, code, T, E)
        ids = R.draw_plan_ids(rng, T, E, k, plan)
        counts = R.counts_of(ids, E)
        off = device_offsets(ids, E)
        assert np.array_equal(np.diff(off.to_numpy(E + 1, np.int64)), counts)
        x = R.floats(b, code)
        for bc, zc in R.AUX_COEFS:
            what = f"{R.CODE_NAME[code]} T{T} E{E} k{k} {plan} {draw} bc={bc} zc={zc}"
            want = R.aux_forward(x, counts, k, bc, zc)
            got, dl = run_aux(code, b, off, k, bc, zc, R.AUX_DLOSS, 0xFF)
            for name, g, r in zip(("loss", "L_bal", "L_z"), got, want):
                print(f"{what}: {name} {g:.9g} ref {r:.9g} err / bound {abs(g - r) / R.loss_bound(r) if r else 0.0:.3f}")
                assert abs(float(g) - r) <= R.loss_bound(r), (what, name, g, r)
            ref = R.aux_backward(x, counts, k, bc, zc, R.AUX_DLOSS)
            err, bound = np.abs(R.floats(dl, code) - ref), R.aux_backward_bound(code, x, counts, k, bc, zc, R.AUX_DLOSS, ref)
            print(f"{what}: dlogits worst err / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (what, "dlogits", float((err / bound).max()))
            # another poison in the workspace and the outputs, pitched rows off an odd base, no parts: the same bits
            got2, dl2 = run_aux(code, b, off, k, bc, zc, R.AUX_DLOSS, 0x7F, pad=3, base=1, parts=False)
            assert got2[0].tobytes() == got[0].tobytes() and np.array_equal(dl2, dl), what
            assert got2[1:].tobytes() == np.full(2, poison_of(np.uint32, 0x7F)).tobytes(), "parts == NULL wrote them"


# ---- the operators ------------------------------------------------------------------------------------------------------------------
def to_tensor(code, b, requires_grad=False):
    if code == R.BF16:
        t = kfunca.from_numpy_bf16(np.ascontiguousarray(b), 0)
    else:
        t = kfunca.from_numpy(np.ascontiguousarray(b).view(np.float16 if code == R.F16 else np.float32), 0)
    t.set_requires_grad(requires_grad)
    return t


def tensor_bits(code, t):
    return np.ascontiguousarray(t.numpy()).view(R.UINT[code])


@pytest.mark.parametrize("code", R.CODES, ids=CODE_IDS)
def test_operators_give_the_entries_bits(code):
    T, E, k = 37, 128, 8
    b, dgb = case(code, T, E, k, "normal")
    for score in R.SCORES:
        for normalize in (False, True):
            logits = to_tensor(code, b, True)
            ids, gate = kfunca.moe_route(logits, k, score=R.SCORE_NAME[score], normalize=normalize)
            want = run_router(code, b, k, score, normalize, dgb)
            assert np.array_equal(ids.numpy(), want[0]) and np.array_equal(tensor_bits(code, gate), want[1])
            assert not ids.requires_grad() and gate.requires_grad()
            gate.backward(to_tensor(code, dgb))
            assert np.array_equal(tensor_bits(code, logits.grad()), want[2]), (score, normalize)
    # the aux loss through the engine, its gradient read from the device
    logits = to_tensor(code, b, True)
    ids, gate = kfunca.moe_route(logits, k)
    plan = kfunca.moe_plan(ids, E)
    loss, parts = kfunca.moe_aux_loss(logits, plan, balance_coef=1e-2, z_coef=1e-3, return_parts=True)
    x, counts = R.floats(b, code), R.counts_of(ids.numpy(), E)
    ref = R.aux_forward(x, counts, k, 1e-2, 1e-3)
    got = (float(loss.numpy()[0]),) + tuple(float(v) for v in parts.numpy())
    assert all(abs(g - r) <= R.loss_bound(r) for g, r in zip(got, ref)), (got, ref)
    assert kfunca.moe_aux_loss(logits, plan, z_coef=1e-3).numpy().shape == (1,)
    loss.backward(kfunca.from_numpy(np.full(1, R.AUX_DLOSS, np.float32), 0))
    ref = R.aux_backward(x, counts, k, 1e-2, 1e-3, R.AUX_DLOSS)
    err = np.abs(R.floats(tensor_bits(code, logits.grad()), code) - ref)
    assert (err <= R.aux_backward_bound(code, x, counts, k, 1e-2, 1e-3, R.AUX_DLOSS, ref)).all()


def test_operator_errors_name_the_operator():
    t = kfunca.from_numpy(np.zeros((4, 8), np.float32), 0)
    for bad, msg in ((lambda: kfunca.moe_route(t, 0), "moe_route"), (lambda: kfunca.moe_route(t, 9), "moe_route"),
                     (lambda: kfunca.moe_route(t, 2, score="tanh"), "moe_route"),
                     (lambda: kfunca.moe_route(kfunca.from_numpy(np.zeros((4, 1025), np.float32), 0), 2), "moe_route"),
                     (lambda: kfunca.moe_aux_loss(t, None), "moe_aux_loss")):
        with pytest.raises(Exception, match=msg):
            bad()
    ids, _ = kfunca.moe_route(t, 2)
    with pytest.raises(Exception, match="moe_aux_loss"):
        kfunca.moe_aux_loss(kfunca.from_numpy(np.zeros((5, 8), np.float32), 0), kfunca.moe_plan(ids, 8))
