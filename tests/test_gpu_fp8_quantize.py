"""-m gpu: kf_fp8_amax and kf_fp8_quantize against tests/fp8_ref.py, bit for bit: amax, scale_inv, q and qt on all 65536 bf16 and f16 bit
patterns (with and without the NaN / infinity rows, both formats), f32 inputs on and beside every rounding boundary of both formats, ragged
shapes with pitched inputs and outputs, the zero pad of qt, and every byte of the output allocations that the entry does not own (the
pitch gaps and a guard band, poisoned beforehand with tests/poison.py)."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import fp8_ref as R
from tests import poison as P

pytestmark = pytest.mark.gpu

CODE = {"f32": H.F32, "f16": H.F16, "bf16": H.BF16}
GAP = {"f32": np.float32("nan"), "f16": np.float16("nan"), "bf16": np.uint16(0xFFFF)}   # what lies between the rows of a pitched x
FILL = 0xA5


def device_image(nbytes):
    buf = H.DevBuf(nbytes + P.GUARD)
    P.fill(buf.ptr, nbytes + P.GUARD, FILL)
    return buf


def run(x, dt, fmt, transpose=True, ld=None, ldq=None, ldqt=None, amax=None):
    """x: stored elements [rows, cols]. Returns (amax bits, scale_inv, the whole q allocation as [rows, ldq] + guard, the same for qt).
    amax: None for kf_fp8_amax's result, else the caller's bound (an f32), uploaded in its place."""
    rows, cols = x.shape
    rows16 = (rows + 15) // 16 * 16
    ld, ldq, ldqt = ld or cols, ldq or cols, ldqt or rows16
    host = np.full((rows, ld), GAP[dt], dtype=R.STORE[dt])
    host[:, :cols] = x
    bx = H.DevBuf.from_numpy(host)
    given, amax, sinv = amax, H.DevBuf(4), H.DevBuf(4)
    P.fill(amax.ptr, 4, 0xFF)
    P.fill(sinv.ptr, 4, 0xFF)
    nq, nqt = rows * ldq, cols * ldqt
    bq, bqt = device_image(nq), device_image(nqt) if transpose else None
    if given is None:
        H.fp8_amax(CODE[dt], rows, cols, ld, bx.ptr, amax.ptr)
    else:
        amax = H.DevBuf.from_numpy(np.array([given], dtype=np.float32))
    H.fp8_quantize(CODE[dt], fmt, rows, cols, ld, bx.ptr, amax.ptr, bq.ptr, ldq, sinv.ptr, bqt.ptr if transpose else None, ldqt if transpose else 0)
    H.device_sync()
    q_all = bq.to_numpy(nq + P.GUARD, np.uint8)
    qt_all = bqt.to_numpy(nqt + P.GUARD, np.uint8) if transpose else None
    return int(amax.to_numpy(1, np.uint32)[0]), sinv.to_numpy(1, np.float32)[0], q_all, qt_all


def expected_images(x, dt, fmt, ldq=None, ldqt=None, amax=None):
    rows, cols = x.shape
    q, qt, sinv, bits = R.quantize(R.to_f32(x, dt), fmt, amax)
    ldq, ldqt = ldq or cols, ldqt or qt.shape[1]
    q_all = np.full(rows * ldq + P.GUARD, FILL, dtype=np.uint8)
    q_all[:rows * ldq].reshape(rows, ldq)[:, :cols] = q
    qt_all = np.full(cols * ldqt + P.GUARD, FILL, dtype=np.uint8)
    qt_all[:cols * ldqt].reshape(cols, ldqt)[:, :qt.shape[1]] = qt
    return bits, sinv, q_all, qt_all


def check(x, dt, fmt, transpose=True, ld=None, ldq=None, ldqt=None, what="", amax=None):
    got = run(x, dt, fmt, transpose, ld, ldq, ldqt, amax)
    want = expected_images(x, dt, fmt, ldq, ldqt, amax)
    assert got[0] == want[0], f"{what}: amax bits {got[0]:#x}, expected {want[0]:#x}"
    assert got[1].view(np.uint32) == want[1].view(np.uint32), f"{what}: scale_inv {got[1]}, expected {want[1]}"
    bad = np.flatnonzero(got[2] != want[2])
    assert bad.size == 0, f"{what}: q differs at {bad.size} bytes, first at {bad[0]} (got {got[2][bad[0]]:#x}, expected {want[2][bad[0]]:#x})"
    if transpose:
        bad = np.flatnonzero(got[3] != want[3])
        assert bad.size == 0, f"{what}: qt differs at {bad.size} bytes, first at {bad[0]} (got {got[3][bad[0]]:#x}, expected {want[3][bad[0]]:#x})"
    return got


def all_patterns(dt, finite_only):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
    x = bits if dt == "bf16" else bits.view(np.float16)
    if finite_only:
        x = x[np.isfinite(R.to_f32(x, dt)).all(axis=1)]
        assert 240 <= x.shape[0] < 256
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("fmt", [R.E4M3, R.E5M2])
@pytest.mark.parametrize("finite_only", [True, False])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_16_bit_pattern(dt, finite_only, fmt):
    x = all_patterns(dt, finite_only)
    got = check(x, dt, fmt, what=f"{dt} patterns")
    if finite_only:
        assert got[1] != 1.0       # the largest finite value is far above both formats' maxima
    else:
        assert got[0] == 0x7fc00000 and got[1] == 1.0


@pytest.mark.parametrize("shift", [0, -7, 5])
@pytest.mark.parametrize("fmt", [R.E4M3, R.E5M2])
def test_f32_inputs_on_and_beside_every_rounding_boundary(fmt, shift):
    g = R.GRID[fmt].astype(np.float32)
    mid = ((R.GRID[fmt][:-1] + R.GRID[fmt][1:]) / 2).astype(np.float32)       # exact: one mantissa bit more than the format
    vals = np.concatenate([g, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)), [np.float32(R.FMT_MAX[fmt])]])
    vals = np.concatenate([vals, -vals]) * np.float32(2.0 ** shift)           # amax = fmt_max 2^shift: the scale is 2^-shift, exactly
    x = np.zeros((32, 48), dtype=np.float32)
    assert vals.size <= x.size
    x.ravel()[:vals.size] = vals
    got = check(x, "f32", fmt, what=f"boundaries, shift {shift}")
    assert got[1] == np.float32(2.0 ** shift)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("rows,cols", [(1, 16), (17, 48), (33, 130), (128, 16), (300, 257)])
def test_ragged_shapes_with_pitched_operands(rows, cols, dt, aligned):
    rng = np.random.default_rng(rows * 1000 + cols)
    x = R.round_to(rng.standard_normal((rows, cols)) * 3.0, dt)
    fmt = R.E4M3 if (rows + len(dt)) % 2 else R.E5M2
    rows16 = (rows + 15) // 16 * 16
    pitch = dict(ld=cols + 16, ldq=cols + 32, ldqt=rows16 + 16) if aligned else dict(ld=cols + 3, ldq=cols + 5, ldqt=rows16 + 7)
    first = check(x, dt, fmt, what=f"{rows}x{cols} {dt}", **pitch)
    again = run(x, dt, fmt, **pitch)
    assert first[0] == again[0] and np.array_equal(first[2], again[2]) and np.array_equal(first[3], again[3])     # two runs, the same bits
    rows_of_qt = first[3][:cols * pitch["ldqt"]].reshape(cols, pitch["ldqt"])
    assert not rows_of_qt[:, rows:rows16].any()                                                                      # the zero pad
    check(x, dt, fmt, transpose=False, ld=pitch["ld"], ldq=pitch["ldq"], what=f"{rows}x{cols} {dt} without qt")


@pytest.mark.parametrize("fmt", [R.E4M3, R.E5M2])
def test_an_all_zero_input_gives_scale_one(fmt):
    got = check(np.zeros((20, 32), dtype=np.uint16), "bf16", fmt, what="zeros")
    assert got[0] == 0 and got[1] == 1.0 and not got[2][:20 * 32].any()


def test_empty_matrices():
    amax, sinv = H.DevBuf(4), H.DevBuf(4)
    P.fill(amax.ptr, 4, 0xFF)
    P.fill(sinv.ptr, 4, 0xFF)
    x, q = H.DevBuf(64), device_image(64)
    for rows, cols in ((0, 16), (4, 0)):
        H.fp8_amax(H.BF16, rows, cols, 16, x.ptr, amax.ptr)
        H.fp8_quantize(H.BF16, H.FP8_E4M3, rows, cols, 16, x.ptr, amax.ptr, q.ptr, 16, sinv.ptr, q.ptr, 16)
        H.device_sync()
        assert amax.to_numpy(1, np.uint32)[0] == 0 and sinv.to_numpy(1, np.float32)[0] == 1.0
        assert (q.to_numpy(64 + P.GUARD, np.uint8) == FILL).all()
