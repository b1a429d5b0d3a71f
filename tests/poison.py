"""Poisoned device allocations for the -m gpu tests: what a kernel reads before anything wrote it.

A fresh kf_malloc block holds whatever the driver hands out - very often zero pages, never an adversarial pattern - while the product
runs on a caching allocator whose blocks still hold the previous tensor's bytes. poisoned_allocations() patches H.DevBuf.__init__ for
the rest of ONE test (pytest's monkeypatch fixture undoes it) so that every new allocation - scratch, pure outputs, the ones the
H.norm_bwd / H.ce_fwd / H.index_add / H.sort_segments helpers make internally - is filled with one byte before it is returned.
DevBuf.from_numpy goes through __init__ and then overwrites the block, so inputs hold what the test uploads.

The patterns, and why these three:
  0x00  the baseline, zero-filled EXPLICITLY (kf_memset_zero): the run the others are compared with must not depend on what kf_malloc
        returns.
  0xFF  NaN in f16 / bf16 / f32 / f64, -1 in every integer and counter. An int64 index of -1 wraps to a valid row: the nastiest case
        for index scratch.
  0x7F  f32 and bf16 0x7f7f... ~ 3.4e38, finite: a NaN can be swallowed by v_max / v_min and by compare-selects, a huge finite value
        cannot. (f16 0x7f7f is a NaN again.)

Nothing here touches the GPU at import.
"""
import numpy as np

from kfunca_amd import hip_abi as H

PATTERNS = (0x00, 0xFF, 0x7F)
GUARD = 4096                     # bytes of guard band behind a buffer a test allocates itself (guarded / guard_intact)
_CHUNK = 1 << 24
_ORIG_INIT = H.DevBuf.__init__   # the unpatched constructor: patches never stack
_host = {}


def fill(ptr, nbytes, byte):
    """Fill nbytes of device memory at ptr with `byte`: 0 by the library's device fill, anything else from a cached host array."""
    if nbytes <= 0:
        return
    if byte == 0:
        H.check(H.lib().kf_memset_zero(ptr, nbytes, None))
        H.device_sync()
        return
    src = _host.get(byte)
    if src is None:
        src = _host[byte] = np.full(_CHUNK, byte, dtype=np.uint8)
    for off in range(0, nbytes, _CHUNK):
        H.check(H.lib().kf_memcpy_h2d(ptr + off, src.ctypes.data, min(_CHUNK, nbytes - off), None))


class Poison:
    """What poisoned_allocations returns: the byte in force, and how many allocations / bytes it has filled (a test can assert that
    the helper it relies on really allocated under the patch)."""

    def __init__(self, byte):
        self.byte, self.allocations, self.nbytes = int(byte), 0, 0


def poisoned_allocations(monkeypatch, byte):
    """From here to the end of the calling test (or the next call), every H.DevBuf(n) comes back filled with `byte`."""
    assert 0 <= byte <= 0xFF
    state = Poison(byte)

    def init(self, nbytes):
        _ORIG_INIT(self, nbytes)
        fill(self.ptr, self.nbytes, state.byte)
        state.allocations += 1
        state.nbytes += self.nbytes

    monkeypatch.setattr(H.DevBuf, "__init__", init)
    return state


def guarded(nbytes, guard=GUARD):
    """A buffer of nbytes with a guard band behind it. Under the patch the whole block holds the pattern; guard_intact checks the band."""
    return H.DevBuf(nbytes + guard)


def guard_intact(buf, nbytes, byte, guard=GUARD):
    tail = np.empty(guard, dtype=np.uint8)
    H.check(H.lib().kf_memcpy_d2h(tail.ctypes.data, buf.ptr + nbytes, guard, None))
    return bool((tail == byte).all())
