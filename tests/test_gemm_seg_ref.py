"""CPU-only: the numpy reference of the segmented GEMM (tests/gemm_seg_ref.py) against a plain per-row loop, the offset sanitising on
malformed inputs, and the mirror of the kernels' row-tile map: every row of [0, T) in exactly one tile, no tile across a segment boundary,
never more tiles than the host-known bound T / 128 + E + 2 the grids are launched on."""
import itertools

import numpy as np
import pytest

from tests import gemm_seg_ref as R


def test_sanitize():
    assert R.sanitize([0, 300, 100, 9999], 400).tolist() == [0, 300, 300, 400]
    assert R.sanitize([-7, -2, 5], 4).tolist() == [0, 0, 4]
    assert R.sanitize([37, 165, 165, 390], 400).tolist() == [37, 165, 165, 390]
    assert R.sanitize([500, 0], 400).tolist() == [400, 400]
    assert R.sanitize([3], 0).tolist() == [0]


def test_segment_offsets():
    assert R.segment_offsets([0, 0, 2, 2, 2, 5], 6).tolist() == [0, 2, 2, 5, 5, 5, 6]
    assert R.segment_offsets([-4, -1, 0, 1, 1, 3, 7, 9], 3).tolist() == [2, 3, 5, 5]   # ids < 0 and >= E lie outside [offsets[0], offsets[E])
    assert R.segment_offsets([], 4).tolist() == [0, 0, 0, 0, 0]
    assert R.segment_offsets([0, 0, 0], 1).tolist() == [0, 3]


@pytest.mark.parametrize("offsets,T", [([0, 1, 129, 129, 300], 300), ([37, 165, 165, 390], 400), ([0, 300, 100, 9999], 400), ([0, 0, 70, 200, 200, 200], 200)])
def test_products_against_a_per_row_loop(offsets, T):
    rng = np.random.default_rng(T + len(offsets))
    E, K, N = len(offsets) - 1, 7, 5
    a, w, c0 = rng.standard_normal((T, K)), rng.standard_normal((E, K, N)), rng.standard_normal((T, N))
    so = R.sanitize(offsets, T)
    want = 2.0 * c0
    owner = np.full(T, -1)
    for r in range(T):
        for e in range(E):
            if so[e] <= r < so[e + 1]:
                owner[r] = e
                want[r] += 0.5 * np.array([sum(a[r, k] * w[e, k, n] for k in range(K)) for n in range(N)])
    assert np.array_equal(owner, R.row_expert(offsets, T))
    assert np.allclose(R.forward(a, w, offsets, 0.5, 2.0, c0), want, rtol=1e-13, atol=1e-13)
    assert np.allclose(R.forward(a, np.swapaxes(w, 1, 2), offsets, 0.5, 2.0, c0, trans_b=True), want, rtol=1e-13, atol=1e-13)
    z = R.forward(a, w, offsets)
    assert not z[owner < 0].any() and not np.signbit(z[owner < 0]).any()   # uncovered rows: +0 with beta = 0
    b, d0 = rng.standard_normal((T, N)), rng.standard_normal((E, K, N))
    wantw = 2.0 * d0
    for e in range(E):
        for r in range(T):
            if owner[r] == e:
                wantw[e] += 0.5 * np.outer(a[r], b[r])
    assert np.allclose(R.wgrad(a, b, offsets, 0.5, 2.0, d0), wantw, rtol=1e-13, atol=1e-13)
    a2 = a.copy()
    a2[owner != 0] = np.nan   # other segments' rows never enter dW_0
    assert np.array_equal(R.wgrad(a2, b, offsets)[0], R.wgrad(a, b, offsets)[0])


def check_tiles(offsets, T):
    E = len(offsets) - 1
    so = R.sanitize(offsets, T).tolist()
    tiles = R.tile_map(offsets, T)
    assert len(tiles) <= R.tile_bound(T, E), (offsets, T, len(tiles))
    at = 0
    for r0, r1, seg in tiles:   # consecutive, non-empty, at most one tile long: every row of [0, T) lies in exactly one
        assert r0 == at and r0 < r1 <= r0 + R.TILE, (offsets, T, tiles)
        at = r1
        if seg == R.UNCOVERED:
            assert r1 <= so[0] or r0 >= so[E], (offsets, T, (r0, r1))
        else:
            assert 0 <= seg < E and so[seg] <= r0 and r1 <= so[seg + 1], (offsets, T, (r0, r1, seg))
            assert (r0 - so[seg]) % R.TILE == 0   # a segment's tiles start at its first row
    assert at == T


def grid(T):
    return sorted({-3, 0, 1, 127, 128, 129, T // 2, T - 1, T, T + 9})


def test_tile_map_one_expert_every_T():
    for T in range(0, 301):
        for offsets in itertools.product(grid(T), repeat=2):
            check_tiles(list(offsets), T)


@pytest.mark.parametrize("E", [2, 3, 4, 5])
def test_tile_map_grid_of_offsets(E):
    rng = np.random.default_rng(E)
    for T in sorted({0, 1, 127, 128, 129, 255, 256, 257, 300} | set(range(0, 301, 37))):
        g = grid(T)
        if len(g) ** (E + 1) <= 12000:
            combos = itertools.product(g, repeat=E + 1)
        else:   # a seeded sample of the product, plus every ascending walk through a coarser grid
            combos = [tuple(g[i] for i in rng.integers(0, len(g), E + 1)) for _ in range(3000)]
            combos += list(itertools.combinations_with_replacement([0, 1, 128, 129, T // 2, T], E + 1))
        for offsets in combos:
            check_tiles(list(offsets), T)


def test_tile_map_layouts_of_the_gpu_suite():
    for offsets, T in (([0, 256], 256), ([0, 1, 129, 129, 300], 300), ([0, 0, 70, 200, 200, 200], 200), ([37, 165, 165, 390], 400), ([0, 650, 700], 700),
                       ([0, 300, 100, 9999], 400)):
        check_tiles(offsets, T)
    assert R.tile_map([0, 300, 100, 9999], 400) == R.tile_map([0, 300, 300, 400], 400)
    assert [t[2] for t in R.tile_map([37, 165, 165, 390], 400)] == [R.UNCOVERED, 0, 2, 2, R.UNCOVERED]
