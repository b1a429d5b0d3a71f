"""The launch geometry of the FP8 kernels, restated in Python, and the shapes tests/test_gpu_fp8_edges.py chose from it. No GPU, numpy only.

kf_fp8_amax (kfunca_amd/csrc/device/fp8.hip): a block is 256 threads of 16 columns, so a column strip is 4096 wide; the grid is
gx = ceil(cols / 4096) by gy = min(rows, ceil(4096 / gx), 65535), and block (bx, by) walks rows by, by + 4 gy, ... of its strip, loading
the rows r, r + gy, r + 2 gy, r + 3 gy of one trip together (a row past the end re-reads the last row).
kf_gemm_fp8 (gemm_fp8.hip): 128 x 128 tiles, hardware block ids dealt to 8 XCDs (q_xcd_remap), logical ids walking groups of 8 tile rows
column by column (q_grouped_tile).
tests/test_fp8_ref.py asserts that the shapes below still reach what they were chosen for, so a retuned launch fails there, on the CPU."""
AMAX_STRIP = 256 * 16
AMAX_BLOCKS = 4096
AMAX_UNROLL = 4

# rows x cols -> what the shape is there for: trips of the row loop, whether the u = 1..3 loads of the first trip are real rows, gx
AMAX_SHAPES = {
    (4097, 16): dict(trips=1, real_u=True, gx=1),
    (16384, 16): dict(trips=1, real_u=True, gx=1),
    (16385, 16): dict(trips=2, real_u=True, gx=1),
    (40000, 17): dict(trips=3, real_u=True, gx=1),
    (3, 4097): dict(trips=1, real_u=False, gx=2),
    (9, 8232): dict(trips=1, real_u=False, gx=3),
    (8193, 4097): dict(trips=2, real_u=True, gx=2),
    (5465, 8193): dict(trips=2, real_u=True, gx=3),
}
AMAX_QUANTIZED = [(3, 4097), (4097, 16)]      # the two smallest: the ones that also go through kf_fp8_quantize


def amax_grid(rows, cols):
    gx = -(-cols // AMAX_STRIP)
    want = -(-AMAX_BLOCKS // gx)
    return gx, min(rows, want, 65535)


def amax_trips(rows, cols):
    """How often the block with the most rows (blockIdx.y = 0) goes round `for (r = blockIdx.y; r < rows; r += 4 * gridDim.y)`."""
    gy = amax_grid(rows, cols)[1]
    return -(-rows // (AMAX_UNROLL * gy))


def amax_vector_path(cols, ld, es, base_offset_bytes, c0):
    """The thread whose first column is c0: does it take the 16-byte loads?"""
    return min(cols - c0, 16) == 16 and base_offset_bytes % 16 == 0 and (ld * es) % 16 == 0


# ---- kf_gemm_fp8's block order ---------------------------------------------------------------------------------------------------
GEMM_TILE = 128
GEMM_GROUP = 8
GEMM_XCDS = 8
TILE_COUNTS = [(8, 1), (9, 1), (9, 3), (12, 5), (16, 2), (17, 2), (23, 7), (1, 17)]      # (tile rows, tile columns)


def xcd_remap(bid, nwg):
    xcd, q, r = bid % GEMM_XCDS, nwg // GEMM_XCDS, nwg % GEMM_XCDS
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + bid // GEMM_XCDS


def grouped_tile(i, tiles_m, tiles_n):
    per = GEMM_GROUP * tiles_n
    grp = i // per
    first = grp * GEMM_GROUP
    rows = min(GEMM_GROUP, tiles_m - first)
    within = i - grp * per
    return first + within % rows, within // rows


def tile_of_block(bid, tiles_m, tiles_n):
    return grouped_tile(xcd_remap(bid, tiles_m * tiles_n), tiles_m, tiles_n)
