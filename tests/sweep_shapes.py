"""The reference's published sweep, shard by shard (no GPU; plain Python over the planner).

The reference's test.sh and data/out/*.csv cover nine squares 600 ... 10200 in
steps of 1200 and ten asymmetric shapes 120 ... 1200 x 60000 in steps of 120 rows, each at
P = 1, 2, 6, 12, 24 for the three algorithms: 285 combinations. `shards` gives every rank's
shard of a combination from the project's own planner (mm.plan_shard); `distinct_shard_shapes`
the (n_rows, n_cols) the sweep multiplies. EXTRAS are kernel-level shapes, one per pick of the
tree dispatch (gemv.hip pick_variant) that no shard of the sweep reaches, each the smallest the
dispatch rules allow, plus one shape just under a boundary.

tests/test_sweep_shapes_host.py asserts the counts and the picks by name on the CPU;
tests/test_gpu_sweep_shapes.py runs all of it on the device.
"""
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import gendata
from matvec_mpi_multiplier_amd import multiplier as mm

lib = _lib.lib

SQUARES = [(n, n) for n in gendata.TEST_SH_SIZES]
ASYMMETRIC = [(r, 60000) for r in range(120, 1201, 120)]
SIZES = SQUARES + ASYMMETRIC
PS = (1, 2, 6, 12, 24)
ALGS = ("rowwise", "colwise", "blockwise")
assert len(SIZES) == 19 and len(SIZES) * len(PS) * len(ALGS) == 285

# the picks the sweep's shards reach (name: the form), and the rest of the dispatch's picks for
# 8-byte-aligned operands, which only EXTRAS reach
SWEEP_PICKS = {
    "vec_l64_r1_u4_nt1_o5": "one row per wave",
    "vec_l64_r4_u4_nt1_o0": "four rows per wave, odd lda",
    "rowblk_w2_r2_u4": "2-wave row form",
    "rowblk_w4_r2_u4_splitk": "split-K",
    "rowblk_w8_r2_u4": "8-wave row form",
    "rowlines_w8_u4_x0": "line-aligned row pairs",
}
EXTRA_PICKS = {
    "vec_l64_r4_u4_nt1_o5": "four rows per wave",
    "vec_l64_r2_u4_nt1_o7": "two rows per wave",
    "rowblk_w4_r2_u8_xcd": "long rows, odd lda, XCD-contiguous workgroup order",
    "rowblk_w4_r2_u8": "long rows",
}

# (m, k, pick): lda = k. The row-pair distance of rowlines_* is p = 16 / gcd(lda, 16); the
# sweep's six shapes of that form all have lda % 16 == 8, p = 2.
EXTRAS = [
    (87382, 1536, "vec_l64_r4_u4_nt1_o5"),    # A >= 1 GiB (2^27 doubles), 768 < K <= 1536
    (87269, 1538, "vec_l64_r2_u4_nt1_o7"),    # A >= 1 GiB, 1536 < K < 4096, odd M
    (1401, 4097, "rowblk_w4_r2_u8_xcd"),      # odd lda, K >= 4096, 701 workgroups (not a multiple of 8)
    (1399, 16400, "rowblk_w4_r2_u8"),         # K >= 16384, 700 workgroups, lda % 16 == 0, odd M
    (4097, 6145, "rowlines_w8_u4_x0"),        # p = 16
    (4099, 6146, "rowlines_w8_u4_x0"),        # p = 8
    (4098, 6148, "rowlines_w8_u4_x0"),        # p = 4
    (1398, 16400, "rowblk_w4_r2_u4_splitk"),  # one row under the long-row form's boundary
]

# where exact mode keeps a column-panel copy (mvg_exact_panel_width == 256): these shards only
PANEL_SHARDS = {(n, n) for n in (6600, 7800, 9000, 10200)} | {(n, n // 2) for n in (6600, 7800, 9000, 10200)}


def combos():
    """(R, C, alg, P), all 285, size-major (a cache of the current size's A and x is reused)."""
    return [(R, C, alg, P) for R, C in SIZES for alg in ALGS for P in PS]


def shards(R, C, alg, P):
    """Every rank's shard of the combination (mvg_shard, from mm.plan_shard); raises
    IndivisibleError where the reference would print its "ERROR!!!"."""
    return [mm.plan_shard(alg, R, C, P, r) for r in range(P)]


def distinct_shard_shapes():
    """{(n_rows, n_cols)} over every rank of every combination."""
    return {(s.n_rows, s.n_cols) for R, C, alg, P in combos() for s in shards(R, C, alg, P)}


def tree_pick(m, k, lda=None):
    """The automatic tree kernel's name for a packed, line-aligned m x k operand."""
    return lib.mvg_gemv_variant_name(lib.mvg_gemv_auto_variant(lda or k, m, k)).decode()


def exact_pick(m, k, lda=None):
    return lib.mvg_gemv_exact_variant_name(lib.mvg_gemv_exact_auto_variant(lda or k, m, k)).decode()
