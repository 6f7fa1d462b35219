"""mvg_gemv_ata's host side, without a GPU: the argument refusals (decided from the arguments alone,
so fake pointers never reach a HIP call), the variant table, each fused variant's max_k, how
mvg_gemv_ata_plan cuts m into bands (csrc/gemv_ata.hip plan_ata): the bands cover m and the grid
fits one launch, and the automatic pick at the swept shapes (MEASUREMENTS "Fused A^T A product").
"""
import ctypes as C

import pytest

from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm

lib = _lib.lib
FAKE_A, FAKE_X, FAKE_T, FAKE_W = 0x10000, 0x20000, 0x30000, 0x40000  # never dereferenced: every call is refused
INT64_MAX = (1 << 63) - 1

NAMES = ["auto", "two_pass", "wrow_w8_c4_u8", "wrow_w8_c8_u4", "wrow_w4_c16_u2", "wgrow_w8_c8_r2", "wgrow_w8_c16_r1",
         "wgrow_w16_c8_r2", "wgrow_w16_c16_r1"]
MAX_K = {"wrow_w8_c4_u8": 256, "wrow_w8_c8_u4": 512, "wrow_w4_c16_u2": 1024, "wgrow_w8_c8_r2": 4096,
         "wgrow_w8_c16_r1": 8192, "wgrow_w16_c8_r2": 8192, "wgrow_w16_c16_r1": 16384}
FUSED = [v for v, n in enumerate(NAMES) if n in MAX_K]
TWO_PASS = NAMES.index("two_pass")


def threads(v):
    return 64 * int(NAMES[v].split("_")[1][1:])  # w<NW>


def test_variant_table_names_and_count():
    assert lib.mvg_gemv_ata_variant_count() == len(NAMES)
    assert [lib.mvg_gemv_ata_variant_name(v).decode() for v in range(len(NAMES))] == NAMES
    assert lib.mvg_gemv_ata_variant_name(-1) == b"invalid"
    assert lib.mvg_gemv_ata_variant_name(len(NAMES)) == b"invalid"
    assert len([n for n in NAMES if n.startswith("wrow_")]) >= 2 and len([n for n in NAMES if n.startswith("wgrow_")]) >= 2


def test_max_k_of_every_variant():
    for v in FUSED:
        assert mm.gemv_ata_plan(8, 8, 8, v)[2] == MAX_K[NAMES[v]]
        if NAMES[v].startswith("wrow_"):
            assert MAX_K[NAMES[v]] >= 128
    assert mm.gemv_ata_plan(8, 8, 8, TWO_PASS) == (0, 0, INT64_MAX)


@pytest.mark.parametrize("args", [
    (FAKE_A, 7, FAKE_X, FAKE_T, FAKE_W, 4, 8, 0),      # lda < k
    (FAKE_A, 8, FAKE_X, FAKE_T, FAKE_W, -1, 8, 0),     # negative m
    (FAKE_A, 8, FAKE_X, FAKE_T, FAKE_W, 4, -1, 0),     # negative k
    (None, 8, FAKE_X, FAKE_T, FAKE_W, 4, 8, 0),        # null A
    (FAKE_A, 8, None, FAKE_T, FAKE_W, 4, 8, 0),        # null x
    (FAKE_A, 8, FAKE_X, None, FAKE_W, 4, 8, 0),        # null t
    (FAKE_A, 8, FAKE_X, FAKE_T, None, 4, 8, 0),        # null w
    (FAKE_A, 8, FAKE_X, FAKE_T, None, 0, 8, 0),        # m == 0 still writes w
    (FAKE_A, 0, FAKE_X, None, FAKE_W, 4, 0, 0),        # k == 0 still writes t
    (FAKE_A, 8, FAKE_X, FAKE_T, FAKE_W, 4, 8, -1),     # variant out of range
    (FAKE_A, 8, FAKE_X, FAKE_T, FAKE_W, 4, 8, len(NAMES)),
], ids=["lda<k", "m<0", "k<0", "null-A", "null-x", "null-t", "null-w", "null-w-m0", "null-t-k0", "variant<0",
        "variant>=count"])
def test_argument_refusals_answer_invalid(args):
    A, lda, x, t, w, m, k, v = args
    variants = [v] if v != 0 else [0, TWO_PASS] + FUSED
    for vv in variants:
        assert lib.mvg_gemv_ata_variant(A, lda, x, t, w, m, k, vv, None) == _lib.MVG_E_INVALID, NAMES[vv]
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata"), lib.mvg_last_error()
    if v == 0:
        assert lib.mvg_gemv_ata(A, lda, x, t, w, m, k, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata")


def test_both_sizes_zero_is_a_no_op_even_on_null_operands():
    for v in range(len(NAMES)):
        assert lib.mvg_gemv_ata_variant(None, 0, None, None, None, 0, 0, v, None) == _lib.MVG_OK


def test_k_zero_is_not_refused_for_null_a_x_and_w():
    """Only t would be touched: with a null t the same call is refused for t, and with a t the
    argument checks let it through (the plan, the host-only path through the same checks, accepts
    it; the launch itself belongs to the GPU tests)."""
    b, n, mk = C.c_int64(), C.c_int64(), C.c_int64()
    for v in range(len(NAMES)):
        assert lib.mvg_gemv_ata_plan(0, 5, 0, v, C.byref(b), C.byref(n), C.byref(mk)) == _lib.MVG_OK
        assert lib.mvg_gemv_ata_variant(None, 0, None, None, None, 5, 0, v, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode() == "mvg_gemv_ata: null t"


@pytest.mark.parametrize("v", FUSED, ids=lambda v: NAMES[v])
def test_an_explicit_fused_variant_is_refused_beyond_its_max_k(v):
    b, n, mk = C.c_int64(), C.c_int64(), C.c_int64()
    out = (C.byref(b), C.byref(n), C.byref(mk))
    k = MAX_K[NAMES[v]]
    assert lib.mvg_gemv_ata_plan(k, 100, k, v, *out) == _lib.MVG_OK  # k == max_k: planned
    assert mk.value == k and n.value * b.value >= 100
    assert lib.mvg_gemv_ata_plan(k + 1, 100, k + 1, v, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata")
    assert lib.mvg_gemv_ata_variant(FAKE_A, k + 1, FAKE_X, FAKE_T, FAKE_W, 100, k + 1, v, None) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata")


def test_plan_refusals():
    b, n, mk = C.c_int64(), C.c_int64(), C.c_int64()
    out = (C.byref(b), C.byref(n), C.byref(mk))
    assert lib.mvg_gemv_ata_plan(7, 4, 8, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_plan(8, -4, 8, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_plan(8, 4, 8, len(NAMES), *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_plan(8, 4, 8, 0, None, None, None) == _lib.MVG_E_INVALID
    # a grid that cannot fit: two_pass on more column strips than one launch of mvg_gemv_t holds
    assert lib.mvg_gemv_ata_plan(1 << 31, 4, 1 << 31, TWO_PASS, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata")
    assert lib.mvg_gemv_ata_variant(FAKE_A, 1 << 31, FAKE_X, FAKE_T, FAKE_W, 4, 1 << 31, TWO_PASS, None) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata")


@pytest.mark.parametrize("m,k", [(1, 1), (31, 5), (1000, 257), (20001, 7), (65538, 3), (2048, 1024), (4_194_304, 64),
                                 (1 << 40, 512)])
def test_bands_cover_m_and_the_grid_fits(m, k):
    for v in FUSED:
        if k > MAX_K[NAMES[v]]:
            continue
        band_rows, bands, max_k = mm.gemv_ata_plan(k, m, k, v)
        assert band_rows >= 32 and bands * band_rows >= m > (bands - 1) * band_rows, (NAMES[v], band_rows, bands)
        assert bands * threads(v) <= 1 << 31, (NAMES[v], band_rows, bands)  # one launch: gridDim.x * blockDim.x < 2^32
        assert max_k == MAX_K[NAMES[v]]


@pytest.mark.parametrize("m", [25_600, 65_536, 524_288, 4_194_304])
def test_workspace_traffic_is_within_one_percent_from_25600_rows_on(m):
    for v in FUSED:
        band_rows, bands, _ = mm.gemv_ata_plan(64, m, 64, v)
        assert 2 * bands <= 0.01 * m, (NAMES[v], band_rows, bands)  # 16 * bands * k against 8 * m * k


def test_empty_problems_plan_no_bands():
    for v in FUSED:
        assert mm.gemv_ata_plan(8, 0, 8, v)[1] == 0


SWEPT = [(16384, 16384), (65536, 8192), (524288, 512), (4_194_304, 64), (2048, 16384), (65536, 32768)]


def test_auto_pick_at_the_swept_shapes():
    """Pinned literally: what the sweeps left (profiles/r08/gemv_ata/sweep.jsonl, sweep_second.jsonl)."""
    picks = {(m, k): NAMES[lib.mvg_gemv_ata_auto_variant(k, m, k)] for m, k in SWEPT}
    assert picks == {
        (16384, 16384): "wgrow_w16_c16_r1",
        (65536, 8192): "wgrow_w16_c8_r2",
        (524288, 512): "wrow_w8_c8_u4",
        (4_194_304, 64): "wrow_w8_c4_u8",
        (2048, 16384): "two_pass",      # fused slower, by 55 %
        (65536, 32768): "two_pass",     # beyond every fused cap
    }
    # the cut-by-k shapes of the sweep take the pick of their bracket
    assert NAMES[lib.mvg_gemv_ata_auto_variant(12288, 16384, 12288)] == "wgrow_w16_c16_r1"
    assert NAMES[lib.mvg_gemv_ata_auto_variant(6144, 65536, 6144)] == "wgrow_w16_c8_r2"
    assert NAMES[lib.mvg_gemv_ata_auto_variant(384, 524288, 384)] == "wrow_w8_c8_u4"
    assert NAMES[lib.mvg_gemv_ata_auto_variant(192, 4_194_304, 192)] == "wrow_w8_c4_u8"
    # not tuned: fewer rows than swept, the brackets nothing was swept in, k below 64
    for m, k in [(16383, 16384), (65535, 8192), (524287, 512), (4_194_303, 64), (65536, 4096), (524288, 1024),
                 (4_194_304, 63), (1000, 257)]:
        assert NAMES[lib.mvg_gemv_ata_auto_variant(k, m, k)] == "two_pass", (m, k)
    # the pick does not depend on lda
    assert lib.mvg_gemv_ata_auto_variant(16385, 16384, 16384) == lib.mvg_gemv_ata_auto_variant(16384, 16384, 16384)
    # beyond every fused cap only two_pass applies
    assert NAMES[lib.mvg_gemv_ata_auto_variant(32768, 65536, 32768)] == "two_pass"
    assert NAMES[lib.mvg_gemv_ata_auto_variant(131072, 131072, 131072)] == "two_pass"
    # how the fused forms cut the swept shapes
    assert mm.gemv_ata_plan(16384, 16384, 16384, NAMES.index("wgrow_w16_c16_r1")) == (64, 256, 16384)
    assert mm.gemv_ata_plan(8192, 65536, 8192, NAMES.index("wgrow_w16_c8_r2")) == (256, 256, 8192)
    assert mm.gemv_ata_plan(512, 524288, 512, NAMES.index("wrow_w8_c8_u4")) == (256, 2048, 512)
    assert mm.gemv_ata_plan(64, 4_194_304, 64, NAMES.index("wrow_w8_c4_u8")) == (1024, 4096, 256)
