"""mvg_gemv_t's host side, without a GPU: the argument refusals (decided from the arguments alone,
so fake pointers never reach a HIP call), the variant table, and how mvg_gemv_t_plan cuts a problem
into bands and strips (csrc/gemv_t.hip plan_t): the bands cover m, the workspace traffic
16 * bands * k stays within 1 % of A's 8 * m * k from 25 600 rows on, short and wide problems still
fill the chip, and the automatic pick at the four swept shapes (MEASUREMENTS "Transposed product").
"""
import ctypes as C

import pytest

from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm

lib = _lib.lib
FAKE_A, FAKE_Z, FAKE_Y = 0x10000, 0x20000, 0x30000  # never dereferenced: every call below is refused

NAMES = ["auto", "strip_w8_c4_u4_b256", "strip_w8_c4_u4_b2048", "strip_w8_c2_u8_b256", "strip_w4_c2_u8_b256",
         "strip_w4_c2_u4_b256", "scalar_w4_c2_u4", "scalar_w4_c2_u4_b2048", "scalar_w4_c2_u8", "scalar_w8_c2_u4",
         "scalar_w4_c1_u8"]


def _variants():
    return range(lib.mvg_gemv_t_variant_count())


def test_variant_table_names_and_count():
    assert lib.mvg_gemv_t_variant_count() == len(NAMES)
    assert [lib.mvg_gemv_t_variant_name(v).decode() for v in _variants()] == NAMES
    assert lib.mvg_gemv_t_variant_name(-1) == b"invalid"
    assert lib.mvg_gemv_t_variant_name(len(NAMES)) == b"invalid"


@pytest.mark.parametrize("args", [
    (FAKE_A, 7, FAKE_Z, FAKE_Y, 4, 8, 0),      # lda < k
    (FAKE_A, 8, FAKE_Z, FAKE_Y, -1, 8, 0),     # negative m
    (FAKE_A, 8, FAKE_Z, FAKE_Y, 4, -1, 0),     # negative k
    (None, 8, FAKE_Z, FAKE_Y, 4, 8, 0),        # null A
    (FAKE_A, 8, None, FAKE_Y, 4, 8, 0),        # null z
    (FAKE_A, 8, FAKE_Z, None, 4, 8, 0),        # null y
    (FAKE_A, 8, FAKE_Z, None, 0, 8, 0),        # m == 0 still writes y
    (FAKE_A, 8, FAKE_Z, FAKE_Y, 4, 8, -1),     # variant out of range
    (FAKE_A, 8, FAKE_Z, FAKE_Y, 4, 8, len(NAMES)),
], ids=["lda<k", "m<0", "k<0", "null-A", "null-z", "null-y", "null-y-m0", "variant<0", "variant>=count"])
def test_argument_refusals_answer_invalid(args):
    A, lda, z, y, m, k, v = args
    assert lib.mvg_gemv_t_variant(A, lda, z, y, m, k, v, None) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_t")
    if v == 0:
        assert lib.mvg_gemv_t(A, lda, z, y, m, k, None) == _lib.MVG_E_INVALID


def test_k_zero_is_a_no_op_even_on_null_operands():
    assert lib.mvg_gemv_t(None, 0, None, None, 5, 0, None) == _lib.MVG_OK


def test_plan_refusals():
    b, n, sc = C.c_int64(), C.c_int64(), C.c_int64()
    out = (C.byref(b), C.byref(n), C.byref(sc))
    assert lib.mvg_gemv_t_plan(7, 4, 8, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_plan(8, -4, 8, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_plan(8, 4, 8, len(NAMES), *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_plan(8, 4, 8, 0, None, None, None) == _lib.MVG_E_INVALID
    # more strips than one grid holds: refused from the arguments alone (2^31 / 512 strips of 256)
    assert lib.mvg_gemv_t_plan(1 << 31, 4, 1 << 31, 1, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_variant(FAKE_A, 1 << 31, FAKE_Z, FAKE_Y, 4, 1 << 31, 1, None) == _lib.MVG_E_INVALID


@pytest.mark.parametrize("m", [25_600, 65_536, 524_288, 4_194_304])
@pytest.mark.parametrize("k", [512, 8192, 16384])
def test_bands_cover_m_and_workspace_traffic_is_within_one_percent(m, k):
    for v in _variants():
        band_rows, bands, strip_cols = mm.gemv_t_plan(k, m, k, v)
        assert bands * band_rows >= m > (bands - 1) * band_rows, (NAMES[v], band_rows, bands)
        assert 16 * bands * k <= 0.01 * 8 * m * k, (NAMES[v], band_rows, bands)
        assert strip_cols in (64, 128, 256)


@pytest.mark.parametrize("m,k", [(1, 1), (31, 5), (33, 257), (1000, 257), (20001, 7), (4099, 129), (65538, 3),
                                 (2048, 16384), (64, 1 << 20), (25_599, 512), (1 << 26, 65536)])
def test_bands_cover_m_at_any_shape_and_the_grid_fits(m, k):
    for v in _variants():
        band_rows, bands, strip_cols = mm.gemv_t_plan(k, m, k, v)
        assert band_rows >= 32 and bands * band_rows >= m > (bands - 1) * band_rows, (NAMES[v], band_rows, bands)
        threads = 512 if "_w8_" in NAMES[v or lib.mvg_gemv_t_auto_variant(k, m, k)] else 256
        assert bands * -(-k // strip_cols) * threads <= 1 << 31, (NAMES[v], band_rows, bands)  # one launch


@pytest.mark.parametrize("m,k", [(64, 1 << 20), (2048, 16384)])
def test_short_problems_fill_the_chip(m, k):
    for v in _variants():
        band_rows, bands, strip_cols = mm.gemv_t_plan(k, m, k, v)
        assert bands * -(-k // strip_cols) >= 512, (NAMES[v], band_rows, bands)


def test_empty_problems_plan_no_bands():
    for v in _variants():
        assert mm.gemv_t_plan(8, 0, 8, v)[1] == 0


def test_auto_pick_at_the_swept_shapes():
    """Pinned literally: the picks the sweep accepted (profiles/r07/gemv_t/sweep.jsonl)."""
    assert NAMES[lib.mvg_gemv_t_auto_variant(16384, 16384, 16384)] == "scalar_w4_c1_u8"
    assert NAMES[lib.mvg_gemv_t_auto_variant(8192, 65536, 8192)] == "scalar_w4_c2_u4_b2048"
    assert NAMES[lib.mvg_gemv_t_auto_variant(32768, 65536, 32768)] == "scalar_w4_c2_u4_b2048"
    assert NAMES[lib.mvg_gemv_t_auto_variant(512, 524288, 512)] == "scalar_w4_c2_u4_b2048"
    # and how they cut those shapes
    assert mm.gemv_t_plan(16384, 16384, 16384) == (256, 64, 64)
    assert mm.gemv_t_plan(8192, 65536, 8192) == (1024, 64, 128)
    assert mm.gemv_t_plan(32768, 65536, 32768) == (2048, 32, 128)
    assert mm.gemv_t_plan(512, 524288, 512) == (512, 1024, 128)
    # both are 8-B forms: an odd lda takes the same pick
    assert lib.mvg_gemv_t_auto_variant(16385, 16384, 16384) == lib.mvg_gemv_t_auto_variant(16384, 16384, 16384)
