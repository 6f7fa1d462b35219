"""mvg_gemv_t_multi's host side, without a GPU: the variant table, the argument refusals (decided
from the arguments alone, so fake pointers never reach a HIP call), the no-ops, and how
mvg_gemv_t_multi_plan cuts a problem (csrc/gemv_t_multi.hip plan_tm): the bands cover m, the grid
fits one launch, the four swept shapes keep 512 workgroups with the partials' traffic within 2 % of
A's, nv vectors go out in groups of the variant's chain count, and the automatic pick.
"""
import ctypes as C
import re

import pytest

from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm

lib = _lib.lib
FAKE_A, FAKE_Z, FAKE_Y = 0x10000, 0x20000, 0x30000  # never dereferenced: every call below is refused

NAMES = ["auto", "separate",
         "tstripm_w4_c1_u8_v2", "tstripm_w4_c1_u4_v4", "tstripm_w4_c1_u4_v8", "tstripm_w4_c1_u2_v16",
         "tstripm_w4_c2_u4_v2", "tstripm_w4_c2_u4_v4", "tstripm_w4_c2_u2_v8", "tstripm_w4_c2_u2_v16",
         "tstripm_w4_c1_u8_v8", "tstripm_w4_c1_u4_v16", "tstripm_w4_c1_u8_v16", "tstripm_w4_c2_u4_v16"]
FUSED = range(2, len(NAMES))
SWEPT = [(16384, 16384), (65536, 8192), (65536, 32768), (524288, 512)]


def chains(v):
    return int(re.search(r"_v(\d+)$", NAMES[v]).group(1))


def threads(v):
    return 64 * int(re.search(r"_w(\d+)_", NAMES[v]).group(1))


def test_variant_table_names_and_count():
    assert lib.mvg_gemv_t_multi_variant_count() == len(NAMES)
    assert [lib.mvg_gemv_t_multi_variant_name(v).decode() for v in range(len(NAMES))] == NAMES
    assert lib.mvg_gemv_t_multi_variant_name(-1) == b"invalid"
    assert lib.mvg_gemv_t_multi_variant_name(len(NAMES)) == b"invalid"
    assert lib.mvg_gemv_t_multi_variant_name(1) == b"separate"
    assert sorted({chains(v) for v in FUSED}) == [2, 4, 8, 16]


@pytest.mark.parametrize("args", [
    (FAKE_A, 7, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, 0),      # lda < k
    (FAKE_A, 8, FAKE_Z, 3, FAKE_Y, 8, 4, 8, 3, 0),      # ldz < m
    (FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 7, 4, 8, 3, 0),      # ldy < k
    (FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, -1, 8, 3, 0),     # negative m
    (FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, -1, 3, 0),     # negative k
    (FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, -1, 0),     # negative nv
    (None, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, 0),        # null A
    (FAKE_A, 8, None, 4, FAKE_Y, 8, 4, 8, 3, 0),        # null Z
    (FAKE_A, 8, FAKE_Z, 4, None, 8, 4, 8, 3, 0),        # null Y
    (FAKE_A, 8, FAKE_Z, 4, None, 8, 0, 8, 3, 0),        # m == 0 still writes Y
    (FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, -1),     # variant out of range
    (FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, len(NAMES)),
], ids=["lda<k", "ldz<m", "ldy<k", "m<0", "k<0", "nv<0", "null-A", "null-Z", "null-Y", "null-Y-m0", "variant<0",
        "variant>=count"])
def test_argument_refusals_answer_invalid(args):
    A, lda, Z, ldz, Y, ldy, m, k, nv, v = args
    for variant in ([v] if v else range(len(NAMES))):
        assert lib.mvg_gemv_t_multi_variant(A, lda, Z, ldz, Y, ldy, m, k, nv, variant, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi"), lib.mvg_last_error()
    if v == 0:
        assert lib.mvg_gemv_t_multi(A, lda, Z, ldz, Y, ldy, m, k, nv, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi")


def test_k_zero_and_nv_zero_are_no_ops_even_on_null_operands():
    for v in range(len(NAMES)):
        assert lib.mvg_gemv_t_multi_variant(None, 0, None, 0, None, 0, 5, 0, 3, v, None) == _lib.MVG_OK
        assert lib.mvg_gemv_t_multi_variant(None, 8, None, 0, None, 0, 5, 8, 0, v, None) == _lib.MVG_OK
    assert lib.mvg_gemv_t_multi(None, 0, None, 0, None, 0, 5, 0, 3, None) == _lib.MVG_OK
    assert lib.mvg_gemv_t_multi(None, 8, None, 0, None, 0, 5, 8, 0, None) == _lib.MVG_OK


def test_plan_refusals():
    b, n, sc, g = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    out = (C.byref(b), C.byref(n), C.byref(sc), C.byref(g))
    assert lib.mvg_gemv_t_multi_plan(7, 4, 8, 3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_multi_plan(8, -4, 8, 3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_multi_plan(8, 4, -8, 3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_multi_plan(8, 4, 8, -3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_multi_plan(8, 4, 8, 3, -1, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_multi_plan(8, 4, 8, 3, len(NAMES), *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_t_multi_plan(8, 4, 8, 3, 0, None, None, None, None) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi")


def test_more_strips_than_one_grid_holds_is_refused_from_the_arguments_alone():
    """lda = k = 2^31: 2^25 strips of 64 columns against 2^31 / 256 = 2^23 workgroups of one launch;
    the 128-column strips (2^24 of them) do not fit either."""
    b, n, sc, g = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    out = (C.byref(b), C.byref(n), C.byref(sc), C.byref(g))
    K = 1 << 31
    for v in FUSED:
        assert -(-K // (64 if "_c1_" in NAMES[v] else 128)) > (1 << 31) // threads(v)
        assert lib.mvg_gemv_t_multi_plan(K, 4, K, 2, v, *out) == _lib.MVG_E_INVALID, NAMES[v]
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi")
        assert lib.mvg_gemv_t_multi_variant(FAKE_A, K, FAKE_Z, 4, FAKE_Y, K, 4, K, 2, v, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi")
        # one vector left goes through mvg_gemv_t: its own strip limit, under this entry's name
        assert lib.mvg_gemv_t_multi_variant(FAKE_A, K, FAKE_Z, 4, FAKE_Y, K, 4, K, 1, v, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi")
    for v in (0, 1):  # separate: mvg_gemv_t's own limit
        assert lib.mvg_gemv_t_multi_plan(K, 4, K, 2, v, *out) == _lib.MVG_E_INVALID
        assert lib.mvg_gemv_t_multi_variant(FAKE_A, K, FAKE_Z, 4, FAKE_Y, K, 4, K, 2, v, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_t_multi")


# tests/test_gemv_t_host.py's coverage lists
COVER = [(m, k) for m in (25_600, 65_536, 524_288, 4_194_304) for k in (512, 8192, 16384)] + \
        [(1, 1), (31, 5), (33, 257), (1000, 257), (20001, 7), (4099, 129), (65538, 3), (2048, 16384), (64, 1 << 20),
         (25_599, 512), (1 << 26, 65536)]


@pytest.mark.parametrize("m,k", COVER)
def test_bands_cover_m_and_the_grid_fits_one_launch(m, k):
    for v in FUSED:
        for nv in (2, chains(v), chains(v) + 3):
            band_rows, bands, strip_cols, group = mm.gemv_t_multi_plan(k, m, k, nv, v)
            assert group == min(nv, chains(v)), (NAMES[v], nv, group)
            assert strip_cols == (64 if "_c1_" in NAMES[v] else 128)
            assert band_rows >= 32 and bands * band_rows >= m > (bands - 1) * band_rows, (NAMES[v], band_rows, bands)
            assert bands * -(-k // strip_cols) * threads(v) <= 1 << 31, (NAMES[v], band_rows, bands)
            # the cut belongs to the variant: not to nv
            assert (band_rows, bands, strip_cols) == mm.gemv_t_multi_plan(k, m, k, chains(v), v)[:3]


@pytest.mark.parametrize("m,k", SWEPT)
def test_swept_shapes_fill_the_chip_with_workspace_traffic_within_two_percent(m, k):
    for v in FUSED:
        NV = chains(v)
        band_rows, bands, strip_cols, group = mm.gemv_t_multi_plan(k, m, k, NV, v)
        assert group == NV
        assert bands * -(-k // strip_cols) >= 512, (NAMES[v], band_rows, bands)
        assert 16 * bands * k * NV <= 0.02 * 8 * m * k, (NAMES[v], band_rows, bands)
        # and at a view's lda
        assert mm.gemv_t_multi_plan(k + 16, m, k, NV, v) == (band_rows, bands, strip_cols, group)


def test_the_example_of_the_design_note():
    """16384^2 at 16 chains over 64-column strips: 256 strips, so 2 <= bands <= 10."""
    band_rows, bands, strip_cols, group = mm.gemv_t_multi_plan(16384, 16384, 16384, 16, NAMES.index("tstripm_w4_c1_u2_v16"))
    assert (strip_cols, group) == (64, 16) and 2 <= bands <= 10 and (band_rows, bands) == (2048, 8)


def _walk(m, k, nv, v):
    groups = []
    while nv > 0:
        band_rows, bands, strip_cols, g = mm.gemv_t_multi_plan(k, m, k, nv, v)
        assert 1 <= g <= nv
        groups.append((g, band_rows, bands, strip_cols))
        nv -= g
    return groups


@pytest.mark.parametrize("nv", [1, 2, 3, 5, 8, 9, 16, 17, 33])
def test_how_nv_vectors_are_cut_into_groups(nv):
    m, k = 5000, 512
    single = mm.gemv_t_plan(k, m, k)
    for v in FUSED:
        NV = chains(v)
        want = [NV] * (nv // NV)
        if nv % NV == 1:
            want += [1]       # a single leftover vector: mvg_gemv_t
        elif nv % NV:
            want += [nv % NV]  # a short group of the same kernel
        groups = _walk(m, k, nv, v)
        assert [g[0] for g in groups] == want, (NAMES[v], nv, groups)
        fused = mm.gemv_t_multi_plan(k, m, k, NV, v)[:3]
        for g, *cut in groups:
            assert tuple(cut) == (single if g == 1 else fused), (NAMES[v], nv, g, cut)
    for v in (0, 1):  # separate: one vector at a time, mvg_gemv_t's own cut
        assert _walk(m, k, nv, v) == [(1, *single)] * nv
    assert mm.gemv_t_multi_plan(k, m, k, 0, 2)[3] == 0


def test_pinned_groups_of_the_16_chain_variant():
    v = NAMES.index("tstripm_w4_c2_u2_v16")
    assert [[g[0] for g in _walk(5000, 512, nv, v)] for nv in (1, 2, 3, 5, 8, 9, 16, 17, 33)] == \
        [[1], [2], [3], [5], [8], [9], [16], [16, 1], [16, 16, 1]]
    v = NAMES.index("tstripm_w4_c1_u8_v2")
    assert [[g[0] for g in _walk(5000, 512, nv, v)] for nv in (1, 2, 3, 5)] == [[1], [2], [2, 1], [2, 2, 1]]


def test_empty_problems_plan_no_bands():
    for v in range(len(NAMES)):
        assert mm.gemv_t_multi_plan(8, 0, 8, 4, v)[1] == 0


def _auto_walk(m, k, nv, lda=None):
    """The automatic choice group by group: [(variant name, vectors)]."""
    lda, out = lda or k, []
    while nv > 0:
        v = lib.mvg_gemv_t_multi_auto_variant(lda, m, m, k, nv)
        g = mm.gemv_t_multi_plan(lda, m, k, nv)[3]
        assert g == (min(nv, chains(v)) if v >= 2 else 1) and (v < 2 or chains(v) <= nv)  # full groups only
        assert mm.gemv_t_multi_plan(lda, m, k, nv)[:3] == \
            (mm.gemv_t_multi_plan(lda, m, k, chains(v), v)[:3] if v >= 2 else mm.gemv_t_plan(lda, m, k))
        out.append((NAMES[v], g))
        nv -= g
    return out


def test_auto_pick_at_the_swept_shapes():
    """Pinned literally from the kept sweeps (profiles/r07/gemv_t_multi/, MEASUREMENTS §18)."""
    c1 = {2: "tstripm_w4_c1_u8_v2", 4: "tstripm_w4_c1_u4_v4", 8: "tstripm_w4_c1_u4_v8"}
    c2 = {2: "tstripm_w4_c2_u4_v2", 4: "tstripm_w4_c2_u4_v4", 8: "tstripm_w4_c1_u8_v8"}
    for nv in (2, 4, 8):
        assert _auto_walk(16384, 16384, nv) == [(c1[nv], nv)]
        assert _auto_walk(16384, 16384, nv, lda=16400) == [(c1[nv], nv)]
        assert _auto_walk(65536, 8192, nv) == [(c1[nv], nv)]
        assert _auto_walk(65536, 32768, nv) == [(c1[nv], nv)]
        assert _auto_walk(524288, 512, nv) == [(c2[nv], nv)]
    assert _auto_walk(16384, 16384, 16) == [("tstripm_w4_c2_u2_v16", 16)]
    assert _auto_walk(16384, 16384, 16, lda=16400) == [("tstripm_w4_c2_u2_v16", 16)]
    assert _auto_walk(65536, 8192, 16) == [("tstripm_w4_c1_u8_v16", 16)]
    assert _auto_walk(65536, 32768, 16) == [("tstripm_w4_c1_u8_v16", 16)]
    assert _auto_walk(524288, 512, 16) == [("tstripm_w4_c2_u4_v16", 16)]
    # k < 128: no more than four chains
    assert [_auto_walk(4_194_304, 64, nv) for nv in (2, 4, 8, 16)] == \
        [[(c1[2], 2)], [(c1[4], 4)], [(c1[4], 4)] * 2, [(c1[4], 4)] * 4]


def test_auto_launches_full_groups_only_and_a_single_leftover_vector():
    c1 = {2: "tstripm_w4_c1_u8_v2", 4: "tstripm_w4_c1_u4_v4", 8: "tstripm_w4_c1_u4_v8"}
    v16, t16 = "tstripm_w4_c2_u2_v16", "tstripm_w4_c1_u8_v16"
    assert _auto_walk(16384, 16384, 1) == [("separate", 1)]
    assert _auto_walk(16384, 16384, 3) == [(c1[2], 2), ("separate", 1)]
    assert _auto_walk(16384, 16384, 7) == [(c1[4], 4), (c1[2], 2), ("separate", 1)]
    assert _auto_walk(16384, 16384, 15) == [(c1[8], 8), (c1[4], 4), (c1[2], 2), ("separate", 1)]
    assert _auto_walk(16384, 16384, 33) == [(v16, 16), (v16, 16), ("separate", 1)]
    assert _auto_walk(65536, 8192, 27) == [(t16, 16), (c1[8], 8), (c1[2], 2), ("separate", 1)]


def test_auto_is_separate_outside_the_swept_range():
    """Fewer than 16384 rows, fewer than 64 columns, or fewer than 2^28 elements: nothing was swept."""
    for m, k in [(16383, 32768), (8_388_608, 63), (16384, 16383), (65536, 4095), (1000, 257), (1, 1)]:
        for nv in (2, 4, 8, 16, 33):
            assert _auto_walk(m, k, nv) == [("separate", 1)] * nv, (m, k, nv)
    assert _auto_walk(65536, 4096, 2) == [("tstripm_w4_c1_u8_v2", 2)]
