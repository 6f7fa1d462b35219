"""mvg_gemv_ata_multi's host side, without a GPU: the variant table, each fused variant's max_k and
group size, the argument refusals (decided from the arguments alone, so fake pointers never reach a
HIP call), the no-ops, how mvg_gemv_ata_multi_plan cuts m into bands (plan_ata's rule per variant,
never per nv), how nv vectors go out in groups, and the automatic pick.
"""
import ctypes as C
import re

import pytest

from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm

lib = _lib.lib
FAKE_A, FAKE_X, FAKE_T, FAKE_W = 0x10000, 0x20000, 0x30000, 0x40000  # never dereferenced: every call is refused
INT64_MAX = (1 << 63) - 1

NAMES = ["auto", "two_pass", "wrowm_w8_c4_u4_v2", "wrowm_w8_c4_u4_v4", "wrowm_w8_c8_u2_v2", "wrowm_w8_c8_u2_v4",
         "wgrowm_w16_c4_r2_v2", "wgrowm_w16_c4_r2_v4", "wgrowm_w16_c8_r1_v2"]
MAX_K = {"wrowm_w8_c4_u4_v2": 256, "wrowm_w8_c4_u4_v4": 256, "wrowm_w8_c8_u2_v2": 512, "wrowm_w8_c8_u2_v4": 512,
         "wgrowm_w16_c4_r2_v2": 4096, "wgrowm_w16_c4_r2_v4": 4096, "wgrowm_w16_c8_r1_v2": 8192}
FUSED = [v for v, n in enumerate(NAMES) if n in MAX_K]
TWO_PASS = NAMES.index("two_pass")
# MEASUREMENTS §17's ten shapes
SWEPT = [(16384, 16384), (65536, 8192), (524288, 512), (4_194_304, 64), (2048, 16384), (65536, 32768), (16384, 12288),
         (65536, 6144), (524288, 384), (4_194_304, 192)]


def chains(v):
    return int(re.search(r"_v(\d+)$", NAMES[v]).group(1))


def threads(v):
    return 64 * int(re.search(r"_w(\d+)_", NAMES[v]).group(1))


def _out():
    b, n, mk, g = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    return (b, n, mk, g), (C.byref(b), C.byref(n), C.byref(mk), C.byref(g))


def test_variant_table_names_and_count():
    assert lib.mvg_gemv_ata_multi_variant_count() == len(NAMES)
    assert [lib.mvg_gemv_ata_multi_variant_name(v).decode() for v in range(len(NAMES))] == NAMES
    assert lib.mvg_gemv_ata_multi_variant_name(-1) == b"invalid"
    assert lib.mvg_gemv_ata_multi_variant_name(len(NAMES)) == b"invalid"
    assert lib.mvg_gemv_ata_multi_variant_name(1) == b"two_pass"


def test_the_table_holds_what_the_registers_allow():
    """NV in {2, 4} for the two narrow wave-per-row widths and at k <= 4096, NV = 2 at k <= 8192."""
    have = {(n.split("_")[0], MAX_K[n], chains(v)) for v, n in enumerate(NAMES) if n in MAX_K}
    for nv in (2, 4):
        assert {("wrowm", 256, nv), ("wrowm", 512, nv), ("wgrowm", 4096, nv)} <= have
    assert ("wgrowm", 8192, 2) in have
    assert max(MAX_K.values()) == 8192  # wider rows have no fused block form


def test_max_k_and_group_of_every_variant():
    for v in FUSED:
        NV = chains(v)
        assert mm.gemv_ata_multi_plan(8, 8, 8, NV, v)[2:] == (MAX_K[NAMES[v]], NV)
        assert mm.gemv_ata_multi_plan(8, 8, 8, NV + 5, v)[2:] == (MAX_K[NAMES[v]], NV)
        assert mm.gemv_ata_multi_plan(8, 8, 8, 0, v)[3] == 0
    assert mm.gemv_ata_multi_plan(8, 8, 8, 5, TWO_PASS) == (0, 0, INT64_MAX, 5)
    assert mm.gemv_ata_multi_plan(8, 8, 8, 1, TWO_PASS) == (0, 0, INT64_MAX, 1)


@pytest.mark.parametrize("args", [
    (FAKE_A, 7, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, 4, 8, 3, 0),      # lda < k
    (FAKE_A, 8, FAKE_X, 7, FAKE_T, 4, FAKE_W, 8, 4, 8, 3, 0),      # ldx < k
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 3, FAKE_W, 8, 4, 8, 3, 0),      # ldt < m
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 7, 4, 8, 3, 0),      # ldw < k
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, -1, 8, 3, 0),     # negative m
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, 4, -1, 3, 0),     # negative k
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, 4, 8, -1, 0),     # negative nv
    (None, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, 4, 8, 3, 0),        # null A
    (FAKE_A, 8, None, 8, FAKE_T, 4, FAKE_W, 8, 4, 8, 3, 0),        # null X
    (FAKE_A, 8, FAKE_X, 8, None, 4, FAKE_W, 8, 4, 8, 3, 0),        # null T
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, None, 8, 4, 8, 3, 0),        # null W
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, None, 8, 0, 8, 3, 0),        # m == 0 still writes W
    (FAKE_A, 0, FAKE_X, 0, None, 4, FAKE_W, 0, 4, 0, 3, 0),        # k == 0 still writes T
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, 4, 8, 3, -1),     # variant out of range
    (FAKE_A, 8, FAKE_X, 8, FAKE_T, 4, FAKE_W, 8, 4, 8, 3, len(NAMES)),
], ids=["lda<k", "ldx<k", "ldt<m", "ldw<k", "m<0", "k<0", "nv<0", "null-A", "null-X", "null-T", "null-W", "null-W-m0",
        "null-T-k0", "variant<0", "variant>=count"])
def test_argument_refusals_answer_invalid(args):
    A, lda, X, ldx, T, ldt, W, ldw, m, k, nv, v = args
    for variant in ([v] if v else range(len(NAMES))):
        rc = lib.mvg_gemv_ata_multi_variant(A, lda, X, ldx, T, ldt, W, ldw, m, k, nv, variant, None)
        assert rc == _lib.MVG_E_INVALID, NAMES[variant]
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi"), lib.mvg_last_error()
    if v == 0:
        assert lib.mvg_gemv_ata_multi(A, lda, X, ldx, T, ldt, W, ldw, m, k, nv, None) == _lib.MVG_E_INVALID
        assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi")


def test_nv_zero_and_both_sizes_zero_are_no_ops_even_on_null_operands():
    for v in range(len(NAMES)):
        assert lib.mvg_gemv_ata_multi_variant(None, 8, None, 0, None, 0, None, 0, 5, 8, 0, v, None) == _lib.MVG_OK
        assert lib.mvg_gemv_ata_multi_variant(None, 0, None, 0, None, 0, None, 0, 0, 0, 3, v, None) == _lib.MVG_OK
    assert lib.mvg_gemv_ata_multi(None, 8, None, 0, None, 0, None, 0, 5, 8, 0, None) == _lib.MVG_OK
    assert lib.mvg_gemv_ata_multi(None, 0, None, 0, None, 0, None, 0, 0, 0, 3, None) == _lib.MVG_OK


@pytest.mark.parametrize("v", FUSED, ids=lambda v: NAMES[v])
def test_an_explicit_fused_variant_is_refused_beyond_its_max_k(v):
    vals, out = _out()
    k = MAX_K[NAMES[v]]
    assert lib.mvg_gemv_ata_multi_plan(k, 100, k, 4, v, *out) == _lib.MVG_OK  # k == max_k: planned
    assert vals[2].value == k and vals[0].value * vals[1].value >= 100
    assert lib.mvg_gemv_ata_multi_plan(k + 1, 100, k + 1, 4, v, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi")
    rc = lib.mvg_gemv_ata_multi_variant(FAKE_A, k + 1, FAKE_X, k + 1, FAKE_T, 100, FAKE_W, k + 1, 100, k + 1, 4, v, None)
    assert rc == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi: k beyond the max_k")


def test_plan_refusals_and_a_grid_that_cannot_fit():
    _, out = _out()
    assert lib.mvg_gemv_ata_multi_plan(7, 4, 8, 3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_multi_plan(8, -4, 8, 3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_multi_plan(8, 4, -8, 3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_multi_plan(8, 4, 8, -3, 0, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_multi_plan(8, 4, 8, 3, -1, *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_multi_plan(8, 4, 8, 3, len(NAMES), *out) == _lib.MVG_E_INVALID
    assert lib.mvg_gemv_ata_multi_plan(8, 4, 8, 3, 0, None, None, None, None) == _lib.MVG_E_INVALID
    assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi")
    # two_pass (and auto, which is two_pass) on more column strips than one launch of the transposed
    # half holds; one vector alone goes through mvg_gemv_ata, whose own limit answers under this name
    K = 1 << 31
    for v in (0, TWO_PASS):
        for nv in (1, 2, 5):
            assert lib.mvg_gemv_ata_multi_plan(K, 4, K, nv, v, *out) == _lib.MVG_E_INVALID
            assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi")
            rc = lib.mvg_gemv_ata_multi_variant(FAKE_A, K, FAKE_X, K, FAKE_T, 4, FAKE_W, K, 4, K, nv, v, None)
            assert rc == _lib.MVG_E_INVALID
            assert lib.mvg_last_error().decode().startswith("mvg_gemv_ata_multi")


@pytest.mark.parametrize("m,k", [(1, 1), (31, 5), (1000, 257), (20001, 7), (65538, 3), (2048, 1024), (4_194_304, 64),
                                 (1 << 40, 512)])
def test_bands_cover_m_the_grid_fits_and_the_cut_does_not_depend_on_nv(m, k):
    for v in FUSED:
        if k > MAX_K[NAMES[v]]:
            continue
        NV = chains(v)
        band_rows, bands, max_k, group = mm.gemv_ata_multi_plan(k, m, k, NV, v)
        assert group == NV
        assert band_rows >= 32 and bands * band_rows >= m > (bands - 1) * band_rows, (NAMES[v], band_rows, bands)
        assert bands * threads(v) <= 1 << 31, (NAMES[v], band_rows, bands)  # gridDim.x * blockDim.x < 2^32
        assert max_k == MAX_K[NAMES[v]]
        for nv in (2, NV + 1, NV + 3, 5 * NV):
            assert mm.gemv_ata_multi_plan(k, m, k, nv, v) == (band_rows, bands, max_k, min(nv, NV)), (NAMES[v], nv)
        assert mm.gemv_ata_multi_plan(k + 16, m, k, NV, v) == (band_rows, bands, max_k, NV)  # nor on lda


def test_the_cut_is_the_one_vector_kernels_rule():
    """plan_ata per (workgroup size, fill): the 1024-thread forms cut like wgrow_w16_*, the 512-thread
    wave-per-row forms like wrow_w8_*."""
    ata = [lib.mvg_gemv_ata_variant_name(v).decode() for v in range(lib.mvg_gemv_ata_variant_count())]
    for m in (1, 1000, 20001, 65536, 524288, 4_194_304, 1 << 40):
        for v in FUSED:
            single = ata.index("wgrow_w16_c8_r2" if NAMES[v].startswith("wgrowm_w16") else "wrow_w8_c4_u8")
            assert mm.gemv_ata_multi_plan(64, m, 64, 2, v)[:2] == mm.gemv_ata_plan(64, m, 64, single)[:2], (NAMES[v], m)


def test_empty_problems_plan_no_bands():
    for v in FUSED:
        assert mm.gemv_ata_multi_plan(8, 0, 8, 4, v)[1] == 0


def _walk(m, k, nv, v):
    groups = []
    while nv > 0:
        band_rows, bands, max_k, g = mm.gemv_ata_multi_plan(k, m, k, nv, v)
        assert 1 <= g <= nv
        groups.append((g, band_rows, bands, max_k))
        nv -= g
    return groups


@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 7, 8, 9, 17])
def test_how_nv_vectors_are_cut_into_groups(nv):
    m, k = 5000, 200
    single = mm.gemv_ata_plan(k, m, k)
    for v in FUSED:
        NV = chains(v)
        want = [NV] * (nv // NV)
        if nv % NV == 1:
            want += [1]        # a single leftover vector: mvg_gemv_ata
        elif nv % NV:
            want += [nv % NV]  # a short group of the same kernel
        groups = _walk(m, k, nv, v)
        assert [g[0] for g in groups] == want, (NAMES[v], nv, groups)
        fused = mm.gemv_ata_multi_plan(k, m, k, NV, v)[:3]
        for g, *cut in groups:
            assert tuple(cut) == (single if g == 1 else fused), (NAMES[v], nv, g, cut)
    assert _walk(m, k, nv, TWO_PASS) == [(nv, 0, 0, INT64_MAX)]  # the pair takes every vector at once


def _auto_walk(m, k, nv, lda=None):
    """The automatic choice group by group: [(variant name, vectors)]; "mvg_gemv_ata" for one vector alone."""
    lda, out = lda or k, []
    while nv > 0:
        v = lib.mvg_gemv_ata_multi_auto_variant(lda, k, m, k, nv)
        g = mm.gemv_ata_multi_plan(lda, m, k, nv)[3]
        assert 1 <= g <= nv
        if nv == 1:
            assert mm.gemv_ata_multi_plan(lda, m, k, 1) == (*mm.gemv_ata_plan(lda, m, k), 1)
            out.append(("mvg_gemv_ata", 1))
        else:
            assert v == TWO_PASS or (chains(v) <= nv and g == chains(v))  # never more chains than vectors left
            out.append((NAMES[v], g))
        nv -= g
    return out


def test_the_groups_auto_produces_never_have_more_chains_than_vectors_left():
    for m, k in SWEPT + [(1000, 257), (1, 1), (20001, 7)]:
        for nv in range(1, 10):
            groups = _auto_walk(m, k, nv)
            assert sum(g for _, g in groups) == nv, (m, k, nv, groups)


def test_auto_pick_at_the_swept_shapes():
    """Pinned literally. No sweep has been kept yet (MEASUREMENTS §20): nothing is tuned, so the pick
    is two_pass at every shape, at a view's lda too, and one vector alone is mvg_gemv_ata."""
    for m, k in SWEPT:
        for nv in (2, 4, 8, 16):
            assert _auto_walk(m, k, nv) == [("two_pass", nv)], (m, k, nv)
            assert _auto_walk(m, k, nv, lda=k + 16) == [("two_pass", nv)], (m, k, nv)
        assert _auto_walk(m, k, 1) == [("mvg_gemv_ata", 1)]
