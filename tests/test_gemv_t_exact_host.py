"""mvg_gemv_t_exact and mvg_gemv_t_exact_multi without a GPU: the variant tables, the automatic
choice, every argument refusal (decided from the arguments alone, so fake pointers never reach a HIP
call), and a guard on the data of tests/test_gpu_gemv_t_exact.py: on its signed uniform inputs the
order of the sum shows in the bits, so a bit-for-bit comparison there does prove the order.
"""
import re

import numpy as np
import pytest

from matvec_mpi_multiplier_amd import _lib
from oracle import oracle
from test_gpu_gemv_t import SHAPES, signed

lib = _lib.lib
FAKE_A, FAKE_Z, FAKE_Y = 0x10000, 0x20000, 0x30000  # 16-B aligned, never dereferenced: every call below is refused
NVAR = lib.mvg_gemv_t_exact_variant_count()
NMVAR = lib.mvg_gemv_t_exact_multi_variant_count()
NAMES = [lib.mvg_gemv_t_exact_variant_name(v).decode() for v in range(NVAR)]
MNAMES = [lib.mvg_gemv_t_exact_multi_variant_name(v).decode() for v in range(NMVAR)]
STAGED = re.compile(r"tseqx_w(\d+)_c(\d+)_t(\d+)_b(\d+)$")
DIRECT = re.compile(r"tseq_c(\d+)_u(\d+)$")
FUSED = re.compile(r"tseqm_c(\d+)_u(\d+)_v(\d+)$")


def staged():
    """(variant, NW, SC, T, NB) of every staged form, read from its name."""
    return [(v,) + tuple(int(g) for g in STAGED.match(n).groups()) for v, n in enumerate(NAMES) if STAGED.match(n)]


def test_variant_tables():
    assert NAMES[0] == "auto" and NAMES[1] == "tseq_c64_u16", NAMES  # variant 1: the direct form that defines the result
    assert len(set(NAMES)) == NVAR and NVAR >= 3
    assert all(DIRECT.match(n) or STAGED.match(n) for n in NAMES[1:]), NAMES
    assert staged() and any(DIRECT.match(n) for n in NAMES[2:])
    assert {sc for _, _, sc, _, _ in staged()} >= {16, 32, 64, 128}  # the strip widths the issue asks to sweep
    assert MNAMES[:2] == ["auto", "separate"], MNAMES
    assert len(set(MNAMES)) == NMVAR
    assert all(FUSED.match(n) for n in MNAMES[2:]), MNAMES
    assert {int(FUSED.match(n).group(3)) for n in MNAMES[2:]} == {2, 4}
    for count, name in ((NVAR, lib.mvg_gemv_t_exact_variant_name), (NMVAR, lib.mvg_gemv_t_exact_multi_variant_name)):
        assert name(-1) == b"invalid" and name(count) == b"invalid"


SPREAD = [(1, 1, 1), (7, 3, 5), (16384, 16384, 16384), (16400, 16384, 16384), (8192, 65536, 8192),
          (32768, 65536, 32768), (512, 524288, 512), (64, 4194304, 64), (129, 4099, 129), (1 << 20, 64, 1 << 20)]


def test_auto_names_a_valid_variant():
    for lda, m, k in SPREAD:
        v = lib.mvg_gemv_t_exact_auto_variant(lda, m, k)
        assert 1 <= v < NVAR, (lda, m, k, v)
        for nv in (1, 2, 3, 4, 5, 9):
            mv = lib.mvg_gemv_t_exact_multi_auto_variant(lda, m, m, k, nv)
            assert 1 <= mv < NMVAR, (lda, m, k, nv, mv)
            if nv < 2:
                assert mv == 1, (lda, m, k, nv, mv)  # one vector: separate
            elif mv > 1:
                assert int(FUSED.match(MNAMES[mv]).group(3)) <= nv, (MNAMES[mv], nv)  # auto launches full groups


def test_auto_names_variant_1_where_a_staged_rule_is_broken():
    """An odd lda, and an lda beyond every staged form's 32-bit offset limit (2^29 / T)."""
    tmin = min(t for _, _, _, t, _ in staged())
    for _, m, k in SPREAD:
        for lda in (k | 1 if k | 1 >= k else k + 1, max(k + (k & 1), (1 << 29) // tmin)):
            assert lda >= k
            assert lib.mvg_gemv_t_exact_auto_variant(lda, m, k) == 1, (lda, m, k)


def test_auto_pick_is_not_tuned_outside_the_swept_classes():
    """Small and odd shapes were never swept: variant 1 / separate (the house rule)."""
    for lda, m, k in [(1, 1, 1), (7, 3, 5), (129, 4099, 129), (300, 70, 300)]:
        assert lib.mvg_gemv_t_exact_auto_variant(lda, m, k) == 1
        assert lib.mvg_gemv_t_exact_multi_auto_variant(lda, m, m, k, 4) == 1


BASIC = [
    ((FAKE_A, 7, FAKE_Z, FAKE_Y, 4, 8, 0), "lda<k"),
    ((FAKE_A, 8, FAKE_Z, FAKE_Y, -1, 8, 0), "m<0"),
    ((FAKE_A, 8, FAKE_Z, FAKE_Y, 4, -1, 0), "k<0"),
    ((None, 8, FAKE_Z, FAKE_Y, 4, 8, 0), "null-A"),
    ((FAKE_A, 8, None, FAKE_Y, 4, 8, 0), "null-z"),
    ((FAKE_A, 8, FAKE_Z, None, 4, 8, 0), "null-y"),
    ((FAKE_A, 8, FAKE_Z, None, 0, 8, 0), "null-y-m0"),
    ((FAKE_A, 8, FAKE_Z, FAKE_Y, 4, 8, -1), "variant<0"),
    ((FAKE_A, 8, FAKE_Z, FAKE_Y, 4, 8, NVAR), "variant>=count"),
]


def _refused(rc, prefix="mvg_gemv_t_exact"):
    assert rc == _lib.MVG_E_INVALID, rc
    assert lib.mvg_last_error().decode().startswith(prefix), lib.mvg_last_error()


@pytest.mark.parametrize("args", [a for a, _ in BASIC], ids=[i for _, i in BASIC])
def test_argument_refusals_answer_invalid(args):
    A, lda, z, y, m, k, v = args
    _refused(lib.mvg_gemv_t_exact_variant(A, lda, z, y, m, k, v, None))
    if v == 0:
        _refused(lib.mvg_gemv_t_exact(A, lda, z, y, m, k, None))
    elif v < 0 or v >= NVAR:
        return
    for w in range(1, NVAR):  # the same refusal from every variant
        _refused(lib.mvg_gemv_t_exact_variant(A, lda, z, y, m, k, w, None))


def test_k_zero_is_a_no_op_even_on_null_operands():
    assert lib.mvg_gemv_t_exact(None, 0, None, None, 5, 0, None) == _lib.MVG_OK
    for v in range(NVAR):
        assert lib.mvg_gemv_t_exact_variant(None, 0, None, None, 5, 0, v, None) == _lib.MVG_OK
    for v in range(NMVAR):
        assert lib.mvg_gemv_t_exact_multi_variant(None, 0, None, 5, None, 0, 5, 0, 3, v, None) == _lib.MVG_OK  # k == 0
        assert lib.mvg_gemv_t_exact_multi_variant(None, 8, None, 5, None, 8, 5, 8, 0, v, None) == _lib.MVG_OK  # nv == 0


@pytest.mark.parametrize("v,nw,sc,t,nb", staged(), ids=[NAMES[s[0]] for s in staged()])
def test_a_staged_form_is_refused_by_number_where_its_operand_rules_are_broken(v, nw, sc, t, nb):
    m, k = 4 * t, 2 * sc
    limit = (1 << 29) // t  # T rows of lda within the 32-bit per-lane byte offset
    for A, lda, z, why in [(FAKE_A, k + 1, FAKE_Z, "odd lda"), (FAKE_A + 8, k, FAKE_Z, "A 8 B off"),
                           (FAKE_A, k, FAKE_Z + 8, "z 8 B off"), (FAKE_A, limit, FAKE_Z, "lda at the limit"),
                           (FAKE_A, limit + 2, FAKE_Z, "lda beyond the limit")]:
        _refused(lib.mvg_gemv_t_exact_variant(A, lda, z, FAKE_Y, m, k, v, None))
        assert "staged" in lib.mvg_last_error().decode(), why


def test_more_column_strips_than_one_grid_holds():
    k = 1 << 34
    for v in range(NVAR):
        _refused(lib.mvg_gemv_t_exact_variant(FAKE_A, k, FAKE_Z, FAKE_Y, 4, k, v, None))
    assert "strips" in lib.mvg_last_error().decode() or "staged" in lib.mvg_last_error().decode()
    _refused(lib.mvg_gemv_t_exact(FAKE_A, k, FAKE_Z, FAKE_Y, 4, k, None))
    assert "strips" in lib.mvg_last_error().decode()
    # the widest k one grid of variant 1 holds is 64 * 2^31 / 64 columns: one more strip is refused
    _refused(lib.mvg_gemv_t_exact_variant(FAKE_A, (1 << 31) + 1, FAKE_Z, FAKE_Y, 4, (1 << 31) + 1, 1, None))
    for v in range(NMVAR):
        _refused(lib.mvg_gemv_t_exact_multi_variant(FAKE_A, k, FAKE_Z, 4, FAKE_Y, k, 4, k, 3, v, None),
                 "mvg_gemv_t_exact_multi")
        assert "strips" in lib.mvg_last_error().decode()


MULTI = [
    ((FAKE_A, 7, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, 0), "lda<k"),
    ((FAKE_A, 8, FAKE_Z, 3, FAKE_Y, 8, 4, 8, 3, 0), "ldz<m"),
    ((FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 7, 4, 8, 3, 0), "ldy<k"),
    ((FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, -1, 8, 3, 0), "m<0"),
    ((FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, -1, 3, 0), "k<0"),
    ((FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, -1, 0), "nv<0"),
    ((None, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, 0), "null-A"),
    ((FAKE_A, 8, None, 4, FAKE_Y, 8, 4, 8, 3, 0), "null-Z"),
    ((FAKE_A, 8, FAKE_Z, 4, None, 8, 4, 8, 3, 0), "null-Y"),
    ((FAKE_A, 8, FAKE_Z, 4, None, 8, 0, 8, 3, 0), "null-Y-m0"),
    ((FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, -1), "variant<0"),
    ((FAKE_A, 8, FAKE_Z, 4, FAKE_Y, 8, 4, 8, 3, NMVAR), "variant>=count"),
]


@pytest.mark.parametrize("args", [a for a, _ in MULTI], ids=[i for _, i in MULTI])
def test_multi_argument_refusals_answer_invalid(args):
    A, lda, Z, ldz, Y, ldy, m, k, nv, v = args
    _refused(lib.mvg_gemv_t_exact_multi_variant(A, lda, Z, ldz, Y, ldy, m, k, nv, v, None), "mvg_gemv_t_exact_multi")
    if v == 0:
        _refused(lib.mvg_gemv_t_exact_multi(A, lda, Z, ldz, Y, ldy, m, k, nv, None), "mvg_gemv_t_exact_multi")
        for w in range(1, NMVAR):
            _refused(lib.mvg_gemv_t_exact_multi_variant(A, lda, Z, ldz, Y, ldy, m, k, nv, w, None),
                     "mvg_gemv_t_exact_multi")


@pytest.mark.parametrize("m,k", [s for s in SHAPES if s[0] >= 64])
def test_the_gpu_tests_signed_data_tells_orders_apart(m, k):
    """numpy's A.T @ z (BLAS: blocked, fused, another order) against the oracle's chain on the
    signed uniform data of tests/test_gpu_gemv_t.py: at least half the columns differ in bits, so a
    kernel that summed in another order could not pass the bit-for-bit GPU test at this shape."""
    A, z, want, _ = signed(m, k)
    assert np.array_equal(want, oracle.multiply_std_rowwise(np.ascontiguousarray(A.T), z))
    other = A.T @ z
    differ = int(np.sum(other.view(np.uint64) != want.view(np.uint64)))
    print(f"{m}x{k}: {differ} of {k} columns differ in bits")
    assert 2 * differ >= k, (m, k, differ)


def _auto(lda, m, k):
    return NAMES[lib.mvg_gemv_t_exact_auto_variant(lda, m, k)]


def _mauto(m, k, nv):
    return MNAMES[lib.mvg_gemv_t_exact_multi_auto_variant(k, m, m, k, nv)]


def test_auto_pick_at_the_swept_shapes():
    """Pinned literally: the picks both kept runs support (profiles/r09/gemv_t_exact/, MEASUREMENTS §19)."""
    assert _auto(16384, 16384, 16384) == "tseqx_w4_c64_t32_b3"
    assert _auto(16400, 16384, 16384) == "tseqx_w4_c64_t32_b3"
    assert _auto(8192, 65536, 8192) == "tseqx_w4_c16_t64_b3"
    assert _auto(32768, 65536, 32768) == "tseqx_w4_c128_t16_b3"
    assert _auto(512, 524288, 512) == "tseqx_w4_c16_t64_b3"
    assert _auto(64, 4194304, 64) == "tseqx_w4_c16_t64_b3"
    for m, k in [(16384, 16384), (65536, 8192), (65536, 32768), (524288, 512), (4194304, 64)]:
        assert [_mauto(m, k, nv) for nv in (1, 2, 3, 4, 9)] == ["separate", "tseqm_c64_u32_v2", "tseqm_c64_u32_v2",
                                                                "tseqm_c64_u16_v4", "tseqm_c64_u16_v4"], (m, k)
    # outside what was swept: fewer rows, a narrower or wider k, a smaller or larger A
    for m, k in [(16383, 32768), (1 << 23, 32), (16384, 65536), (16384, 8192), (131072, 32768)]:
        assert _auto(k, m, k) == "tseq_c64_u16" and _mauto(m, k, 4) == "separate", (m, k)


def test_resolve_names_what_a_call_runs():
    """The pick on 16-B aligned operands; variant 1 where A or z is 8 bytes off or lda breaks the pick's rule."""
    m, k = 16384, 16384
    pick = lib.mvg_gemv_t_exact_auto_variant(k, m, k)
    assert pick > 1
    assert lib.mvg_gemv_t_exact_resolve_variant(FAKE_A, k, FAKE_Z, m, k) == pick
    assert lib.mvg_gemv_t_exact_resolve_variant(FAKE_A + 8, k, FAKE_Z, m, k) == 1
    assert lib.mvg_gemv_t_exact_resolve_variant(FAKE_A, k, FAKE_Z + 8, m, k) == 1
    assert lib.mvg_gemv_t_exact_resolve_variant(FAKE_A, k + 1, FAKE_Z, m, k) == 1
    assert lib.mvg_gemv_t_exact_resolve_variant(FAKE_A, 1 << 26, FAKE_Z, m, k) == 1
    assert lib.mvg_gemv_t_exact_resolve_variant(FAKE_A + 8, 300, FAKE_Z, 70, 300) == 1


def test_the_swept_range_hook():
    assert lib.mvg_debug_set_gemv_t_exact_swept(-1, 0) == _lib.MVG_E_INVALID
    assert _auto(600, 200, 600) == "tseq_c64_u16"
    try:
        assert lib.mvg_debug_set_gemv_t_exact_swept(64, 4096) == _lib.MVG_OK
        assert _auto(600, 200, 600) == "tseqx_w4_c16_t64_b3"
        assert _auto(8200, 70, 8200) == "tseqx_w4_c64_t32_b3"
        assert _auto(32768, 70, 32768) == "tseqx_w4_c128_t16_b3"
        assert _auto(601, 200, 600) == "tseq_c64_u16"  # odd lda
        assert _mauto(200, 600, 5) == "tseqm_c64_u16_v4"
        assert _auto(600, 63, 600) == "tseq_c64_u16"
    finally:
        assert lib.mvg_debug_set_gemv_t_exact_swept(0, 0) == _lib.MVG_OK
    assert _auto(600, 200, 600) == "tseq_c64_u16" and _auto(16384, 16384, 16384) == "tseqx_w4_c64_t32_b3"
