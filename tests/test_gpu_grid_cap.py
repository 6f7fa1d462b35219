"""The grid-cap branch of for_row_pieces (csrc/common.h): problems so tall that one launch would
pass HIP's grid limit go out as several launches over consecutive row ranges.

The three forms of the cap, as the launch code states them:
    tree (launch, gemv.hip) and multi (mvg_gemv_multi_variant):  (2^31 / threads) workgroups
    exact (mvg_gemv_exact_variant):                              2^32 / (64 * waves) - 1
    exact_multi (mvg_gemv_exact_multi_variant):                  2^31 / 64 - 1
times the form's rows per workgroup; threads, waves and rows come from the variant's name. With
k = 2 (k = 1 for the exact families) the cut is cheap to reach: rowblk_w16_r1_* is cut at 2^21
rows, 32 MiB of A. m = piece + 37, A from mvg_synth_fill_device.

Per variant: the whole y is bit-equal to the same variant called on consecutive ranges of 2^20
rows (one launch each; a row's sum does not depend on its piece); 40-row slices at row 0, across
the cut and at the ragged end match the oracle on oracle.synth_block (tree and multi within 1e-12,
the data being non-negative; the exact families bit for bit); 16 NaNs past the last row of every
vector survive. The row-pair form repeats at lda = 3, where its 16 spare workgroups of a full
piece own the rows past it. An explicit split-K variant with more row blocks than the grid holds
is refused before its workspace is allocated.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import max_rel
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle
from test_gpu_exact import _hip_runtime

pytestmark = pytest.mark.gpu
lib = _lib.lib
TOL = 1e-12          # relative, non-negative data (tests/test_gpu_parity.py)
BOUND = 1 << 25      # every tree and multi variant cut at or under this many rows is run
RANGE = 1 << 20      # rows per sub-range call
GUARD = 16
LIMIT_BYTES = 1 << 32  # the largest A or Y a template's smallest-piece variant may need
K_BLOCK = 256        # gemv.hip kBlock: the workgroup of the wave-owns-rows forms


def _names(count, name):
    return [name(v).decode() for v in range(count())]


TREE = _names(lib.mvg_gemv_variant_count, lib.mvg_gemv_variant_name)
MULTI = _names(lib.mvg_gemv_multi_variant_count, lib.mvg_gemv_multi_variant_name)
EXACT = _names(lib.mvg_gemv_exact_variant_count, lib.mvg_gemv_exact_variant_name)
EXACT_MULTI = _names(lib.mvg_gemv_exact_multi_variant_count, lib.mvg_gemv_exact_multi_variant_name)


def _num(name, key):
    return int(re.search(rf"_{key}(\d+)", name).group(1))


def tree_shape(name):
    """(threads, rows per workgroup) of a tree or multi variant, from its name."""
    head = name.split("_")[0]
    if head in ("vec", "scl", "mvec", "mxres"):  # wave-owns-rows: 4 waves, 64 / L groups of R rows each
        return K_BLOCK, (K_BLOCK // 64) * (64 // _num(name, "l")) * _num(name, "r")
    if head == "mlds":
        return K_BLOCK, (K_BLOCK // 64) * _num(name, "r")
    if head in ("rowblk", "mrow"):
        return 64 * _num(name, "w"), _num(name, "r")
    if head == "rowlines":
        return 64 * _num(name, "w"), 2
    assert head in ("mdma", "m16"), name
    return 64 * _num(name, "w"), 16 * _num(name, "r")


def tree_piece(name):
    threads, rows = tree_shape(name)
    return ((1 << 31) // threads) * rows


def exact_shape(name):
    """(waves, rows per workgroup) of an exact variant."""
    if name == "seq_scalar":
        return 1, 64
    if name.startswith(("seq_r", "seqx_r")):
        return 1, _num(name, "r")
    waves = _num(name, "n") if name.startswith(("hop8e_", "hopxl_")) else 1
    return waves, waves * 64 // _num(name, "l")


def short_row_cut(k, rows):
    """short_row_piece_rows (common.h): 1 GiB of the bytes read, never under 65536 rows."""
    return max((1 << 30) // (8 * k), 65536) // rows * rows


def exact_grid_cut(name):
    waves, rows = exact_shape(name)
    return ((1 << 32) // (64 * waves) - 1) * rows


def exact_multi_grid_cut(name):
    return ((1 << 31) // 64 - 1) * (64 // _num(name, "l"))


def under_bound_or_smallest(names, nv):
    """Every variant cut at <= BOUND rows, and for a kernel template with none the variant with
    the smallest cut, if its A (k = lda = 2) and Y stay under 4 GiB."""
    names = [n for n in names if n != "auto" and not n.endswith("_splitk")]
    picked = [n for n in names if tree_piece(n) <= BOUND]
    for head in sorted({n.split("_")[0] for n in names}):
        own = [n for n in names if n.split("_")[0] == head]
        if not any(n in picked for n in own):
            small = min(own, key=tree_piece)
            m = tree_piece(small) + 37
            if m * 2 * 8 < LIMIT_BYTES and nv * (m + GUARD) * 8 < LIMIT_BYTES:
                picked.append(small)
    return picked


TREE_CASES = under_bound_or_smallest(TREE, 1)
MULTI_CASES = under_bound_or_smallest(MULTI, 2)
# the exact forms whose grid cut lies below their 1 GiB short-row cut at k = 1: established here
EXACT_CASES = [n for n in EXACT[1:] if exact_grid_cut(n) < short_row_cut(1, exact_shape(n)[1])]
EXACT_MULTI_CASES = [n for n in EXACT_MULTI if n.startswith("hopm_") and
                     exact_multi_grid_cut(n) < short_row_cut(1, 64 // _num(n, "l"))]


def test_the_lists_are_what_the_launch_code_implies():
    """Not vacuous: every family's list is non-empty and holds what the tables say."""
    assert tree_piece("rowblk_w16_r1_u4") == 1 << 21 and tree_piece("vec_l64_r1_u4_nt1_o5") == 1 << 25
    assert tree_piece("rowlines_w8_u4_x0") == 1 << 23 and tree_piece("mrow_w4_r4_u1") == 1 << 25
    assert tree_piece("mdma_r1_t16_b3_w8") == 1 << 26 and tree_piece("m16_r1_t16_b2_w4_s5") == 1 << 27
    assert len(TREE_CASES) >= 30 and len(MULTI_CASES) >= 12, (len(TREE_CASES), len(MULTI_CASES))
    heads = lambda names: {n.split("_")[0] for n in names}  # noqa: E731
    assert heads(TREE_CASES) == {"vec", "scl", "rowblk", "rowlines"}  # every template of the table
    assert heads(MULTI_CASES) == {"mvec", "mrow", "mlds", "mxres", "mdma", "m16"}
    assert all(n in TREE_CASES for n in TREE if n.startswith("rowlines_"))
    assert all(n in TREE_CASES for n in TREE if n.startswith("rowblk_") and not n.endswith("_splitk") and
               _num(n, "w") >= 4 and _num(n, "r") <= _num(n, "w"))
    assert any(n.endswith("_xcd") for n in TREE_CASES) and any("_xq" in n for n in TREE_CASES)  # the XCD remaps
    # the 32-lane exact forms and wider; the 16-lane multi forms and wider
    assert EXACT_CASES == [n for n in EXACT if re.match(r"hop8?_l(32|64)_", n)] and len(EXACT_CASES) == 4
    assert EXACT_MULTI_CASES == [n for n in EXACT_MULTI if re.match(r"hopm_l(16|32)_", n)] and len(EXACT_MULTI_CASES) == 8
    assert exact_grid_cut("hop_l64_w8_u4") == (1 << 26) - 1 and exact_multi_grid_cut("hopm_l32_w8_u2_v2") == (1 << 26) - 2


# ------------------------------------------------------------------ the runs
_hip = None


def nan_fill(ptr, doubles):
    global _hip
    if _hip is None:
        _hip = _hip_runtime()
        _hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    assert _hip.hipMemset(ptr, 0xFF, 8 * doubles) == 0 and _hip.hipDeviceSynchronize() == 0


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def tall(family, name, piece, k, lda):
    """m = piece + 37 rows of synthetic A: the whole call against sub-range calls, slices against
    the oracle, the guard past every vector."""
    exact = family.startswith("exact")
    nv = 2 if family.endswith("multi") else 1
    v = {"tree": TREE, "multi": MULTI, "exact": EXACT, "exact_multi": EXACT_MULTI}[family].index(name)
    m = piece + 37
    ldy = m + GUARD
    X = oracle.synth(nv, k, 4242)
    # (32 spare doubles behind A and X: a form that reads whole 16-B pairs or 128-B lines stays inside)
    dA, dX = mm.DeviceBuffer(m * lda + 32), mm.DeviceBuffer(nv * k + 32).upload(X)
    dY, dZ = mm.DeviceBuffer(nv * ldy), mm.DeviceBuffer(nv * ldy)

    def call(y, r0, rows):
        a = dA.ptr + 8 * r0 * lda
        if family == "tree":
            return lib.mvg_gemv_variant(a, lda, dX.ptr, y + 8 * r0, rows, k, v, None)
        if family == "exact":
            return lib.mvg_gemv_exact_variant(a, lda, dX.ptr, y + 8 * r0, rows, k, v, None)
        fn = lib.mvg_gemv_multi_variant if family == "multi" else lib.mvg_gemv_exact_multi_variant
        return fn(a, lda, dX.ptr, k, y + 8 * r0, ldy, rows, k, nv, v, None)

    try:
        _lib.check(lib.mvg_synth_fill_device(dA.ptr, lda, m, lda, 0, 0, lda, 42, None), "fill A")
        nan_fill(dY.ptr, nv * ldy)
        nan_fill(dZ.ptr, nv * ldy)
        _lib.check(call(dY.ptr, 0, m), name)  # one call: the library cuts it at `piece`
        for r0 in range(0, m, RANGE):         # the test's own cuts: one launch each
            assert min(RANGE, m - r0) <= piece
            _lib.check(call(dZ.ptr, r0, min(RANGE, m - r0)), name)
        sync()
        y, z = dY.download().reshape(nv, ldy), dZ.download().reshape(nv, ldy)
        where = (name, m, k, lda)
        assert np.isnan(y[:, m:]).all() and np.isnan(z[:, m:]).all(), where  # the guard past every vector
        assert not np.isnan(y[:, :m]).any(), (where, np.argwhere(np.isnan(y[:, :m]))[:4])
        same = y[:, :m].view(np.uint64) == z[:, :m].view(np.uint64)
        assert same.all(), (where, "whole call differs from the sub-range calls at", np.argwhere(~same)[:4])
        # the start; both sides of the cut, which with 37 rows past it is the ragged end too
        assert piece - 3 == m - 40
        for r0 in (0, piece - 3):
            Ar = oracle.synth_block(r0, 40, 0, k, lda, 42)
            for j in range(nv):
                want = oracle.multiply_std_rowwise(Ar, X[j])
                got = y[j, r0:r0 + 40]
                if exact:
                    assert np.array_equal(got, want), (where, r0, j)
                else:
                    print(f"{name} rows {r0}..: max rel {max_rel(got, want):.3e}")
                    assert max_rel(got, want) <= TOL, (where, r0, j)
    finally:
        for b in (dA, dX, dY, dZ):
            b.free()


@pytest.mark.parametrize("name", TREE_CASES)
def test_tree_past_the_grid_cut(name):
    tall("tree", name, tree_piece(name), 2, 2)


@pytest.mark.parametrize("name", [n for n in TREE_CASES if n.startswith("rowlines_")])
def test_row_pair_form_past_the_grid_cut_with_rows_off_the_lines(name):
    """lda = 3: rows start mid-line, p = 16 row pairs to a block, and a full piece's 16 spare
    workgroups (theirs are the rows past the piece: clamped loads, no store) are launched."""
    tall("tree", name, tree_piece(name), 2, 3)


@pytest.mark.parametrize("name", MULTI_CASES)
def test_multi_past_the_grid_cut(name):
    tall("multi", name, tree_piece(name), 2, 2)


@pytest.mark.parametrize("name", EXACT_CASES)
def test_exact_past_the_grid_cut(name):
    piece = exact_grid_cut(name)
    assert piece < short_row_cut(1, exact_shape(name)[1])  # the grid cap is the one that cuts
    tall("exact", name, piece, 1, 2)


@pytest.mark.parametrize("name", EXACT_MULTI_CASES)
def test_exact_multi_past_the_grid_cut(name):
    piece = exact_multi_grid_cut(name)
    assert piece < short_row_cut(1, 64 // _num(name, "l"))
    tall("exact_multi", name, piece, 1, 2)


def test_split_k_refuses_a_grid_it_cannot_launch():
    """An explicit split-K variant launches all its row blocks at once: more of them than
    2^31 / threads is MVG_E_INVALID, before the workspace is allocated and with y untouched."""
    split = [n for n in TREE if n.endswith("_splitk")]
    assert len(split) >= 5
    k = lda = 2  # shorter than a chunk: one K range, so the row blocks alone make the grid
    ms = {n: ((1 << 31) // tree_shape(n)[0]) * tree_shape(n)[1] + 1 for n in split}
    m_max = max(ms.values())
    dA, dx, dy = mm.DeviceBuffer(m_max * lda), mm.DeviceBuffer(k + 32).upload(oracle.synth(1, k, 4242)[0]), mm.DeviceBuffer(m_max)
    try:
        _lib.check(lib.mvg_synth_fill_device(dA.ptr, lda, m_max, lda, 0, 0, lda, 42, None), "fill A")
        nan_fill(dy.ptr, m_max)
        for n in split:
            rc = lib.mvg_gemv_variant(dA.ptr, lda, dx.ptr, dy.ptr, ms[n], k, TREE.index(n), None)
            assert rc == _lib.MVG_E_INVALID and b"split-K grid too large" in lib.mvg_last_error(), (n, rc)
        sync()
        assert np.isnan(dy.download()).all()
    finally:
        for b in (dA, dx, dy):
            b.free()
