"""The wide views (tests/wide_views.py) on the CPU: their threshold tables, the truncation
model, and the library's own limits on both sides of each limit view.

No device: the arena is a SparseImage (written ranges, NaN elsewhere), the GEMV numpy / the
oracle, and the library is asked only through calls that launch nothing (the dispatch's
*_auto_variant calls, and explicit variants on fake pointers that are refused as arguments).
"""
import numpy as np
import pytest

import adversarial_cases as AC
import gpu_guarded as G
import wide_views as W
from matvec_mpi_multiplier_amd import _lib
from oracle import oracle

lib = _lib.lib
SIGNED_TOL = 1e-13  # tests/test_gpu_adversarial.py: times sum_j |a_ij x_j|

# the table of the module's docstring
TABLE = {
    "LIMIT_A": (33, 65, None, None),
    "LIMIT_A64": (65, None, None, None),
    "LIMIT_A16": (17, 33, None, None),
    "FAR_A": (4, 8, 32, 64),
    "FAR_A_ODD": (5, 9, 33, 65),
    "FAR_A_OFF8": (4, 8, 32, 64),
    "LIMIT_X16": (None, None, None, None),
    "LIMIT_X8": (None, None, None, None),
    "FAR_X": (1, 2, 8, None),
    "FAR_Y": (1, 2, 8, None),
    "FAR_PANELS": (1, 1, 4, 8),
}
# The truncations a view can show are the thresholds it crosses, column by column: all four on
# the far views of A and on the panels; three on FAR_X and FAR_Y (16 vectors 2^28 apart end at
# 15 * 2^28 elements, under 2^32: no geometry of at most 16 vectors inside the arena reaches it);
# on LIMIT_A and LIMIT_A16 the two of the byte offset, on LIMIT_A64 the signed one; none on the
# LIMIT_X views, which sit under 2^31 bytes by construction (what they test is that the kernels
# take the largest stride the host lets through).
SHOWS = {name: tuple(t for t, first in zip(W.TRUNCATIONS, row) if first is not None) for name, row in TABLE.items()}
assert all(len(SHOWS[v.name]) == 4 for v in (W.FAR_A, W.FAR_A_ODD, W.FAR_A_OFF8, W.FAR_PANELS))
assert SHOWS["FAR_X"] == SHOWS["FAR_Y"] == ("int32 bytes", "uint32 bytes", "int32 elements")
assert SHOWS["LIMIT_A"] == SHOWS["LIMIT_A16"] == ("int32 bytes", "uint32 bytes")
assert SHOWS["LIMIT_A64"] == ("int32 bytes",) and SHOWS["LIMIT_X16"] == SHOWS["LIMIT_X8"] == ()


@pytest.mark.parametrize("view", W.VIEWS, ids=repr)
def test_thresholds_are_what_the_docstring_says(view):
    assert tuple(view.thresholds().values()) == TABLE[view.name]
    assert f"    {view.name} " in W.__doc__
    # the arithmetic itself: the vector before each threshold is under it, the one named is not
    for (label, first), (scale, limit) in zip(view.thresholds().items(), ((8, 1 << 31), (8, 1 << 32), (1, 1 << 31), (1, 1 << 32))):
        if first is None:
            assert (view.nvec - 1) * view.ld * scale < limit, label
        else:
            assert first * view.ld * scale >= limit > (first - 1) * view.ld * scale and first < view.nvec, label
    # every view fits the arena with its widest payload and a fringe on either side
    widest = W.M * 32 if view is W.FAR_PANELS else 1031
    assert W.default_base((view.nvec - 1) * view.ld + widest + view.shift) >= 1 << 20


def test_limit_views_sit_one_step_under_the_host_checks():
    # LIMIT_A: row 63 of the first 64-row tile is past 2^31 bytes and under 2^32
    off = 63 * W.LIMIT_A.ld * 8
    assert off == 4227857424 and (1 << 31) < off < (1 << 32)
    assert W.LIMIT_A.ld + 2 == 1 << 23 and W.LIMIT_A.ld % 2 == 0
    # 32 rows of it are the most the DMA multi forms' 2^31 bytes hold; the 64-row forms take half
    assert 32 * W.LIMIT_A.ld * 8 < (1 << 31) <= 32 * (W.LIMIT_A.ld + 2) * 8
    assert 16 * W.LIMIT_X16.ld * 8 == (1 << 31) - 256 and 8 * W.LIMIT_X8.ld * 8 == (1 << 31) - 128
    assert 64 * W.LIMIT_A64.ld * 8 == (1 << 31) - 1024 and 16 * W.LIMIT_A16.ld * 8 == (1 << 31) - 256


@pytest.mark.parametrize("view", W.VIEWS, ids=repr)
def test_truncations_move_a_payload_vector_onto_payload_or_fill(view):
    for trunc in W.TRUNCATIONS:
        moved = W.moved(view, trunc)
        assert bool(moved) == (trunc in SHOWS[view.name]), (view, trunc, moved[:4])
        n = 130
        payload = np.arange(view.nvec * n, dtype=np.float64).reshape(view.nvec, n) + 1.0
        got = W.gather(W.place(view, payload), view, n, trunc)
        for v in range(view.nvec):
            if v not in moved:
                assert np.array_equal(got[v], payload[v]), (view, trunc, v)
                continue
            # another vector's payload (whole or in part) or NaN fill, never its own
            assert not np.array_equal(got[v], payload[v]), (view, trunc, v)
            live = got[v][~np.isnan(got[v])]
            assert np.isin(live, payload).all() and not np.isin(live, payload[v]).any(), (view, trunc, v)
    if view is W.FAR_A:  # the power-of-two stride: row 8's truncated byte offset is row 0's
        assert W.TRUNCATIONS["uint32 bytes"](view.offset(8)) == 0 == W.TRUNCATIONS["int32 bytes"](view.offset(8))
        assert W.TRUNCATIONS["uint32 elements"](view.offset(64)) == 0


def _tree_ok(A, X, want):
    scale = (np.abs(A) @ np.abs(X).T).T
    return lambda got: np.abs(got - want) <= SIGNED_TOL * scale


def _failures(img, lay, compare):
    return G.check_image(img, lay, compare, "model")


@pytest.mark.parametrize("view", W.A_VIEWS, ids=repr)
def test_checker_tells_every_truncation_of_a_row_offset(view):
    """A numpy GEMV over the sparse image of a wide A, its row offsets truncated: the exact and
    the tolerance checkers pass the right one and fail each truncation the view can show."""
    k = 300
    A, X = AC.payload(W.M, k, 1, sign=True)
    want = oracle.multiply_std_rowwise(A, X[0])[None, :]
    img = W.place(view, A, base=1 << 26)
    lay = G.Layout(1, W.M, W.M + 3, nvec=2)
    for trunc in (None,) + tuple(W.TRUNCATIONS):
        rows = W.gather(img, view, k, trunc, base=1 << 26)
        y = np.array([oracle.multiply_std_rowwise(rows[i:i + 1], X[0])[0] for i in range(W.M)])
        bad_exact = _failures(lay.image(y[None, :]), lay, G.exact_ok(want))
        bad_tree = _failures(lay.image(y[None, :]), lay, _tree_ok(A, X, want))
        shown = trunc in SHOWS[view.name]
        assert bool(bad_exact) == bool(bad_tree) == shown, (view, trunc, bad_exact[:2])
        if shown:  # exactly the moved rows
            assert len(bad_exact) == len(bad_tree) == len(W.moved(view, trunc)), (view, trunc)


@pytest.mark.parametrize("view", (W.FAR_X, W.LIMIT_X16, W.LIMIT_X8), ids=repr)
def test_checker_tells_every_truncation_of_a_vector_offset_of_x(view):
    k, nv = 130, view.nvec
    A, X = AC.payload(W.M, k, nv, sign=True)
    want = np.stack([oracle.multiply_std_rowwise(A, X[v]) for v in range(nv)])
    img = W.place(view, X, base=1 << 28)
    lay = G.Layout(nv, W.M, W.M + 3, nvec=nv + 1)
    for trunc in (None,) + tuple(W.TRUNCATIONS):
        Xr = W.gather(img, view, k, trunc, base=1 << 28)
        y = np.stack([oracle.multiply_std_rowwise(A, Xr[v]) for v in range(nv)])
        for compare in (G.exact_ok(want), _tree_ok(A, X, want)):
            bad = _failures(lay.image(y), lay, compare)
            assert bool(bad) == (trunc in SHOWS[view.name]), (view, trunc, bad[:2])


def test_checker_tells_every_truncation_of_a_vector_offset_of_y():
    """Stores with a truncated vector offset land in the payload of vector 0 or 1, in a fringe or
    in the fill: the payload-plus-fringe image of the wide Y shows each."""
    view, nv = W.FAR_Y, W.FAR_Y.nvec
    A, X = AC.payload(W.M, 130, nv, sign=True)
    want = np.stack([oracle.multiply_std_rowwise(A, X[v]) for v in range(nv)])
    for trunc in (None,) + tuple(W.TRUNCATIONS):
        img, lay = W.operand_image(W.scatter(view, want, trunc, base=1 << 28), view, W.M, base=1 << 28)
        bad = _failures(img, lay, G.exact_ok(want))
        assert bool(bad) == (trunc in SHOWS[view.name]), (trunc, bad[:2])
        if bad:  # the moved vectors are still NaN where they belong ...
            moved = W.moved(view, trunc)
            assert all(any(f"wrong value at vector {v} row" in b for b in bad) for v in moved), bad[:4]
            if trunc.startswith("uint32 bytes"):  # ... and were stored over vectors 0 and 1
                assert any("wrong value at vector 0 row" in b for b in bad) and \
                    any("wrong value at vector 1 row" in b for b in bad), bad[:4]


def test_checker_tells_every_truncation_of_a_panel_offset():
    view, P, k = W.FAR_PANELS, 16, W.PANEL_K
    A, X = AC.payload(W.M, k, 1, sign=True)
    want = oracle.multiply_std_rowwise(A, X[0])[None, :]
    panels = np.full((view.nvec, W.M, P), np.nan)
    for p in range(view.nvec):
        w = min(P, k - p * P)
        panels[p, :, :w] = A[:, p * P:p * P + w]
    assert np.isnan(panels[-1, :, 2:]).all() and not np.isnan(panels[-1, :, :2]).any()  # the last one: 2 columns
    img = W.place(view, panels.reshape(view.nvec, W.M * P), base=1 << 27)
    lay = G.Layout(1, W.M, W.M + 3, nvec=2)
    for trunc in (None,) + tuple(W.TRUNCATIONS):
        got = W.gather(img, view, W.M * P, trunc, base=1 << 27).reshape(view.nvec, W.M, P)
        rows = np.concatenate([got[p] for p in range(view.nvec)], axis=1)[:, :k]
        y = oracle.multiply_std_rowwise(np.ascontiguousarray(rows), X[0])[None, :]
        bad = _failures(lay.image(y), lay, G.exact_ok(want))
        assert bool(bad) == (trunc in SHOWS[view.name]), (trunc, bad[:2])


# ------------------------------------------------------------------ the library's limits
def _names(count, name):
    return [name(v).decode() for v in range(count())]


def test_limit_views_agree_with_the_exact_dispatch_and_its_refusals():
    """lda < 2^23 for the LDS-DMA exact forms (operands_ok): the dispatch takes one at the largest
    lda a multiple of 16 under it and steps aside at 2^23; every explicit LDS-DMA variant takes the
    argument check's answer at 2^23 (fake, 16-B aligned pointers: the alignment check passes, the
    limit answers, nothing is launched) and no other form is refused there."""
    names = _names(lib.mvg_gemv_exact_variant_count, lib.mvg_gemv_exact_variant_name)
    auto = lambda lda: names[lib.mvg_gemv_exact_auto_variant(lda, 32768, 4096)]  # noqa: E731
    assert W.lds_dma_exact(auto((1 << 23) - 16)) and auto(1 << 23).startswith("hop")
    assert (1 << 23) - 16 <= W.LIMIT_A.ld < 1 << 23
    fake = 1 << 20
    lds = [v for v, n in enumerate(names) if W.lds_dma_exact(n)]
    assert len(lds) >= 11
    for v in lds:
        assert W.refuses("exact", names[v], 1 << 23) and not W.refuses("exact", names[v], W.LIMIT_A.ld)
        assert lib.mvg_gemv_exact_variant(fake, 1 << 23, fake, fake, W.M, 300, v, None) == _lib.MVG_E_INVALID, names[v]
        assert b"lda < 2^23" in lib.mvg_last_error()
        # 8 bytes off, or an odd lda under the limit: the alignment check's answer
        assert lib.mvg_gemv_exact_variant(fake + 8, W.LIMIT_A.ld, fake, fake, W.M, 300, v, None) == _lib.MVG_E_INVALID
        assert lib.mvg_gemv_exact_variant(fake, W.LIMIT_A.ld - 1, fake, fake, W.M, 300, v, None) == _lib.MVG_E_INVALID
    for n in names[1:]:
        if not W.lds_dma_exact(n):
            assert not W.refuses("exact", n, 1 << 26), n


def test_limit_views_agree_with_the_multi_dispatch_and_its_refusals():
    """dma_ok: rows_per_block * lda * 8 < 2^31 and nvec * ldx * 8 < 2^31 (nvec 8, or 16 for the
    m16_* forms), rows per workgroup from the names."""
    names = _names(lib.mvg_gemv_multi_variant_count, lib.mvg_gemv_multi_variant_name)
    auto = lambda lda, ldx, nv: names[lib.mvg_gemv_multi_auto_variant(lda, ldx, 16384, 16384, nv)]  # noqa: E731
    # the dispatch's picks are 32-row forms: LIMIT_A is their last lda, 2^23 is past it
    assert auto(W.LIMIT_A.ld, 16384, 8) == "mdma_r2_t16_b2_w4_s5" and W.dma_rows("mdma_r2_t16_b2_w4_s5") == 32
    assert not auto(1 << 23, 16384, 8).startswith(("mdma", "m16"))
    assert auto(W.LIMIT_A.ld, 16384, 16) == "m16_r2_t16_b2_w4_s5" and not auto(1 << 23, 16384, 16).startswith("m16")
    # ldx: 8 vectors up to LIMIT_X8, 16 up to LIMIT_X16
    assert auto(16384, W.LIMIT_X8.ld, 8).startswith("mdma") and not auto(16384, 1 << 25, 8).startswith("mdma")
    assert auto(16384, W.LIMIT_X16.ld, 16).startswith("m16") and not auto(16384, 1 << 24, 16).startswith("m16")
    assert auto(16384, W.LIMIT_X8.ld, 16).startswith("mdma")  # two passes of 8 where 16 do not fit
    fake = 1 << 20
    dma = [v for v, n in enumerate(names) if W.dma_rows(n)]
    assert len(dma) == sum(n.startswith(("mdma_", "m16_")) for n in names) >= 22
    call = lambda v, lda, ldx: lib.mvg_gemv_multi_variant(fake, lda, fake, ldx, fake, W.M, W.M, 130, 8, v, None)  # noqa: E731
    for v in dma:
        n, rows = names[v], W.dma_rows(names[v])
        assert rows in (16, 32, 64), n
        lda_limit = (1 << 28) // rows  # rows * lda * 8 < 2^31
        ldx_limit = (1 << 24) if n.startswith("m16_") else (1 << 25)
        assert W.dma_ok(n, lda_limit - 2, ldx_limit - 2) and not W.dma_ok(n, lda_limit, 132) and not W.dma_ok(n, 132, ldx_limit)
        assert call(v, lda_limit, 132) == _lib.MVG_E_INVALID and b"too large for the DMA variant" in lib.mvg_last_error(), n
        assert call(v, 132, ldx_limit) == _lib.MVG_E_INVALID and b"too large for the DMA variant" in lib.mvg_last_error(), n
        assert call(v, lda_limit - 1, 132) == _lib.MVG_E_INVALID and b"even lda/ldx" in lib.mvg_last_error(), n
        # the views: LIMIT_A is taken by the 16- and 32-row forms, LIMIT_X16 by all, LIMIT_X8 by the 8-vector ones
        assert W.refuses("multi", n, W.LIMIT_A.ld, 132) == (rows == 64), n
        # and each form's own last lda is one of the three limit views of A
        own = {64: W.LIMIT_A64, 32: W.LIMIT_A, 16: W.LIMIT_A16}[rows]
        assert own.ld == lda_limit - 2 and not W.refuses("multi", n, own.ld, 132), n
        assert W.refuses("multi", n, W.LIMIT_A16.ld, 132) == (rows > 16) and not W.refuses("multi", n, W.LIMIT_A64.ld, 132), n
        assert not W.refuses("multi", n, 132, W.LIMIT_X16.ld), n
        assert W.refuses("multi", n, 132, W.LIMIT_X8.ld) == n.startswith("m16_"), n
        assert W.refuses("multi", n, 1 << 26, 132) and W.refuses("multi", n, 132, 1 << 28), n
    for n in names[1:]:
        if not W.dma_rows(n):
            assert not W.refuses("multi", n, 1 << 26, 1 << 28), n


def test_every_variant_runs_on_a_far_view_and_every_32_bit_form_on_its_limit_view():
    """The coverage the GPU module (tests/test_gpu_wide_views.py) asserts run by run, from the
    same predicates: no variant is refused on every far layout, and the forms with 32-bit offsets
    run on a limit view."""
    for family, k in (("tree", 300), ("exact", 300), ("multi", 130), ("exact_multi", 300)):
        names = set(W.family_names(family))
        far_a = set().union(*(W.live_names(family, v, "A", k) for v in (W.FAR_A, W.FAR_A_ODD, W.FAR_A_OFF8)))
        far_x = set(W.live_names(family, W.FAR_X, "X", k))
        rest = names - far_a
        if family == "exact":  # the LDS-DMA forms: far x only (lda < 2^23), and LIMIT_A
            assert rest == {n for n in names if W.lds_dma_exact(n)} and rest <= far_x
            assert rest <= set(W.live_names(family, W.LIMIT_A, "A", k))
        elif family == "multi":  # the DMA forms refuse every far stride; they run far in Y, and at their limits
            assert rest == {n for n in names if W.dma_rows(n)} and not rest & far_x
            at_limit = set(W.live_names(family, W.LIMIT_A, "A", k)) | set(W.live_names(family, W.LIMIT_X16, "X", k))
            assert rest <= at_limit
            assert {n for n in rest if n.startswith("mdma_")} <= set(W.live_names(family, W.LIMIT_X8, "X", k))
        else:
            assert not rest
