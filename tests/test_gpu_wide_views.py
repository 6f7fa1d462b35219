"""Every kernel on wide views: a row, a vector or a panel 2^31 .. 2^35 bytes from its operand's
base, and the forms with deliberate 32-bit per-lane offsets at the largest strides their host
checks let through (tests/wide_views.py: the arena, the views and what each crosses;
tests/test_wide_views_host.py: the views can show every truncation).

One operand is wide at a time, the others are ordinary guarded images (tests/gpu_guarded.py).
m = 67; k = 300 for the tree, exact and exact_multi families (two or more tiles of every LDS form
plus a tail), k = 130 for multi (four 32-column DMA tiles plus a 2-column tail; also 1030 on
LIMIT_A) and for the panels (9 panels of 16 columns, the last 2 wide). The exact families are
compared bit for bit with oracle.multiply_std_rowwise, tree and multi held to the signed-data bar
of tests/test_gpu_adversarial.py (1e-13 x sum |a x|), and no store may land outside y. A form that
refuses a layout must return MVG_E_INVALID and leave the NaN-filled y alone.

Every test asserts which forms ran and which refused against wide_views.live_names, so a form that
silently stopped running here fails the test; test_wide_views_host.py shows from the same
predicates that every variant runs on a far view and every 32-bit-offset form on a limit view.
"""
import functools

import numpy as np
import pytest

import adversarial_cases as AC
import gpu_guarded as G
import wide_views as W
from matvec_mpi_multiplier_amd import _lib
from test_gpu_adversarial import reference, tree_ok

pytestmark = pytest.mark.gpu
lib = _lib.lib
M = W.M
NVS = (1, 3, 8, 16)
X_PICKS = (0, 2, 8, 15)  # the vectors of a wide X fed to the single-vector families
VECTOR_FAMILIES = ("multi", "exact_multi")
EXACT = ("exact", "exact_multi", "panels")
FAMILIES = ("tree", "exact", "multi", "exact_multi")


@pytest.fixture(scope="module")
def arena():
    a = W.Arena()
    yield a
    a.free()


@functools.lru_cache(maxsize=None)
def data(k):
    """A (67 x k), X (16 x k), both signed, and the oracle's Y (16 x 67): made once, never changed."""
    A, X = AC.payload(M, k, 16, sign=True)
    want = reference(A, X)
    for a in (A, X, want):
        a.setflags(write=False)
    return A, X, want


def ks_for(family, view):
    if family != "multi":
        return (300,)
    return (130, 1030) if view is W.LIMIT_A else (130,)  # the other two limit views: the tiles and the tail alone


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


class Call:
    """One product's operands as addresses and strides; `Y` is the result operand (a guarded
    image or a WideOperand: both have ptr, lay and image())."""

    def __init__(self, A, lda, X, ldx, Y, ldy, m, k, nv):
        self.A, self.lda, self.X, self.ldx, self.Y, self.ldy, self.m, self.k, self.nv = A, lda, X, ldx, Y, ldy, m, k, nv

    def run(self, family, v):
        """Variant v into a NaN-filled Y: the return code and Y's image."""
        if isinstance(self.Y, W.WideOperand):
            self.Y.poison()
        else:
            self.Y.fill()
        a = self
        if family == "tree":
            rc = lib.mvg_gemv_variant(a.A, a.lda, a.X, a.Y.ptr, a.m, a.k, v, None)
        elif family == "exact":
            rc = lib.mvg_gemv_exact_variant(a.A, a.lda, a.X, a.Y.ptr, a.m, a.k, v, None)
        elif family == "multi":
            rc = lib.mvg_gemv_multi_variant(a.A, a.lda, a.X, a.ldx, a.Y.ptr, a.ldy, a.m, a.k, a.nv, v, None)
        else:
            assert family == "exact_multi"
            rc = lib.mvg_gemv_exact_multi_variant(a.A, a.lda, a.X, a.ldx, a.Y.ptr, a.ldy, a.m, a.k, a.nv, v, None)
        sync()
        return rc, self.Y.image()


def ok_for(family, A, X, want):
    return G.exact_ok(want) if family in EXACT else tree_ok(A, X, want, True)


def padded(want, lay):
    """want (nv x m) as the payload of Y's layout: the vectors past nv and the rows past m NaN."""
    full = np.full((lay.nv, lay.n), np.nan)
    full[:want.shape[0], :want.shape[1]] = want
    return full


def run_all(family, call, want, compare_for, refused_if, where):
    """Every variant of the family on `call`: a refusing form says MVG_E_INVALID and leaves Y all
    NaN; every other form gives `want` (nv x m) and stores nowhere else. Returns the names that
    ran and those that refused."""
    ran, refused = [], []
    lay = call.Y.lay
    for v, name in enumerate(W.family_names(family)):
        rc, img = call.run(family, v)
        if refused_if(name):
            assert rc == _lib.MVG_E_INVALID, (name, where, rc)
            assert np.isnan(img).all(), (name, where, "a refused call wrote y")
            refused.append(name)
            continue
        _lib.check(rc, name)
        bad = G.check_image(img, lay, compare_for(padded(want, lay)), f"{name} {where}")
        # the payloads a truncated store would land in (vectors 0 and 1) after the others
        bad.sort(key=lambda b: "vector 0 row" in b or "vector 1 row" in b)
        assert not bad, f"{len(bad)} failures, first: " + "; ".join(bad[:6])
        ran.append(name)
    return ran, refused


def nan_ok(want_nan):
    """Compare for the controls: NaN exactly where want_nan says."""
    return lambda got: np.isnan(got) == want_nan


def controls(family, call, base, variants, where):
    """Valid calls only. One column more: every row reads the NaN past the payload (the wide
    operand's fringe, the narrow one's padding), so every row of every vector is NaN. One row
    fewer: row m - 1 stays NaN and the rows before it keep their bits."""
    lay = call.Y.lay
    for v in variants:
        name = W.family_names(family)[v]
        call.k += 1
        rc, img = call.run(family, v)
        call.k -= 1
        _lib.check(rc, name)
        want_nan = ~np.isnan(padded(np.zeros((call.nv, call.m)), lay))
        bad = G.check_image(img, lay, nan_ok(want_nan), f"{name} {where} k + 1")
        assert not bad, bad[:6]
        call.m -= 1
        rc, img = call.run(family, v)
        call.m += 1
        _lib.check(rc, name)
        fewer = padded(base[name][:, :call.m - 1], lay)
        bad = G.check_image(img, lay, G.exact_ok(fewer), f"{name} {where} m - 1")
        assert not bad, bad[:6]


def first_live(family, live):
    """The controls' variants: the automatic path and the first explicit form that runs."""
    names = W.family_names(family)
    return [0] + [names.index(n) for n in live if n != "auto"][:1]


def baseline(family, call, variants):
    """The payload each control variant gives on the plain call (for the m - 1 control)."""
    out = {}
    for v in variants:
        rc, img = call.run(family, v)
        _lib.check(rc, str(v))
        out[W.family_names(family)[v]] = call.Y.lay.payload(img)[:call.nv, :call.m]
    return out


# ------------------------------------------------------------------ A far or at the limit
@pytest.mark.parametrize("view", W.A_VIEWS, ids=repr)
@pytest.mark.parametrize("family", FAMILIES)
def test_a_far_or_at_the_limit(arena, family, view):
    off16 = bool(view.shift)
    launches = 0
    for k in ks_for(family, view):
        A, X, want = data(k)
        live = W.live_names(family, view, "A", k)
        assert "auto" in live
        wA = W.WideOperand(arena, M, k, view.ld, view.shift).write(A)
        # the controls' x has one finite column more: their NaN can only come from A's far fringe
        Xc = np.concatenate([X, np.ones((16, 1))], axis=1)
        try:
            for nv in NVS if family in VECTOR_FAMILIES else (1,):
                dX = G.vectors(Xc[:nv], k + 2, view.shift)
                dY = G.result(nv, M, M + 3, spare=1)
                try:
                    call = Call(wA.ptr, view.ld, dX.ptr, k + 2, dY, M + 3, M, k, nv)
                    where = f"{view} k={k} nv={nv}"
                    ran, refused = run_all(family, call, want[:nv], lambda w: ok_for(family, A, X[:nv], w),
                                           lambda n: W.refuses(family, n, view.ld, k + 2, off16, k), where)
                    assert ran == live and sorted(ran + refused) == sorted(W.family_names(family)), where
                    launches += len(ran)
                    if nv == NVS[-1] or family not in VECTOR_FAMILIES:
                        picks = first_live(family, live)
                        controls(family, call, baseline(family, call, picks), picks, where)
                finally:
                    dX.free()
                    dY.free()
        finally:
            wA.release()
    # not silently vacuous: the whole family on the far strides, what the limits let through at LIMIT_A
    # (the 11 LDS-DMA exact forms stop at lda < 2^23, the 22 DMA multi forms at 2^31 bytes per
    # workgroup: the 4 with 64 rows past LIMIT_A64, the 12 with 32 rows past LIMIT_A, the 6 with 16
    # rows past LIMIT_A16; odd or shifted: the 8-B forms)
    n = len(W.family_names(family))
    forms = {"tree": n, "exact_multi": n,
             "exact": {W.LIMIT_A: n, W.LIMIT_A64: n, W.LIMIT_A16: n - 11, W.FAR_A: n - 11}.get(view, 15),
             "multi": {W.LIMIT_A: n - 4, W.LIMIT_A64: n, W.LIMIT_A16: n - 16, W.FAR_A: n - 22}.get(view, 1)}[family]
    runs = len(ks_for(family, view)) * (len(NVS) if family in VECTOR_FAMILIES else 1)
    assert launches >= runs * forms, (family, view, launches, runs, forms)


# ------------------------------------------------------------------ X far or at the limit
@pytest.mark.parametrize("view", W.X_VIEWS, ids=repr)
@pytest.mark.parametrize("family", FAMILIES)
def test_x_far_or_at_the_limit(arena, family, view):
    k = 130 if family == "multi" else 300
    A, X, want = data(k)
    live = W.live_names(family, view, "X", k)
    assert "auto" in live
    launches = 0
    wX = W.WideOperand(arena, view.nvec, k, view.ld).write(X[:view.nvec])
    # the controls' A has one finite column more: their NaN can only come from X's far fringe
    dA = G.matrix(np.concatenate([A, np.ones((M, 1))], axis=1), 1)
    lda = k + 2
    try:
        if family in VECTOR_FAMILIES:
            cases = [(0, nv) for nv in NVS if nv <= view.nvec]
        else:
            cases = [(v, 1) for v in X_PICKS if v < view.nvec]
        for v0, nv in cases:
            dY = G.result(nv, M, M + 3, spare=1)
            try:
                call = Call(dA.ptr, lda, wX.ptr + 8 * v0 * view.ld, view.ld, dY, M + 3, M, k, nv)
                where = f"{view} k={k} nv={nv} first vector {v0}"
                ran, refused = run_all(family, call, want[v0:v0 + nv], lambda w: ok_for(family, A, X[v0:v0 + nv], w),
                                       lambda n: W.refuses(family, n, lda, view.ld, False, k), where)
                assert ran == live and sorted(ran + refused) == sorted(W.family_names(family)), where
                launches += len(ran)
                if (v0, nv) == cases[-1]:
                    picks = first_live(family, live)
                    controls(family, call, baseline(family, call, picks), picks, where)
            finally:
                dY.free()
    finally:
        dA.free()
        wX.release()
    assert launches >= len(cases) * len(live) > len(cases), (family, view, launches)
    if family == "multi":  # the forms with 32-bit offsets on their limit views, refused past them
        dma = [n for n in W.family_names(family) if W.dma_rows(n)]
        want_live = {W.LIMIT_X16: dma, W.LIMIT_X8: [n for n in dma if n.startswith("mdma_")], W.FAR_X: []}[view]
        assert [n for n in live if W.dma_rows(n)] == want_live and len(dma) >= 22


# ------------------------------------------------------------------ Y far
@pytest.mark.parametrize("family", FAMILIES)
def test_y_far(arena, family):
    """Y's vectors 2^28 doubles apart: vector 2 past 2^32 bytes, vector 8 past 2^31 elements. Every
    vector's payload right, every fringe (rows -16 .. -1 and m .. m + 15 of each vector) and every
    vector past nv still NaN."""
    view = W.FAR_Y
    k = 130 if family == "multi" else 300
    A, X, want = data(k)
    dA = G.matrix(A, 2)
    dX = G.vectors(X, k + 2)
    wY = W.WideOperand(arena, view.nvec, M, view.ld)
    names = W.family_names(family)
    launches = 0
    try:
        if family in VECTOR_FAMILIES:
            cases = [(0, nv) for nv in NVS]
        else:
            cases = [(v, 1) for v in X_PICKS]
        for v0, nv in cases:
            # a single-vector family writes vector v0 of the wide Y from x_v0
            call = Call(dA.ptr, k + 2, dX.ptr + 8 * v0 * (k + 2), k + 2, wY, view.ld, M, k, nv)
            where = f"{view} k={k} nv={nv} first vector {v0}"
            full = np.full((view.nvec, M), np.nan)
            full[v0:v0 + nv] = want[v0:v0 + nv]
            scale = np.ones((view.nvec, M))
            scale[v0:v0 + nv] = (np.abs(A) @ np.abs(X[v0:v0 + nv]).T).T
            tol = lambda w: (lambda got: (np.isnan(w) & np.isnan(got)) | (np.abs(got - w) <= 1e-13 * scale))  # noqa: E731
            if family in VECTOR_FAMILIES:
                shifted = call
            else:  # y = Y + v0 * ldy: the image still starts at vector 0
                shifted = _YOffset(call, v0)
            ran, refused = run_all(family, shifted, full, G.exact_ok if family in EXACT else tol,
                                   lambda n: W.refuses(family, n, k + 2, k + 2, False, k), where)
            assert ran == names and not refused, where
            launches += len(ran)
        if family in VECTOR_FAMILIES:  # the m - 1 control: row 66 of every vector stays NaN
            call = Call(dA.ptr, k + 2, dX.ptr, k + 2, wY, view.ld, M, k, 16)
            picks = first_live(family, names)
            base = baseline(family, call, picks)
            for v in picks:
                call.m -= 1
                rc, img = call.run(family, v)
                call.m += 1
                _lib.check(rc, names[v])
                bad = G.check_image(img, wY.lay, G.exact_ok(padded(base[names[v]][:, :M - 1], wY.lay)), f"{names[v]} m - 1")
                assert not bad, bad[:6]
    finally:
        wY.release()
        dA.free()
        dX.free()
    assert launches == len(cases) * len(names) >= 4 * 13


class _YOffset:
    """A Call whose y is vector v0 of the wide Y."""

    def __init__(self, call, v0):
        self.call, self.v0, self.Y = call, v0, call.Y

    def run(self, family, v):
        c = self.call
        c.Y.poison()
        y = c.Y.ptr + 8 * self.v0 * c.ldy
        fn = lib.mvg_gemv_variant if family == "tree" else lib.mvg_gemv_exact_variant
        rc = fn(c.A, c.lda, c.X, y, c.m, c.k, v, None)
        sync()
        return rc, c.Y.image()


# ------------------------------------------------------------------ panels
@pytest.mark.parametrize("P", (16, 32))
@pytest.mark.parametrize("src", (W.FAR_A, W.FAR_A_ODD), ids=repr)
def test_panels_far(arena, src, P):
    """mvg_panel_relayout from a far row-major source into panels 2^29 doubles apart (panel 1 past
    2^32 bytes, panel 4 past 2^31 elements, panel 8 at 2^32 elements with P = 16), the panel
    image read back panel by panel against the host restatement of the layout, then every panel
    variant at that pstride, bit for bit."""
    view, k = W.FAR_PANELS, W.PANEL_K
    npan = -(-k // P)
    assert (P, npan) in ((16, view.nvec), (32, 5))
    A, X, want = data(k)
    names = W.family_names("panels")
    wA = W.WideOperand(arena, M, k, src.ld, base=1 << 26).write(A)
    wP = W.WideOperand(arena, npan, M * P, view.ld, base=(1 << 27) + (1 << 20))  # clear of A's rows
    dX = G.vectors(np.concatenate([X[:1], np.ones((1, 1))], axis=1), k + 2)
    dY = G.result(1, M, M + 3, spare=1)
    ran = []
    try:
        _lib.check(lib.mvg_panel_relayout(wA.ptr, src.ld, M, k, wP.ptr, view.ld, P, None), "mvg_panel_relayout")
        sync()
        exp = np.full((npan, M, P), np.nan)
        for p in range(npan):
            w = min(P, k - p * P)
            exp[p, :, :w] = A[:, p * P:p * P + w]
        bad = G.check_image(wP.image(), wP.lay, G.exact_ok(exp.reshape(npan, M * P)), f"relayout {src} P={P}")
        assert not bad, bad[:6]
        assert not G.violations(wA.image(), wA.lay) and G.same_or_both_nan(wA.lay.payload(wA.image()), A)  # the source is read only

        def run(v, m=M, kk=k):
            dY.fill()
            rc = lib.mvg_gemv_exact_panels(wP.ptr, view.ld, P, dX.ptr, dY.ptr, m, kk, v, None)
            sync()
            return rc, dY.image()

        for v, name in enumerate(names):
            seg = 32 if name.startswith("panel_l16") else 16
            rc, img = run(v)
            if P % seg:
                assert rc == _lib.MVG_E_INVALID and np.isnan(img).all(), (name, P)
                continue
            _lib.check(rc, name)
            G.assert_clean(img, dY.lay, G.exact_ok(want[:1]), f"{name} P={P}")
            ran.append(name)
        # controls: column k of the last panel is NaN fill; row 66 stays NaN
        for v in (0, names.index(ran[-1])):
            rc, img = run(v, kk=k + 1)
            _lib.check(rc, names[v])
            G.assert_clean(img, dY.lay, lambda got: np.isnan(got), f"{names[v]} k + 1")
            rc, img = run(v, m=M - 1)
            _lib.check(rc, names[v])
            fewer = want[:1].copy()
            fewer[0, M - 1] = np.nan
            G.assert_clean(img, dY.lay, G.exact_ok(fewer), f"{names[v]} m - 1")
    finally:
        wP.release()
        wA.release()
        dX.free()
        dY.free()
    assert ran == [n for n in names if P % (32 if n.startswith("panel_l16") else 16) == 0]
    assert len(ran) >= (5 if P == 32 else 4) and ran[0] == "auto"
