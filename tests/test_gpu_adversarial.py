"""Every GEMV kernel on adversarial inputs inside poisoned surroundings.

The operands sit in guarded images (tests/gpu_guarded.py): NaN in front of and behind A, x / X
and y / Y, in the padding columns of A (lda > k) and X (ldx > k), in the rows m..ldy-1 of Y and
in a spare vector past nv. A kernel that reads a padding column into a sum, or stores outside
its rows, fails here however small the leak. The inputs (tests/adversarial_cases.py; their
properties are asserted on the CPU in tests/test_adversarial_host.py):

  0. positive controls with valid calls: one column more reads the poison, one row fewer leaves
     the last row of y untouched;
  1. ordinary synthetic data, plain and signed, in every lda / alignment class a form takes;
  2. special rows (inf, NaN, inf - inf, inf * 0) and special x elements: the oracle's class for
     the special row, every other row bit for bit as in the all-finite run of the same kernel;
  3. exponents over +-300 binades: power-of-two row and column scalings are exact;
  4. gradual underflow: sums of subnormal products (see the contract in DESIGN.md §6);
  5. sums that overflow and cancel (the exact kernels: the reference's chain goes inf, then NaN);
  6. two split-K launches back to back on one stream, sharing and regrowing the workspace.

Families: `tree` every mvg_gemv_variant, `exact` every mvg_gemv_exact_variant, `panels` every
mvg_gemv_exact_panels variant over mvg_panel_relayout's output at three panel widths, `multi`
every mvg_gemv_multi_variant (the m16_* matrix-core forms included) and the automatic path.
"""
import numpy as np
import pytest

import adversarial_cases as AC
import gpu_guarded as G
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle
from test_gpu_exact import needs_16b, xl_k_limited

pytestmark = pytest.mark.gpu
lib = _lib.lib
TOL = 1e-12          # relative, non-negative data (BASELINE north star; tests/test_gpu_parity.py)
SIGNED_TOL = 1e-13   # times sum_j |a_ij x_j|, signed data (test_gemv_all_variants_on_signed_data)
PANEL_WIDTHS = (16, 32, 256)
FAMILIES = ("tree", "exact", "panels", "multi")
EXACT_FAMILIES = ("exact", "panels")


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ operands and runners
class Case:
    """A (m x k, lda = k + pad), X (nv vectors, ldx) and Y (nv vectors, ldy, one spare vector)
    as guarded device images; `shift` moves A and X 8 bytes off their 16-B boundaries."""

    def __init__(self, A, X, pad, ldx=None, shift=0, shift_x=None):
        self.m, self.k = A.shape
        self.nv = X.shape[0]
        self.lda, self.ldx, self.ldy = self.k + pad, ldx or self.k + 2, self.m + 3
        self.shift = shift
        self.shift_x = shift if shift_x is None else shift_x
        self.dA = G.matrix(A, pad, shift)
        self.dX = G.vectors(X, self.ldx, self.shift_x)
        self.dY = G.result(self.nv, self.m, self.ldy, spare=1)
        self._panels = {}

    def set_A(self, A):
        self.dA.fill(A)
        self._drop_panels()

    def set_X(self, X):
        self.dX.fill(X)

    def poke_A(self, row, col, value):
        self.dA.poke(row, col, value)
        self._drop_panels()

    def _drop_panels(self):
        for g in self._panels.values():
            g.free()
        self._panels = {}

    def panels(self, P):
        """The panel copy of A at width P (mvg_panel_relayout from the guarded row-major image
        into a guarded, NaN-filled panel image), rebuilt after A changes."""
        if P not in self._panels:
            npan = max(-(-self.k // P), 1)
            g = G.Guarded(G.Layout(npan * self.m, P, P))
            _lib.check(lib.mvg_panel_relayout(self.dA.ptr, self.lda, self.m, self.k, g.ptr, self.m * P, P, None),
                       "mvg_panel_relayout")
            sync()
            self._panels[P] = g
        return self._panels[P]

    def run(self, runner):
        """One launch into a NaN-filled Y; nothing outside the payload may change. Returns the
        payload, nv x m."""
        self.dY.fill()
        _lib.check(runner.call(self), runner.name)
        sync()
        img = self.dY.image()
        bad = G.violations(img, self.dY.lay)
        assert not bad, (runner.name, self.m, self.k, self.nv, self.lda, self.shift, bad[:4])
        return self.dY.lay.payload(img)

    def free(self):
        self._drop_panels()
        for g in (self.dA, self.dX, self.dY):
            g.free()


class Runner:
    def __init__(self, name, call, refuses=lambda c: False):
        self.name, self.call, self.refuses = name, call, refuses


def runners(family):
    """Every kernel of the family, from the library's own count and name calls."""
    out = []
    if family == "tree":
        for v in range(lib.mvg_gemv_variant_count()):
            out.append(Runner(lib.mvg_gemv_variant_name(v).decode(),
                              lambda c, v=v: lib.mvg_gemv_variant(c.dA.ptr, c.lda, c.dX.ptr, c.dY.ptr, c.m, c.k, v, None)))
    elif family == "exact":
        for v in range(lib.mvg_gemv_exact_variant_count()):
            name = lib.mvg_gemv_exact_variant_name(v).decode()
            out.append(Runner(name,
                              lambda c, v=v: lib.mvg_gemv_exact_variant(c.dA.ptr, c.lda, c.dX.ptr, c.dY.ptr, c.m, c.k, v, None),
                              lambda c, name=name: bool((needs_16b(name) and (c.lda % 2 or c.shift)) or
                                                        (xl_k_limited(name) and c.k > 8192))))
    elif family == "panels":
        for v in range(lib.mvg_gemv_exact_panel_variant_count()):
            name = lib.mvg_gemv_exact_panel_variant_name(v).decode()
            seg = 32 if name.startswith("panel_l16") else 16
            for P in PANEL_WIDTHS:
                out.append(Runner(f"{name}/P{P}",
                                  lambda c, v=v, P=P: lib.mvg_gemv_exact_panels(c.panels(P).ptr, c.m * P, P, c.dX.ptr, c.dY.ptr,
                                                                                c.m, c.k, v, None),
                                  # 16-B loads of x; the row-major source of the relayout may sit anywhere
                                  lambda c, seg=seg, P=P: bool(P % seg or c.shift_x)))
    else:
        assert family == "multi"
        for v in range(lib.mvg_gemv_multi_variant_count()):
            out.append(Runner(lib.mvg_gemv_multi_variant_name(v).decode(),
                              lambda c, v=v: lib.mvg_gemv_multi_variant(c.dA.ptr, c.lda, c.dX.ptr, c.ldx, c.dY.ptr, c.ldy,
                                                                        c.m, c.k, c.nv, v, None),
                              # explicit variants: 16-B loads of A and X; the automatic path takes anything
                              (lambda c: bool(c.lda % 2 or c.ldx % 2 or c.shift)) if v else (lambda c: False)))
    assert len(out) > 1 and out[0].name.startswith("auto")
    return out


def even_pads(k):
    """The pads that make lda = k + pad even (16-B forms), and ldx to match."""
    return [p for p in AC.PADS if (k + p) % 2 == 0]


def layouts(k, every=False):
    """(pad, ldx, shift). every: all four pads, aligned and 8 bytes off; else one layout the
    16-B forms take and one they refuse (odd lda or lda % 16 == 8, shifted)."""
    ldx_even = k + 2 if k % 2 == 0 else k + 3
    if every:
        return [(p, ldx_even if (k + p) % 2 == 0 else k + 2, s) for p in AC.PADS for s in (0, 1)]
    ev, odd = even_pads(k), [p for p in AC.PADS if (k + p) % 2]
    return [(ev[(k // 2) % 2], ldx_even, 0), (odd[(k // 2) % 2], k + 2, 1)]


def make_case(family, A, X, pad, ldx, shift):
    """The family's operands: the panel kernels need a 16-B aligned x, so there only A shifts."""
    return Case(A, X, pad, ldx, shift, shift_x=0 if family == "panels" else None)


def nv_for(family, m, k):
    """Multi-vector tests 2-4: per shape one nv up to 8 and one past 8 (a second group, or one
    pass of the 16-vector forms), so that the 13 shapes cover every nv of the list."""
    i = AC.SHAPES.index((m, k))
    small, big = [n for n in AC.NVS if n <= 8], [n for n in AC.NVS if n > 8]
    return (small[i % len(small)], big[i % len(big)]) if family == "multi" else (1,)


# tests 2-4: (family, m, k, nv)
CASES = [(f, m, k, nv) for f in FAMILIES for m, k in AC.SHAPES for nv in nv_for(f, m, k)]


def live(family, case):
    rs = [r for r in runners(family) if not r.refuses(case)]
    assert rs, (family, case.lda, case.shift)  # every layout runs at least the automatic path
    return rs


def reference(A, X):
    return np.stack([oracle.multiply_std_rowwise(A, X[v]) for v in range(X.shape[0])])


def tree_ok(A, X, want, sign):
    if not sign:
        return lambda got: np.abs(got - want) <= TOL * np.maximum(np.abs(want), np.finfo(np.float64).tiny)
    scale = (np.abs(A) @ np.abs(X).T).T
    return lambda got: np.abs(got - want) <= SIGNED_TOL * scale


# ------------------------------------------------------------------ 0. the poison is live
@pytest.mark.parametrize("m,k", [(5, 7), (65, 127), (33, 6002)])
@pytest.mark.parametrize("family", FAMILIES)
def test_0_controls_one_more_column_is_nan_one_row_fewer_stays_nan(family, m, k):
    """Positive controls of the harness on the device, with valid calls only: asked for k + 1
    columns (lda allows it) every kernel reads the NaN padding column of A and x, so every row
    must come out NaN; asked for m - 1 rows it must leave row m - 1 of the NaN-filled y alone."""
    nv = nv_for(family, m, k)[-1]
    A, X = AC.payload(m, k, nv, sign=True)
    pad, ldx, shift = layouts(k)[0]
    case = make_case(family, A, X, pad, ldx, shift)
    try:
        rs = live(family, case)
        base = {r.name: case.run(r) for r in rs}
        case.k += 1
        case._drop_panels()
        for r in rs:
            if not r.refuses(case):  # k + 1 may pass a form's own limit
                assert np.isnan(case.run(r)).all(), (r.name, m, k)
        case.k -= 1
        case.m -= 1
        case._drop_panels()
        for r in rs:
            y = case.run(r)
            assert np.isnan(y[:, m - 1]).all(), (r.name, m, k)
            assert np.array_equal(bits(y[:, :m - 1]), bits(base[r.name][:, :m - 1])), (r.name, m, k)
    finally:
        case.free()


# ------------------------------------------------------------------ 1. poisoned surroundings
@pytest.mark.parametrize("m,k", AC.SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_1_poisoned_surroundings(family, m, k):
    nvs = AC.NVS if family == "multi" else (1,)
    for sign in (False, True):
        A, Xall = AC.payload(m, k, max(nvs), sign)
        for nv in nvs:
            X = Xall[:nv]
            want = reference(A, X)
            ok = G.exact_ok(want) if family in EXACT_FAMILIES else tree_ok(A, X, want, sign)
            for pad, ldx, shift in layouts(k, every=True):
                case = make_case(family, A, X, pad, ldx, shift)
                try:
                    ran = 0
                    for r in runners(family):
                        if r.refuses(case):  # the form says so: an error, nothing launched
                            assert r.call(case) == _lib.MVG_E_INVALID, (r.name, m, k, pad, shift)
                            continue
                        y = case.run(r)  # the guards are checked in there
                        good = np.broadcast_to(ok(y), y.shape)
                        assert good.all(), (r.name, m, k, nv, pad, shift, sign, np.argwhere(~good)[:4], y[~good][:4])
                        ran += 1
                    assert ran >= 1
                    if family == "panels" and not sign:
                        check_relayout(case, A)
                finally:
                    case.free()


def check_relayout(case, A):
    """mvg_panel_relayout wrote the k columns of every row and nothing else: the panel image
    against the host restatement of the layout, NaN where nothing belongs."""
    m, k = A.shape
    for P in PANEL_WIDTHS:
        npan = max(-(-k // P), 1)
        exp = np.full((npan, m, P), np.nan)
        for p in range(npan):
            w = max(min(P, k - p * P), 0)
            exp[p, :, :w] = A[:, p * P:p * P + w]
        g = case.panels(P)
        want = g.lay.image(exp.reshape(npan * m, P))
        wrong = np.flatnonzero(~G.exact_ok(want)(g.image()))
        assert wrong.size == 0, (m, k, P, case.lda, case.shift, [g.lay.describe(i) for i in wrong[:4]])


# ------------------------------------------------------------------ 2. special values
@pytest.mark.parametrize("family,m,k,nv", CASES)
def test_2_special_rows_stay_in_their_row(family, m, k, nv):
    A, X = AC.payload(m, k, nv, sign=True)
    for pad, ldx, shift in layouts(k):
        case = make_case(family, A, X, pad, ldx, shift)
        try:
            rs = live(family, case)
            for j in AC.col_positions(k):
                for group in (("inf", "nan", "inf_minus_inf"), ("inf_times_zero",)):  # the two x of special_x
                    kinds = [kd for kd in group if kd in AC.kinds_for(k)]
                    case.set_X(AC.special_x(X, j, kinds[0]))
                    base = {r.name: case.run(r) for r in rs}  # the all-finite run of the same kernel
                    for r in rs:
                        assert np.isfinite(base[r.name]).all(), r.name
                    for row in AC.row_positions(m):
                        others = np.arange(m) != row
                        for kind in kinds:
                            pokes = AC.special_row(A[row], j, kind)
                            for c, v in pokes:
                                case.poke_A(row, c, v)
                            want = np.full(nv, AC.wanted_class(kind))
                            for r in rs:
                                y = case.run(r)
                                where = (r.name, m, k, nv, pad, shift, "row", row, "col", j, kind)
                                assert G.same_class(want)(y[:, row]).all(), (where, y[:, row])
                                assert np.array_equal(bits(y[:, others]), bits(base[r.name][:, others])), where
                            for c, _ in pokes:
                                case.poke_A(row, c, A[row, c])
        finally:
            case.free()


@pytest.mark.parametrize("family,m,k,nv", CASES)
def test_2_special_x_reaches_every_row(family, m, k, nv):
    """A NaN or an infinity in x[j] makes every row of that vector non-finite (every row reads
    every column; 0 * inf is NaN too) and leaves the other vectors' bits alone."""
    A, X = AC.payload(m, k, nv, sign=True)
    for pad, ldx, shift in layouts(k):
        case = make_case(family, A, X, pad, ldx, shift)
        try:
            rs = live(family, case)
            base = {r.name: case.run(r) for r in rs}
            for n, j in enumerate(AC.col_positions(k)):
                v = (n + m) % nv
                others = np.arange(nv) != v
                for val in (np.nan, np.inf):
                    case.dX.poke(v, j, val)
                    for r in rs:
                        y = case.run(r)
                        where = (r.name, m, k, nv, pad, shift, "vector", v, "col", j, val)
                        assert not np.isfinite(y[v]).any(), (where, np.flatnonzero(np.isfinite(y[v]))[:8])
                        assert np.array_equal(bits(y[others]), bits(base[r.name][others])), where
                case.dX.poke(v, j, X[v, j])
        finally:
            case.free()


# ------------------------------------------------------------------ 3. exponent range
@pytest.mark.parametrize("family,m,k,nv", CASES)
def test_3_power_of_two_scalings_are_exact(family, m, k, nv):
    """Column scales 2^f_j on A against 2^-f_j on x leave every product, so every sum, unchanged;
    row scales 2^e_i scale every product and partial sum of row i exactly (nothing over- or
    underflows at |e|, |f| <= 300): y_i * 2^e_i bit for bit, whatever the order of summation."""
    A, X = AC.payload(m, k, nv, sign=True)
    re, cf, e = AC.exponent_scales(m, k)
    Ac, Xc, Ar = A * cf[None, :], X / cf[None, :], A * re[:, None]
    want_both = reference(Ar * cf[None, :], Xc) if family in EXACT_FAMILIES else None
    for pad, ldx, shift in layouts(k):
        case = make_case(family, A, X, pad, ldx, shift)
        try:
            rs = live(family, case)
            base = {r.name: case.run(r) for r in rs}
            case.set_A(Ar)
            rows = {r.name: case.run(r) for r in rs}
            case.set_A(Ar * cf[None, :])
            case.set_X(Xc)
            both = {r.name: case.run(r) for r in rs}
            case.set_A(Ac)
            cols = {r.name: case.run(r) for r in rs}
            for r in rs:
                where = (r.name, m, k, nv, pad, shift)
                assert np.isfinite(base[r.name]).all(), where
                scaled = np.ldexp(base[r.name], e[None, :])
                assert np.array_equal(bits(cols[r.name]), bits(base[r.name])), where
                assert np.array_equal(bits(rows[r.name]), bits(scaled)), where
                assert np.array_equal(bits(both[r.name]), bits(scaled)), where
                if want_both is not None:
                    assert G.same_or_both_nan(both[r.name], want_both), where
        finally:
            case.free()


# ------------------------------------------------------------------ 4. gradual underflow
@pytest.mark.parametrize("family,m,k,nv", CASES)
def test_4_gradual_underflow(family, m, k, nv):
    """Products of a few units of 2^-1074, sums that stay subnormal. The exact kernels give the
    reference's bits. The tree kernels stay within k units: adds of subnormals are exact, and each
    rounded product (reference) or FMA (kernel) errs by at most half a unit, on either side; a
    kernel that flushed subnormal products or sums to zero would miss that by a factor of two or
    more, since every reference y_i is at least 2k units (asserted here and on the CPU). The
    matrix-core forms (m16_*) are held to the same bound: measured on MI355X, the fp64 MFMA does
    not flush (worst error of any tree or multi-vector variant: 1 unit, at 130 x 4226)."""
    As, Xs, ref = AC.underflow_inputs(m, k, nv)
    assert AC.units(ref).min() >= 2 * k
    for pad, ldx, shift in layouts(k):
        case = make_case(family, As, Xs, pad, ldx, shift)
        try:
            for r in live(family, case):
                y = case.run(r)
                where = (r.name, m, k, nv, pad, shift)
                if family in EXACT_FAMILIES:
                    assert G.same_or_both_nan(y, ref), where
                else:
                    err = float(np.max(np.abs(AC.units(y) - AC.units(ref))))
                    assert err <= k, (where, "units off:", err, "smallest reference y:", AC.units(ref).min())
        finally:
            case.free()


# ------------------------------------------------------------------ 5. overflow and cancel
@pytest.mark.parametrize("m,k", [s for s in AC.SHAPES if s[1] >= 4])
@pytest.mark.parametrize("family", EXACT_FAMILIES)
def test_5_overflow_then_cancel_is_the_reference_chain(family, m, k):
    """Rows of 1e308 against x = [10, 10, -10, -10]: the reference's chain goes +inf, then NaN
    (a tree order could give anything); rows of 1e307: the running sum overflows and stays +inf.
    Every exact form gives exactly that, and the oracle's bits in every other row. (Shapes with
    k < 4 cannot hold the four columns.)"""
    for j in sorted({0, min(AC.boundary_col(k), k - 4), k - 4}):
        for ordinary in (False, True):
            A, x, rows = AC.overflow_cancel(m, k, j, ordinary)
            want = reference(A, x[None, :])
            assert np.isnan(want[0, rows[0]])
            for pad, ldx, shift in layouts(k):
                case = make_case(family, A, x[None, :], pad, ldx, shift)
                try:
                    for r in live(family, case):
                        y = case.run(r)
                        assert G.same_or_both_nan(y, want), (r.name, m, k, pad, shift, j, ordinary,
                                                             np.flatnonzero(~G.exact_ok(want)(y))[:8])
                finally:
                    case.free()


# ------------------------------------------------------------------ 6. split-K back to back
def test_6_split_k_launches_back_to_back_share_the_workspace():
    """Two split-K launches of different shapes on one stream with no sync between them: the
    second regrows the per-stream workspace the first is still using (and a third, smaller one
    reuses it). Every y must be its own product."""
    names = [lib.mvg_gemv_variant_name(v).decode() for v in range(lib.mvg_gemv_variant_count())]
    split = [v for v, n in enumerate(names) if n.endswith("_splitk")]
    assert split
    shapes = [(7, 20001), (130, 16388), (9, 16388)]  # workspace m * S: small, larger, smaller
    for m, k in shapes:
        assert names[lib.mvg_gemv_auto_variant(k + 2, m, k)].endswith("_splitk")  # the dispatch's own pick too
    cases = []
    comm = mm.Comm.init_all([0])
    try:
        # a stream of its own (a fresh engine's): its workspace starts empty, whatever the tests
        # before this one ran on the library's default stream
        with mm.Multiplier("rowwise", 8, 8, comm) as e:
            s = e.stream()
            assert s
            for m, k in shapes:
                A, X = AC.payload(m, k, 1, sign=True)
                cases.append((Case(A, X, 2), A, X, reference(A, X)))
            for v in [0] + split:
                for c, _, _, _ in cases:
                    c.dY.fill()
                for c, _, _, _ in cases:  # no sync in between
                    _lib.check(lib.mvg_gemv_variant(c.dA.ptr, c.lda, c.dX.ptr, c.dY.ptr, c.m, c.k, v, s), names[v])
                _lib.check(lib.mvg_stream_sync(s), "sync")
                for c, A, X, want in cases:
                    G.assert_clean(c.dY.image(), c.dY.lay, tree_ok(A, X, want, True), f"{names[v]} {c.m}x{c.k}")
    finally:
        for c, _, _, _ in cases:
            c.free()
        comm.destroy()
