"""mvg_gemv_ata_multi on the GPU: every variant and the automatic pick, through mm.multiply_ata_multi
(host arrays) and mm.gemv_ata_multi (device pointers). Column v of T is held to mvg_gemv's contract
against A x_v, column v of W to mvg_gemv_t's against A^T (the returned column of T): W is defined on
the stored T, so each has its own reference and no compounded bound is needed.

References: oracle.multiply_std_rowwise(A, x_v) for T, the same function on the contiguous A^T and
the returned column of T for W. Bars (tests/test_gpu_gemv_ata.py's): on oracle.synth data
(non-negative) max_rel <= 1e-12 for both; on signed uniform(-1, 1) data
|T - ref| <= 1e-13 * (|A| |x_v|) and |W - ref| <= 1e-13 * (|A|^T |t_v|).

A fused variant is skipped on a shape only where k exceeds its max_k; the call must then answer
MVG_E_INVALID and leave T and W untouched.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import gpu_guarded as G
from conftest import max_rel
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
TOL = 1e-12
SIGNED_TOL = 1e-13
NVAR = lib.mvg_gemv_ata_multi_variant_count()
VARIANTS = list(range(NVAR))
TWO_PASS = 1
FUSED = VARIANTS[2:]

SHAPES = [(1, 1), (3, 5), (63, 129), (65, 127), (255, 257), (1000, 257), (7, 1000), (20001, 7), (4099, 129)]
NVS = [1, 2, 3, 4, 5, 7, 9]  # full groups, a short last group and the single leftover vector


def name(v):
    return lib.mvg_gemv_ata_multi_variant_name(v).decode()


def chains(v):
    """A fused variant's chain count; 2 for auto and two_pass (any nv serves them alike)."""
    hit = re.search(r"_v(\d+)$", name(v))
    return int(hit.group(1)) if hit else 2


def max_k(v):
    return mm.gemv_ata_multi_plan(1, 1, 1, 2, v)[2]


def applies(v, k):
    return v < 2 or k <= max_k(v)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ref_t(A, X):
    return np.stack([oracle.multiply_std_rowwise(A, np.ascontiguousarray(X[:, v])) for v in range(X.shape[1])], axis=1)


def ref_w(A, T):
    At = np.ascontiguousarray(A.T)
    return np.stack([oracle.multiply_std_rowwise(At, np.ascontiguousarray(T[:, v])) for v in range(T.shape[1])], axis=1)


@functools.lru_cache(maxsize=64)
def synth(m, k, nv):
    A, X = oracle.synth(m, k, 42), np.ascontiguousarray(oracle.synth(nv, k, 4242).T)
    for a in (A, X):
        a.setflags(write=False)
    return A, X, ref_t(A, X)


@functools.lru_cache(maxsize=64)
def signed(m, k, nv):
    rng = np.random.default_rng(m * 7919 + k)
    A, X = rng.uniform(-1.0, 1.0, size=(m, k)), rng.uniform(-1.0, 1.0, size=(k, nv))
    for a in (A, X):
        a.setflags(write=False)
    return A, X, ref_t(A, X), np.abs(A) @ np.abs(X)


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cached_inputs_after_the_module():
    yield
    synth.cache_clear()
    signed.cache_clear()


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def check_synth(A, T, W, want_t, what):
    assert T.shape == want_t.shape and W.shape == (A.shape[1], want_t.shape[1]), (what, T.shape, W.shape)
    want_w = ref_w(A, T)
    nv = T.shape[1]
    rt = max((max_rel(T[:, c], want_t[:, c]) for c in range(nv)), default=0.0)
    rw = max((max_rel(W[:, c], want_w[:, c]) for c in range(nv)), default=0.0)
    print(f"{what}: synth max_rel T {rt:.3e} W {rw:.3e}")
    assert rt <= TOL and rw <= TOL, (what, rt, rw)


def check_signed(A, T, W, want_t, scale_t, what):
    assert T.shape == want_t.shape and W.shape == (A.shape[1], want_t.shape[1]), (what, T.shape, W.shape)
    et = float(np.max(np.abs(T - want_t) / scale_t))
    ew = float(np.max(np.abs(W - ref_w(A, T)) / (np.abs(A).T @ np.abs(T))))
    print(f"{what}: signed err T {et:.3e} W {ew:.3e}")
    assert et <= SIGNED_TOL and ew <= SIGNED_TOL, (what, et, ew)


class Dev:
    """A (rows lda apart), X (vectors ldx apart), a T (ldt) and a W (ldw) on the device, each `off`
    doubles into its buffer; everything around the payloads is NaN, a spare column after T and W too."""

    def __init__(self, A, X, lda=None, ldx=None, ldt=None, ldw=None, off=0):
        self.m, self.k = A.shape
        self.nv = X.shape[1]
        self.lda, self.ldx, self.ldt, self.ldw, self.off = lda or self.k, ldx or self.k, ldt or self.m, ldw or self.k, off
        img = np.full(self.m * self.lda + off + 2, np.nan)
        img[off + np.arange(self.m)[:, None] * self.lda + np.arange(self.k)[None, :]] = A
        self.A = mm.DeviceBuffer(img.size).upload(img)
        self.X = mm.DeviceBuffer(self.nv * self.ldx + off + 2)
        self.set_x(X)
        self.T = mm.DeviceBuffer((self.nv + 1) * self.ldt + off + 2)
        self.W = mm.DeviceBuffer((self.nv + 1) * self.ldw + off + 2)

    def set_x(self, X):
        xi = np.full(self.X.n, np.nan)
        xi[self.off + np.arange(self.nv)[:, None] * self.ldx + np.arange(self.k)[None, :]] = X.T
        self.X.upload(xi)

    def _payload(self, buf, img, n, ld, nv, what, v):
        pay = np.zeros(img.size, dtype=bool)
        pay[(self.off + np.arange(nv)[:, None] * ld + np.arange(n)[None, :]).ravel()] = True
        assert np.all(np.isnan(img[~pay])), (name(v), "stored outside " + what)
        return img[pay].reshape(nv, n).T.copy()

    def run(self, v, nv=None, first=0):
        """Vectors first .. first + nv - 1 through variant v: (T, W), m x nv and k x nv, after checking
        that nothing outside them was stored; None where k exceeds v's max_k, after asserting the
        refusal."""
        nv = self.nv - first if nv is None else nv
        self.T.upload(np.full(self.T.n, np.nan))
        self.W.upload(np.full(self.W.n, np.nan))
        o = 8 * self.off
        rc = lib.mvg_gemv_ata_multi_variant(self.A.ptr + o, self.lda, self.X.ptr + o + 8 * first * self.ldx, self.ldx,
                                            self.T.ptr + o, self.ldt, self.W.ptr + o, self.ldw, self.m, self.k, nv, v, None)
        sync()
        ti, wi = self.T.download(), self.W.download()
        if not applies(v, self.k):
            assert rc == _lib.MVG_E_INVALID, (name(v), self.k, rc)
            assert np.all(np.isnan(ti)) and np.all(np.isnan(wi)), "a refused call stored something"
            return None
        assert rc == _lib.MVG_OK, (name(v), rc, lib.mvg_last_error().decode())
        return self._payload(self.T, ti, self.m, self.ldt, nv, "T", v), self._payload(self.W, wi, self.k, self.ldw, nv, "W", v)

    def free(self):
        for b in (self.A, self.X, self.T, self.W):
            b.free()


def run_both(m, k, nv, variants, do_signed=True, host_arrays=False, **view):
    """Every variant in `variants` on the synth and the signed m x k x nv problem through device
    pointers (host_arrays: the synth one through mm.multiply_ata_multi instead); returns how many ran."""
    A, X, want = synth(m, k, nv)
    d = Dev(A, X, **view)
    ds = Dev(*signed(m, k, nv)[:2], **view) if do_signed else None
    ran = 0
    try:
        for v in variants:
            got = d.run(v)
            if got is None:
                continue
            ran += 1
            what = f"{name(v)} {m}x{k} nv={nv}"
            check_synth(A, *got, want, what)
            if host_arrays:
                T, W = mm.multiply_ata_multi(A, X, variant=v)
                assert np.array_equal(bits(T), bits(got[0])) and np.array_equal(bits(W), bits(got[1])), what
            if ds:
                As, _, want_s, scale = signed(m, k, nv)
                check_signed(As, *ds.run(v), want_s, scale, what)
    finally:
        d.free()
        if ds:
            ds.free()
    return ran


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("m,k", SHAPES)
def test_every_variant_on_synth_and_signed_data(m, k, nv):
    ran = run_both(m, k, nv, VARIANTS, host_arrays=True)
    assert ran == sum(applies(v, k) for v in VARIANTS)


def test_every_fused_variant_runs_at_least_6_of_the_fixed_shapes():
    for v in FUSED:
        assert sum(k <= max_k(v) for _, k in SHAPES) >= 6, name(v)


@pytest.mark.parametrize("v", FUSED, ids=name)
def test_at_the_variants_own_limits(v):
    """k just under and at max_k (the kernel cut by k and the whole-row one) at a full group and a
    group with a vector more; one column more is refused, nothing stored."""
    mk, NV = max_k(v), chains(v)
    for k in (mk - 1, mk):
        assert run_both(37, k, NV + 1, [v]) == 1
    d = Dev(*synth(37, mk + 1, NV)[:2])
    try:
        assert d.run(v) is None
    finally:
        d.free()


@pytest.mark.parametrize("v", FUSED, ids=name)
def test_band_edges(v):
    """m around one and two bands, as mvg_gemv_ata_multi_plan cuts each m, k around a 64-column chunk,
    at a full group and at a short one."""
    NV = chains(v)
    band_rows = mm.gemv_ata_multi_plan(129, 1000, 129, NV, v)[0]
    for m in (band_rows - 1, band_rows, band_rows + 1, 2 * band_rows + 1):
        for k, nv in ((63, NV), (65, NV), (129, NV + NV - 1 if NV > 2 else NV)):
            b, bands, _, group = mm.gemv_ata_multi_plan(k, m, k, nv, v)
            assert b == band_rows and bands == -(-m // band_rows) and group == NV, (name(v), m, k, b, bands, group)
            assert run_both(m, k, nv, [v]) == 1
    assert mm.gemv_ata_multi_plan(65, 2 * band_rows + 1, 65, NV, v)[:2] == (band_rows, 3)


@pytest.mark.parametrize("m,k,lda,ldx,ldt,ldw,off", [(70, 300, 512, 333, 75, 307, 0), (70, 300, 301, 301, 71, 303, 1),
                                                     (257, 1000, 1000, 1001, 259, 1003, 1)],
                         ids=["lda>k", "odd-ld-off8", "even-lda-off8"])
def test_views(m, k, lda, ldx, ldt, ldw, off):
    """A sub-block view (lda > k), odd leading dimensions, ldx, ldt, ldw larger than the columns; A, X,
    T and W each 8 bytes off a 16-B boundary. nv = 5: two groups and a single vector, or a group and
    a single vector."""
    ran = run_both(m, k, 5, VARIANTS, do_signed=False, lda=lda, ldx=ldx, ldt=ldt, ldw=ldw, off=off)
    assert ran == sum(applies(v, k) for v in VARIANTS)


@pytest.mark.parametrize("m,k,nv,pad,shift", [(257, 255, 4, 9, 0), (70, 300, 5, 1, 1), (33, 513, 7, 2, 0)])
def test_guarded_operands(m, k, nv, pad, shift):
    """NaN around A, X, T and W, in every padding column of A and in the gaps of X, T and W: a read
    outside A[i, 0..k) or X[0..k, v) turns sums into NaN, a store outside T[0..m, v) or W[0..k, v)
    replaces a NaN of their images (the gaps between the columns and a spare column included)."""
    A, X, want = synth(m, k, nv)
    gA, gX = G.matrix(A, pad, shift), G.vectors(X.T, k + pad, shift)
    gT, gW = G.result(nv, m, m + pad, spare=1), G.result(nv, k, k + pad, spare=1)
    try:
        for v in VARIANTS:
            if not applies(v, k):
                continue
            gT.fill()
            gW.fill()
            mm.gemv_ata_multi(gA.ptr, k + pad, gX.ptr, k + pad, gT.ptr, m + pad, gW.ptr, k + pad, m, k, nv, None, v)
            sync()
            G.assert_clean(gT.image(), gT.lay, lambda got: np.abs(got - want.T) <= TOL * np.abs(want.T), name(v) + " T")
            want_w = ref_w(A, gT.lay.payload(gT.image()).T)
            G.assert_clean(gW.image(), gW.lay, lambda got: np.abs(got - want_w.T) <= TOL * np.abs(want_w.T), name(v) + " W")
    finally:
        for g in (gA, gX, gT, gW):
            g.free()


def _malloc(n):
    p = ctypes.c_void_p()
    _lib.check(lib.mvg_malloc(ctypes.byref(p), 8 * n), "mvg_malloc")
    return p.value


def _put(dst, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    _lib.check(lib.mvg_memcpy_h2d(dst, a.ctypes.data, a.nbytes, None), "h2d")
    sync()


def _get(src, n):
    out = np.empty(n)
    _lib.check(lib.mvg_memcpy_d2h(out.ctypes.data, src, 8 * n, None), "d2h")
    sync()
    return out


def test_wide_view_rows_2_to_the_26_and_vectors_2_to_the_28_doubles_apart():
    """64-bit row and vector offsets: 5 rows of 130 columns 512 MiB apart (the last starts 2 GiB in),
    3 vectors of X, T and W 2 GiB apart (the third starts 4 GiB in), each between NaN fringes."""
    m, k, nv, lda, ld, fringe = 5, 130, 3, 1 << 26, 1 << 28, G.GUARD
    A, X, want = synth(m, k, nv)
    pa = _malloc((m - 1) * lda + k + 2 * fringe)
    px, pt, pw = (_malloc((nv - 1) * ld + n + 2 * fringe) for n in (k, m, k))
    try:
        for i in range(m):
            row = np.full(k + 2 * fringe, np.nan)
            row[fringe:fringe + k] = A[i]
            _put(pa + 8 * i * lda, row)
        for c in range(nv):
            col = np.full(k + 2 * fringe, np.nan)
            col[fringe:fringe + k] = X[:, c]
            _put(px + 8 * c * ld, col)
        for v in VARIANTS:
            assert applies(v, k)
            for c in range(nv):
                _put(pt + 8 * c * ld, np.full(m + 2 * fringe, np.nan))
                _put(pw + 8 * c * ld, np.full(k + 2 * fringe, np.nan))
            mm.gemv_ata_multi(pa + 8 * fringe, lda, px + 8 * fringe, ld, pt + 8 * fringe, ld, pw + 8 * fringe, ld, m, k, nv,
                              None, v)
            sync()
            cols = []
            for p, n in ((pt, m), (pw, k)):
                got = [_get(p + 8 * c * ld, n + 2 * fringe) for c in range(nv)]
                for g in got:
                    assert np.all(np.isnan(g[:fringe])) and np.all(np.isnan(g[fringe + n:])), (name(v), "stored outside")
                cols.append(np.stack([g[fringe:fringe + n] for g in got], axis=1))
            check_synth(A, *cols, want, name(v))
    finally:
        for p in (pa, px, pt, pw):
            lib.mvg_free(p)


def test_two_pass_is_mvg_gemv_multi_then_mvg_gemv_t_multi_bit_for_bit():
    """T is mvg_gemv_multi's Y on the same operands and W is mvg_gemv_t_multi's Y on that T: what the
    definition means. auto, which is two_pass wherever nothing is tuned, gives the same bits for
    nv >= 2, and mvg_gemv_ata's for one vector."""
    for m, k, nv in [(257, 255, 4), (1000, 257, 5), (7, 1000, 2), (4099, 129, 9), (255, 257, 1)]:
        for A, X in (synth(m, k, nv)[:2], signed(m, k, nv)[:2]):
            d = Dev(A, X)
            y, yt = mm.DeviceBuffer(m * nv), mm.DeviceBuffer(k * nv)
            try:
                T, W = d.run(TWO_PASS)
                _lib.check(lib.mvg_gemv_multi(d.A.ptr, k, d.X.ptr, k, y.ptr, m, m, k, nv, None), "mvg_gemv_multi")
                mm.gemv_t_multi(d.A.ptr, k, d.T.ptr, m, yt.ptr, k, m, k, nv)
                sync()
                assert np.array_equal(bits(T), bits(y.download().reshape(nv, m).T)), (m, k, nv)
                assert np.array_equal(bits(W), bits(yt.download().reshape(nv, k).T)), (m, k, nv)
                auto = d.run(0)
                if nv == 1:
                    t1, w1 = mm.multiply_ata(A, X[:, 0])
                    assert np.array_equal(bits(auto[0][:, 0]), bits(t1)) and np.array_equal(bits(auto[1][:, 0]), bits(w1))
                elif lib.mvg_gemv_ata_multi_auto_variant(k, k, m, k, nv) == TWO_PASS:
                    assert np.array_equal(bits(auto[0]), bits(T)) and np.array_equal(bits(auto[1]), bits(W))
            finally:
                for b in (y, yt):
                    b.free()
                d.free()


@pytest.mark.parametrize("m,k,nv", [(300, 200, 5), (4099, 129, 9), (20001, 7, 3)])
def test_a_single_leftover_vector_is_mvg_gemv_ata_bit_for_bit(m, k, nv):
    A, X, _, _ = signed(m, k, nv)
    t1, w1 = mm.multiply_ata(A, X[:, -1])
    ran = 0
    for v in FUSED:
        if nv % chains(v) == 1 and applies(v, k):  # the last column went through mvg_gemv_ata
            T, W = mm.multiply_ata_multi(A, X, variant=v)
            assert np.array_equal(bits(T[:, -1]), bits(t1)) and np.array_equal(bits(W[:, -1]), bits(w1)), name(v)
            ran += 1
    assert ran


@pytest.mark.parametrize("v", VARIANTS, ids=name)
def test_a_column_does_not_depend_on_the_other_columns_or_on_its_place(v):
    """Permuting the vectors of a full group permutes the columns of T and W bit for bit; column c's
    bits stay with every other vector replaced (by other numbers, by NaN); and the same vector at
    another place of a group of the same kernel (first of a second group, first of a short group)
    gives the same bits."""
    NV = chains(v)
    m, k = 300, 200  # several bands
    if v in FUSED:
        assert mm.gemv_ata_multi_plan(k, m, k, NV, v)[1] > 1
    A, X, _, _ = signed(m, k, 2 * NV)
    d = Dev(A, X)
    try:
        T0, W0 = d.run(v, NV)
        assert not np.any(np.isnan(T0)) and not np.any(np.isnan(W0))
        perm = np.roll(np.arange(NV), 1)
        Xp = X.copy()
        Xp[:, :NV] = X[:, perm]
        d.set_x(Xp)
        Tp, Wp = d.run(v, NV)
        assert np.array_equal(bits(Tp), bits(T0[:, perm])) and np.array_equal(bits(Wp), bits(W0[:, perm])), name(v)
        c = NV - 1
        others = np.arange(2 * NV) != c
        X2 = X.copy()
        X2[:, others] = np.random.default_rng(5).uniform(-3.0, 3.0, size=(k, 2 * NV - 1))
        d.set_x(X2)
        T2, W2 = d.run(v, NV)
        assert np.array_equal(bits(T2[:, c]), bits(T0[:, c])) and np.array_equal(bits(W2[:, c]), bits(W0[:, c])), name(v)
        X2[:, others] = np.nan
        d.set_x(X2)
        T3, W3 = d.run(v, NV)
        assert np.array_equal(bits(T3[:, c]), bits(T0[:, c])) and np.array_equal(bits(W3[:, c]), bits(W0[:, c])), name(v)
        assert np.all(np.isnan(T3[:, :c])) and np.all(np.isnan(W3[:, :c])), name(v)
        if v in FUSED:
            X4 = X.copy()
            X4[:, NV] = X[:, c]  # column NV of NV + 2 vectors opens the second group
            d.set_x(X4)
            T4, W4 = d.run(v, NV + 2)
            assert np.array_equal(bits(T4[:, NV]), bits(T0[:, c])) and np.array_equal(bits(W4[:, NV]), bits(W0[:, c])), name(v)
            if NV > 2:  # first of a short group of NV - 1 vectors
                T5, W5 = d.run(v, NV - 1, first=NV)
                assert np.array_equal(bits(T5[:, 0]), bits(T0[:, c])) and np.array_equal(bits(W5[:, 0]), bits(W0[:, c])), name(v)
    finally:
        d.free()


@pytest.mark.parametrize("nv", [3, 5])
def test_special_values_stay_in_their_row_and_their_column(nv):
    """A NaN in A[i, j] reaches row i of T in every column and all of W, and no other entry of T; a
    NaN in X[j, c] stays in column c of T and W."""
    m, k, i, j, c = 300, 200, 171, 133, 1  # several bands; every X[j, v] > 0
    A, X, _ = synth(m, k, nv)
    X = X + 0.5
    B = A.copy()
    B[i, j] = np.nan
    Xn = X.copy()
    Xn[j, c] = np.nan
    for v in VARIANTS:
        T0, W0 = mm.multiply_ata_multi(A, X, variant=v)
        T1, W1 = mm.multiply_ata_multi(B, X, variant=v)
        rows = np.arange(m) != i
        assert np.all(np.isnan(T1[i])), (name(v), T1[i])
        assert np.array_equal(bits(T1[rows]), bits(T0[rows])), name(v)
        assert np.all(np.isnan(W1)), name(v)
        T2, W2 = mm.multiply_ata_multi(A, Xn, variant=v)
        cols = np.arange(nv) != c
        assert np.array_equal(bits(T2[:, cols]), bits(T0[:, cols])) and np.array_equal(bits(W2[:, cols]), bits(W0[:, cols])), name(v)
        assert np.all(np.isnan(T2[:, c])) and np.all(np.isnan(W2[:, c])), name(v)


def test_empty_sums():
    m, k, nv, ldt, ldw = 200, 100, 5, 203, 107  # k within every fused variant's max_k
    one = mm.DeviceBuffer(4).upload(np.ones(4))
    T, W = mm.DeviceBuffer((nv + 1) * ldt + 1), mm.DeviceBuffer((nv + 1) * ldw + 1)
    pay_t, pay_w = np.zeros(T.n, dtype=bool), np.zeros(W.n, dtype=bool)
    pay_t[(1 + np.arange(nv)[:, None] * ldt + np.arange(m)[None, :]).ravel()] = True
    pay_w[(1 + np.arange(nv)[:, None] * ldw + np.arange(k)[None, :]).ravel()] = True
    try:
        for v in VARIANTS:
            T.upload(np.full(T.n, np.nan))
            W.upload(np.full(W.n, np.nan))
            # m == 0: k x nv zeros over the poison, T untouched
            mm.gemv_ata_multi(one.ptr, k, one.ptr, k, T.ptr, ldt, W.ptr + 8, ldw, 0, k, nv, None, v)
            sync()
            img = W.download()
            assert np.all(np.isnan(img[~pay_w])) and np.array_equal(bits(img[pay_w]), bits(np.zeros(nv * k))), name(v)
            assert np.all(np.isnan(T.download())), name(v)
            W.upload(np.full(W.n, np.nan))
            # k == 0: m x nv zeros, null A, X and W
            mm.gemv_ata_multi(None, 0, None, 0, T.ptr + 8, ldt, None, 0, m, 0, nv, None, v)
            sync()
            img = T.download()
            assert np.all(np.isnan(img[~pay_t])) and np.array_equal(bits(img[pay_t]), bits(np.zeros(nv * m))), name(v)
            assert np.all(np.isnan(W.download())), name(v)
            T.upload(np.full(T.n, np.nan))
            mm.gemv_ata_multi(None, 0, None, 0, None, 0, None, 0, 0, 0, nv, None, v)  # both zero: a no-op
            mm.gemv_ata_multi(one.ptr, k, one.ptr, k, T.ptr, ldt, W.ptr, ldw, m, k, 0, None, v)  # nv == 0: a no-op
            sync()
            assert np.all(np.isnan(T.download())) and np.all(np.isnan(W.download())), name(v)
    finally:
        for b in (one, T, W):
            b.free()


def test_deterministic_and_independent_of_the_workspace():
    """The same call twice; a call after others that leave the (null stream's) workspace dirty and
    make it regrow; every variant on a fresh set of buffers: the same bits every time."""
    shapes = [(4099, 129, 5), (257, 1000, 9), (20001, 7, 7)]
    data = {s: signed(*s)[:2] for s in shapes}
    devs = {s: Dev(*data[s]) for s in shapes}
    first_shape = shapes[0]
    try:
        for v in FUSED:
            assert mm.gemv_ata_multi_plan(129, 4099, 129, 5, v)[1] > 1, name(v)
        for v in VARIANTS:
            first = devs[first_shape].run(v)  # before this variant's larger shapes have dirtied the workspace
            again = devs[first_shape].run(v)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), name(v)
            for s in shapes[1:]:
                devs[s].run(v)  # dirties and regrows (or is refused by max_k: asserted in run)
                devs[s].run(TWO_PASS)
            after = devs[first_shape].run(v)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, after)), name(v)
            fresh = Dev(*data[first_shape])
            try:
                b = fresh.run(v)
            finally:
                fresh.free()
            assert all(np.array_equal(bits(a), bits(c)) for a, c in zip(first, b)), name(v)
    finally:
        for d in devs.values():
            d.free()


def test_multiply_ata_multi_returns_t_and_w():
    A, X, want = synth(255, 257, 3)
    T, W = mm.multiply_ata_multi(A, X)
    assert T.shape == (255, 3) and W.shape == (257, 3)
    check_synth(A, T, W, want, "multiply_ata_multi")
    with pytest.raises(ValueError):
        mm.multiply_ata_multi(A, X[:-1])
    with pytest.raises(ValueError):
        mm.multiply_ata_multi(A, X[:, 0])
