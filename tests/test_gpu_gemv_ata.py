"""mvg_gemv_ata on the GPU: every variant and the automatic pick, through mm.multiply_ata (host arrays)
and mm.gemv_ata (device pointers). t is held to mvg_gemv's contract against A x, w to mvg_gemv_t's
against A^T (the returned t): w is defined on the stored t, so each has its own reference and no
compounded bound is needed.

References: t_ref = oracle.multiply_std_rowwise(A, x), w_ref = oracle.multiply_std_rowwise(A^T
contiguous, t returned). Bars: on oracle.synth data (non-negative) max_rel <= 1e-12 for both; on
signed uniform(-1, 1) data |t - t_ref| <= 1e-13 * (|A| |x|) and |w - w_ref| <= 1e-13 * (|A|^T |t|):
the bars of tests/test_gpu_gemv_t.py and tests/test_gpu_parity.py.

A fused variant is skipped on a shape only where k exceeds its max_k; the call must then answer
MVG_E_INVALID and leave t and w untouched.
"""
import ctypes
import functools

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
NVAR = lib.mvg_gemv_ata_variant_count()
VARIANTS = list(range(NVAR))
TWO_PASS = 1
FUSED = VARIANTS[2:]

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (5, 7), (63, 129), (64, 128), (65, 127), (255, 257), (257, 255), (1000, 257),
          (513, 130), (100, 1), (7, 1000), (20001, 7), (4099, 129), (65538, 3)]


def name(v):
    return lib.mvg_gemv_ata_variant_name(v).decode()


def max_k(v):
    return mm.gemv_ata_plan(1, 1, 1, v)[2]


def applies(v, k):
    return v < 2 or k <= max_k(v)


def ref_t(A, x):
    return oracle.multiply_std_rowwise(A, x)


def ref_w(A, t):
    return oracle.multiply_std_rowwise(np.ascontiguousarray(A.T), t)


@functools.lru_cache(maxsize=None)
def synth(m, k):
    A, x = oracle.synth(m, k, 42), oracle.synth(1, k, 4242)[0]
    for a in (A, x):
        a.setflags(write=False)
    return A, x, ref_t(A, x)


@functools.lru_cache(maxsize=None)
def signed(m, k):
    rng = np.random.default_rng(m * 7919 + k)
    A, x = rng.uniform(-1.0, 1.0, size=(m, k)), rng.uniform(-1.0, 1.0, size=k)
    for a in (A, x):
        a.setflags(write=False)
    return A, x, ref_t(A, x), np.abs(A) @ np.abs(x)


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def check_synth(A, t, w, want_t, what):
    assert t.shape == (A.shape[0],) and w.shape == (A.shape[1],), what
    rt, rw = max_rel(t, want_t), max_rel(w, ref_w(A, t))
    print(f"{what}: synth max_rel t {rt:.3e} w {rw:.3e}")
    assert rt <= TOL and rw <= TOL, (what, rt, rw)


def check_signed(A, t, w, want_t, scale_t, what):
    et = float(np.max(np.abs(t - want_t) / scale_t))
    ew = float(np.max(np.abs(w - ref_w(A, t)) / (np.abs(A).T @ np.abs(t))))
    print(f"{what}: signed err t {et:.3e} w {ew:.3e}")
    assert et <= SIGNED_TOL and ew <= SIGNED_TOL, (what, et, ew)


class Dev:
    """A, x on the device (rows lda apart, everything `off` doubles into its buffer), a t and a w."""

    def __init__(self, A, x, lda=None, off=0):
        self.m, self.k = A.shape
        self.lda, self.off = lda or self.k, off
        img = np.full(self.m * self.lda + off + 2, np.nan)
        img[off + np.arange(self.m)[:, None] * self.lda + np.arange(self.k)[None, :]] = A
        xi = np.full(self.k + off + 2, np.nan)
        xi[off:off + self.k] = x
        self.A, self.x = mm.DeviceBuffer(img.size).upload(img), mm.DeviceBuffer(xi.size).upload(xi)
        self.t, self.w = mm.DeviceBuffer(self.m + off + 2), mm.DeviceBuffer(self.k + off + 2)

    def call(self, v):
        o = 8 * self.off
        return lib.mvg_gemv_ata_variant(self.A.ptr + o, self.lda, self.x.ptr + o, self.t.ptr + o, self.w.ptr + o, self.m,
                                        self.k, v, None)

    def run(self, v):
        """(t, w) of variant v; None where k exceeds its max_k, after asserting the refusal."""
        self.t.upload(np.full(self.t.n, np.nan))
        self.w.upload(np.full(self.w.n, np.nan))
        rc = self.call(v)
        sync()
        ti, wi = self.t.download(), self.w.download()
        if not applies(v, self.k):
            assert rc == _lib.MVG_E_INVALID, (name(v), self.k, rc)
            assert np.all(np.isnan(ti)) and np.all(np.isnan(wi)), "a refused call stored something"
            return None
        assert rc == _lib.MVG_OK, (name(v), rc, lib.mvg_last_error().decode())
        off = self.off
        assert np.all(np.isnan(ti[:off])) and np.all(np.isnan(ti[off + self.m:])), "stored outside t"
        assert np.all(np.isnan(wi[:off])) and np.all(np.isnan(wi[off + self.k:])), "stored outside w"
        return ti[off:off + self.m], wi[off:off + self.k]

    def free(self):
        for b in (self.A, self.x, self.t, self.w):
            b.free()


def run_both(m, k, variants, lda=None, off=0, do_signed=True):
    """Every variant in `variants` on the synth and the signed m x k problem; returns how many ran."""
    A, x, want = synth(m, k)
    d = Dev(A, x, lda=lda, off=off)
    ds = Dev(*signed(m, k)[:2], lda=lda, off=off) if do_signed else None
    ran = 0
    try:
        for v in variants:
            got = d.run(v)
            if got is None:
                continue
            ran += 1
            check_synth(A, *got, want, f"{name(v)} {m}x{k}")
            if ds:
                As, _, want_s, scale = signed(m, k)
                check_signed(As, *ds.run(v), want_s, scale, f"{name(v)} {m}x{k}")
    finally:
        d.free()
        if ds:
            ds.free()
    return ran


@pytest.mark.parametrize("m,k", SHAPES)
def test_every_variant_on_synth_and_signed_data(m, k):
    ran = run_both(m, k, VARIANTS)
    assert ran == sum(applies(v, k) for v in VARIANTS)


def test_every_fused_variant_runs_at_least_12_of_the_fixed_shapes():
    for v in FUSED:
        if name(v).startswith("wrow_"):
            assert max_k(v) >= 128, name(v)
        assert sum(k <= max_k(v) for _, k in SHAPES) >= 12, name(v)


@pytest.mark.parametrize("v", FUSED, ids=name)
def test_at_the_variants_own_limits(v):
    """k just under and at max_k (the whole-row kernel and the one cut by k), and three bands."""
    mk = max_k(v)
    band_rows = mm.gemv_ata_plan(65, 1000, 65, v)[0]
    for m, k in [(37, mk - 1), (37, mk), (2 * band_rows + 1, 65)]:
        assert run_both(m, k, [v]) == 1
    assert mm.gemv_ata_plan(65, 2 * band_rows + 1, 65, v)[:2] == (band_rows, 3)
    d = Dev(*synth(37, mk + 1)[:2])  # one column more: refused, nothing stored
    try:
        assert d.run(v) is None
    finally:
        d.free()


def test_two_pass_is_the_composed_pair_bit_for_bit():
    """t is mvg_gemv's y on the same operands and w is mvg_gemv_t's y on that t: what the
    definition means."""
    for m, k in [(257, 255), (1000, 257), (7, 1000), (4099, 129)]:
        for A, x in (synth(m, k)[:2], signed(m, k)[:2]):
            d = Dev(A, x)
            y, yt = mm.DeviceBuffer(m), mm.DeviceBuffer(k)
            try:
                t, w = d.run(TWO_PASS)
                mm.gemv(d.A.ptr, k, d.x.ptr, y.ptr, m, k)
                mm.gemv_t(d.A.ptr, k, d.t.ptr, yt.ptr, m, k)
                sync()
                assert np.array_equal(_bits(t), _bits(y.download())), (m, k)
                assert np.array_equal(_bits(w), _bits(yt.download())), (m, k)
                auto = d.run(0)
                if lib.mvg_gemv_ata_auto_variant(k, m, k) == TWO_PASS:
                    assert np.array_equal(_bits(auto[0]), _bits(t)) and np.array_equal(_bits(auto[1]), _bits(w))
            finally:
                for b in (y, yt):
                    b.free()
                d.free()


@pytest.mark.parametrize("v", FUSED, ids=name)
def test_band_edges(v):
    """m around one and two bands, as mvg_gemv_ata_plan cuts each m, k around a 64-column chunk."""
    band_rows = mm.gemv_ata_plan(129, 1000, 129, v)[0]
    for m in (band_rows - 1, band_rows, band_rows + 1, 2 * band_rows + 1):
        for k in (63, 64, 65, 129):
            if not applies(v, k):
                continue
            b, bands, _ = mm.gemv_ata_plan(k, m, k, v)
            assert b == band_rows and bands == -(-m // band_rows), (name(v), m, k, b, bands)
            assert run_both(m, k, [v]) == 1


@pytest.mark.parametrize("m,k,lda,off", [(70, 300, 512, 0), (70, 300, 301, 1), (257, 1000, 1000, 1)],
                         ids=["lda>k", "odd-lda-off8", "even-lda-off8"])
def test_views(m, k, lda, off):
    """A sub-block view (lda > k); an odd lda; A, x, t and w each 8 bytes off a 16-B boundary."""
    assert run_both(m, k, VARIANTS, lda=lda, off=off, do_signed=False) == sum(applies(v, k) for v in VARIANTS)


def test_wide_view_rows_2_to_the_26_doubles_apart():
    """64-bit row offsets: 5 rows of 130 columns, 512 MiB apart (the last starts 2 GiB in), each
    between NaN fringes (tests/wide_views.py FAR_A is the model)."""
    m, k, lda, fringe = 5, 130, 1 << 26, G.GUARD
    A, x, want = synth(m, k)
    p = ctypes.c_void_p()
    _lib.check(lib.mvg_malloc(ctypes.byref(p), 8 * ((m - 1) * lda + k + 2 * fringe)), "mvg_malloc")
    dx, dt, dw = mm.DeviceBuffer(k).upload(x), mm.DeviceBuffer(m), mm.DeviceBuffer(k)
    try:
        for i in range(m):
            row = np.full(k + 2 * fringe, np.nan)
            row[fringe:fringe + k] = A[i]
            _lib.check(lib.mvg_memcpy_h2d(p.value + 8 * i * lda, row.ctypes.data, row.nbytes, None), "h2d")
        sync()
        for v in VARIANTS:
            if not applies(v, k):
                continue
            dt.upload(np.full(m, np.nan))
            dw.upload(np.full(k, np.nan))
            mm.gemv_ata(p.value + 8 * fringe, lda, dx.ptr, dt.ptr, dw.ptr, m, k, None, v)
            sync()
            check_synth(A, dt.download(), dw.download(), want, name(v))
    finally:
        lib.mvg_free(p.value)
        for b in (dx, dt, dw):
            b.free()


@pytest.mark.parametrize("m,k,pad,shift", [(257, 255, 9, 0), (70, 300, 1, 1), (33, 513, 2, 0)])
def test_guarded_operands(m, k, pad, shift):
    """NaN around A, x, t and w and in every padding column of A: a read outside A[i, 0..k) or
    x[0..k) turns sums into NaN, a store outside t[0..m) or w[0..k) replaces a NaN of their images."""
    A, x, want = synth(m, k)
    gA, gx = G.matrix(A, pad, shift), G.vectors(x, k + pad, shift)
    gt, gw = G.result(1, m, m + pad, spare=1), G.result(1, k, k + pad, spare=1)
    try:
        for v in VARIANTS:
            if not applies(v, k):
                continue
            gt.fill()
            gw.fill()
            mm.gemv_ata(gA.ptr, k + pad, gx.ptr, gt.ptr, gw.ptr, m, k, None, v)
            sync()
            G.assert_clean(gt.image(), gt.lay, lambda got: np.abs(got - want) <= TOL * np.abs(want), name(v) + " t")
            want_w = ref_w(A, gt.lay.payload(gt.image())[0])
            G.assert_clean(gw.image(), gw.lay, lambda got: np.abs(got - want_w) <= TOL * np.abs(want_w), name(v) + " w")
    finally:
        for g in (gA, gx, gt, gw):
            g.free()


def test_a_nan_reaches_its_row_of_t_and_all_of_w():
    m, k, i, j = 300, 600, 171, 333  # several bands; every x[j] > 0
    A, x, _ = synth(m, k)
    x = x + 0.5
    B = A.copy()
    B[i, j] = np.nan
    for v in VARIANTS:
        if not applies(v, k):
            continue
        (t0, _), (t1, w1) = mm.multiply_ata(A, x, variant=v), mm.multiply_ata(B, x, variant=v)
        others = np.arange(m) != i
        assert np.isnan(t1[i]), (name(v), t1[i])
        assert np.array_equal(_bits(t1[others]), _bits(t0[others])), name(v)
        assert np.all(np.isnan(w1)), name(v)


def test_empty_sums():
    m, k = 200, 100  # k within every fused variant's max_k
    one = mm.DeviceBuffer(4).upload(np.ones(4))
    t, w = mm.DeviceBuffer(m + 2), mm.DeviceBuffer(k + 2)
    try:
        for v in VARIANTS:
            t.upload(np.full(m + 2, np.nan))
            w.upload(np.full(k + 2, np.nan))
            mm.gemv_ata(one.ptr, k, one.ptr, t.ptr, w.ptr + 8, 0, k, None, v)  # m == 0: k zeros over the poison
            sync()
            img = w.download()
            assert np.isnan(img[0]) and np.isnan(img[-1]) and np.array_equal(img[1:-1], np.zeros(k)), name(v)
            assert np.all(np.isnan(t.download())), name(v)  # t untouched
            w.upload(np.full(k + 2, np.nan))
            mm.gemv_ata(None, 0, None, t.ptr + 8, None, m, 0, None, v)  # k == 0: m zeros, null A, x and w
            sync()
            img = t.download()
            assert np.isnan(img[0]) and np.isnan(img[-1]) and np.array_equal(img[1:-1], np.zeros(m)), name(v)
            assert np.all(np.isnan(w.download())), name(v)  # w untouched
            mm.gemv_ata(None, 0, None, None, None, 0, 0, None, v)  # both zero: a no-op
            sync()
    finally:
        for b in (one, t, w):
            b.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_deterministic_and_independent_of_the_workspace():
    """The same call twice; a call after others that leave the (null stream's) workspace dirty and
    make it regrow; every variant on two fresh sets of buffers: the same bits every time."""
    shapes = [(4099, 129), (257, 1000), (20001, 7)]
    data = {s: signed(*s)[:2] for s in shapes}
    devs = {s: Dev(*data[s]) for s in shapes}
    first_shape = shapes[0]
    try:
        for v in FUSED:
            assert mm.gemv_ata_plan(129, 4099, 129, v)[1] > 1, name(v)
        for v in VARIANTS:
            if not applies(v, 129):
                continue
            first = devs[first_shape].run(v)  # before this variant's larger shapes have dirtied the workspace
            again = devs[first_shape].run(v)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, again)), name(v)
            for s in shapes[1:]:
                devs[s].run(v)  # dirties and regrows (or is refused by max_k: asserted in run)
                devs[s].run(TWO_PASS)
            after = devs[first_shape].run(v)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, after)), name(v)
            fresh = Dev(*data[first_shape])
            try:
                b = fresh.run(v)
            finally:
                fresh.free()
            assert all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(first, b)), name(v)
    finally:
        for d in devs.values():
            d.free()


def test_multiply_ata_returns_t_and_w():
    A, x, want = synth(255, 257)
    t, w = mm.multiply_ata(A, x)
    assert t.shape == (255,) and w.shape == (257,)
    check_synth(A, t, w, want, "multiply_ata")
    with pytest.raises(ValueError):
        mm.multiply_ata(A, x[:-1])
