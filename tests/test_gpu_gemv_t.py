"""mvg_gemv_t on the GPU: every variant and the automatic pick, through mm.multiply_t (host arrays)
and mm.gemv_t (device pointers), against the sequential sum over the rows — the oracle's
multiply_std_rowwise on a contiguous transposed copy.

Bars: on oracle.synth data (non-negative) max_rel <= 1e-12 per element; on signed uniform data
|y - y_ref| <= 1e-13 * (|A|^T |z|) per column, the bar and the generator of
tests/test_gpu_parity.py::test_gemv_all_variants_on_signed_data: the forward-error bound of a sum of
m products is m * eps * sum|.| (2.2e-12 at m = 20001), and a fixed order of short FMA chains does
far better.
"""
import ctypes

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
NVAR = lib.mvg_gemv_t_variant_count()
VARIANTS = list(range(NVAR))

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (5, 7), (63, 129), (64, 128), (65, 127), (255, 257), (256, 256), (257, 255),
          (1000, 257), (257, 1000), (513, 130), (100, 1), (1, 4096), (7, 20001), (20001, 7), (4099, 129), (65538, 3)]


def name(v):
    return lib.mvg_gemv_t_variant_name(v).decode()


def ref(A, z):
    return oracle.multiply_std_rowwise(np.ascontiguousarray(A.T), z)


def synth(m, k):
    A, z = oracle.synth(m, k, 42), oracle.synth(1, m, 4343)[0]
    return A, z, ref(A, z)


def signed(m, k):
    rng = np.random.default_rng(m * 7919 + k)
    A, z = rng.uniform(-1.0, 1.0, size=(m, k)), rng.uniform(-1.0, 1.0, size=m)
    return A, z, ref(A, z), np.abs(A).T @ np.abs(z)


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


class Dev:
    """A, z on the device (rows lda apart, everything `off` doubles into its buffer) and a y."""

    def __init__(self, A, z, lda=None, off=0):
        self.m, self.k = A.shape
        self.lda, self.off = lda or self.k, off
        img = np.full(self.m * self.lda + off + 2, np.nan)
        img[off + np.arange(self.m)[:, None] * self.lda + np.arange(self.k)[None, :]] = A
        zi = np.full(self.m + off + 2, np.nan)
        zi[off:off + self.m] = z
        self.A, self.z = mm.DeviceBuffer(img.size).upload(img), mm.DeviceBuffer(zi.size).upload(zi)
        self.y = mm.DeviceBuffer(self.k + off + 2)

    def run(self, v):
        self.y.upload(np.full(self.y.n, np.nan))
        mm.gemv_t(self.A.ptr + 8 * self.off, self.lda, self.z.ptr + 8 * self.off, self.y.ptr + 8 * self.off, self.m, self.k,
                  None, v)
        sync()
        img = self.y.download()
        assert np.all(np.isnan(img[:self.off])) and np.all(np.isnan(img[self.off + self.k:])), "stored outside y"
        return img[self.off:self.off + self.k]

    def free(self):
        for b in (self.A, self.z, self.y):
            b.free()


@pytest.mark.parametrize("m,k", SHAPES)
def test_every_variant_on_synth_and_signed_data(m, k):
    A, z, want = synth(m, k)
    As, zs, want_s, scale = signed(m, k)
    for v in VARIANTS:
        y = mm.multiply_t(A, z, variant=v)
        print(f"{name(v)} {m}x{k}: synth max_rel {max_rel(y, want):.3e}")
        assert y.shape == (k,) and max_rel(y, want) <= TOL, (name(v), m, k, max_rel(y, want))
        ys = mm.multiply_t(As, zs, variant=v)
        err = float(np.max(np.abs(ys - want_s) / scale))
        print(f"{name(v)} {m}x{k}: signed err {err:.3e}")
        assert err <= SIGNED_TOL, (name(v), m, k, err)


@pytest.mark.parametrize("v", VARIANTS, ids=name)
def test_band_and_strip_edges(v):
    """m around one and two bands, k around one and two strips, as mvg_gemv_t_plan cuts them."""
    band_rows, _, strip_cols = mm.gemv_t_plan(1000, 1000, 1000, v)
    for m in (band_rows - 1, band_rows, band_rows + 1, 2 * band_rows + 1):
        for k in (strip_cols - 1, strip_cols, strip_cols + 1, 2 * strip_cols + 1):
            b, bands, sc = mm.gemv_t_plan(k, m, k, v)
            assert (b, sc) == (band_rows, strip_cols) and bands == -(-m // band_rows), (name(v), m, k, b, bands, sc)
            A, z, want = synth(m, k)
            As, zs, want_s, scale = signed(m, k)
            d, ds = Dev(A, z), Dev(As, zs)
            try:
                y, ys = d.run(v), ds.run(v)
            finally:
                d.free()
                ds.free()
            assert max_rel(y, want) <= TOL, (name(v), m, k, max_rel(y, want))
            err = float(np.max(np.abs(ys - want_s) / scale))
            assert err <= SIGNED_TOL, (name(v), m, k, err)


@pytest.mark.parametrize("m,k", [(25_601, 257), (2_097_153, 3)], ids=["256-row-bands", "512-row-bands"])
def test_tall_bands(m, k):
    """From 25 600 rows on the bands are 256 rows: every wave runs its unrolled main loop, on whole
    strips and on the strip cut by k = 257. At 2 097 153 x 3 the _b2048 variants (and the automatic
    pick) take 512-row bands; the others keep 256."""
    for v in VARIANTS:
        b = mm.gemv_t_plan(k, m, k, v)[0]
        assert b == (512 if m > 2_000_000 and ("_b2048" in name(v) or v == 0) else 256), (name(v), b)
    A, z, want = synth(m, k)
    As, zs, want_s, scale = signed(m, k)
    d, ds = Dev(A, z), Dev(As, zs)
    try:
        for v in VARIANTS:
            y, ys = d.run(v), ds.run(v)
            assert max_rel(y, want) <= TOL, (name(v), m, k, max_rel(y, want))
            err = float(np.max(np.abs(ys - want_s) / scale))
            assert err <= SIGNED_TOL, (name(v), m, k, err)
    finally:
        d.free()
        ds.free()


@pytest.mark.parametrize("m,k,lda,off", [(70, 300, 512, 0), (70, 300, 301, 1), (257, 1000, 1000, 1)],
                         ids=["lda>k", "odd-lda-off8", "even-lda-off8"])
def test_views(m, k, lda, off):
    """A sub-block view (lda > k); an odd lda; A, z and y each 8 bytes off a 16-B boundary."""
    A, z, want = synth(m, k)
    d = Dev(A, z, lda=lda, off=off)
    try:
        for v in VARIANTS:
            y = d.run(v)
            assert max_rel(y, want) <= TOL, (name(v), m, k, lda, off, max_rel(y, want))
    finally:
        d.free()


def test_wide_view_rows_2_to_the_26_doubles_apart():
    """64-bit row offsets: 5 rows of 130 columns, 512 MiB apart (the last starts 2 GiB in), each
    between NaN fringes (tests/wide_views.py FAR_A is the model)."""
    m, k, lda, fringe = 5, 130, 1 << 26, G.GUARD
    A, z, want = synth(m, k)
    p = ctypes.c_void_p()
    _lib.check(lib.mvg_malloc(ctypes.byref(p), 8 * ((m - 1) * lda + k + 2 * fringe)), "mvg_malloc")
    dz, dy = mm.DeviceBuffer(m).upload(z), mm.DeviceBuffer(k)
    try:
        for i in range(m):
            row = np.full(k + 2 * fringe, np.nan)
            row[fringe:fringe + k] = A[i]
            _lib.check(lib.mvg_memcpy_h2d(p.value + 8 * i * lda, row.ctypes.data, row.nbytes, None), "h2d")
        sync()
        for v in VARIANTS:
            dy.upload(np.full(k, np.nan))
            mm.gemv_t(p.value + 8 * fringe, lda, dz.ptr, dy.ptr, m, k, None, v)
            sync()
            assert max_rel(dy.download(), want) <= TOL, name(v)
    finally:
        lib.mvg_free(p.value)
        dz.free()
        dy.free()


@pytest.mark.parametrize("m,k,pad,shift", [(257, 255, 9, 0), (70, 300, 1, 1), (33, 513, 2, 0)])
def test_guarded_operands(m, k, pad, shift):
    """NaN around A, z and y and in every padding column of A: a read outside A[i, 0..k) or
    z[0..m) turns a sum into NaN, a store outside y[0..k) replaces a NaN of y's image."""
    A, z, want = synth(m, k)
    gA, gz, gy = G.matrix(A, pad, shift), G.vectors(z, m + pad, shift), G.result(1, k, k + pad, spare=1)
    try:
        for v in VARIANTS:
            gy.fill()
            mm.gemv_t(gA.ptr, k + pad, gz.ptr, gy.ptr, m, k, None, v)
            sync()
            G.assert_clean(gy.image(), gy.lay, lambda got: np.abs(got - want) <= TOL * np.abs(want), name(v))
    finally:
        for g in (gA, gz, gy):
            g.free()


@pytest.mark.parametrize("special", [np.nan, np.inf])
def test_a_special_value_reaches_exactly_its_column(special):
    m, k, i, j = 300, 600, 171, 333  # several bands and strips; every z[i] > 0
    A, z, _ = synth(m, k)
    z = z + 0.5
    B = A.copy()
    B[i, j] = special
    for v in VARIANTS:
        clean, hit = mm.multiply_t(A, z, variant=v), mm.multiply_t(B, z, variant=v)
        others = np.arange(k) != j
        assert np.array_equal(hit[others].view(np.uint64), clean[others].view(np.uint64)), name(v)
        assert np.isnan(hit[j]) if np.isnan(special) else hit[j] == np.inf, (name(v), hit[j])


def test_empty_sums():
    k = 300
    z = mm.DeviceBuffer(4).upload(np.ones(4))
    A = mm.DeviceBuffer(4).upload(np.ones(4))
    y = mm.DeviceBuffer(k + 2)
    try:
        for v in VARIANTS:
            y.upload(np.full(k + 2, np.nan))
            mm.gemv_t(A.ptr, k, z.ptr, y.ptr + 8, 0, k, None, v)  # m == 0: k zeros over the poison
            sync()
            img = y.download()
            assert np.isnan(img[0]) and np.isnan(img[-1]) and np.array_equal(img[1:-1], np.zeros(k)), name(v)
            y.upload(np.full(k + 2, np.nan))
            mm.gemv_t(A.ptr, 0, z.ptr, y.ptr, 4, 0, None, v)  # k == 0: y untouched
            sync()
            assert np.all(np.isnan(y.download())), name(v)
    finally:
        for b in (A, z, y):
            b.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_deterministic_and_independent_of_the_workspace():
    """The same call twice; a call after others that leave the (null stream's) workspace dirty and
    make it regrow; explicit variants on two fresh sets of buffers: the same bits every time."""
    shapes = [(4099, 129), (257, 1000), (20001, 7)]
    data = {s: signed(*s)[:2] for s in shapes}
    devs = {s: Dev(*data[s]) for s in shapes}
    try:
        first = devs[4099, 129].run(0)  # before anything larger has grown or dirtied the workspace
        assert mm.gemv_t_plan(129, 4099, 129)[1] > 1
        assert np.array_equal(_bits(devs[4099, 129].run(0)), _bits(first))
        devs[257, 1000].run(0)
        devs[20001, 7].run(0)
        assert np.array_equal(_bits(devs[4099, 129].run(0)), _bits(first))
        for v in VARIANTS[1:]:
            a = devs[4099, 129].run(v)
            devs[257, 1000].run(v)
            fresh = Dev(*data[4099, 129])
            try:
                b = fresh.run(v)
            finally:
                fresh.free()
            assert np.array_equal(_bits(a), _bits(b)), name(v)
    finally:
        for d in devs.values():
            d.free()
