"""mvg_gemv_t_multi on the GPU: every variant and the automatic pick, through mm.multiply_t_multi
(host arrays) and mm.gemv_t_multi (device pointers), against the sequential sum over the rows per
column — the oracle's multiply_std_rowwise on a contiguous transposed copy of A and Z[:, v].

Bars (tests/test_gpu_gemv_t.py's, unchanged): on oracle.synth data (non-negative) max_rel <= 1e-12
per element; on signed uniform data |y - y_ref| <= 1e-13 * (|A|^T |z_v|) per column.
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
NVAR = lib.mvg_gemv_t_multi_variant_count()
VARIANTS = list(range(NVAR))
SEPARATE = 1
FUSED = VARIANTS[2:]


def name(v):
    return lib.mvg_gemv_t_multi_variant_name(v).decode()


def chains(v):
    """A fused variant's chain count; 2 for auto and separate (any nv serves them alike)."""
    hit = re.search(r"_v(\d+)$", name(v))
    return int(hit.group(1)) if hit else 2


def ref(A, Z):
    At = np.ascontiguousarray(A.T)
    return np.stack([oracle.multiply_std_rowwise(At, np.ascontiguousarray(Z[:, v])) for v in range(Z.shape[1])], axis=1)


@functools.lru_cache(maxsize=64)
def synth(m, k, nv):
    A, Z = oracle.synth(m, k, 42), np.ascontiguousarray(oracle.synth(nv, m, 4343).T)
    return A, Z, ref(A, Z)


@functools.lru_cache(maxsize=64)
def signed(m, k, nv):
    rng = np.random.default_rng(m * 7919 + k)
    A, Z = rng.uniform(-1.0, 1.0, size=(m, k)), rng.uniform(-1.0, 1.0, size=(m, nv))
    return A, Z, ref(A, Z), np.abs(A).T @ np.abs(Z)


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cached_inputs_after_the_module():
    yield
    synth.cache_clear()
    signed.cache_clear()


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_synth(Y, want, what):
    assert Y.shape == want.shape, (what, Y.shape)
    err = max(max_rel(Y[:, c], want[:, c]) for c in range(want.shape[1])) if want.size else 0.0
    print(f"{what}: synth max_rel {err:.3e}")
    assert err <= TOL, (what, err)


def check_signed(Y, want, scale, what):
    assert Y.shape == want.shape, (what, Y.shape)
    err = float(np.max(np.abs(Y - want) / scale)) if want.size else 0.0
    print(f"{what}: signed err {err:.3e}")
    assert err <= SIGNED_TOL, (what, err)


class Dev:
    """A (rows lda apart), Z (vectors ldz apart) and a Y (vectors ldy apart) on the device, each `off`
    doubles into its buffer; everything around the payloads is NaN."""

    def __init__(self, A, Z, lda=None, ldz=None, ldy=None, off=0):
        self.m, self.k = A.shape
        self.nv = Z.shape[1]
        self.lda, self.ldz, self.ldy, self.off = lda or self.k, ldz or self.m, ldy or self.k, off
        if self.lda == self.k:
            img = np.concatenate([np.full(off, np.nan), A.ravel(), np.full(2, np.nan)])
        else:
            img = np.full(self.m * self.lda + off + 2, np.nan)
            img[off + np.arange(self.m)[:, None] * self.lda + np.arange(self.k)[None, :]] = A
        zi = np.full(self.nv * self.ldz + off + 2, np.nan)
        zi[off + np.arange(self.nv)[:, None] * self.ldz + np.arange(self.m)[None, :]] = Z.T
        self.A, self.Z = mm.DeviceBuffer(img.size).upload(img), mm.DeviceBuffer(zi.size).upload(zi)
        self.Y = mm.DeviceBuffer((self.nv + 1) * self.ldy + off + 2)  # a spare column no call may touch

    def set_z(self, Z):
        zi = np.full(self.Z.n, np.nan)
        zi[self.off + np.arange(self.nv)[:, None] * self.ldz + np.arange(self.m)[None, :]] = Z.T
        self.Z.upload(zi)

    def run(self, v, nv=None, first=0):
        """Vectors first .. first + nv - 1 through variant v: the k x nv result, after checking that
        nothing outside it was stored."""
        nv = self.nv - first if nv is None else nv
        self.Y.upload(np.full(self.Y.n, np.nan))
        mm.gemv_t_multi(self.A.ptr + 8 * self.off, self.lda, self.Z.ptr + 8 * (self.off + first * self.ldz), self.ldz,
                        self.Y.ptr + 8 * self.off, self.ldy, self.m, self.k, nv, None, v)
        sync()
        img = self.Y.download()
        pay = np.zeros(img.size, dtype=bool)
        pay[(self.off + np.arange(nv)[:, None] * self.ldy + np.arange(self.k)[None, :]).ravel()] = True
        assert np.all(np.isnan(img[~pay])), (name(v), "stored outside Y")
        return img[self.off:self.off + nv * self.ldy].reshape(nv, self.ldy)[:, :self.k].T.copy() if nv else np.zeros((self.k, 0))

    def free(self):
        for b in (self.A, self.Z, self.Y):
            b.free()


# tests/test_gpu_gemv_t.py's SHAPES by class, and the group boundaries: every nv meets every class once
CLASSES = {
    "tiny": [(1, 1), (1, 2), (2, 1), (3, 5), (5, 7)],
    "one-strip": [(63, 129), (64, 128), (65, 127), (100, 1)],
    "bands-and-strips": [(255, 257), (256, 256), (257, 255), (513, 130)],
    "wide": [(257, 1000), (1, 4096), (7, 20001)],
    "tall": [(1000, 257), (20001, 7), (4099, 129), (65538, 3)],
}
NVS = [1, 2, 3, 4, 5, 8, 9, 16, 17]
CASES = [(*shapes[i % len(shapes)], nv) for shapes in CLASSES.values() for i, nv in enumerate(NVS)]


def test_the_pruned_cross_product_covers_every_shape_and_every_nv_per_class():
    assert sorted({(m, k) for m, k, _ in CASES}) == sorted(s for shapes in CLASSES.values() for s in shapes)
    for shapes in CLASSES.values():
        assert sorted(nv for m, k, nv in CASES if (m, k) in shapes) == NVS


@pytest.mark.parametrize("m,k,nv", CASES)
def test_every_variant_on_synth_and_signed_data(m, k, nv):
    A, Z, want = synth(m, k, nv)
    As, Zs, want_s, scale = signed(m, k, nv)
    for v in VARIANTS:
        check_synth(mm.multiply_t_multi(A, Z, variant=v), want, f"{name(v)} {m}x{k} nv={nv}")
        check_signed(mm.multiply_t_multi(As, Zs, variant=v), want_s, scale, f"{name(v)} {m}x{k} nv={nv}")


@pytest.mark.parametrize("v", VARIANTS, ids=name)
def test_band_and_strip_edges(v):
    """m around one and two bands, k around one and two strips, as mvg_gemv_t_multi_plan cuts them, at
    a full group and at one vector less (a short group), on device pointers with Y inside NaN."""
    NV = chains(v)
    band_rows, _, strip_cols, group = mm.gemv_t_multi_plan(1000, 1000, 1000, NV, v)
    assert group == (NV if v in FUSED else 1)
    for m in (band_rows - 1, band_rows, band_rows + 1, 2 * band_rows + 1):
        for k in (strip_cols - 1, strip_cols, strip_cols + 1, 2 * strip_cols + 1):
            b, bands, sc, _ = mm.gemv_t_multi_plan(k, m, k, NV, v)
            assert (b, sc) == (band_rows, strip_cols) and bands == -(-m // band_rows), (name(v), m, k, b, bands, sc)
            A, Z, want = synth(m, k, NV)
            As, Zs, want_s, scale = signed(m, k, NV)
            d, ds = Dev(A, Z), Dev(As, Zs)
            try:
                for nv in (NV, NV - 1):
                    what = f"{name(v)} {m}x{k} nv={nv}"
                    check_synth(d.run(v, nv), want[:, :nv], what)
                    check_signed(ds.run(v, nv), want_s[:, :nv], scale[:, :nv], what)
            finally:
                d.free()
                ds.free()


def test_tall_bands():
    """The bands reach the height the plan picks for 16 chains at the swept shapes (128 rows per
    chain), on whole strips and on the strip cut by k = 257: the smallest m at which 5 strips of 64
    columns still leave 512 workgroups."""
    v16 = next(v for v in FUSED if name(v).endswith("_c1_u2_v16"))
    tall = mm.gemv_t_multi_plan(16384, 16384, 16384, 16, v16)[0]
    assert tall == mm.gemv_t_multi_plan(512, 524288, 512, 16, v16)[0] == 2048
    k = 257
    m = (-(-512 // 5) - 1) * tall + 1
    assert mm.gemv_t_multi_plan(k, m, k, 16, v16)[:3] == (tall, 103, 64)
    for v in FUSED:  # the 128-column strips (3 of them) settle for half that height, no less
        assert mm.gemv_t_multi_plan(k, m, k, chains(v), v)[0] >= 64 * chains(v), name(v)
    As, Zs, want_s, scale = signed.__wrapped__(m, k, 16)  # 430 MB: not kept
    d = Dev(As, Zs)
    try:
        for v in VARIANTS:
            check_signed(d.run(v), want_s, scale, f"{name(v)} {m}x{k}")
    finally:
        d.free()


@pytest.mark.parametrize("m,k,lda,ldz,ldy,off", [(70, 300, 512, 75, 333, 0), (70, 300, 301, 71, 301, 1),
                                                 (257, 1000, 1000, 259, 1001, 1)],
                         ids=["lda>k", "odd-ld-off8", "even-lda-off8"])
def test_views(m, k, lda, ldz, ldy, off):
    """A sub-block view (lda > k), odd lda, ldz > m and ldy > k with odd values; A, Z and Y each 8
    bytes off a 16-B boundary. nv = 5: two groups and a single vector, a group and a single vector,
    or one short group."""
    A, Z, want = synth(m, k, 5)
    d = Dev(A, Z, lda=lda, ldz=ldz, ldy=ldy, off=off)
    try:
        for v in VARIANTS:
            check_synth(d.run(v), want, f"{name(v)} {m}x{k} lda={lda} ldz={ldz} ldy={ldy} off={off}")
    finally:
        d.free()


def _malloc(n):
    p = ctypes.c_void_p()
    _lib.check(lib.mvg_malloc(ctypes.byref(p), 8 * n), "mvg_malloc")
    return p.value


def _put(dst, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    _lib.check(lib.mvg_memcpy_h2d(dst, a.ctypes.data, a.nbytes, None), "h2d")


def _get(src, n):
    out = np.empty(n)
    _lib.check(lib.mvg_memcpy_d2h(out.ctypes.data, src, 8 * n, None), "d2h")
    sync()
    return out


def test_wide_view_rows_2_to_the_26_doubles_apart():
    """64-bit row offsets: 5 rows of 130 columns, 512 MiB apart (the last starts 2 GiB in), each
    between NaN fringes (tests/test_gpu_gemv_t.py's wide view), times 3 vectors."""
    m, k, nv, lda, fringe = 5, 130, 3, 1 << 26, G.GUARD
    A, Z, want = synth(m, k, nv)
    p = _malloc((m - 1) * lda + k + 2 * fringe)
    dZ, dY = mm.DeviceBuffer(m * nv).upload(Z.T), mm.DeviceBuffer(k * nv)
    try:
        for i in range(m):
            row = np.full(k + 2 * fringe, np.nan)
            row[fringe:fringe + k] = A[i]
            _put(p + 8 * i * lda, row)
        sync()
        for v in VARIANTS:
            dY.upload(np.full(k * nv, np.nan))
            mm.gemv_t_multi(p + 8 * fringe, lda, dZ.ptr, m, dY.ptr, k, m, k, nv, None, v)
            sync()
            check_synth(dY.download().reshape(nv, k).T, want, name(v))
    finally:
        lib.mvg_free(p)
        dZ.free()
        dY.free()


def test_vectors_2_to_the_27_doubles_apart():
    """64-bit vector offsets: ldz = ldy = 2^27 doubles (1 GiB), 3 vectors, each between NaN fringes:
    the third vector of Z and of Y starts 2 GiB into its buffer."""
    m, k, nv, ld, fringe = 300, 200, 3, 1 << 27, G.GUARD
    A, Z, want = synth(m, k, nv)
    pz, py = _malloc((nv - 1) * ld + m + 2 * fringe), _malloc((nv - 1) * ld + k + 2 * fringe)
    dA = mm.DeviceBuffer(m * k).upload(A)
    try:
        for c in range(nv):
            col = np.full(m + 2 * fringe, np.nan)
            col[fringe:fringe + m] = Z[:, c]
            _put(pz + 8 * c * ld, col)
        sync()
        for v in VARIANTS:
            for c in range(nv):
                _put(py + 8 * c * ld, np.full(k + 2 * fringe, np.nan))
            sync()
            mm.gemv_t_multi(dA.ptr, k, pz + 8 * fringe, ld, py + 8 * fringe, ld, m, k, nv, None, v)
            sync()
            got = [_get(py + 8 * c * ld, k + 2 * fringe) for c in range(nv)]
            for g in got:
                assert np.all(np.isnan(g[:fringe])) and np.all(np.isnan(g[fringe + k:])), (name(v), "stored outside Y")
            check_synth(np.stack([g[fringe:fringe + k] for g in got], axis=1), want, name(v))
    finally:
        for p in (pz, py):
            lib.mvg_free(p)
        dA.free()


@pytest.mark.parametrize("m,k,nv,pad,shift", [(257, 255, 4, 9, 0), (70, 300, 5, 1, 1), (33, 513, 17, 2, 0)])
def test_guarded_operands(m, k, nv, pad, shift):
    """NaN around A, Z and Y, in every padding column of A and in the gaps of Z and Y: a read outside
    A[i, 0..k) or Z[0..m, v) turns a sum into NaN, a store outside Y[0..k, v) replaces a NaN of Y's
    image (the gaps between the columns and a spare column after the last included)."""
    A, Z, want = synth(m, k, nv)
    gA, gZ, gY = G.matrix(A, pad, shift), G.vectors(Z.T, m + pad, shift), G.result(nv, k, k + pad, spare=1)
    try:
        for v in VARIANTS:
            gY.fill()
            mm.gemv_t_multi(gA.ptr, k + pad, gZ.ptr, m + pad, gY.ptr, k + pad, m, k, nv, None, v)
            sync()
            G.assert_clean(gY.image(), gY.lay, lambda got: np.abs(got - want.T) <= TOL * np.abs(want.T), name(v))
    finally:
        for g in (gA, gZ, gY):
            g.free()


@pytest.mark.parametrize("v", VARIANTS, ids=name)
def test_a_column_does_not_depend_on_the_other_columns_or_on_its_place(v):
    """Column c's bits with every other column replaced (by other numbers, by NaN), and with the same
    vector at another place of a group of the same kernel: last of a full group, first of a second
    group (two vectors long), first of a short group."""
    NV = chains(v)
    m, k = 300, 200  # several bands and strips
    assert mm.gemv_t_multi_plan(k, m, k, NV, v)[1] > 1
    A, Z, _, _ = signed(m, k, 2 * NV)
    Z = Z.copy()
    z = Z[:, NV - 1].copy()
    d = Dev(A, Z)
    try:
        base = d.run(v, NV)[:, NV - 1]
        assert not np.any(np.isnan(base))
        others = np.arange(2 * NV) != NV - 1
        Z2 = Z.copy()
        Z2[:, others] = np.random.default_rng(5).uniform(-3.0, 3.0, size=(m, 2 * NV - 1))
        d.set_z(Z2)
        assert np.array_equal(bits(d.run(v, NV)[:, NV - 1]), bits(base)), name(v)
        Z2[:, others] = np.nan
        d.set_z(Z2)
        Y = d.run(v, NV)
        assert np.array_equal(bits(Y[:, NV - 1]), bits(base)), name(v)
        assert np.all(np.isnan(Y[:, :NV - 1])), name(v)
        # another place: column NV of NV + 2 vectors opens the second group
        Z3 = Z.copy()
        Z3[:, NV] = z
        d.set_z(Z3)
        assert np.array_equal(bits(d.run(v, NV + 2)[:, NV]), bits(base)), name(v)
        if NV > 2:  # first of a short group of NV - 1 vectors
            assert np.array_equal(bits(d.run(v, NV - 1, first=NV)[:, 0]), bits(base)), name(v)
    finally:
        d.free()


@pytest.mark.parametrize("nv", [5, 16])
def test_special_values_reach_exactly_their_row_and_their_column(nv):
    m, k, i, j, c = 300, 600, 171, 333, 1  # several bands and strips; every Z[i, v] > 0
    A, Z, _ = synth(m, k, nv)
    Z = Z + 0.5
    for v in VARIANTS:
        clean = mm.multiply_t_multi(A, Z, variant=v)
        for special in (np.nan, np.inf):
            B = A.copy()
            B[i, j] = special
            hit = mm.multiply_t_multi(B, Z, variant=v)
            rows = np.arange(k) != j
            assert np.array_equal(bits(hit[rows]), bits(clean[rows])), (name(v), special)
            assert np.all(np.isnan(hit[j])) if np.isnan(special) else np.all(hit[j] == np.inf), (name(v), hit[j])
        Zn = Z.copy()
        Zn[i, c] = np.nan
        hit = mm.multiply_t_multi(A, Zn, variant=v)
        cols = np.arange(nv) != c
        assert np.array_equal(bits(hit[:, cols]), bits(clean[:, cols])), name(v)
        assert np.all(np.isnan(hit[:, c])), name(v)


@pytest.mark.parametrize("m,k,nv", [(300, 600, 5), (4099, 129, 17), (20001, 7, 3)])
def test_separate_and_a_single_leftover_vector_are_mvg_gemv_t_bit_for_bit(m, k, nv):
    A, Z, _, _ = signed(m, k, nv)
    single = np.stack([mm.multiply_t(A, Z[:, c]) for c in range(nv)], axis=1)
    for v in (0, SEPARATE):
        assert np.array_equal(bits(mm.multiply_t_multi(A, Z, variant=v)), bits(single)), name(v)
    for v in FUSED:
        if nv % chains(v) == 1:  # the last column went through mvg_gemv_t
            assert np.array_equal(bits(mm.multiply_t_multi(A, Z, variant=v)[:, -1]), bits(single[:, -1])), name(v)


def test_empty_sums():
    k, nv, ldy = 300, 5, 307
    Z = mm.DeviceBuffer(4).upload(np.ones(4))
    A = mm.DeviceBuffer(4).upload(np.ones(4))
    Y = mm.DeviceBuffer((nv + 1) * ldy + 1)
    pay = np.zeros(Y.n, dtype=bool)
    pay[(1 + np.arange(nv)[:, None] * ldy + np.arange(k)[None, :]).ravel()] = True
    try:
        for v in VARIANTS:
            Y.upload(np.full(Y.n, np.nan))
            mm.gemv_t_multi(A.ptr, k, Z.ptr, 0, Y.ptr + 8, ldy, 0, k, nv, None, v)  # m == 0: zeros over the poison
            sync()
            img = Y.download()
            assert np.all(np.isnan(img[~pay])) and np.array_equal(bits(img[pay]), bits(np.zeros(nv * k))), name(v)
            Y.upload(np.full(Y.n, np.nan))
            mm.gemv_t_multi(A.ptr, 0, Z.ptr, 4, Y.ptr, ldy, 4, 0, nv, None, v)  # k == 0: Y untouched
            mm.gemv_t_multi(A.ptr, k, Z.ptr, 4, Y.ptr, ldy, 4, k, 0, None, v)  # nv == 0: Y untouched
            sync()
            assert np.all(np.isnan(Y.download())), name(v)
    finally:
        for b in (A, Z, Y):
            b.free()


def test_deterministic_and_independent_of_the_workspace():
    """The same call twice; a call after others that leave the (null stream's) workspace dirty and
    make it regrow; the call on a fresh set of buffers: the same bits every time."""
    shapes = [(4099, 129, 9), (257, 1000, 16), (20001, 7, 17)]
    data = {s: signed(*s)[:2] for s in shapes}
    devs = {s: Dev(*data[s]) for s in shapes}
    try:
        for v in VARIANTS:
            first = devs[4099, 129, 9].run(v)
            if v in FUSED:
                assert mm.gemv_t_multi_plan(129, 4099, 129, 9, v)[1] > 1
            assert np.array_equal(bits(devs[4099, 129, 9].run(v)), bits(first)), name(v)
            devs[257, 1000, 16].run(v)
            devs[20001, 7, 17].run(v)
            assert np.array_equal(bits(devs[4099, 129, 9].run(v)), bits(first)), name(v)
            fresh = Dev(*data[4099, 129, 9])
            try:
                assert np.array_equal(bits(fresh.run(v)), bits(first)), name(v)
            finally:
                fresh.free()
    finally:
        for d in devs.values():
            d.free()
