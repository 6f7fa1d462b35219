"""mvg_gemv_t_exact and mvg_gemv_t_exact_multi on the GPU, bit for bit: every variant and the
automatic pick against the oracle's multiply_std_rowwise on a contiguous transposed copy of A (the
`ref` of tests/test_gpu_gemv_t.py, compared there at 1e-12), on the raw bits (`view(np.uint64)`).

The signed uniform data is the one whose order shows in the bits
(tests/test_gemv_t_exact_host.py::test_the_gpu_tests_signed_data_tells_orders_apart). Shapes: the
list of tests/test_gpu_gemv_t.py, and per staged variant the edges read from its name
(tseqx_w<NW>_c<SC>_t<T>_b<NB>): m around one tile and the ring, k around one and two strips.
"""
import functools
import re

import numpy as np
import pytest

import wide_views as W
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from test_gpu_gemv_t import SHAPES, ref, signed, synth

pytestmark = pytest.mark.gpu
lib = _lib.lib
NVAR = lib.mvg_gemv_t_exact_variant_count()
NMVAR = lib.mvg_gemv_t_exact_multi_variant_count()
VARIANTS = list(range(NVAR))
MVARIANTS = list(range(NMVAR))
STAGED_RE = re.compile(r"tseqx_w(\d+)_c(\d+)_t(\d+)_b(\d+)$")


def name(v):
    return lib.mvg_gemv_t_exact_variant_name(v).decode()


def mname(v):
    return lib.mvg_gemv_t_exact_multi_variant_name(v).decode()


STAGED = {v: tuple(int(g) for g in STAGED_RE.match(name(v)).groups()) for v in VARIANTS if STAGED_RE.match(name(v))}


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    """Bit for bit; a NaN of the oracle's is matched by any NaN (payloads are not compared)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.all(np.isnan(got[nan]))) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def staged_ok(v, lda, off):
    """Whether staged variant v takes this layout: 16-B aligned A and z, an even lda < 2^29 / T."""
    return off % 2 == 0 and lda % 2 == 0 and lda < (1 << 29) // STAGED[v][2]


class Dev:
    """A, z on the device (rows lda apart, everything `off` doubles into its buffer) between NaN, and
    a y whose fringes must stay NaN."""

    def __init__(self, A, z, lda=None, off=0):
        self.m, self.k = A.shape
        self.lda, self.off = lda or self.k, off
        img = np.full(self.m * self.lda + off + 2, np.nan)
        img[off + np.arange(self.m)[:, None] * self.lda + np.arange(self.k)[None, :]] = A
        zi = np.full(self.m + off + 2, np.nan)
        zi[off:off + self.m] = z
        self.A, self.z = mm.DeviceBuffer(img.size).upload(img), mm.DeviceBuffer(zi.size).upload(zi)
        self.y = mm.DeviceBuffer(self.k + off + 2)

    def call(self, v, fill=np.nan):
        """The return code and y's whole image after variant v ran over a y filled with `fill`."""
        self.y.upload(np.full(self.y.n, fill))
        o = 8 * self.off
        rc = lib.mvg_gemv_t_exact_variant(self.A.ptr + o, self.lda, self.z.ptr + o, self.y.ptr + o, self.m, self.k, v, None)
        sync()
        return rc, self.y.download()

    def run(self, v, fill=np.nan):
        rc, img = self.call(v, fill)
        _lib.check(rc, name(v))
        out = np.concatenate([img[:self.off], img[self.off + self.k:]])
        assert np.array_equal(bits(out), bits(np.full(out.size, fill))), "stored outside y"
        return img[self.off:self.off + self.k]

    def free(self):
        for b in (self.A, self.z, self.y):
            b.free()


def check_shape(m, k):
    """Every variant and auto on both data sets; rows an even lda apart (k, or k + 1 for an odd k), so
    that the staged forms run at every shape (odd lda: test_views_and_alignments)."""
    A, z, want = synth(m, k)
    As, zs, want_s, _ = signed(m, k)
    d, ds = Dev(A, z, lda=k + (k & 1)), Dev(As, zs, lda=k + (k & 1))
    try:
        for v in VARIANTS:
            y, ys = d.run(v), ds.run(v)
            assert np.array_equal(bits(y), bits(want)), (name(v), m, k, "synth", int(np.sum(bits(y) != bits(want))))
            assert np.array_equal(bits(ys), bits(want_s)), (name(v), m, k, "signed", int(np.sum(bits(ys) != bits(want_s))))
    finally:
        d.free()
        ds.free()


@pytest.mark.parametrize("m,k", SHAPES)
def test_every_variant_on_synth_and_signed_data(m, k):
    check_shape(m, k)


@pytest.mark.parametrize("v", sorted(STAGED), ids=name)
def test_every_variant_at_the_edges_of_a_staged_form(v):
    """m around one tile, the ring and one row more; k around one strip, two strips and one column more."""
    _, sc, t, nb = STAGED[v]
    for m in (t - 1, t, t + 1, nb * t, nb * t + 1):
        for k in (sc - 1, sc, sc + 1, 2 * sc + 1):
            check_shape(m, k)


@pytest.mark.parametrize("m,k,lda,off", [(70, 300, 303, 1), (70, 300, 302, 1), (70, 300, 303, 0), (70, 300, 512, 0),
                                         (257, 1000, 1003, 1)],
                         ids=["odd-lda-off8", "even-lda-off8", "odd-lda", "lda>k", "257x1000-odd-lda-off8"])
def test_views_and_alignments(m, k, lda, off):
    """lda = k + 3 with A, z and y 8 bytes off a 16-B boundary, NaN fringes everywhere: the direct
    forms and auto are exact, a staged form is refused by number and leaves y alone; on an aligned
    even lda > k the staged forms run too."""
    A, z, want, _ = signed(m, k)
    d = Dev(A, z, lda=lda, off=off)
    try:
        ran = 0
        for v in VARIANTS:
            if v in STAGED and not staged_ok(v, lda, off):
                rc, img = d.call(v)
                assert rc == _lib.MVG_E_INVALID and lib.mvg_last_error().decode().startswith("mvg_gemv_t_exact"), (name(v), rc)
                assert np.all(np.isnan(img)), (name(v), "a refused call wrote y")
                continue
            assert np.array_equal(bits(d.run(v)), bits(want)), (name(v), m, k, lda, off)
            ran += 1
        assert ran == (NVAR if staged_ok(min(STAGED), lda, off) else NVAR - len(STAGED))
    finally:
        d.free()


def test_empty_sums():
    k = 300
    z, A, y = mm.DeviceBuffer(4).upload(np.ones(4)), mm.DeviceBuffer(4).upload(np.ones(4)), mm.DeviceBuffer(k + 2)
    try:
        for v in VARIANTS:
            y.upload(np.full(k + 2, np.nan))
            mm.gemv_t_exact(A.ptr, k, z.ptr, y.ptr + 8, 0, k, None, v)  # m == 0: k times +0.0 over the poison
            sync()
            img = y.download()
            assert np.isnan(img[0]) and np.isnan(img[-1]) and np.array_equal(bits(img[1:-1]), bits(np.zeros(k))), name(v)
            y.upload(np.full(k + 2, np.nan))
            mm.gemv_t_exact(A.ptr, 0, z.ptr, y.ptr, 4, 0, None, v)  # k == 0: y untouched
            sync()
            assert np.all(np.isnan(y.download())), name(v)
        Y = mm.DeviceBuffer(3 * (k + 5))
        for v in MVARIANTS:
            Y.upload(np.full(Y.n, np.nan))
            mm.gemv_t_exact_multi(A.ptr, k, z.ptr, 4, Y.ptr, k + 5, 0, k, 3, None, v)  # m == 0: zeros, the gaps stay
            sync()
            img = Y.download().reshape(3, k + 5)
            assert np.array_equal(bits(img[:, :k]), bits(np.zeros((3, k)))) and np.all(np.isnan(img[:, k:])), mname(v)
            Y.upload(np.full(Y.n, np.nan))
            mm.gemv_t_exact_multi(A.ptr, k, z.ptr, 4, Y.ptr, k + 5, 4, 0, 3, None, v)  # k == 0
            mm.gemv_t_exact_multi(A.ptr, k, z.ptr, 4, Y.ptr, k + 5, 4, k, 0, None, v)  # nv == 0
            sync()
            assert np.all(np.isnan(Y.download())), mname(v)
        Y.free()
    finally:
        for b in (A, z, y):
            b.free()


SPECIALS = [np.nan, np.inf, -np.inf, -0.0, 5e-324, 2.0 ** -1040]


@pytest.mark.parametrize("special", SPECIALS, ids=["nan", "+inf", "-inf", "-0.0", "min-subnormal", "subnormal"])
def test_special_values(special):
    """One special in A[i, j]: y[j] is the oracle's, every other column keeps the clean run's bits.
    One special in z[i]: it reaches every column, as the oracle's chain has it."""
    m, k, i, j = 150, 330, 77, 201  # several tiles and strips of every form, a cut strip
    A, z, want, _ = signed(m, k)
    B, zb = A.copy(), z.copy()
    B[i, j] = special
    zb[i] = special
    want_a, want_z = ref(B, z), ref(A, zb)
    others = np.arange(k) != j
    assert same_bits(want_a[others], want[others])  # the oracle agrees that the column is alone
    da, dz = Dev(B, z), Dev(A, zb)
    try:
        for v in VARIANTS:
            ya, yz = da.run(v), dz.run(v)
            assert same_bits(ya, want_a), (name(v), "A", special)
            assert np.array_equal(bits(ya[others]), bits(want[others])), (name(v), "a special left its column")
            assert same_bits(yz, want_z), (name(v), "z", special)
    finally:
        da.free()
        dz.free()


def test_signed_zeros_follow_the_chain():
    """Every product -0.0: the chain starts at +0.0 and +0.0 + -0.0 = +0.0."""
    m, k = 70, 130
    A, z = np.full((m, k), -0.0), np.ones(m)
    A[:, ::2] = 0.0
    want = ref(A, z)
    assert np.array_equal(bits(want), bits(np.zeros(k)))
    d = Dev(A, z)
    try:
        for v in VARIANTS:
            assert np.array_equal(bits(d.run(v)), bits(want)), name(v)
    finally:
        d.free()


def test_the_same_call_twice_over_different_garbage():
    m, k = 4099, 129
    A, z, want, _ = signed(m, k)
    d = Dev(A, z, lda=k + 1)  # even: the staged forms run too
    try:
        for v in VARIANTS:
            a, b = d.run(v, fill=np.nan), d.run(v, fill=-1.5e300)
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(want)), name(v)
    finally:
        d.free()


@pytest.mark.parametrize("m,k", [(150, 330), (4099, 129), (67, 64)])
def test_multi_columns_equal_the_single_vector_call(m, k):
    """nv = 1 .. 5 and 9 with ldz > m and ldy > k: column v has the bits of mvg_gemv_t_exact on z_v
    (and of the oracle) for every multi variant, and the gaps between the columns of Y stay NaN."""
    nvmax, ldz, ldy = 9, m + 3, k + 5
    rng = np.random.default_rng(m * 31 + k)
    A, Z = rng.uniform(-1.0, 1.0, size=(m, k)), rng.uniform(-1.0, 1.0, size=(nvmax, m))
    want = np.stack([ref(A, Z[v]) for v in range(nvmax)])
    zimg = np.full((nvmax, ldz), np.nan)
    zimg[:, :m] = Z
    dA, dZ = mm.DeviceBuffer(m * k).upload(A), mm.DeviceBuffer(zimg.size).upload(zimg)
    dY, dy = mm.DeviceBuffer(nvmax * ldy), mm.DeviceBuffer(k)
    try:
        single = []
        for v in range(nvmax):
            mm.gemv_t_exact(dA.ptr, k, dZ.ptr + 8 * v * ldz, dy.ptr, m, k)
            sync()
            single.append(dy.download())
        single = np.stack(single)
        assert np.array_equal(bits(single), bits(want))
        for mv in MVARIANTS:
            for nv in (1, 2, 3, 4, 5, 9):
                dY.upload(np.full(dY.n, np.nan))
                mm.gemv_t_exact_multi(dA.ptr, k, dZ.ptr, ldz, dY.ptr, ldy, m, k, nv, None, mv)
                sync()
                img = dY.download().reshape(nvmax, ldy)
                assert np.array_equal(bits(img[:nv, :k]), bits(single[:nv])), (mname(mv), nv)
                assert np.all(np.isnan(img[:nv, k:])) and np.all(np.isnan(img[nv:])), (mname(mv), nv, "stored outside Y")
    finally:
        for b in (dA, dZ, dY, dy):
            b.free()


def test_host_array_forms_agree_with_the_pointer_forms():
    m, k, nv = 257, 300, 5
    A, z, want, _ = signed(m, k)
    rng = np.random.default_rng(7)
    Z = rng.uniform(-1.0, 1.0, size=(m, nv))
    want_m = np.stack([ref(A, Z[:, v]) for v in range(nv)], axis=1)
    for v in VARIANTS:
        assert np.array_equal(bits(mm.multiply_t(A, z, variant=v, exact=True)), bits(want)), name(v)
    for mv in MVARIANTS:
        Y = mm.multiply_t_multi(A, Z, variant=mv, exact=True)
        assert Y.shape == (k, nv) and np.array_equal(bits(Y), bits(want_m)), mname(mv)
    # without `exact` both return what they return today: mvg_gemv_t / mvg_gemv_t_multi
    dA, dz, dy = mm.DeviceBuffer(m * k).upload(A), mm.DeviceBuffer(m).upload(z), mm.DeviceBuffer(k)
    dZ, dY = mm.DeviceBuffer(m * nv).upload(np.ascontiguousarray(Z.T)), mm.DeviceBuffer(k * nv)
    try:
        mm.gemv_t(dA.ptr, k, dz.ptr, dy.ptr, m, k)
        sync()
        assert np.array_equal(bits(mm.multiply_t(A, z)), bits(dy.download()))
        assert np.array_equal(bits(mm.multiply_t(A, z, 0, False)), bits(dy.download()))
        mm.gemv_t_multi(dA.ptr, k, dZ.ptr, m, dY.ptr, k, m, k, nv)
        sync()
        assert np.array_equal(bits(mm.multiply_t_multi(A, Z)), bits(dY.download().reshape(nv, k).T))
    finally:
        for b in (dA, dz, dy, dZ, dY):
            b.free()


# ------------------------------------------------------------------ wide views (tests/wide_views.py)
@pytest.fixture(scope="module")
def arena():
    a = W.Arena()
    yield a
    a.free()


@functools.lru_cache(maxsize=None)
def wide_data(k):
    rng = np.random.default_rng(k)
    A, z = rng.uniform(-1.0, 1.0, size=(W.M, k)), rng.uniform(-1.0, 1.0, size=W.M)
    want = ref(A, z)
    for a in (A, z, want):
        a.setflags(write=False)
    return A, z, want


def run_on_view(arena, view, k, variants):
    """The variants on a 67-row A inside the arena, rows view.ld apart: those whose check lets the
    lda through are exact, the others answer MVG_E_INVALID and leave y alone. Returns the names that ran."""
    A, z, want = wide_data(k)
    wa = W.WideOperand(arena, W.M, k, view.ld, view.shift).write(A)
    dz, dy = mm.DeviceBuffer(W.M).upload(z), mm.DeviceBuffer(k + 2)
    ran = []
    try:
        for v in variants:
            dy.upload(np.full(k + 2, np.nan))
            rc = lib.mvg_gemv_t_exact_variant(wa.ptr, view.ld, dz.ptr, dy.ptr + 8, W.M, k, v, None)
            sync()
            img = dy.download()
            if v in STAGED and not staged_ok(v, view.ld, view.shift):
                assert rc == _lib.MVG_E_INVALID and np.all(np.isnan(img)), (name(v), view, rc)
                continue
            _lib.check(rc, name(v))
            assert np.isnan(img[0]) and np.isnan(img[-1]), (name(v), view, "stored outside y")
            assert np.array_equal(bits(img[1:-1]), bits(want)), (name(v), view, int(np.sum(bits(img[1:-1]) != bits(want))))
            ran.append(name(v))
        assert np.all(np.isnan(wa.read()[:, :W.FRINGE])) and np.all(np.isnan(wa.read()[:, -W.FRINGE:]))
    finally:
        wa.release()
        dz.free()
        dy.free()
    return ran


@pytest.mark.parametrize("view", (W.FAR_A, W.FAR_A_ODD), ids=repr)
def test_rows_2_to_the_26_doubles_apart(arena, view):
    """64-bit row offsets: row 4 starts 2^31 bytes in, row 64 2^32 doubles in. Every staged form's
    lda limit is below this stride, so they refuse it; every direct form and auto run."""
    ran = run_on_view(arena, view, 300, VARIANTS)
    assert ran == [name(v) for v in VARIANTS if v not in STAGED], ran


@pytest.mark.parametrize("v", sorted(STAGED), ids=name)
def test_a_staged_form_at_the_largest_lda_its_check_lets_through(arena, v):
    """lda = 2^29 / T - 2: the last row of a tile lies just under 2^32 bytes from the tile's first,
    so the 32-bit per-lane offset must be zero-extended; one lda further the form is refused."""
    t = STAGED[v][2]
    lda = (1 << 29) // t - 2
    assert staged_ok(v, lda, 0) and not staged_ok(v, lda + 2, 0)
    assert (t - 1) * lda * 8 >= 1 << 31  # past what a signed 32-bit offset holds
    assert run_on_view(arena, W.View(f"LIMIT_T{t}", lda, W.M), 300, [v]) == [name(v)]


@pytest.mark.parametrize("m,k", [(200, 600), (70, 8200), (70, 32768)], ids=["narrow", "mid", "wide"])
def test_auto_through_a_staged_pick_and_through_its_fallback(m, k):
    """With the swept range's lower bounds lowered (the test hook) auto takes the staged pick of the
    k class on aligned operands, and variant 1 inside the same call where the operands break the
    pick's rules (8 bytes off a 16-B boundary, an odd lda); a block of 5 goes out as a fused group
    of 4 and one vector through the staged pick. The oracle's bits every time."""
    A, z, want, _ = signed(m, k)
    rng = np.random.default_rng(k)
    Z = np.concatenate([z[None, :], rng.uniform(-1.0, 1.0, size=(4, m))])
    want_m = np.stack([ref(A, Z[v]) for v in range(5)])
    devs = {"aligned": Dev(A, z), "off8": Dev(A, z, off=1), "odd-lda": Dev(A, z, lda=k + 1)}
    dZ, dY = mm.DeviceBuffer(5 * m).upload(Z), mm.DeviceBuffer(5 * k)
    try:
        _lib.check(lib.mvg_debug_set_gemv_t_exact_swept(64, 4096), "hook")
        for how, d in devs.items():
            o = 8 * d.off
            v = lib.mvg_gemv_t_exact_resolve_variant(d.A.ptr + o, d.lda, d.z.ptr + o, m, k)
            assert (v in STAGED) == (how == "aligned"), (how, name(v))
            assert v == (lib.mvg_gemv_t_exact_auto_variant(d.lda, m, k) if how == "aligned" else 1), (how, name(v))
            assert np.array_equal(bits(d.run(0)), bits(want)), (how, name(v))
        assert mname(lib.mvg_gemv_t_exact_multi_auto_variant(k, m, m, k, 5)).endswith("_v4")
        dY.upload(np.full(dY.n, np.nan))
        mm.gemv_t_exact_multi(devs["aligned"].A.ptr, k, dZ.ptr, m, dY.ptr, k, m, k, 5)
        sync()
        assert np.array_equal(bits(dY.download().reshape(5, k)), bits(want_m))
    finally:
        lib.mvg_debug_set_gemv_t_exact_swept(0, 0)
        for b in list(devs.values()) + [dZ, dY]:
            b.free()
