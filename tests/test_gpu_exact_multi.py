"""mvg_gemv_exact_multi: every entry of its variant table, and the automatic choice, bit for bit
against the reference's chain per vector (oracle.multiply_std_rowwise, matr_utils.c:86-96) and
against mvg_gemv_exact on the same device buffers.

The shapes are the smallest at which gemv_seq_hop_multi<L, W, U, NV> takes another path. With
S = L * W columns per segment and U segments in flight (both read from the variant's name;
"auto" and "separate" run the single-vector kernels, whose 8-lane pick is l8_w2_u16):

  K  0, 1, 15, 16, S-1, S, S+15, U*S, U*S+1, (U+1)*S+15, (2U+1)*S+17: the head alone, no main
     segment, the drain alone, exactly one group, a group and a drain, two groups, with 0, 1 and 2
     masked tails;
  M  1, 64/L - 1, 64/L + 1, 2*64/L + 3: the clamp to the last row, partial waves;
  operands  A on a 128-B line with lda a multiple of 16 / lda = K + 13 (every row its own head) /
     A and X shifted by 8 bytes;
  nv 1, 2, 3, 4, 5, 7, 8, 11: every remainder of the groups of 4 and of 2.

Data with mixed signs (adversarial_cases.payload(sign=True)), so a different order of summation
shows in the bits. Operands are guarded images (tests/gpu_guarded.py): NaN around A, X and Y, in
every padding column, in rows m .. ldy-1 of Y and in a spare vector past nv.
"""
import re

import numpy as np
import pytest

import adversarial_cases as AC
import gpu_guarded as G
from matvec_mpi_multiplier_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
NVS = (1, 2, 3, 4, 5, 7, 8, 11)
NAMES = [lib.mvg_gemv_exact_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_exact_multi_variant_count())]


def form(name):
    """(L, W, U) of a variant."""
    m = re.fullmatch(r"hopm_l(\d+)_w(\d+)_u(\d+)_v(\d+)", name)
    return (int(m[1]), int(m[2]), int(m[3])) if m else (8, 2, 16)


def k_values(name):
    L, W, U = form(name)
    S = L * W
    return sorted({0, 1, 15, 16, S - 1, S, S + 15, U * S, U * S + 1, (U + 1) * S + 15, (2 * U + 1) * S + 17})


def m_values(name):
    R = 64 // form(name)[0]
    return sorted({1, R - 1, R + 1, 2 * R + 3} - {0})


def layouts(k):
    """(lda, ldx, shift in doubles)."""
    lined = (k // 16 + 1) * 16
    return [("lines", lined, k + 2, 0), ("mid_line", k + 13, k + 3, 0), ("off_8_bytes", lined, k + 3, 1)]


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


_data = {}


def data(k, m_max):
    """A (m_max x k), X (11 x k) and the reference's Y (11 x m_max), made once per K: the first m
    rows and nv vectors serve every smaller case (a row's chain does not depend on the others)."""
    if (k, m_max) not in _data:
        A, X = AC.payload(m_max, k, max(NVS), sign=True)
        want = np.stack([oracle.multiply_std_rowwise(A, X[v]) if k else np.zeros(m_max) for v in range(max(NVS))])
        _data[(k, m_max)] = (A, X, want)
    return _data[(k, m_max)]


class Operands:
    def __init__(self, A, X, lda, ldx, shift):
        self.m, self.k = A.shape
        self.nv, self.lda, self.ldx, self.ldy = X.shape[0], lda, ldx, self.m + 3
        self.dA = G.matrix(A, lda - self.k, shift)
        self.dX = G.vectors(X, ldx, shift)
        self.dY = G.result(self.nv, self.m, self.ldy, spare=1)
        self.dY1 = G.result(self.nv, self.m, self.ldy, spare=1)

    def multi(self, variant):
        """One call into a NaN-filled Y; the guard image must be clean. Returns nv x m."""
        self.dY.fill()
        _lib.check(lib.mvg_gemv_exact_multi_variant(self.dA.ptr, self.lda, self.dX.ptr, self.ldx, self.dY.ptr, self.ldy,
                                                    self.m, self.k, self.nv, variant, None), NAMES[variant])
        sync()
        img = self.dY.image()
        bad = G.violations(img, self.dY.lay)
        assert not bad, (NAMES[variant], self.m, self.k, self.nv, self.lda, bad[:4])
        return self.dY.lay.payload(img)

    def single(self):
        """mvg_gemv_exact per vector on the same A and X."""
        self.dY1.fill()
        for v in range(self.nv):
            _lib.check(lib.mvg_gemv_exact(self.dA.ptr, self.lda, self.dX.ptr + 8 * v * self.ldx,
                                          self.dY1.ptr + 8 * v * self.ldy, self.m, self.k, None), "mvg_gemv_exact")
        sync()
        img = self.dY1.image()
        assert not G.violations(img, self.dY1.lay)
        return self.dY1.lay.payload(img)

    def free(self):
        for g in (self.dA, self.dX, self.dY, self.dY1):
            g.free()


@pytest.mark.parametrize("variant", range(len(NAMES)), ids=NAMES)
def test_every_column_has_the_reference_chains_bits(variant):
    name = NAMES[variant]
    ms = m_values(name)
    for k in k_values(name):
        A, X, want = data(k, max(ms))
        for label, lda, ldx, shift in layouts(k):
            for m in ms:
                for nv in NVS:
                    ops = Operands(A[:m], X[:nv], lda, ldx, shift)
                    try:
                        where = (name, label, "m", m, "k", k, "nv", nv)
                        got = ops.multi(variant)
                        good = G.exact_ok(want[:nv, :m])(got)
                        assert good.all(), (where, np.argwhere(~good)[:4], got[~good][:4])
                        assert G.same_or_both_nan(got, ops.single()), where  # the device's own single-vector chains
                    finally:
                        ops.free()


def special_shape(name):
    L, W, U = form(name)
    return 2 * (64 // L) + 3, (U + 1) * L * W + 15


@pytest.mark.parametrize("variant", range(len(NAMES)), ids=NAMES)
def test_special_values_stay_in_their_row_and_their_vector(variant):
    """A NaN, and an inf - inf, in one row of A reach that row of every vector and no other row;
    a NaN in one x reaches every row of that vector and no other vector."""
    name = NAMES[variant]
    m, k = special_shape(name)
    nv, row, vec = 5, m // 2, 3
    A, X0 = AC.payload(m, k, nv, sign=True)
    for j in AC.col_positions(k):
        X = AC.special_x(X0, j, "nan")
        ops = Operands(A, X, k + 13, k + 3, 0)
        try:
            base = ops.multi(variant)
            assert np.isfinite(base).all()
            for kind in ("nan", "inf_minus_inf"):
                As = A.copy()
                for c, val in AC.special_row(A[row], j, kind):
                    As[row, c] = val
                    ops.dA.poke(row, c, val)
                want = np.stack([oracle.multiply_std_rowwise(As, X[v]) for v in range(nv)])
                got = ops.multi(variant)
                where = (name, kind, "row", row, "col", j)
                assert np.isnan(want[:, row]).all() and np.isfinite(np.delete(want, row, axis=1)).all(), where
                assert G.exact_ok(want)(got).all() and G.same_or_both_nan(got, want), (where, got[:, row])
                assert G.same_or_both_nan(np.delete(got, row, axis=1), np.delete(base, row, axis=1)), where
                for c, _ in AC.special_row(A[row], j, kind):
                    ops.dA.poke(row, c, A[row, c])
            ops.dX.poke(vec, j, np.nan)
            got = ops.multi(variant)
            assert np.isnan(got[vec]).all(), (name, "x", j)
            assert G.same_or_both_nan(np.delete(got, vec, axis=0), np.delete(base, vec, axis=0)), (name, "x", j)
        finally:
            ops.free()


@pytest.mark.parametrize("variant", range(len(NAMES)), ids=NAMES)
def test_overflow_and_cancel_in_one_vector_alone(variant):
    """The reference's chain on 1e308 * [10, 10, -10, -10] goes +inf and then NaN, on 1e307 it
    overflows to +inf and stays; only the vector that holds those x shows either."""
    name = NAMES[variant]
    m, k = special_shape(name)
    nv, vec = 5, 2
    j = AC.boundary_col(k) - 2  # the four columns straddle a segment boundary
    A, x, rows = AC.overflow_cancel(m, k, j, ordinary=True)
    X = AC.payload(m, k, nv, sign=True)[1]
    X[:, j:j + 4] = [0.25, 0.25, -0.25, -0.25]
    X[vec] = x
    want = np.stack([oracle.multiply_std_rowwise(A, X[v]) for v in range(nv)])
    assert np.isfinite(np.delete(want, vec, axis=0)).all()
    assert np.isnan(want[vec, rows[0::2]]).all() and (want[vec, rows[1::2]] == np.inf).all()
    ops = Operands(A, X, k + 13, k + 3, 1)
    try:
        got = ops.multi(variant)
        assert G.exact_ok(want)(got).all() and G.same_or_both_nan(got, want), (name, got[vec, rows])
        assert G.same_or_both_nan(got, ops.single()), name
    finally:
        ops.free()


# the smallest shape of every class in which the automatic choice takes multi kernels
# (csrc/gemv_exact.hip pick_seq_multi_variant): (m, k, lda, the picks for 4 and for 2 vectors)
AUTO_CLASSES = [(6144, 769, 769, "hopm_l8_w2_u4_v4", "hopm_l8_w2_u8_v2"),
                (2048, 8193, 8208, "hopm_l16_w4_u4_v4", "hopm_l16_w4_u4_v2"),
                (5, 4097, 4097, "hopm_l32_w8_u4_v2", "hopm_l32_w8_u4_v2")]


@pytest.mark.parametrize("m,k,lda,pick4,pick2", AUTO_CLASSES, ids=[f"{c[0]}x{c[1]}" for c in AUTO_CLASSES])
def test_automatic_choice_mixes_groups_of_four_two_and_one(m, k, lda, pick4, pick2):
    """Seven vectors through variant 0 where it takes multi kernels: a pass of 4, a pass of 2 and
    a single-vector pass (the 32-lane class: three passes of 2 and one), every column the
    reference's bits, nothing stored outside Y."""
    from matvec_mpi_multiplier_amd import multiplier as mm

    nv = 7
    assert NAMES[lib.mvg_gemv_exact_multi_auto_variant(lda, k, m, k, nv)] == pick4
    assert NAMES[lib.mvg_gemv_exact_multi_auto_variant(lda, k, m, k, 3)] == pick2
    A, X = AC.payload(m, k, nv, sign=True)
    want = np.stack([oracle.multiply_std_rowwise(A, X[v]) for v in range(nv)])
    Ap = np.zeros((m, lda))
    Ap[:, :k] = A
    dA, dX = mm.DeviceBuffer(m * lda).upload(Ap), mm.DeviceBuffer(nv * k).upload(X)
    dY = G.result(nv, m, m + 3, spare=1)
    try:
        _lib.check(lib.mvg_gemv_exact_multi(dA.ptr, lda, dX.ptr, k, dY.ptr, m + 3, m, k, nv, None), "mvg_gemv_exact_multi")
        sync()
        G.assert_clean(dY.image(), dY.lay, G.exact_ok(want), f"auto {m}x{k}")
    finally:
        for b in (dA, dX, dY):
            b.free()
